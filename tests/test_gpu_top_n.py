"""The top-N columns of each row of Theta = W^T H, ranked on the device: nbmf_top_n, Context.top_n, NBMF.top_n.

REFERENCE.  Always ``host_top_n(ctx.predict_rows(...float64...), top, exclude)`` (tests/test_top_n_cpu.py: np.lexsort over
the eligible columns, theta descending, ties by ascending column, -1 / NaN padding), with the same clip flag.  Columns must
be equal and scores equal BIT FOR BIT (NaN padding by isnan): the device ranks the very panel predict_rows returns, so
there is no tolerance anywhere in this file.  One test is independent of predict_rows: dyadic factors, whose products
and sums are exact in float64 in any order, against NumPy's ``W.T @ H``.

SHAPES.  The smallest at which each path of the kernel runs: n = 300 (two 256-column chunks, the second ragged, pad columns
up to the padded width), top = 1 / 7 / 256 (the sort network at 2, 8 and 256 entries), n = 5 < top, K = 130 (sliced factor
layout) at n = 8195 (a row of 64 KiB + 24 B: not resident in LDS), several panels, offsets inside a 16-row tile."""
import ctypes

import numpy as np
import pytest

from conftest import config1_X, config1_mask
from test_top_n_cpu import host_top_n, same_ranking

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


_cases = {}


def case(k, m, n, seed=0):
    """(W k x m with columns on the simplex, H k x n in (0.1, 0.9)) of one shape, made once and shared (read-only)."""
    key = (k, m, n, seed)
    if key not in _cases:
        r = np.random.default_rng(2000 + 97 * seed + k)
        W = r.uniform(0.1, 0.9, (k, m))
        W /= W.sum(0)
        H = r.uniform(0.1, 0.9, (k, n))
        W.setflags(write=False)
        H.setflags(write=False)
        _cases[key] = (W, H)
    return _cases[key]


def context(hip, W, H):
    ctx = hip.Context(W.shape[1], H.shape[1], W.shape[0])
    ctx.set_factors(W, H)
    return ctx


def reference(ctx, top, row0=0, nrows=None, exclude=None, clip=True):
    return host_top_n(ctx.predict_rows(row0, nrows, clip_theta=clip), top, exclude)


def well_formed(cols, scores, n, top, nrows):
    """What holds for every result whatever the data: shapes, no pad column, pads only at the end, no repeats."""
    assert cols.shape == (nrows, top) and scores.shape == (nrows, top)
    assert cols.dtype == np.int64 and scores.dtype == np.float64
    assert np.all((cols >= -1) & (cols < n)), "a pad column or a stray index was returned"
    pad = cols < 0
    assert np.array_equal(pad, np.isnan(scores))
    assert np.all(pad[:, 1:] >= pad[:, :-1]), "a real entry follows a pad"
    for row in cols:
        real = row[row >= 0]
        assert real.size == np.unique(real).size


# ---- 1. ragged shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [1, 7, 256])
def test_ragged_shape(hip, top):
    W, H = case(5, 37, 300)
    with context(hip, W, H) as ctx:
        cols, scores = ctx.top_n(top)
        well_formed(cols, scores, 300, top, 37)
        assert np.all(cols >= 0)                                           # 300 eligible columns: nothing is padded
        same_ranking((cols, scores), reference(ctx, top))
        only_cols, none = ctx.top_n(top, return_scores=False)
        assert none is None and np.array_equal(only_cols, cols)


# ---- 2. independent of predict_rows ---------------------------------------------------------------------------------------
def test_dyadic_factors_against_numpy(hip):
    """Entries in {0, 1, 2, 3} / 16, K = 3: every product and every partial sum is a multiple of 1/256 below 1 -- exact in
    float64 in any order, with or without FMA -- so NumPy's W.T @ H is the truth, and it has thousands of ties per row."""
    r = np.random.default_rng(31)
    W = r.integers(0, 4, (3, 40)) / 16.0
    H = r.integers(0, 4, (3, 1000)) / 16.0
    truth = W.T @ H
    assert truth.max() < 1.0 and np.unique(truth).size <= 28
    with context(hip, W, H) as ctx:
        assert np.array_equal(ctx.predict_rows(), truth)
        for top in (10, 256):
            got = ctx.top_n(top)
            well_formed(*got, 1000, top, 40)
            same_ranking(got, host_top_n(truth, top))


# ---- 3. / 4. rows that are one big tie -----------------------------------------------------------------------------------------
def test_constant_rows_of_h_give_the_first_columns(hip):
    W, _ = case(5, 37, 300)
    H = np.repeat(np.array([[0.3], [0.5], [0.2], [0.7], [0.4]]), 300, axis=1)
    with context(hip, W, H) as ctx:
        for top in (7, 256):
            cols, scores = ctx.top_n(top)
            assert np.array_equal(cols, np.tile(np.arange(top), (37, 1)))
            assert np.all(scores == scores[:, :1])
            same_ranking((cols, scores), reference(ctx, top))


@pytest.mark.parametrize("n,top", [(300, 256), (300, 7), (200, 256)])
def test_zero_row_of_w_ties_with_the_pad_columns_and_none_is_returned(hip, n, top):
    W, H = case(5, 37, 300)
    W, H = W.copy(), H[:, :n]
    W[:, [0, 17, 36]] = 0.0
    with context(hip, W, H) as ctx:
        cols, scores = ctx.top_n(top)
        well_formed(cols, scores, n, top, 37)
        want = np.where(np.arange(top) < n, np.arange(top), -1)
        for i in (0, 17, 36):
            assert np.array_equal(cols[i], want)
            assert np.all(scores[i, :min(n, top)] == 0.0)
        same_ranking((cols, scores), reference(ctx, top))


# ---- 5. fewer columns than slots ------------------------------------------------------------------------------------------------
def test_top_beyond_n_pads(hip):
    W, H = case(3, 20, 5)
    with context(hip, W, H) as ctx:
        cols, scores = ctx.top_n(7)
        well_formed(cols, scores, 5, 7, 20)
        assert np.all(cols[:, 5:] == -1) and np.all(np.isnan(scores[:, 5:]))
        assert np.array_equal(np.sort(cols[:, :5], axis=1), np.tile(np.arange(5), (20, 1)))
        same_ranking((cols, scores), reference(ctx, 7))


# ---- 6. exclude ---------------------------------------------------------------------------------------------------------------------
def test_exclude(hip):
    m, n, top = 37, 300, 7
    W, H = case(5, m, n)
    r = np.random.default_rng(8)
    ex = r.random((m, n)) < 0.5
    ex[3] = True                                                            # nothing left
    ex[9] = True
    ex[9, r.choice(n, top - 1, replace=False)] = False                      # exactly top - 1 left
    ex[20] = False
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        want = host_top_n(theta, top, ex)
        got = ctx.top_n(top, exclude=ex)
        well_formed(*got, n, top, m)
        same_ranking(got, want)
        cols, scores = got
        assert not ex[np.nonzero(cols >= 0)[0], cols[cols >= 0]].any(), "an excluded column was returned"
        assert np.all(cols[3] == -1) and np.all(np.isnan(scores[3]))
        assert np.all(cols[9, :top - 1] >= 0) and cols[9, top - 1] == -1
        assert np.array_equal(np.sort(cols[9, :top - 1]), np.nonzero(~ex[9])[0])
        # bytes: any nonzero value means skip
        same_ranking(ctx.top_n(top, exclude=ex.astype(np.uint8) * r.integers(1, 256, (m, n), dtype=np.uint8)), want)
        # a slice of a wider array: ldx > n, and what lies beside the slice says "skip everything"
        wide = np.ones((m + 2, n + 40), dtype=bool)
        wide[1:m + 1, 7:7 + n] = ex
        same_ranking(ctx.top_n(top, exclude=wide[1:m + 1, 7:7 + n]), want)
        # a slab of rows with its own exclude rows
        same_ranking(ctx.top_n(top, 2, 9, exclude=ex[2:11]), tuple(a[2:11] for a in want))
        # no exclude and an exclude of zeros: the same bits
        same_ranking(ctx.top_n(top, exclude=np.zeros((m, n), dtype=np.uint8)), ctx.top_n(top))
        # top = 256 with about half the columns gone: every row is short
        got = ctx.top_n(256, exclude=ex)
        well_formed(*got, n, 256, m)
        same_ranking(got, host_top_n(theta, 256, ex))


# ---- 7. NaN ---------------------------------------------------------------------------------------------------------------------------
def test_nan_is_never_returned(hip):
    m, n, top = 37, 300, 7
    W, H = case(5, m, n)
    Wn, Hn = W.copy(), H.copy()
    Hn[2, 123] = np.nan                                                     # column 123 of Theta is NaN in every row
    Wn[1, 30] = np.nan                                                      # row 30 of Theta is NaN in every column
    with context(hip, W, H) as ctx:
        clean = ctx.predict_rows()
    with context(hip, Wn, Hn) as ctx:
        theta = ctx.predict_rows()
        assert np.all(np.isnan(theta[:, 123])) and np.all(np.isnan(theta[30]))
        assert np.isnan(theta).sum() == m + n - 1
        for t in (top, 256):
            cols, scores = ctx.top_n(t)
            well_formed(cols, scores, n, t, m)
            assert not np.any(cols == 123)
            assert np.all(cols[30] == -1) and np.all(np.isnan(scores[30]))
            same_ranking((cols, scores), host_top_n(theta, t))
            # the other rows and columns are what they are without the NaNs, column 123 left out
            skip = np.zeros((m, n), dtype=bool)
            skip[:, 123] = True
            keep = np.arange(m) != 30
            want = host_top_n(clean, t, skip)
            same_ranking((cols[keep], scores[keep]), (want[0][keep], want[1][keep]))


# ---- 8. clip ---------------------------------------------------------------------------------------------------------------------------
def test_clip_ties_at_one_and_raw_order_without_it(hip):
    m, n, top = 37, 300, 7
    W, H = case(5, m, n)
    H3 = 3.0 * H
    with context(hip, W, H3) as ctx:
        raw = ctx.predict_rows(clip_theta=False)
        over = raw > 1.0
        assert np.all(over.sum(1) >= 2 * top) and not np.all(over)
        clipped = ctx.top_n(top, clip_theta=True)
        same_ranking(clipped, reference(ctx, top, clip=True))
        assert np.all(clipped[1] == 1.0)
        for i in range(m):                                                  # the tie at 1.0 goes to the lowest columns
            assert np.array_equal(clipped[0][i], np.nonzero(over[i])[0][:top])
        unclipped = ctx.top_n(top, clip_theta=False)
        same_ranking(unclipped, host_top_n(raw, top))
        assert np.all(unclipped[1] > 1.0) and not np.array_equal(unclipped[0], clipped[0])
        same_ranking(ctx.top_n(256, clip_theta=True), reference(ctx, 256, clip=True))
        same_ranking(ctx.top_n(256, clip_theta=False), host_top_n(raw, 256))


# ---- 9. panels and offsets ------------------------------------------------------------------------------------------------------------------
def test_panels_offsets_and_repeats_do_not_change_a_bit(hip, monkeypatch):
    m, n, top = 130, 257, 7
    W, H = case(5, m, n)
    ex = np.random.default_rng(4).random((m, n)) < 0.3
    with context(hip, W, H) as ctx:
        whole, whole_x = ctx.top_n(top), ctx.top_n(top, exclude=ex)
        same_ranking(whole, reference(ctx, top))
        same_ranking(whole_x, reference(ctx, top, exclude=ex))
        same_ranking(ctx.top_n(top), whole)                                 # twice: the same bits
        same_ranking(ctx.top_n(top, exclude=ex), whole_x)
        part, part_x = ctx.top_n(top, 5, 20), ctx.top_n(top, 5, 20, exclude=ex[5:25])
        same_ranking(part, tuple(a[5:25] for a in whole))
        same_ranking(part_x, tuple(a[5:25] for a in whole_x))
        for rows_per_panel in ("16", "7"):
            monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", rows_per_panel)
            same_ranking(ctx.top_n(top), whole)
            same_ranking(ctx.top_n(top, exclude=ex), whole_x)
            same_ranking(ctx.top_n(top, 5, 20), part)
            same_ranking(ctx.top_n(top, 5, 20, exclude=ex[5:25]), part_x)
            same_ranking(ctx.top_n(256, 100, 30), tuple(a[100:130] for a in reference(ctx, 256)))
        assert ctx.top_n(top, 3, 0)[0].shape == (0, top)


# ---- 10. sliced factor layout, a row beyond 64 KiB ---------------------------------------------------------------------------------------------
def test_sliced_layout_and_a_row_larger_than_64_kib(hip):
    m, n = 16, 8192 + 3
    W, H = case(130, m, n)
    ex = np.random.default_rng(6).random((m, n)) < 0.1
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        for top in (10, 256):
            got = ctx.top_n(top)
            well_formed(*got, n, top, m)
            same_ranking(got, host_top_n(theta, top))
        same_ranking(ctx.top_n(10, exclude=ex), host_top_n(theta, 10, ex))
    # the last real columns win when they hold the largest values: nothing stops short of column n - 1
    H2 = H.copy()
    H2[:, n - 3:] = 0.95
    with context(hip, W, H2) as ctx:
        cols, scores = ctx.top_n(3)
        assert np.array_equal(np.sort(cols, axis=1), np.tile(np.arange(n - 3, n), (m, 1)))
        same_ranking((cols, scores), reference(ctx, 3))


# ---- 11. after a fit ------------------------------------------------------------------------------------------------------------------------------
def test_ranking_follows_a_fit(hip, both_small_paths):
    X, mask = config1_X(), config1_mask()
    r = np.random.default_rng(21)
    W0 = r.uniform(0.1, 0.9, (6, 100))
    W0 /= W0.sum(0)
    H0 = r.uniform(0.1, 0.9, (6, 500))
    with hip.Context(100, 500, 6) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X, mask=mask)
        ctx.set_factors(W0, H0)
        before = ctx.top_n(10)
        ctx.run(5, 0.0)
        after = ctx.top_n(10)
        same_ranking(after, reference(ctx, 10))
        assert not np.array_equal(after[0], before[0])
        same_ranking(ctx.top_n(10, exclude=X != 0), reference(ctx, 10, exclude=X != 0))
    assert both_small_paths.served() == ((1, 0, 0) if both_small_paths == "single-launch" else (0, 0, 1))


# ---- 12. C-level errors ----------------------------------------------------------------------------------------------------------------------------
def test_c_level_errors_leave_the_context_usable(hip):
    m, n, top = 37, 53, 7
    W, H = case(4, m, n)
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    cols = np.full((m, top), -5, dtype=np.int64)
    scores = np.full((m, top), -7.25)
    ex = np.zeros((m, n), dtype=np.uint8)
    with hip.Context(m, n, 4) as ctx:
        assert lib.nbmf_top_n(ctx._h, 0, m, top, 1, None, 0, ptr(cols), ptr(scores), top) == hip.NBMF_ERR_STATE
        assert b"no factors" in lib.nbmf_last_error()
        with pytest.raises(hip.NBMFHipError, match="no factors"):
            ctx.top_n(top)
        ctx.set_factors(W, H)
        want = reference(ctx, top)
        bad = [(0, m, top, 1, None, 0, ptr(cols), ptr(scores), top - 1),     # ldout < top
               (0, m, 0, 1, None, 0, ptr(cols), ptr(scores), top),           # top < 1
               (0, m, 257, 1, None, 0, ptr(cols), ptr(scores), 257),         # top > NBMF_TOP_N_MAX
               (-1, 2, top, 1, None, 0, ptr(cols), ptr(scores), top),        # rows outside [0, m)
               (m, 1, top, 1, None, 0, ptr(cols), ptr(scores), top),
               (m - 1, 2, top, 1, None, 0, ptr(cols), ptr(scores), top),
               (0, -1, top, 1, None, 0, ptr(cols), ptr(scores), top),
               (0, m, top, 1, ptr(ex), n - 1, ptr(cols), ptr(scores), top),  # ldx < n with an exclude
               (0, m, top, 1, None, 0, None, ptr(scores), top)]              # no out_cols
        for args in bad:
            assert lib.nbmf_top_n(ctx._h, *args) == hip.NBMF_ERR_ARG, args
            assert np.all(cols == -5) and np.all(scores == -7.25)
            same_ranking(ctx.top_n(top), want)                              # as usable as before
        assert lib.nbmf_top_n(ctx._h, 5, 0, top, 1, None, 0, None, None, top) == hip.NBMF_OK   # nothing to do, nothing touched
        assert lib.nbmf_top_n(ctx._h, 0, m, top, 1, ptr(ex), n, ptr(cols), None, top) == hip.NBMF_OK
        assert np.array_equal(cols, want[0]) and np.all(scores == -7.25)    # no scores asked for: none written


# ---- 13. sentinels -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("panel_rows", [None, "16"])
def test_nothing_outside_the_slots_is_written(hip, monkeypatch, panel_rows):
    m, n, top = 37, 300, 7
    W, H = case(5, m, n)
    lib = hip.load()
    if panel_rows:
        monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", panel_rows)
    with context(hip, W, H) as ctx:
        want = reference(ctx, top, 6, 25)
        cols = np.full((25 + 2, top + 3), -5, dtype=np.int64)
        scores = np.full((25 + 2, top + 3), -7.25)
        rc = lib.nbmf_top_n(ctx._h, 6, 25, top, 1, None, 0, cols[1:].ctypes.data_as(ctypes.c_void_p),
                            scores[1:].ctypes.data_as(ctypes.c_void_p), top + 3)
        assert rc == hip.NBMF_OK
        same_ranking((np.ascontiguousarray(cols[1:26, :top]), np.ascontiguousarray(scores[1:26, :top])), want)
        cols[1:26, :top] = -5
        scores[1:26, :top] = -7.25
        assert np.all(cols == -5) and np.all(scores == -7.25), "something outside the slots was written"


# ---- 14. estimator --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_estimator(hip, orientation, monkeypatch):
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF, _solver
    g = np.random.default_rng(11)
    X = (g.random((60, 80)) < 0.3).astype(np.float64)
    model = NBMF(4, random_state=0, max_iter=30, tol=0, orientation=orientation).fit(X)
    assert model.W_.shape == (60, 4) and model.components_.shape == (4, 80)
    proba = model.predict_proba()
    cols, scores = model.top_n(10, exclude=X)
    well_formed(cols, scores, 80, 10, 60)
    assert np.all(cols >= 0)
    assert not X[np.arange(60)[:, None], cols].any(), "a feature the row already has was recommended"
    want = host_top_n(proba, 10, X)
    same_ranking((cols, scores), want)
    same_ranking(model.top_n(10, exclude=sp.csr_matrix(X)), want)
    same_ranking(model.top_n(10, exclude=sp.coo_matrix(X)), want)
    same_ranking(model.top_n(10, exclude=X.astype(bool)), want)
    monkeypatch.setattr(_solver, "TOP_N_EXCLUDE_BLOCK_BYTES", 80 * 7)         # row blocks of 7: nine calls, the last ragged
    same_ranking(model.top_n(10, exclude=X), want)
    same_ranking(model.top_n(10, exclude=sp.csr_matrix(X)), want)
    monkeypatch.undo()
    same_ranking(model.top_n(), host_top_n(proba, 10))                       # n defaults to 10, nothing excluded
    Wnew = model.transform(X[:7])
    same_ranking(model.top_n(5, W=Wnew, exclude=X[:7]), host_top_n(model.predict_proba(W=Wnew), 5, X[:7]))
