"""Per-row and per-column log-likelihood of Theta = W^T H against data, summed on the device: nbmf_score_rows,
Context.score_rows, NBMF.score_samples.

REFERENCE.  Always ``host_score_rows(ctx.predict_rows(...float64, same clip...), x, mask, eps)`` (tests/test_score_samples_cpu.py:
the semantics in NumPy, ``math.fsum`` per row and per column).  The device scores the very Theta predict_rows returns and
forms the logarithm's argument in the same operation order, so what separates the two is the logarithm (both within 1 ulp),
the roundings of a term and the summation order:

    |got - want| <= (c + 8) 2^-52 sum|t|,   c = the observed terms of that row or column   (assert_sums_within_bound)

and counts are equal exactly.  Wherever two device results are compared with each other (offsets, panels, repeats, bytes
against exactly binary float64) they are equal BIT FOR BIT.

SHAPES.  The smallest at which each path runs: n = 297 (staged width 300: three pad columns inside one lane's four, a ragged
last strip, five strips over two workgroups), m = 37 / 53 (pad rows in the last 16-row tile, several 16-row blocks, an
offset inside a tile), K = 5 (a ragged k block) and K = 130 (the sliced factor layout)."""
import ctypes

import numpy as np
import pytest

from conftest import config1_X, config1_mask
from test_score_samples_cpu import assert_sums_within_bound, host_score_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


_cases = {}


def case(k, m, n, seed=0):
    """(W k x m with columns on the simplex, H k x n in (0.1, 0.9), X bool m x n at 30 % ones, mask bool at about 70 %
    observed with row m // 3 and column n // 3 fully unobserved) of one shape, made once and shared (read-only)."""
    key = (k, m, n, seed)
    if key not in _cases:
        r = np.random.default_rng(3000 + 97 * seed + k)
        W = r.uniform(0.1, 0.9, (k, m))
        W /= W.sum(0)
        H = r.uniform(0.1, 0.9, (k, n))
        X = r.random((m, n)) < 0.3
        mask = r.random((m, n)) < 0.7
        mask[m // 3] = False
        mask[:, n // 3] = False
        for a in (W, H, X, mask):
            a.setflags(write=False)
        _cases[key] = (W, H, X, mask)
    return _cases[key]


def context(hip, W, H):
    ctx = hip.Context(W.shape[1], H.shape[1], W.shape[0])
    ctx.set_factors(W, H)
    return ctx


def reference(ctx, x, mask=None, row0=0, nrows=None, clip=True, eps=1e-8):
    return host_score_rows(ctx.predict_rows(row0, nrows, clip_theta=clip), x, mask, eps)


def within_bound(got, want):
    row_ll, row_obs, col_ll, col_obs = got
    if row_ll is not None:
        assert_sums_within_bound(row_ll, row_obs, want[0], want[1], want[2])
    if col_ll is not None:
        assert_sums_within_bound(col_ll, col_obs, want[3], want[4], want[5])


def same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g.dtype == w.dtype and g.shape == w.shape
            assert np.array_equal(g.view(np.uint64), w.view(np.uint64))


# ---- 1. ragged tile ----------------------------------------------------------------------------------------------------------
def test_ragged_tile_bytes(hip):
    m, n = 37, 297
    W, H, X, mask = case(5, m, n)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        got = ctx.score_rows(X, rows=True, cols=True)
        assert got[0].shape == (m,) and got[2].shape == (n,)
        assert np.all(got[1] == n) and np.all(got[3] == m)
        within_bound(got, host_score_rows(theta, X, None))
        got = ctx.score_rows(X, mask, rows=True, cols=True)
        within_bound(got, host_score_rows(theta, X, mask))
        assert got[1][m // 3] == 0 and got[0][m // 3] == 0.0 and not np.signbit(got[0][m // 3])   # a fully unobserved row
        assert got[3][n // 3] == 0 and got[2][n // 3] == 0.0                                      # ... and column
        assert got[1].sum() == mask.sum() == got[3].sum()
        # bytes: any nonzero value means 1 / observed
        r = np.random.default_rng(9)
        xb = X.astype(np.uint8) * r.integers(1, 256, (m, n), dtype=np.uint8)
        mb = mask.astype(np.uint8) * r.integers(1, 256, (m, n), dtype=np.uint8)
        same_bits(ctx.score_rows(xb, mb, rows=True, cols=True), got)
        # one half at a time: the same bits, None for the other
        same_bits(ctx.score_rows(X, mask), got[:2] + (None, None))
        same_bits(ctx.score_rows(X, mask, rows=False, cols=True), (None, None) + got[2:])
        # another eps
        within_bound(ctx.score_rows(X, mask, eps=1e-3, rows=True, cols=True), host_score_rows(theta, X, mask, 1e-3))


# ---- 2. float64 data ------------------------------------------------------------------------------------------------------------
def test_float64_data(hip):
    m, n = 37, 297
    W, H, X, mask = case(5, m, n)
    xr = np.random.default_rng(12).random((m, n))
    xr[0, :5] = [0.0, 1.0, 0.5, 1.0, 0.0]
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        within_bound(ctx.score_rows(xr, rows=True, cols=True), host_score_rows(theta, xr, None))
        within_bound(ctx.score_rows(xr, mask, rows=True, cols=True), host_score_rows(theta, xr, mask))
        # exactly binary float64 data: x * la + 0 * lb = la, the bits of the byte path
        same_bits(ctx.score_rows(X.astype(np.float64), mask, rows=True, cols=True), ctx.score_rows(X, mask, rows=True, cols=True))
        same_bits(ctx.score_rows(X.astype(np.float64), rows=True, cols=True), ctx.score_rows(X, rows=True, cols=True))


# ---- 3. sliced factor layout ------------------------------------------------------------------------------------------------------
def test_sliced_layout(hip):
    W, H, X, mask = case(130, 20, 130)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        within_bound(ctx.score_rows(X, mask, rows=True, cols=True), host_score_rows(theta, X, mask))
        within_bound(ctx.score_rows(X, rows=True, cols=True), host_score_rows(theta, X, None))


# ---- 4. row offsets inside a tile -----------------------------------------------------------------------------------------------------
def test_row_offsets_inside_a_tile(hip):
    m, n = 53, 297
    W, H, X, mask = case(5, m, n)
    with context(hip, W, H) as ctx:
        whole = ctx.score_rows(X, mask, rows=True, cols=True)
        within_bound(whole, reference(ctx, X, mask))
        part = ctx.score_rows(X[5:25], mask[5:25], 5, 20, rows=True, cols=True)
        same_bits(part[:2], tuple(a[5:25] for a in whole[:2]))               # a row does not know its neighbours or row0
        within_bound(part, reference(ctx, X[5:25], mask[5:25], 5, 20))        # the columns: over those rows only
        assert part[3].sum() == mask[5:25].sum()
        tail = ctx.score_rows(X[48:], None, 48, rows=True, cols=True)          # the last, ragged 16-row block alone
        within_bound(tail, reference(ctx, X[48:], None, 48, 5))
        empty = ctx.score_rows(X[7:7], mask[7:7], 7, 0, rows=True, cols=True)  # no rows: empty, and sums over nothing
        assert empty[0].shape == (0,) and empty[1].shape == (0,)
        assert not empty[2].any() and not empty[3].any() and empty[2].shape == (n,)


# ---- 5. panels --------------------------------------------------------------------------------------------------------------------------
def test_panels_do_not_change_a_bit(hip, monkeypatch):
    m, n = 53, 297
    W, H, X, mask = case(5, m, n)
    xr = np.random.default_rng(13).random((m, n))
    with context(hip, W, H) as ctx:
        calls = [lambda: ctx.score_rows(X, mask, rows=True, cols=True),
                 lambda: ctx.score_rows(X, rows=True, cols=True),
                 lambda: ctx.score_rows(xr, mask, rows=True, cols=True),
                 lambda: ctx.score_rows(X[5:25], mask[5:25], 5, 20, rows=True, cols=True),
                 lambda: ctx.score_rows(X[20:], mask[20:], 20, rows=True, cols=True),
                 lambda: ctx.score_rows(X, mask, rows=False, cols=True)]
        unset = [call() for call in calls]
        for rows_per_panel in ("16", "48", "7"):
            monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", rows_per_panel)
            for call, want in zip(calls, unset):
                same_bits(call(), want)


# ---- 6. strided inputs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bytes", "float64"])
def test_strided_inputs_and_nothing_beyond_the_last_column_is_read(hip, kind):
    m, n = 37, 297
    W, H, X, mask = case(5, m, n)
    x = X if kind == "bytes" else np.random.default_rng(14).random((m, n))
    # what lies beside the slices would change every sum and count if it were read: ones / NaN and "observed"
    wide_x = np.ones((m + 2, n + 40), dtype=bool) if kind == "bytes" else np.full((m + 2, n + 40), np.nan)
    wide_m = np.ones((m + 3, n + 9), dtype=np.uint8)
    wide_x[1:m + 1, 7:7 + n] = x
    wide_m[2:m + 2, 0:n] = mask
    with context(hip, W, H) as ctx:
        want = ctx.score_rows(x, mask, rows=True, cols=True)
        same_bits(ctx.score_rows(wide_x[1:m + 1, 7:7 + n], wide_m[2:m + 2, 0:n], rows=True, cols=True), want)
        same_bits(ctx.score_rows(wide_x[6:26, 7:7 + n], wide_m[7:27, 0:n], 5, 20), tuple(a[5:25] for a in want[:2]) + (None, None))
        # the last columns count: nothing stops short of column n - 1
        m2 = np.zeros((m, n), dtype=bool)
        m2[:, n - 3:] = True
        got = ctx.score_rows(x, m2, rows=True, cols=True)
        assert np.all(got[1] == 3) and np.all(got[3][n - 3:] == m) and not got[3][:n - 3].any()
        within_bound(got, reference(ctx, x, m2))


# ---- 7. no clip ---------------------------------------------------------------------------------------------------------------------------
def test_without_the_clip_a_theta_beyond_one_has_no_likelihood(hip):
    m, n = 37, 297
    W, H, X, mask = case(5, m, n)
    with context(hip, W, 2.2 * H) as ctx:
        raw = ctx.predict_rows(clip_theta=False)
        over = raw > 1.0 + 1e-8
        assert over.any(axis=1).all() and not over.all()
        x = X.copy()
        x[:10] |= over[:10]                                                 # rows 0..9: x = 1 wherever theta > 1, so no NaN term
        want = host_score_rows(raw, x, None)
        assert not np.isnan(want[0][:10]).any() and np.isnan(want[0][10:]).all()
        got = ctx.score_rows(x, clip_theta=False, rows=True, cols=True)
        within_bound(got, want)                                             # NaN where the reference is NaN, the bound elsewhere
        assert np.any(raw[:10][x[:10]] > 1.0 + 1e-8)                        # (terms with theta > 1 are in those sums)
        # masking the NaN terms away leaves finite sums everywhere
        mk = ~(over & ~x)
        got = ctx.score_rows(x, mk, clip_theta=False, rows=True, cols=True)
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
        within_bound(got, host_score_rows(raw, x, mk))
        # and with the clip every theta beyond 1 is 1
        within_bound(ctx.score_rows(x, rows=True, cols=True), reference(ctx, x))


# ---- 8. the same call twice ------------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bits(hip):
    W, H, X, mask = case(5, 53, 297)
    xr = np.random.default_rng(15).random((53, 297))
    with context(hip, W, H) as ctx:
        for x in (X, xr):
            first = ctx.score_rows(x, mask, rows=True, cols=True)
            same_bits(ctx.score_rows(x, mask, rows=True, cols=True), first)
    with context(hip, W, H) as ctx:                                          # another context, the same factors
        same_bits(ctx.score_rows(xr, mask, rows=True, cols=True), first)


# ---- 9. against the existing scalar --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [True, False])
def test_sums_agree_with_loglik_strict(hip, masked):
    X, mask = config1_X(), (config1_mask() if masked else None)
    r = np.random.default_rng(21)
    W = r.uniform(0.1, 0.9, (6, 100))
    W /= W.sum(0)
    H = r.uniform(0.1, 0.9, (6, 500))
    with hip.Context(100, 500, 6) as ctx:
        ctx.set_hyper(1.2, 1.2, 1e-8)
        ctx.upload(X, mask=mask)
        ctx.set_factors(W, H)
        want = ctx.loglik_strict()
        row_ll, row_obs, col_ll, col_obs = ctx.score_rows(X.astype(np.uint8), mask, clip_theta=False, rows=True, cols=True)
        assert row_obs.sum() == ctx.n_obs() == col_obs.sum()
        assert abs(row_ll.sum() - want) <= 1e-10 * abs(want)
        assert abs(col_ll.sum() - want) <= 1e-10 * abs(want)
        assert ctx.loglik_strict() == want                                  # the data context is as it was


# ---- 10. the estimator ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_estimator(hip, orientation, masked, monkeypatch):
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF, _solver
    g = np.random.default_rng(11)
    X = (g.random((60, 90)) < 0.3).astype(np.float64)
    fit_mask = g.random((60, 90)) < 0.9 if masked else None
    model = NBMF(4, random_state=0, max_iter=20, tol=0, orientation=orientation).fit(X, mask=fit_mask)
    assert model.W_.shape == (60, 4) and model.components_.shape == (4, 90)
    mask = None
    if masked:
        mask = fit_mask.copy()
        mask[7] = False                                                      # nothing of row 7 is observed
    want = host_score_rows(model.predict_proba(), X, mask)
    for axis, (w_ll, w_obs, w_abs) in ((0, want[:3]), (1, want[3:])):
        sums, counts = _solver.device_score_samples(model.W_, model.components_, X, mask=mask, axis=axis)
        assert_sums_within_bound(sums, counts, w_ll, w_obs, w_abs)
        scores, got_counts = model.score_samples(X, mask=mask, axis=axis, return_counts=True)
        assert scores.dtype == np.float64 and scores.shape == w_ll.shape and np.array_equal(got_counts, counts)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(scores, np.where(counts > 0, sums / np.maximum(counts, 1), np.nan), equal_nan=True)
        assert np.array_equal(model.score_samples(X, mask=mask, axis=axis), scores, equal_nan=True)
        assert np.array_equal(np.isnan(scores), counts == 0)
        if masked and axis == 0:
            assert np.isnan(scores[7]) and counts[7] == 0 and np.isnan(scores).sum() == 1
        # the same data in other clothes: bool, a float mask, CSR -- rows bit for bit
        fmask = None if mask is None else 2.5 * mask
        smask = None if mask is None else sp.csr_matrix(mask)
        for Xo, mo in ((X.astype(bool), mask), (X, fmask), (sp.csr_matrix(X), smask), (sp.coo_matrix(X), mask)):
            assert np.array_equal(model.score_samples(Xo, mask=mo, axis=axis), scores, equal_nan=True)
        # ... and in row blocks of 16: rows bit for bit, features to the bound (the blocks' sums are added on the host)
        monkeypatch.setattr(_solver, "SCORE_SAMPLES_BLOCK_BYTES", 16 * 8 * 90)
        b_sums, b_counts = _solver.device_score_samples(model.W_, model.components_, sp.csr_matrix(X), mask=smask, axis=axis)
        if axis == 0:
            assert np.array_equal(b_sums, sums) and np.array_equal(b_counts, counts)
        else:
            assert_sums_within_bound(b_sums, b_counts, w_ll, w_obs, w_abs)
        monkeypatch.undo()
    # new rows: transform first, then score them with W=
    Wnew = model.transform(X[:7])
    m7 = None if mask is None else mask[:7]
    w7 = host_score_rows(model.predict_proba(W=Wnew), X[:7], m7)
    sums, counts = _solver.device_score_samples(Wnew, model.components_, X[:7], mask=m7, axis=0)
    assert_sums_within_bound(sums, counts, *w7[:3])
    assert np.array_equal(model.score_samples(X[:7], mask=m7, W=Wnew), sums / counts)
    # without a mask the mean over everything is score's summand: the model's mean log-likelihood on its own W_
    if not masked:
        scores, counts = model.score_samples(X, return_counts=True)
        assert np.all(counts == 90) and abs(scores.mean() - want[0].sum() / X.size) <= 1e-12 * abs(scores.mean())


# ---- errors that need a device ------------------------------------------------------------------------------------------------------------------------
def test_state_errors_leave_the_context_usable(hip):
    m, n = 37, 53
    W, H, X, mask = case(4, m, n)
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    xb = np.ascontiguousarray(X).view(np.uint8)
    row_ll = np.full(m, -7.25)
    with hip.Context(m, n, 4) as ctx:
        args = (0, m, 1, 1e-8, ptr(xb), hip.DATA_U8, n, None, 0, ptr(row_ll), None, None, None)
        assert lib.nbmf_score_rows(ctx._h, *args) == hip.NBMF_ERR_STATE       # no factors
        assert b"no factors" in lib.nbmf_last_error()
        with pytest.raises(hip.NBMFHipError, match="no factors"):
            ctx.score_rows(X)
        ctx.set_factors(W, H)
        want = ctx.score_rows(X, mask, rows=True, cols=True)
        within_bound(want, reference(ctx, X, mask))
        bad = [(-1, 2) + args[2:], (m, 1) + args[2:], (m - 1, 2) + args[2:], (0, -1) + args[2:],     # rows outside [0, m)
               args[:5] + (7,) + args[6:], args[:5] + (hip.DATA_F32,) + args[6:],                    # an unknown x_kind
               args[:6] + (n - 1,) + args[7:],                                                       # ldx < n
               args[:7] + (ptr(xb), n - 1) + args[9:],                                               # ldmask < n with a mask
               args[:3] + (float("nan"),) + args[4:], args[:3] + (-1e-8,) + args[4:],                # eps
               args[:4] + (None,) + args[5:],                                                        # no data
               args[:9] + (None, None, None, None)]                                                  # nothing asked for
        for a in bad:
            assert lib.nbmf_score_rows(ctx._h, *a) == hip.NBMF_ERR_ARG, a
            assert np.all(row_ll == -7.25)
        same_bits(ctx.score_rows(X, mask, rows=True, cols=True), want)       # as usable as before
        # no rows: nothing is read (null data), the row outputs are left alone, the column outputs are zeroed
        col_ll, col_obs = np.full(n, -7.25), np.full(n, -5, dtype=np.int64)
        assert lib.nbmf_score_rows(ctx._h, 5, 0, 1, 1e-8, None, hip.DATA_U8, n, None, 0, ptr(row_ll), None, ptr(col_ll),
                                   ptr(col_obs)) == hip.NBMF_OK
        assert np.all(row_ll == -7.25) and not col_ll.any() and not col_obs.any()
        # only what was asked for is written
        row_obs = np.full(m, -5, dtype=np.int64)
        assert lib.nbmf_score_rows(ctx._h, 0, m, 1, 1e-8, ptr(xb), hip.DATA_U8, n, None, 0, None, ptr(row_obs), None,
                                   None) == hip.NBMF_OK
        assert np.all(row_obs == n) and np.all(row_ll == -7.25)
    # a sharded context refuses, and answers again once detached
    with hip.Context(m, n, 4) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X, mask=mask)
        ctx.set_factors(W, H)
        ctx.comm_init_host(lambda arr: None, 1, 0)
        assert lib.nbmf_score_rows(ctx._h, *args) == hip.NBMF_ERR_STATE
        assert b"unsharded" in lib.nbmf_last_error()
        with pytest.raises(hip.NBMFHipError, match="unsharded"):
            ctx.score_rows(X, mask)
        ctx.comm_detach()
        same_bits(ctx.score_rows(X, mask, rows=True, cols=True), want)
