"""Where given columns of a row of Theta = W^T H stand in top_n's order, counted on the device: nbmf_rank_rows,
Context.rank_of, NBMF.rank_of / ranking_metrics.

REFERENCE.  Always ``host_rank_of(ctx.predict_rows(...float64...), indptr, indices, exclude)`` (tests/test_rank_of_cpu.py:
plain NumPy comparisons of doubles over the eligible columns), with the same clip flag.  The integer arrays must be EQUAL and
the scores equal BIT FOR BIT (NaN by isnan): the device counts keys of the very panel predict_rows returns, so there is no
tolerance anywhere in this file.  Two tests are independent of the host reference: the ranks against ``ctx.top_n`` (a
rank is the slot top_n gives the column), and dyadic factors, whose products and sums are exact in float64 in any order,
against NumPy's ``W.T @ H``.

SHAPES.  The smallest at which each path of the kernel runs: n = 300 (two 256-column strides, the second ragged, pad columns
up to the padded width), m = 37 (rows at every offset inside a 16-row tile), 0 / 1 / 7 / 8 / 9 / 300 targets in a row (no
pass, one ragged group, one full group, a second group, many passes), K = 130 (sliced factor layout) at n = 8195 (a row of
64 KiB + 24 B: longer than anything a kernel could stage in LDS, with a ragged end), several panels."""
import ctypes

import numpy as np
import pytest

from test_rank_of_cpu import csr_of, host_rank_of, same_ranks

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
        r = np.random.default_rng(3000 + 97 * seed + k)
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


def targets(m, n, seed, counts=(0, 1, 7, 8, 9), repeats=True):
    """Per-row target lists: the counts cycle over the rows; unsorted, and (with ``repeats``) every third row repeats one."""
    r = np.random.default_rng(seed)
    lists = []
    for i in range(m):
        c = counts[i % len(counts)]
        t = r.choice(n, size=min(c, n), replace=False).tolist()
        if repeats and i % 3 == 1 and t:
            t.append(t[0])
        lists.append(t)
    return lists


def reference(ctx, indptr, indices, row0=0, nrows=None, exclude=None, clip=True):
    return host_rank_of(ctx.predict_rows(row0, nrows, clip_theta=clip), indptr, indices, exclude)


# ---- 1. ragged shape ------------------------------------------------------------------------------------------------------
def test_ragged_shape(hip):
    m, n = 37, 300
    W, H = case(5, m, n)
    lists = targets(m, n, 1)
    lists[4] = np.random.default_rng(2).permutation(n).tolist()            # every column of the row: 38 passes
    assert {len(t) for t in lists} >= {0, 1, 7, 8, 9, 10, 300}
    indptr, indices = csr_of(lists)
    lib = hip.load()
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    with context(hip, W, H) as ctx:
        got = ctx.rank_of(indptr, indices)
        want = reference(ctx, indptr, indices)
        same_ranks(got, want)
        assert np.all(got[4] == n) and np.all(got[0] >= 0)
        assert np.array_equal(np.sort(got[0][indptr[4]:indptr[5]]), np.arange(n))   # all columns of a row: a permutation
        # some outputs NULL: the same arrays for the rest
        for keep in ((0,), (3,), (4,), (1, 2), (0, 3, 4), (1, 2, 3)):
            out = [np.full(indices.size, -5, dtype=np.int64) for _ in range(3)] + [np.full(indices.size, -7.25),
                                                                                     np.full(m, -5, dtype=np.int64)]
            args = [ptr(out[q]) if q in keep else None for q in range(5)]
            assert lib.nbmf_rank_rows(ctx._h, 0, m, 1, ptr(indptr), ptr(indices), None, 0, *args) == hip.NBMF_OK
            for q in range(5):
                if q in keep:
                    assert out[q].tobytes() == want[q].tobytes()
                else:
                    assert np.all(out[q] == (-7.25 if q == 3 else -5))


# ---- 2. against top_n, independently of the host reference ------------------------------------------------------------------
def test_rank_is_the_slot_of_top_n(hip):
    m, n = 37, 300
    W, H = case(5, m, n)
    ex = np.random.default_rng(12).random((m, n)) < 0.2
    lists = targets(m, n, 3, counts=(9, 40, 300, 0, 1), repeats=False)
    lists = [t if len(t) < 300 else list(range(n)) for t in lists]
    indptr, indices = csr_of(lists)
    rows = np.repeat(np.arange(m), np.diff(indptr))
    with context(hip, W, H) as ctx:
        rank, above, tied, scores, eligible = ctx.rank_of(indptr, indices, exclude=ex)
        cols, top_scores = ctx.top_n(256, exclude=ex)
        shown = (rank >= 0) & (rank < 256)
        assert shown.sum() > 1500
        assert np.array_equal(cols[rows[shown], rank[shown]], indices[shown])
        assert np.array_equal(top_scores[rows[shown], rank[shown]].view(np.uint64), scores[shown].view(np.uint64))
        for i, j in zip(rows[~shown], indices[~shown]):
            assert j not in cols[i]
        assert np.array_equal(rank < 0, ex[rows, indices])
        assert np.array_equal(eligible, n - ex.sum(1))
        assert np.array_equal(np.minimum(eligible, 256), (cols >= 0).sum(1))


def test_rank_beyond_the_slots_of_top_n(hip):
    m, n = 20, 8195
    W, H = case(130, m, n)
    ex = np.random.default_rng(13).random((m, n)) < 0.2
    lists = targets(m, n, 4, counts=(12, 3, 0, 8), repeats=False)
    indptr, indices = csr_of(lists)
    rows = np.repeat(np.arange(m), np.diff(indptr))
    with context(hip, W, H) as ctx:
        rank = ctx.rank_of(indptr, indices, exclude=ex)[0]
        cols = ctx.top_n(256, exclude=ex)[0]
        assert (rank >= 256).sum() > 50
        for i, j, rk in zip(rows, indices, rank):
            if 0 <= rk < 256:
                assert cols[i, rk] == j
            else:
                assert j not in cols[i]


# ---- the sliced factor layout, a row beyond 64 KiB ---------------------------------------------------------------------------
def test_sliced_layout_and_a_row_larger_than_64_kib(hip):
    m, n = 20, 8192 + 3
    W, H = case(130, m, n)
    ex = np.random.default_rng(6).random((m, n)) < 0.1
    lists = targets(m, n, 5, counts=(0, 1, 7, 8, 9, 20))
    lists[2] += [n - 1, n - 2, n - 3, 0]                                    # the ragged end and the first column
    indptr, indices = csr_of(lists)
    with context(hip, W, H) as ctx:
        same_ranks(ctx.rank_of(indptr, indices), reference(ctx, indptr, indices))
        same_ranks(ctx.rank_of(indptr, indices, exclude=ex), reference(ctx, indptr, indices, exclude=ex))
    # the last real columns hold the largest values: nothing stops short of column n - 1, nothing beyond it is counted
    H2 = H.copy()
    H2[:, n - 3:] = 0.95
    with context(hip, W, H2) as ctx:
        got = ctx.rank_of(*csr_of([[n - 1, n - 3, 5]] * m))
        same_ranks(got, reference(ctx, *csr_of([[n - 1, n - 3, 5]] * m)))
        assert np.all(got[0].reshape(m, 3)[:, :2] < 3) and np.all(got[0].reshape(m, 3)[:, 2] >= 3) and np.all(got[4] == n)


# ---- 3. dyadic factors: independent of predict_rows ----------------------------------------------------------------------------
def test_dyadic_factors_against_numpy(hip):
    """Entries in {0, 1, 2, 3} / 16, K = 3: every product and every partial sum is a multiple of 1/256 below 1 -- exact in
    float64 in any order, with or without FMA -- so NumPy's W.T @ H is the truth, and it has thousands of ties per row."""
    r = np.random.default_rng(31)
    W = r.integers(0, 4, (3, 40)) / 16.0
    H = r.integers(0, 4, (3, 1000)) / 16.0
    truth = W.T @ H
    assert truth.max() < 1.0 and np.unique(truth).size <= 28
    indptr, indices = csr_of(targets(40, 1000, 7, counts=(3, 8, 17, 0, 1)))
    with context(hip, W, H) as ctx:
        got = ctx.rank_of(indptr, indices)
        same_ranks(got, host_rank_of(truth, indptr, indices))
        assert np.median(got[2]) > 30 and got[2].max() > 200                # tied is large


# ---- 4. / 5. rows that are one big tie -------------------------------------------------------------------------------------------
def test_constant_rows_of_h_are_one_big_tie(hip):
    m, n = 37, 300
    W, _ = case(5, m, n)
    H = np.repeat(np.array([[0.3], [0.5], [0.2], [0.7], [0.4]]), n, axis=1)
    ex = np.random.default_rng(14).random((m, n)) < 0.3
    lists = targets(m, n, 8, repeats=False)
    indptr, indices = csr_of(lists)
    rows = np.repeat(np.arange(m), np.diff(indptr))
    with context(hip, W, H) as ctx:
        rank, above, tied, scores, eligible = got = ctx.rank_of(indptr, indices, exclude=ex)
        same_ranks(got, reference(ctx, indptr, indices, exclude=ex))
        ok = rank >= 0
        assert np.array_equal(eligible, n - ex.sum(1))
        assert np.all(above[ok] == 0) and np.array_equal(tied[ok], eligible[rows[ok]] - 1)
        lower = np.array([(~ex[i, :j]).sum() for i, j in zip(rows, indices)])
        assert np.array_equal(rank[ok], lower[ok])                         # the eligible columns left of the target


@pytest.mark.parametrize("n", [300, 200])
def test_zero_row_of_w_ties_with_the_pad_columns_and_no_pad_is_counted(hip, n):
    m = 37
    W, H = case(5, m, 300)
    W, H = W.copy(), H[:, :n]
    W[:, [0, 17, 36]] = 0.0
    ex = np.random.default_rng(15).random((m, n)) < 0.25
    lists = targets(m, n, 9)
    for i in (0, 17, 36):
        lists[i] = [n - 1, 0, 5, n - 2]
        ex[i, [n - 1, 0]] = False
    indptr, indices = csr_of(lists)
    with context(hip, W, H) as ctx:
        for x in (None, ex):
            rank, above, tied, scores, eligible = got = ctx.rank_of(indptr, indices, exclude=x)
            same_ranks(got, reference(ctx, indptr, indices, exclude=x))
            gone = 0 if x is None else x.sum(1)
            assert np.all(eligible == n - gone)
            for i in (0, 17, 36):
                t = slice(indptr[i], indptr[i] + 2)                         # the last and the first column of a zero row
                assert np.all(scores[t] == 0.0) and np.all(above[t] == 0) and np.all(tied[t] == eligible[i] - 1)
                assert rank[t].tolist() == [eligible[i] - 1, 0]


# ---- 6. unclipped and clipped --------------------------------------------------------------------------------------------------------
def test_clip_creates_the_ties_and_raw_order_without_it(hip):
    m, n = 37, 300
    W, H = case(5, m, n)
    H3 = 4.0 * H - 1.5                                                      # Theta below 0 and above 1
    lists = targets(m, n, 10)
    indptr, indices = csr_of(lists)
    with context(hip, W, H3) as ctx:
        raw = ctx.predict_rows(clip_theta=False)
        assert np.all((raw < 0.0).sum(1) >= 5) and np.all((raw > 1.0).sum(1) >= 5)
        unclipped = ctx.rank_of(indptr, indices, clip_theta=False)
        same_ranks(unclipped, host_rank_of(raw, indptr, indices))
        assert np.all(unclipped[2] == 0) and unclipped[3].min() < 0.0 and unclipped[3].max() > 1.0
        clipped = ctx.rank_of(indptr, indices, clip_theta=True)
        same_ranks(clipped, reference(ctx, indptr, indices, clip=True))
        assert clipped[3].min() == 0.0 and clipped[3].max() == 1.0
        at_edge = (clipped[3] == 0.0) | (clipped[3] == 1.0)
        assert at_edge.sum() > 20 and np.all(clipped[2][at_edge] >= 4) and np.all(clipped[2][~at_edge] == 0)


# ---- 7. NaN columns and excluded targets ------------------------------------------------------------------------------------------------
def test_nan_columns_and_excluded_targets(hip):
    m, n = 37, 300
    W, H = case(5, m, n)
    Hn = H.copy()
    Hn[2, 123] = np.nan                                                     # column 123 of Theta is NaN in every row
    r = np.random.default_rng(16)
    ex = (r.random((m, n)) < 0.2).astype(np.uint8) * 2                      # a byte of 2 excludes
    lists = [[123, int(np.flatnonzero(ex[i])[0]), int(np.flatnonzero(ex[i] == 0)[1]), 7] for i in range(m)]
    indptr, indices = csr_of(lists)
    with context(hip, W, H) as ctx:
        clean = ctx.predict_rows()
    with context(hip, W, Hn) as ctx:
        theta = ctx.predict_rows()
        assert np.all(np.isnan(theta[:, 123])) and np.isnan(theta).sum() == m
        rank, above, tied, scores, eligible = got = ctx.rank_of(indptr, indices, exclude=ex)
        same_ranks(got, host_rank_of(theta, indptr, indices, ex))
        at_nan, at_ex, at_ok = (np.arange(indices.size) % 4 == q for q in (0, 1, 2))
        for a in (rank, above, tied):
            assert np.all(a[at_nan] == -1) and np.all(a[at_ex] == -1) and np.all(a[at_ok] >= 0)
        assert np.all(np.isnan(scores[at_nan]))
        assert np.array_equal(scores[at_ex], clean[np.arange(m), indices[at_ex]])   # an excluded target reports its Theta
        assert np.array_equal(eligible, n - (ex != 0).sum(1) - (ex[:, 123] == 0))
        # the column is counted nowhere: the other targets are what they are without the NaN, column 123 excluded
        skip = ex.copy()
        skip[:, 123] = 1
        want = host_rank_of(clean, indptr, indices, skip)
        for q in (0, 1, 2):
            assert np.array_equal(got[q][~at_nan], want[q][~at_nan])
        assert np.array_equal(eligible, want[4])
        # bool instead of bytes, and a slice of a wider array: ldx > n, what lies beside the slice says "skip everything"
        same_ranks(ctx.rank_of(indptr, indices, exclude=ex != 0), got)
        wide = np.ones((m + 2, n + 40), dtype=np.uint8)
        wide[1:m + 1, 7:7 + n] = ex
        same_ranks(ctx.rank_of(indptr, indices, exclude=wide[1:m + 1, 7:7 + n]), got)
        # no exclude and an exclude of zeros: the same bits
        same_ranks(ctx.rank_of(indptr, indices, exclude=np.zeros((m, n), dtype=np.uint8)), ctx.rank_of(indptr, indices))


# ---- 8. panels and row offsets ---------------------------------------------------------------------------------------------------------------
def test_panels_offsets_and_repeats_do_not_change_a_bit(hip, monkeypatch):
    m, n = 37, 300
    W, H = case(5, m, n)
    ex = np.random.default_rng(4).random((m, n)) < 0.3
    lists = targets(m, n, 11)
    lists[20] = np.random.default_rng(5).permutation(n).tolist()
    indptr, indices = csr_of(lists)
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    with context(hip, W, H) as ctx:
        whole, whole_x = ctx.rank_of(indptr, indices), ctx.rank_of(indptr, indices, exclude=ex)
        same_ranks(whole, reference(ctx, indptr, indices))
        same_ranks(whole_x, reference(ctx, indptr, indices, exclude=ex))
        same_ranks(ctx.rank_of(indptr, indices), whole)                     # twice: the same bits
        same_ranks(ctx.rank_of(indptr, indices, exclude=ex), whole_x)

        def part_of(full):
            """Rows 3 .. 22 of a whole call, as a call with a slice of indptr gives them: -1 / NaN below the base."""
            out = [np.full(int(indptr[23]), -1, dtype=np.int64) for _ in range(3)] + [np.full(int(indptr[23]), np.nan)]
            for o, f in zip(out, full):
                o[indptr[3]:] = f[indptr[3]:indptr[23]]
            return (*out, full[4][3:23])

        for rows_per_panel in (None, "16", "5"):
            if rows_per_panel:
                monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", rows_per_panel)
            same_ranks(ctx.rank_of(indptr, indices), whole)
            same_ranks(ctx.rank_of(indptr, indices, exclude=ex), whole_x)
            assert indptr[3] > 0
            same_ranks(ctx.rank_of(indptr[3:24], indices, 3, 20), part_of(whole))
            same_ranks(ctx.rank_of(indptr[3:24], indices, 3, 20, exclude=ex[3:23]), part_of(whole_x))
            # the C call itself: what lies below the base and beyond the end keeps its sentinels
            out = [np.full(indices.size, -5, dtype=np.int64) for _ in range(3)] + [np.full(indices.size, -7.25),
                                                                                     np.full(22, -5, dtype=np.int64)]
            sub = np.ascontiguousarray(indptr[3:24])
            rc = lib.nbmf_rank_rows(ctx._h, 3, 20, 1, ptr(sub), ptr(indices), None, 0, ptr(out[0]), ptr(out[1]), ptr(out[2]),
                                    ptr(out[3]), ptr(out[4][1:]))
            assert rc == hip.NBMF_OK
            inside = (np.arange(indices.size) >= indptr[3]) & (np.arange(indices.size) < indptr[23])
            for q in range(4):
                assert out[q][inside].tobytes() == whole[q][inside].tobytes()
                assert np.all(out[q][~inside] == (-7.25 if q == 3 else -5)), "something outside the targets was written"
            assert np.array_equal(out[4][1:21], whole[4][3:23]) and out[4][0] == -5 and out[4][21] == -5


# ---- 9. nrows = 0 --------------------------------------------------------------------------------------------------------------------------------
def test_no_rows_touch_nothing(hip):
    m, n = 37, 53
    W, H = case(4, m, n)
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    out = np.full(4, -5, dtype=np.int64)
    with context(hip, W, H) as ctx:
        got = ctx.rank_of(np.array([0]), np.zeros(0, dtype=np.int32), 5, 0)
        assert [a.size for a in got] == [0] * 5
        got = ctx.rank_of(np.array([2]), np.array([1, 1, 1]), 5, 0)         # a base above 0 and no rows: all sentinels
        assert [a.size for a in got] == [2, 2, 2, 2, 0] and np.all(got[0] == -1) and np.all(np.isnan(got[3]))
        indptr = np.array([1], dtype=np.int64)
        assert lib.nbmf_rank_rows(ctx._h, 5, 0, 1, ptr(indptr), None, None, 0, ptr(out), ptr(out), ptr(out), None,
                                  ptr(out)) == hip.NBMF_OK
        assert lib.nbmf_rank_rows(ctx._h, 5, 0, 1, None, None, None, 0, None, None, None, None, None) == hip.NBMF_OK
        assert np.all(out == -5)
        # rows without any target: eligible alone
        got = ctx.rank_of(np.zeros(m + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
        assert [a.size for a in got] == [0, 0, 0, 0, m] and np.all(got[4] == n)


# ---- 10. errors ----------------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_and_the_context_alone(hip):
    m, n = 37, 53
    W, H = case(4, m, n)
    lib = hip.load()
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    lists = targets(m, n, 12)
    indptr, indices = csr_of(lists)
    ex = np.zeros((m, n), dtype=np.uint8)
    out = [np.full(indices.size, -5, dtype=np.int64) for _ in range(3)] + [np.full(indices.size, -7.25),
                                                                             np.full(m, -5, dtype=np.int64)]
    outs = [ptr(a) for a in out]
    with hip.Context(m, n, 4) as ctx:
        assert lib.nbmf_rank_rows(ctx._h, 0, m, 1, ptr(indptr), ptr(indices), None, 0, *outs) == hip.NBMF_ERR_STATE
        assert b"no factors" in lib.nbmf_last_error()
        with pytest.raises(hip.NBMFHipError, match="no factors"):
            ctx.rank_of(indptr, indices)
        ctx.set_factors(W, H)
        want = reference(ctx, indptr, indices)

        def changed(pos, value):
            a = indices.copy()
            a[pos] = value
            return a
        down = indptr.copy()
        down[10] = down[9] - 1
        below = indptr.copy()
        below[0] = -1
        bad = [((0, m, 1, ptr(indptr), ptr(changed(17, n)), None, 0, *outs), b"position 17"),       # a column == n
               ((0, m, 1, ptr(indptr), ptr(changed(40, -1)), None, 0, *outs), b"position 40"),      # a negative column
               ((0, m, 1, ptr(indptr), ptr(changed([30, 12], [n + 5, -3])), None, 0, *outs), b"position 12"),   # the lowest
               ((0, m, 1, ptr(down), ptr(indices), None, 0, *outs), b"decreases"),
               ((0, m, 1, ptr(below), ptr(indices), None, 0, *outs), b"negative"),
               ((0, m, 1, None, ptr(indices), None, 0, *outs), b"null indptr"),
               ((0, m, 1, ptr(indptr), None, None, 0, *outs), b"null indices"),
               ((-1, 2, 1, ptr(indptr), ptr(indices), None, 0, *outs), b"rows"),
               ((m, 1, 1, ptr(indptr), ptr(indices), None, 0, *outs), b"rows"),
               ((m - 1, 2, 1, ptr(indptr), ptr(indices), None, 0, *outs), b"rows"),
               ((0, -1, 1, ptr(indptr), ptr(indices), None, 0, *outs), b"rows"),
               ((0, m, 1, ptr(indptr), ptr(indices), ptr(ex), n - 1, *outs), b"ldx"),
               ((0, m, 1, ptr(indptr), ptr(indices), None, 0, None, None, None, None, None), b"no output")]
        for args, message in bad:
            assert lib.nbmf_rank_rows(ctx._h, *args) == hip.NBMF_ERR_ARG, message
            assert message in lib.nbmf_last_error()
            assert all(np.all(a == (-7.25 if q == 3 else -5)) for q, a in enumerate(out)), "an output was touched"
            same_ranks(ctx.rank_of(indptr, indices), want)                  # as usable as before
        # the same through Python: ValueError that names the position, before any launch
        with pytest.raises(ValueError, match="column 53 at position 17"):
            ctx.rank_of(indptr, changed(17, n))
        with pytest.raises(ValueError, match="column -1 at position 40"):
            ctx.rank_of(indptr, changed(40, -1))
        with pytest.raises(ValueError, match="decreases at row 9"):
            ctx.rank_of(down, indices)
        same_ranks(ctx.rank_of(indptr, indices), want)


# ---- 11. estimator ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fitted(hip):
    """A 12 x 40 model, its training matrix and its held-out ones, made once and shared (read-only)."""
    from nbmf_mm_amd import NBMF
    g = np.random.default_rng(11)
    full = (g.random((12, 40)) < 0.4).astype(np.float64)
    held = full * (g.random((12, 40)) < 0.3)
    held[3] = 0                                                             # a row without held-out entries
    train = full - held
    model = NBMF(3, random_state=0, max_iter=30, tol=0).fit(train)
    for a in (train, held):
        a.setflags(write=False)
    return model, train, held


def host_ranks(model, held, exclude):
    from nbmf_mm_amd._metrics import Ranks
    rows, cols = np.nonzero(held)
    indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=held.shape[0]))))
    rank, above, tied, score, eligible = host_rank_of(model.predict_proba(), indptr, cols, exclude)
    return Ranks(rows.astype(np.int64), cols.astype(np.int64), rank, score, above, tied, eligible)


def same_named(got, want):
    assert np.array_equal(got.rows, want.rows) and np.array_equal(got.cols, want.cols)
    assert got.rows.dtype == np.int64 and got.cols.dtype == np.int64
    same_ranks((got.rank, got.above, got.tied, got.score, got.eligible),
               (want.rank, want.above, want.tied, want.score, want.eligible))


def test_estimator_rank_of(fitted, monkeypatch):
    import scipy.sparse as sp
    from nbmf_mm_amd import _solver
    model, train, held = fitted
    want = host_ranks(model, held, train)
    assert np.all(want.rank >= 0) and np.array_equal(want.eligible, 40 - (train != 0).sum(1))
    same_named(model.rank_of(held, exclude=train), want)
    same_named(model.rank_of(sp.csr_matrix(held), exclude=sp.csr_matrix(train)), want)
    same_named(model.rank_of(sp.coo_matrix(held), exclude=train.astype(bool)), want)
    same_named(model.rank_of(held.astype(bool), exclude=sp.csc_matrix(train)), want)
    same_named(model.rank_of(held), host_ranks(model, held, None))          # nothing excluded
    # a target that is excluded: -1s and its score
    both = model.rank_of(held, exclude=held)
    assert np.all(both.rank == -1) and np.array_equal(both.score, want.score)
    # exclude streamed in row blocks of 5: three calls, the last ragged, each with its slice of indptr
    monkeypatch.setattr(_solver, "TOP_N_EXCLUDE_BLOCK_BYTES", 40 * 5)
    same_named(model.rank_of(held, exclude=train), want)
    same_named(model.rank_of(sp.csr_matrix(held), exclude=sp.csr_matrix(train)), want)
    monkeypatch.undo()
    # and the ranks are the slots of top_n
    cols = model.top_n(40, exclude=train)[0]
    assert np.array_equal(cols[want.rows, want.rank], want.cols)
    Wnew = model.transform(train[:7])
    got = model.rank_of(held[:7], W=Wnew, exclude=train[:7])
    assert np.array_equal(model.top_n(40, W=Wnew, exclude=train[:7])[0][got.rows, got.rank], got.cols)


def test_estimator_ranking_metrics(fitted):
    from sklearn.metrics import roc_auc_score
    from nbmf_mm_amd._metrics import ranking_from_ranks
    model, train, held = fitted
    for k in (3, 10, 1000):
        got = model.ranking_metrics(held, exclude=train, k=k)
        assert got == ranking_from_ranks(host_ranks(model, held, train), k=k)   # exactly: the same integers went in
        assert got["rows_scored"] == 11 and f"recall@{k}" in got
    assert model.ranking_metrics(held, exclude=train) == model.ranking_metrics(held, exclude=train, k=10)
    proba = model.predict_proba()
    aucs = [roc_auc_score(held[i][train[i] == 0], proba[i][train[i] == 0]) for i in range(12) if held[i].any()]
    assert abs(model.ranking_metrics(held, exclude=train)["auc"] - np.mean(aucs)) <= 1e-12
