"""The best entries of Theta = W^T H over a whole row range as (row, column) pairs, selected on the device: nbmf_top_pairs,
Context.top_pairs, NBMF.top_pairs, NBMF.least_likely.

REFERENCE.  Always ``host_top_pairs`` (tests/test_top_pairs_cpu.py: np.lexsort over the eligible non-NaN entries by score,
then row, then column) over the device's own ``predict_rows`` slab with the same clip flag.  Rows, columns and count must be
equal and scores equal BIT FOR BIT: there is no tolerance anywhere in this file.  One test is independent of predict_rows:
dyadic factors, whose products and sums are exact in float64 in any order, against NumPy's ``W.T @ H``.

PATHS.  At these shapes every entry fits the candidate buffer's default slack (65 536), so the default call ends after one
digit pass; ``NBMF_PAIRS_SLACK=0`` takes the slack away, which sends the same request through every digit of the key, the
per-row tie count, the boundary row and the boundary column.  The tests that can tell the paths apart run under both
(``slack``), the last shape is large enough to refine under the default.

SHAPES.  The smallest at which each path can go wrong: 37 x 300 (rows off the 16-grid, columns off 4 / 64 / 256, two
workgroups of columns, three of rows), 40 x 1000 with thousands of ties, K = 1 / 16 / 64 and K = 130 (sliced factor layout)
at 520 x 8195."""
import numpy as np
import pytest

from test_top_pairs_cpu import host_top_pairs, merge_pairs, same_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


@pytest.fixture(params=["default", "0"])
def slack(request, monkeypatch):
    """The candidate buffer's slack: the default (the selection ends early) and none (every digit, then the tie pass)."""
    if request.param != "default":
        monkeypatch.setenv("NBMF_PAIRS_SLACK", request.param)
    return request.param


_cases = {}


def case(k, m, n, seed=0):
    """(W k x m with columns on the simplex, H k x n in (0.1, 0.9)) of one shape, made once and shared (read-only)."""
    key = (k, m, n, seed)
    if key not in _cases:
        r = np.random.default_rng(4000 + 97 * seed + k)
        W = r.uniform(0.1, 0.9, (k, m))
        W /= W.sum(0)
        H = r.uniform(0.1, 0.9, (k, n))
        W.setflags(write=False)
        H.setflags(write=False)
        _cases[key] = (W, H)
    return _cases[key]


def context(hip, W, H):
    ctx = hip.Context(W.shape[1], H.shape[1], W.shape[0])
    ctx.set_factors(np.ascontiguousarray(W), np.ascontiguousarray(H))
    return ctx


def well_formed(got, m, n, top, row0=0, nrows=None):
    rows, cols, scores = got
    nrows = m - row0 if nrows is None else nrows
    assert rows.ndim == cols.ndim == 1 and rows.size == cols.size <= top
    assert np.all((rows >= row0) & (rows < row0 + nrows)), "a row outside the request was returned"
    assert np.all((cols >= 0) & (cols < n)), "a pad column was returned"
    assert np.unique(rows * n + cols).size == rows.size, "an entry was returned twice"
    assert rows.base is None and cols.base is None, "a view of the staging was returned"
    if scores is not None:
        assert scores.shape == rows.shape and not np.any(np.isnan(scores))


# ---- 1. ragged shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [1, 7, 300, 5000, 11100, 11101, 50000])
def test_ragged_shape(hip, slack, top):
    W, H = case(5, 37, 300)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        got = ctx.top_pairs(top)
        well_formed(got, 37, 300, top)
        assert got[0].size == min(top, 37 * 300)                           # top > m n: count = m n
        same_pairs(got, host_top_pairs(theta, top))
        rows, cols, none = ctx.top_pairs(top, return_scores=False)
        assert none is None and np.array_equal(rows, got[0]) and np.array_equal(cols, got[1])


# ---- 2. row windows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row0,nrows", [(5, 20), (16, 16), (36, 1), (0, 0), (37, 0)])
def test_row_windows(hip, slack, row0, nrows):
    W, H = case(5, 37, 300)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows(row0, nrows)
        for top in (1, 290, 2000):
            got = ctx.top_pairs(top, row0=row0, nrows=nrows)
            well_formed(got, 37, 300, top, row0, nrows)
            same_pairs(got, host_top_pairs(theta, top, row0=row0))
            assert got[0].size == min(top, nrows * 300)


def test_a_range_is_the_merge_of_its_parts(hip, slack):
    W, H = case(5, 37, 300)
    r = np.random.default_rng(8)
    exclude = r.random((37, 300)) < 0.3
    with context(hip, W, H) as ctx:
        for top in (7, 3000):
            whole = ctx.top_pairs(top, x=exclude)
            a = ctx.top_pairs(top, x=exclude[:17], row0=0, nrows=17)
            b = ctx.top_pairs(top, x=exclude[17:], row0=17, nrows=20)
            same_pairs(merge_pairs(a, b, top), whole)


# ---- 3. exact products with heavy ties: independent of predict_rows ---------------------------------------------------------
@pytest.fixture(scope="module")
def dyadic():
    """Entries in {0, 1, 2, 3} / 16, K = 3: every product and every partial sum is a multiple of 1/256 below 1 -- exact in
    float64 in any order, with or without FMA -- so NumPy's W.T @ H is the truth, and it has thousands of ties."""
    r = np.random.default_rng(31)
    W = r.integers(0, 4, (3, 40)) / 16.0
    H = r.integers(0, 4, (3, 1000)) / 16.0
    truth = W.T @ H
    truth.setflags(write=False)
    # the smallest top that lands strictly inside the tie group of its threshold value AND strictly inside a row
    flat = np.sort(truth.ravel())[::-1]
    inside = None
    for top in range(2, flat.size - 1):
        T = flat[top - 1]
        if flat[top] != T or flat[top - 2] != T:
            continue                                                       # the threshold's group starts or ends here
        rows, cols, _ = host_top_pairs(truth, top)
        rs, cs = rows[-1], cols[-1]                                        # (ties come last in the list, in row-major order)
        row_ties = np.flatnonzero(truth[rs] == T)
        if row_ties[0] < cs < row_ties[-1]:
            inside = top
            break
    assert inside is not None
    return W, H, truth, inside


def test_dyadic_factors_against_numpy(hip, slack, dyadic):
    W, H, truth, inside = dyadic
    with context(hip, W, H) as ctx:
        assert np.array_equal(ctx.predict_rows(), truth)
        for top in (1, 7, 1000, inside, 25000):
            got = ctx.top_pairs(top)
            well_formed(got, 40, 1000, top)
            same_pairs(got, host_top_pairs(truth, top))
        for top in (1, 7, inside):                                         # smallest first: x = 0 everywhere, so 1 - theta
            got = ctx.top_pairs(top, kind="likelihood", x=np.zeros((40, 1000), dtype=np.uint8))
            same_pairs(got, host_top_pairs(1.0 - truth, top, largest=False))


# ---- 4. constant Theta ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [300, 600, 900, 450, 1, 11100])
def test_constant_theta_is_row_major_order(hip, slack, top):
    W = np.full((4, 37), 0.25)
    H = np.full((4, 300), 0.375)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        assert np.unique(theta).size == 1
        rows, cols, scores = ctx.top_pairs(top)
        assert np.array_equal(rows, np.arange(top) // 300) and np.array_equal(cols, np.arange(top) % 300)
        assert np.all(scores == theta[0, 0])


# ---- 5. adjacent doubles ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", [100, 37 * 150 + 9])
def test_adjacent_doubles_resolve_the_lowest_digit(hip, slack, top):
    """K = 1, W = 1: theta = H exactly, a shuffled chain of 300 consecutive doubles from 0.5 upward.  Every column ties
    across all 37 rows; neighbours differ in the last bit of the key."""
    chain = 0.5 + np.arange(300) * np.spacing(0.5)
    assert np.all(np.diff(chain.view(np.uint64)) == 1)
    H = np.random.default_rng(12).permutation(chain)[None, :]
    W = np.ones((1, 37))
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        assert np.array_equal(theta, np.broadcast_to(H, (37, 300)))
        same_pairs(ctx.top_pairs(top), host_top_pairs(theta, top))
        x = np.random.default_rng(13).random((37, 300)) < 0.5
        same_pairs(ctx.top_pairs(top, kind="likelihood", x=x),
                   host_top_pairs(np.where(x, theta, 1.0 - theta), top, largest=False))


# ---- 6. clip and NaN --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", [True, False])
def test_clip_and_raw_values(hip, slack, clip):
    """Columns of W that sum above 1 and negative entries: with the clip on, mass ties at exactly 1.0 and at +-0.0; with
    it off, the order of the raw values (negative ones included)."""
    r = np.random.default_rng(21)
    W = r.uniform(-0.6, 1.2, (5, 37))
    H = r.uniform(0.1, 0.9, (5, 300))
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows(clip_theta=clip)
        if clip:
            assert (theta == 1.0).sum() > 300 and (theta == 0.0).sum() > 300
        else:
            assert theta.min() < 0.0 and theta.max() > 1.0
        for top in (1, 50, 2000, 9000, 11100):
            got = ctx.top_pairs(top, clip_theta=clip)
            same_pairs(got, host_top_pairs(theta, top))
        x = r.random((37, 300)) < 0.5
        for top in (50, 9000):
            same_pairs(ctx.top_pairs(top, kind="likelihood", x=x, clip_theta=clip),
                       host_top_pairs(np.where(x, theta, 1.0 - theta), top, largest=False))


@pytest.mark.parametrize("n", [300, 200])
def test_zeros_tie_with_pad_columns_and_none_of_those_is_returned(hip, slack, n):
    W, H = case(5, 37, n)
    W = W.copy()
    W[:, 3] = 0.0                                                          # a zero row of Theta
    W[:, 20] = -W[:, 20]                                                   # and a row below it (clipped: -0.0 / 0.0 ties)
    with context(hip, W, H) as ctx:
        for clip in (True, False):
            theta = ctx.predict_rows(clip_theta=clip)
            for top in (36 * n - n + 5, 36 * n + 7, 37 * n, 37 * n + 100):
                got = ctx.top_pairs(top, clip_theta=clip)
                well_formed(got, 37, n, top)
                same_pairs(got, host_top_pairs(theta, top))


def test_nan_is_never_returned(hip, slack):
    W, H = case(5, 37, 300)
    W, H = W.copy(), H.copy()
    W[2, 11] = np.nan                                                      # a NaN row of Theta
    H[0, 77] = np.nan                                                      # a NaN column
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        assert np.isnan(theta).sum() == 300 + 37 - 1
        for top in (5, 11100):
            got = ctx.top_pairs(top)
            well_formed(got, 37, 300, top)
            same_pairs(got, host_top_pairs(theta, top))
        assert ctx.top_pairs(11100)[0].size == 36 * 299
        x = np.random.default_rng(3).random((37, 300)) < 0.3
        got = ctx.top_pairs(11100, kind="likelihood", x=x)
        assert got[0].size == 36 * 299
        same_pairs(got, host_top_pairs(np.where(x, theta, 1.0 - theta), 11100, largest=False))


def test_everything_excluded_or_unobserved_is_an_empty_result(hip, slack):
    W, H = case(5, 37, 300)
    with context(hip, W, H) as ctx:
        rows, cols, scores = ctx.top_pairs(10, x=np.ones((37, 300), dtype=bool))
        assert rows.size == cols.size == scores.size == 0
        rows, cols, scores = ctx.top_pairs(10, kind="likelihood", x=np.ones((37, 300), dtype=bool),
                                           mask=np.zeros((37, 300), dtype=np.uint8))
        assert rows.size == cols.size == scores.size == 0


# ---- 7. exclude -------------------------------------------------------------------------------------------------------------
def test_exclude_in_every_form(hip, slack):
    from nbmf_mm_amd import PackedBits
    W, H = case(5, 37, 300)
    r = np.random.default_rng(41)
    ex = r.integers(0, 3, (37, 300)).astype(np.uint8)                      # 0 / 1 / 2: nonzero means skip
    wide = np.zeros((37, 420), dtype=np.uint8)
    wide[:, 60:360] = ex
    wide[:, :60] = 1
    wide[:, 360:] = 1                                                      # what lies outside the view is never read
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        for top in (1, 40, 3000, 11100):
            want = host_top_pairs(theta, top, eligible=ex == 0)
            assert want[0].size == min(top, int((ex == 0).sum()))
            for form in (ex, ex != 0, PackedBits.from_dense(ex), wide[:, 60:360]):
                got = ctx.top_pairs(top, x=form)
                well_formed(got, 37, 300, top)
                same_pairs(got, want)
        sparse = r.random((37, 300)) < 0.1                                 # a 10 %-dense exclude
        same_pairs(ctx.top_pairs(500, x=sparse), host_top_pairs(theta, 500, eligible=~sparse))
        same_pairs(ctx.top_pairs(500, x=PackedBits.from_dense(sparse)), host_top_pairs(theta, 500, eligible=~sparse))
        same_pairs(ctx.top_pairs(300, x=sparse[5:25], row0=5, nrows=20),
                   host_top_pairs(theta[5:25], 300, eligible=~sparse[5:25], row0=5))


# ---- 8. the likelihood kind -------------------------------------------------------------------------------------------------
def test_likelihood_kind(hip, slack):
    from nbmf_mm_amd import PackedBits
    W, H = case(5, 37, 300)
    r = np.random.default_rng(51)
    X = r.random((37, 300)) < 0.3
    mask = r.random((37, 300)) < 0.9
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        prob = np.where(X, theta, 1.0 - theta)
        for top in (1, 60, 4000, 11100):
            want = host_top_pairs(prob, top, largest=False)
            for x in (X, X.view(np.uint8), PackedBits.from_dense(X)):
                same_pairs(ctx.top_pairs(top, kind="likelihood", x=x), want)
            want = host_top_pairs(prob, top, eligible=mask, largest=False)
            assert want[0].size == min(top, int(mask.sum()))
            assert np.all(np.diff(want[2]) >= 0)                           # smallest first
            for x in (X, PackedBits.from_dense(X)):
                for mk in (mask, mask.view(np.uint8) * 3, PackedBits.from_dense(mask)):
                    got = ctx.top_pairs(top, kind="likelihood", x=x, mask=mk)
                    well_formed(got, 37, 300, top)
                    assert np.all(mask[got[0], got[1]]), "an unobserved entry was returned"
                    same_pairs(got, want)
        got = ctx.top_pairs(200, kind="likelihood", x=X[16:32], mask=mask[16:32], row0=16, nrows=16)
        same_pairs(got, host_top_pairs(prob[16:32], 200, eligible=mask[16:32], largest=False, row0=16))


# ---- 9. factor layouts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16, 64])
def test_factor_layouts(hip, slack, k):
    W, H = case(k, 37, 300)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        for top in (7, 2500):
            same_pairs(ctx.top_pairs(top), host_top_pairs(theta, top))


def test_sliced_layout_at_a_size_that_refines(hip):
    """K = 130 at 520 x 8195, top = 100 000: 4.26 million entries against a buffer of 165 536, so the default call goes
    through several digit passes before it collects."""
    W, H = case(130, 520, 8195)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        got = ctx.top_pairs(100000)
        well_formed(got, 520, 8195, 100000)
        flat = theta.ravel()
        keep = np.argpartition(-flat, 100000 + 64)[:100000 + 64]           # (no ties here: a margin of 64 holds every one)
        sub = np.full(flat.size, np.nan)
        sub[keep] = flat[keep]
        same_pairs(got, host_top_pairs(sub.reshape(theta.shape), 100000))


# ---- 10. blocking and repeatability -----------------------------------------------------------------------------------------
def test_same_call_twice_and_one_copy_of_the_counters(hip, slack, monkeypatch):
    W, H = case(5, 37, 300)
    r = np.random.default_rng(61)
    X = r.random((37, 300)) < 0.3
    with context(hip, W, H) as ctx:
        first = ctx.top_pairs(4000, x=X)
        same_pairs(ctx.top_pairs(4000, x=X), first)
        second = ctx.top_pairs(4000, kind="likelihood", x=X)
        monkeypatch.setenv("NBMF_HIST_COPIES", "1")
        same_pairs(ctx.top_pairs(4000, x=X), first)
        same_pairs(ctx.top_pairs(4000, kind="likelihood", x=X), second)


def test_library_refuses_what_the_header_says(hip):
    import ctypes
    W, H = case(5, 37, 300)
    lib = hip.load()
    rows, cols = np.full(4, 7, dtype=np.int64), np.full(4, 7, dtype=np.int64)
    count = ctypes.c_int64(7)
    ptr = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    cnt = ctypes.cast(ctypes.byref(count), ctypes.c_void_p)
    ex = np.zeros((37, 300), dtype=np.uint8)
    with context(hip, W, H) as ctx:
        def call(row0=0, nrows=37, top=4, kind=0, x=None, xk=hip.DATA_U8, ldx=300, mask=None, mk=hip.MASK_NONE, ldm=300,
                 r=rows, c=cols, n=cnt):
            return lib.nbmf_top_pairs(ctx._h, row0, nrows, top, 1, kind, ptr(x), xk, ldx, ptr(mask), mk, ldm, ptr(r), ptr(c), None, n)
        for bad in (dict(top=0), dict(top=(1 << 22) + 1), dict(row0=30, nrows=8), dict(row0=-1), dict(kind=2),
                    dict(x=ex, ldx=299), dict(x=ex, xk=hip.DATA_BITS, ldx=37), dict(x=ex, xk=hip.DATA_F64),
                    dict(mask=ex, mk=hip.MASK_U8), dict(kind=1), dict(kind=1, x=ex, mask=ex, mk=hip.MASK_U8, ldm=10),
                    dict(kind=1, x=ex, mk=hip.MASK_U8), dict(r=None), dict(c=None), dict(n=None)):
            assert call(**bad) == hip.NBMF_ERR_ARG, bad
            assert count.value == 7 and np.all(rows == 7) and np.all(cols == 7), bad
        assert call(nrows=0, kind=1) == 0 and count.value == 0 and np.all(rows == 7)   # nrows == 0 reads nothing
        assert call() == 0 and count.value == 4


# ---- 11. the estimator ------------------------------------------------------------------------------------------------------
def planted_flips(seed=7, m=60, n=90, flips=20):
    """Block-structured binary data with ``flips`` entries flipped against their block: ``(X, flipped bool)``."""
    r = np.random.default_rng(seed)
    theta = np.where((np.arange(m)[:, None] // 20) == (np.arange(n)[None, :] // 30), 0.95, 0.03)
    clean = r.random((m, n)) < theta
    flat = r.choice(m * n, flips, replace=False)
    flipped = np.zeros(m * n, dtype=bool)
    flipped[flat] = True
    flipped = flipped.reshape(m, n)
    return clean ^ flipped, flipped


@pytest.fixture(scope="module")
def fitted(hip):
    from nbmf_mm_amd import NBMF
    X, flipped = planted_flips()
    model = NBMF(n_components=3, random_state=0, max_iter=300, tol=0).fit(X.astype(np.float64))
    return model, X, flipped


def test_estimator_top_pairs(hip, fitted):
    import scipy.sparse as sp
    from nbmf_mm_amd import PackedBits
    model, X, _ = fitted
    rows, cols, scores = model.top_pairs(200, exclude=X)
    assert rows.size == 200 and not np.any(X[rows, cols]), "an entry of X was returned"
    assert np.all(np.diff(scores) <= 0)
    with context(hip, model.W_.T, model.components_) as ctx:
        same_pairs((rows, cols, scores), ctx.top_pairs(200, x=X))
        same_pairs(model.top_pairs(50), ctx.top_pairs(50))
    for form in (sp.csr_matrix(X.astype(np.float64)), sp.coo_matrix(X.astype(np.int8)), X.astype(np.float64),
                 PackedBits.from_dense(X)):
        same_pairs(model.top_pairs(200, exclude=form), (rows, cols, scores))
    theta = model.predict_proba()
    same_pairs((rows, cols, scores), host_top_pairs(theta, 200, eligible=~X))
    W_new = model.W_[10:25]
    same_pairs(model.top_pairs(30, W=W_new, exclude=X[10:25]), host_top_pairs(model.predict_proba(W=W_new), 30, eligible=~X[10:25]))


def test_estimator_least_likely(hip, fitted):
    """A weak sanity check of the use, not of the kernels: on block data with 20 planted flips, at least one flip is among
    the 20 least likely entries and every flip ranks above the median unflipped entry (checked on the CPU with the oracle's
    fit of the same data and ``host_top_pairs`` before this seed was chosen: 2 flips in the first 20)."""
    import scipy.sparse as sp
    model, X, flipped = fitted
    rows, cols, prob = model.least_likely(X, n=20)
    assert np.all(np.diff(prob) >= 0)
    assert flipped[rows, cols].sum() >= 1
    theta = model.predict_proba()
    same_pairs((rows, cols, prob), host_top_pairs(np.where(X, theta, 1.0 - theta), 20, largest=False))
    same_pairs(model.least_likely(sp.csr_matrix(X.astype(np.float64)), n=20), (rows, cols, prob))
    rows, cols, _ = model.least_likely(X, n=X.size)
    assert rows.size == X.size
    position = np.empty(X.shape, dtype=np.int64)
    position[rows, cols] = np.arange(X.size)
    assert np.all(position[flipped] < np.median(position[~flipped]))
    mask = np.random.default_rng(2).random(X.shape) < 0.9
    rows, cols, prob = model.least_likely(X, mask=mask, n=40)
    assert np.all(mask[rows, cols])
    same_pairs((rows, cols, prob), host_top_pairs(np.where(X, theta, 1.0 - theta), 40, eligible=mask, largest=False))
