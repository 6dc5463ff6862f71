"""Per-row and per-feature log-likelihood on the device (nbmf_score_rows, Context.score_rows, NBMF.score_samples): what can
be said without a GPU -- the symbol is declared and exported, a null context is an argument error, every malformed request
raises ValueError BEFORE any device call -- and the reference ``host_score_rows`` that tests/test_gpu_score_samples.py
compares the device against, checked here on hand-written cases (a fully masked row, theta on both clips, real-valued x)."""
import ctypes
import math
import os

import numpy as np
import pytest


def host_score_rows(theta, x, mask=None, eps=1e-8):
    """The semantics of nbmf_score_rows in NumPy.  ``theta`` is what predict_rows returned (already clipped or not).
    Byte data (bool / uint8, nonzero means 1): ``t = log(where(x, theta + eps, (1 - theta) + eps))``; float64 data:
    ``t = x log(theta + eps) + (1 - x) log((1 - theta) + eps)``.  Observed = no mask or mask != 0.  Sums are ``math.fsum``
    over the observed entries of a row / a column (exactly rounded: the reference's own summation error is nil).
    Returns ``(row_ll, row_obs, row_abs, col_ll, col_obs, col_abs)``: sums, int64 counts and the sums of \\|t\\|."""
    theta = np.asarray(theta, dtype=np.float64)
    x = np.asarray(x)
    assert x.shape == theta.shape
    obs = np.ones(theta.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    assert obs.shape == theta.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        if x.dtype == np.bool_ or x.dtype == np.uint8:
            t = np.log(np.where(x != 0, theta + eps, (1.0 - theta) + eps))
        else:
            x = np.asarray(x, dtype=np.float64)
            t = x * np.log(theta + eps) + (1.0 - x) * np.log((1.0 - theta) + eps)
    m, n = theta.shape
    row_ll = np.array([math.fsum(t[i, obs[i]]) for i in range(m)], dtype=np.float64)
    col_ll = np.array([math.fsum(t[obs[:, j], j]) for j in range(n)], dtype=np.float64)
    a = np.abs(t)
    row_abs = np.array([math.fsum(a[i, obs[i]]) for i in range(m)], dtype=np.float64)
    col_abs = np.array([math.fsum(a[obs[:, j], j]) for j in range(n)], dtype=np.float64)
    return row_ll, obs.sum(1).astype(np.int64), row_abs, col_ll, obs.sum(0).astype(np.int64), col_abs


def assert_sums_within_bound(got_ll, got_obs, want_ll, want_obs, want_abs):
    """Counts exactly; sums to \\|got - want\\| <= (c + 8) 2^-52 sum\\|t\\|, c the number of observed terms: both logarithms
    within 1 ulp of the same argument and at most two roundings to form a term (8 2^-52 \\|t\\| in all, generously), and at
    most c - 1 roundings of 2^-53 sum\\|t\\| for any summation order.  NaN sums must be NaN on both sides."""
    assert got_ll.dtype == np.float64 and got_obs.dtype == np.int64
    assert got_ll.shape == want_ll.shape and got_obs.shape == want_obs.shape
    assert np.array_equal(got_obs, want_obs)
    nan = np.isnan(want_ll)
    assert np.array_equal(np.isnan(got_ll), nan)
    inf = np.isinf(want_ll)
    assert np.array_equal(got_ll[inf], want_ll[inf])
    ok = ~nan & ~inf
    err = np.abs(got_ll[ok] - want_ll[ok])
    bound = (want_obs[ok] + 8) * 2.0 ** -52 * want_abs[ok]
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))
    print(f"worst error / bound = {worst:.3f} over {int(ok.sum())} sums")
    assert np.all(err <= bound), f"worst error / bound = {worst}"


# ---- the reference itself -------------------------------------------------------------------------------------------------
def near(got, want, ulps=4):
    """Equal to a few ulps: NumPy's array logarithm and math.log may round differently (both are within 1 ulp)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= ulps * 2.0 ** -52 * np.abs(want)))


def test_host_score_rows_bytes_mask_and_a_fully_masked_row():
    eps = 1e-8
    theta = np.array([[0.25, 0.5, 0.75],
                      [0.1, 0.2, 0.3],
                      [0.9, 0.8, 0.7]])
    x = np.array([[1, 0, 1], [0, 0, 7], [1, 1, 0]], dtype=np.uint8)          # nonzero, not just 1, means x = 1
    mask = np.array([[1, 1, 0], [0, 0, 0], [5, 0, 1]], dtype=np.uint8)       # nonzero, not just 1, means observed
    row_ll, row_obs, row_abs, col_ll, col_obs, col_abs = host_score_rows(theta, x, mask, eps)
    assert row_obs.tolist() == [2, 0, 2] and col_obs.tolist() == [2, 1, 1]
    assert row_ll[1] == 0.0 and row_abs[1] == 0.0                             # a fully masked row: sum 0.0, count 0
    assert near(row_ll[0], math.fsum([math.log(0.25 + eps), math.log((1 - 0.5) + eps)]))
    assert near(row_ll[2], math.fsum([math.log(0.9 + eps), math.log((1 - 0.7) + eps)]))
    assert near(col_ll[0], math.fsum([math.log(0.25 + eps), math.log(0.9 + eps)]))
    assert near(col_ll[1], math.log((1 - 0.5) + eps)) and near(col_ll[2], math.log((1 - 0.7) + eps))
    assert np.array_equal(row_abs, -row_ll) and np.array_equal(col_abs, -col_ll)   # every term is negative here
    # no mask: every entry, and bool data is the same as bytes
    full = host_score_rows(theta, x != 0, None, eps)
    assert full[1].tolist() == [3, 3, 3] and full[4].tolist() == [3, 3, 3]
    assert near(full[0][1], math.fsum([math.log((1 - 0.1) + eps), math.log((1 - 0.2) + eps), math.log(0.3 + eps)]))
    same = host_score_rows(theta, x, np.ones((3, 3)), eps)
    assert all(near(a, b) for a, b in zip(full, same))


def test_host_score_rows_on_both_clips():
    eps = 1e-8
    theta = np.clip(np.array([[-0.5, 1.5, 0.0, 1.0]]), 0.0, 1.0)             # theta = 0 and theta = 1 after the clip
    ones = host_score_rows(theta, np.ones((1, 4), dtype=np.uint8), None, eps)
    zeros = host_score_rows(theta, np.zeros((1, 4), dtype=np.uint8), None, eps)
    lo, hi = math.log(eps), math.log(1.0 + eps)
    assert near(ones[3], [lo, hi, lo, hi])                                   # x = 1: log(theta + eps)
    assert near(zeros[3], [hi, lo, hi, lo])                                  # x = 0: log((1 - theta) + eps)
    assert hi > 0.0 and near(ones[5], [-lo, hi, -lo, hi])                    # the sums of |t|
    assert near(ones[0][0], math.fsum([lo, hi, lo, hi]))
    # without the clip a theta beyond 1 + eps has no likelihood where x = 0
    raw = host_score_rows(np.array([[1.5, 0.5]]), np.zeros((1, 2), dtype=np.uint8), None, eps)
    assert np.isnan(raw[0][0]) and np.isnan(raw[3][0]) and near(raw[3][1], math.log(0.5 + eps))


def test_host_score_rows_real_valued_x():
    eps = 1e-8
    theta = np.array([[0.25, 0.5], [0.75, 0.125]])
    x = np.array([[0.5, 0.25], [1.0, 0.0]])
    row_ll, row_obs, row_abs, col_ll, col_obs, col_abs = host_score_rows(theta, x, None, eps)
    t = [[0.5 * math.log(0.25 + eps) + 0.5 * math.log(0.75 + eps), 0.25 * math.log(0.5 + eps) + 0.75 * math.log(0.5 + eps)],
         [math.log(0.75 + eps), math.log(0.875 + eps)]]
    assert near(row_ll, [math.fsum(t[0]), math.fsum(t[1])])
    assert near(col_ll, [math.fsum([t[0][0], t[1][0]]), math.fsum([t[0][1], t[1][1]])])
    assert row_obs.tolist() == [2, 2] and col_obs.tolist() == [2, 2]
    # exactly binary float64 data and the same data as bytes: the same terms (x * la + 0 * lb = la)
    xb = np.array([[1, 0], [0, 1]], dtype=np.uint8)
    a, b = host_score_rows(theta, xb.astype(np.float64), None, eps), host_score_rows(theta, xb, None, eps)
    assert all(near(p, q) for p, q in zip(a, b))


def test_the_bound_is_what_the_docstring_says():
    want_ll, want_obs, want_abs = np.array([-10.0, 0.0]), np.array([3, 0], dtype=np.int64), np.array([10.0, 0.0])
    edge = 11 * 2.0 ** -52 * 10.0
    assert_sums_within_bound(np.array([-10.0 + 0.9 * edge, 0.0]), want_obs, want_ll, want_obs, want_abs)
    with pytest.raises(AssertionError):
        assert_sums_within_bound(np.array([-10.0 + 1.2 * edge, 0.0]), want_obs, want_ll, want_obs, want_abs)
    with pytest.raises(AssertionError):
        assert_sums_within_bound(np.array([-10.0, 1e-300]), want_obs, want_ll, want_obs, want_abs)   # an empty sum is exact
    with pytest.raises(AssertionError):
        assert_sums_within_bound(want_ll, np.array([3, 1], dtype=np.int64), want_ll, want_obs, want_abs)


# ---- the C entry point, as far as a host without a GPU reaches it ---------------------------------------------------------
def test_symbol_is_declared_and_exported():
    from nbmf_mm_amd import _hip
    assert "nbmf_score_rows" in _hip.SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "nbmf_score_rows")
    # tests/asan_null_calls.py builds its null call from the argtypes: only these kinds
    plain = {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}
    assert len(lib.nbmf_score_rows.argtypes) == 14 and set(lib.nbmf_score_rows.argtypes) <= plain
    assert lib.nbmf_abi_version() == 4
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbmf_hip.h")).read()
    assert "int nbmf_score_rows(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int clip_theta, double eps," in header
    assert "nbmf_loglik_strict" in header.split("int nbmf_top_n(")[1].split("int nbmf_score_rows(")[0]   # says whose summand it is


def test_null_context_is_an_argument_error():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    assert lib.nbmf_score_rows(None, 0, 0, 0, 0.0, None, 0, 0, None, 0, None, None, None, None) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    x = np.zeros((2, 3), dtype=np.uint8)
    out = np.full(2, -7.25)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    assert lib.nbmf_score_rows(None, 0, 2, 1, 1e-8, ptr(x), _hip.DATA_U8, 3, None, 0, ptr(out), None, None, None) == _hip.NBMF_ERR_ARG
    assert np.all(out == -7.25)


# ---- Context.score_rows: every argument error before any device call ------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called for a request that is malformed")


@pytest.fixture
def bare_context():
    """A Context of a 12 x 9 problem that has no library behind it: touching the device is an error of the test."""
    from nbmf_mm_amd import _hip
    ctx = object.__new__(_hip.Context)
    ctx._lib, ctx._h = _NoDevice(), None
    ctx.m, ctx.n, ctx.k = 12, 9, 3
    return ctx


@pytest.mark.parametrize("row0,nrows", [(-1, 2), (12, 1), (11, 2), (0, -1), (0, 13)])
def test_context_refuses_rows_outside_the_matrix(bare_context, row0, nrows):
    with pytest.raises(ValueError, match="rows"):
        bare_context.score_rows(np.zeros((max(nrows, 0), 9), dtype=np.uint8), row0=row0, nrows=nrows)


def test_context_refuses_a_bad_x(bare_context):
    ctx = bare_context
    for shape in ((12, 8), (11, 9), (12 * 9,)):
        with pytest.raises(ValueError, match="shape"):
            ctx.score_rows(np.zeros(shape, dtype=np.uint8))
    with pytest.raises(ValueError, match="shape"):
        ctx.score_rows(np.zeros((12, 9)), row0=2, nrows=4)                  # the shape follows the request: (nrows, n)
    for dtype in (np.float32, np.int64, np.int8, np.float16):
        with pytest.raises(ValueError, match="dtype"):
            ctx.score_rows(np.zeros((12, 9), dtype=dtype))
    for dtype in (np.uint8, np.float64):
        with pytest.raises(ValueError, match="stride"):
            ctx.score_rows(np.zeros((12, 18), dtype=dtype)[:, ::2])          # not unit stride along a row
        with pytest.raises(ValueError, match="stride"):
            ctx.score_rows(np.zeros((9, 12), dtype=dtype).T)                 # column-major
        with pytest.raises(ValueError, match="stride"):
            ctx.score_rows(np.zeros((12, 9), dtype=dtype)[::-1])             # rows run backwards
        with pytest.raises(ValueError, match="stride"):
            ctx.score_rows(np.broadcast_to(np.zeros(9, dtype=dtype), (12, 9)))


def test_context_refuses_a_bad_mask(bare_context):
    ctx, x = bare_context, np.zeros((12, 9), dtype=np.uint8)
    for shape in ((12, 8), (11, 9), (9,)):
        with pytest.raises(ValueError, match="mask must have shape"):
            ctx.score_rows(x, mask=np.ones(shape, dtype=bool))
    for dtype in (np.float64, np.int64, np.float32):
        with pytest.raises(ValueError, match="mask must be a bool or uint8"):
            ctx.score_rows(x, mask=np.ones((12, 9), dtype=dtype))
    with pytest.raises(ValueError, match="mask must have unit stride"):
        ctx.score_rows(x, mask=np.ones((9, 12), dtype=bool).T)


def test_context_refuses_a_bad_eps_and_an_empty_request(bare_context):
    ctx, x = bare_context, np.zeros((12, 9), dtype=np.uint8)
    for eps in (float("nan"), -1e-8, -np.inf):
        with pytest.raises(ValueError, match="eps"):
            ctx.score_rows(x, eps=eps)
    with pytest.raises(ValueError, match="nothing requested"):
        ctx.score_rows(x, rows=False, cols=False)


def test_row_array_passes_a_wider_array_through():
    from nbmf_mm_amd import _hip
    score_panel = lambda a, nrows, n: _hip.row_array(a, nrows, n, "x", _hip.ANY_KINDS)   # noqa: E731
    wide = np.zeros((12, 20), dtype=bool)
    view, kind, ld = score_panel(wide[:, 3:12], 12, 9)
    assert (kind, ld) == (_hip.DATA_U8, 20) and view.dtype == np.uint8 and np.shares_memory(view, wide)
    widef = np.zeros((12, 20))
    view, kind, ld = score_panel(widef[:, 3:12], 12, 9)
    assert (kind, ld) == (_hip.DATA_F64, 20) and np.shares_memory(view, widef)
    assert score_panel(np.ones((12, 9), dtype=np.uint8), 12, 9)[1:] == (_hip.DATA_U8, 9)
    assert score_panel(widef[4:5, :9], 1, 9)[2] == 9                         # one row: its stride does not matter
    assert score_panel(np.zeros((0, 9)), 0, 9)[2] == 9


def test_row_array_checks_the_out_of_predict_rows(bare_context):
    """The float64 ``out`` of ``predict_rows`` goes through the same rule: a 12 x 9 slice of a 12 x 16 array, one row and
    zero rows are passed through with the right leading dimension, nothing copied; a column-major array is refused."""
    from nbmf_mm_amd import _hip
    out_array = lambda a, nrows: _hip.row_array(a, nrows, 9, "out", (np.float64,))   # noqa: E731
    wide = np.zeros((12, 16))
    view, kind, ld = out_array(wide[:, :9], 12)
    assert (kind, ld) == (_hip.DATA_F64, 16) and view.dtype == np.float64 and np.shares_memory(view, wide)
    view, kind, ld = out_array(wide[4:5, :9], 1)                             # one row: its stride does not matter
    assert (kind, ld) == (_hip.DATA_F64, 9) and np.shares_memory(view, wide)
    assert out_array(wide[3:3, :9], 0)[1:] == (_hip.DATA_F64, 9)
    with pytest.raises(ValueError, match="out must have unit stride"):
        out_array(np.asfortranarray(np.zeros((12, 9))), 12)
    with pytest.raises(ValueError, match="out must be a float64 array"):
        out_array(np.zeros((12, 9), dtype=np.uint8), 12)
    with pytest.raises(ValueError, match="out must have shape"):
        out_array(wide[:, :8], 12)
    # ... and predict_rows refuses before it touches the device: a malformed out, a list (it could not be written in
    # place), rows outside the matrix (the text the library itself gives)
    ctx = bare_context
    with pytest.raises(ValueError, match="stride"):
        ctx.predict_rows(out=np.asfortranarray(np.zeros((12, 9))))
    with pytest.raises(ValueError, match="out must be a bool or uint8 array"):
        ctx.predict_rows(threshold=0.5, out=np.zeros((12, 9)))
    with pytest.raises(ValueError, match="out must be a NumPy array"):
        ctx.predict_rows(out=[[0.0] * 9] * 12)
    with pytest.raises(ValueError, match=r"rows \[11, 11 \+ 2\) are not inside \[0, 12\)"):
        ctx.predict_rows(11, 2)


# ---- _solver: how a row block reaches the device ----------------------------------------------------------------------------
def test_row_block_picks_the_narrowest_exact_form():
    import scipy.sparse as sp
    from nbmf_mm_amd import _solver
    r = np.random.default_rng(3)
    xb = (r.random((40, 7)) < 0.4).astype(np.float64)
    got = _solver._row_block(xb, 16, 16, False)
    assert got.dtype == np.uint8 and np.array_equal(got, xb[16:32])
    xr = xb.copy()
    xr[20, 3] = 0.5
    assert _solver._row_block(xr, 16, 16, False).dtype == np.float64 and _solver._row_block(xr, 0, 16, False).dtype == np.uint8
    u8 = xb.astype(np.uint8)
    assert np.shares_memory(_solver._row_block(u8, 16, 16, False), u8)                      # bytes: passed as they are
    got = _solver._row_block(sp.csr_matrix(xr), 16, 24, False)
    assert got.dtype == np.float64 and np.array_equal(got, xr[16:40])
    mk = _solver._row_block(sp.csr_matrix(3.0 * xb), 32, 8, True)
    assert mk.dtype == np.bool_ and np.array_equal(mk, xb[32:40] != 0)
    assert np.array_equal(_solver._row_block(2.5 * xb, 0, 40, True), xb != 0)               # any numeric mask: nonzero = observed
    t = _solver._row_block(np.asfortranarray(u8), 0, 40, False)
    assert t.flags.c_contiguous and np.array_equal(t, u8)


# ---- NBMF.score_samples -------------------------------------------------------------------------------------------------------
def test_not_fitted_is_transforms_error():
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError) as want:
        NBMF().transform(np.zeros((3, 4)))
    with pytest.raises(ValueError) as got:
        NBMF().score_samples(np.zeros((3, 4)))
    assert str(got.value) == str(want.value)


@pytest.fixture
def hand_set(monkeypatch):
    """An estimator with hand-set factors (12 x 9, k = 3), in a process where creating a context is an error of the test."""
    from nbmf_mm_amd import NBMF, _hip
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))

    def no_device_call(*a, **k):
        raise AssertionError("a context was created for a request that is malformed")
    monkeypatch.setattr(_hip, "Context", no_device_call)
    return model


def test_estimator_refuses_malformed_requests_before_any_device_call(hand_set):
    import scipy.sparse as sp
    model = hand_set
    X = np.zeros((12, 9))
    for axis in (2, -1, "0", None, 0.5, True):
        with pytest.raises(ValueError, match="axis"):
            model.score_samples(X, axis=axis)
    with pytest.raises(ValueError, match="components"):
        model.score_samples(X[:4], W=np.full((4, 2), 0.5))
    for bad in (np.zeros((12, 8)), np.zeros((9, 12)), sp.csr_matrix((11, 9))):
        with pytest.raises(ValueError, match="shape"):
            model.score_samples(bad)
    with pytest.raises(ValueError, match="shape"):
        model.score_samples(X, W=np.full((4, 3), 1 / 3))                    # X follows W, not W_
    for bad in (np.ones((12, 8)), np.ones((9, 12)), np.ones(9), sp.csr_matrix((12, 8))):
        with pytest.raises(ValueError, match="mask has shape"):
            model.score_samples(X, mask=bad)
    with pytest.raises(ValueError, match="dtype"):
        model.score_samples(X, mask=np.full((12, 9), "a"))
    # NaN and values outside [0, 1]: the errors fit gives
    from nbmf_mm_amd import NBMF
    for poke in (np.nan, np.inf, 1.5, -0.25):
        bad = X.copy()
        bad[3, 4] = poke
        with pytest.raises(ValueError) as want:
            NBMF(n_components=3).fit(bad)
        with pytest.raises(ValueError) as got:
            model.score_samples(bad)
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError, match="X must be binary"):
        model.score_samples(np.full((12, 9), 2, dtype=np.uint8))
    with pytest.raises(ValueError, match="X must be binary"):
        model.score_samples(sp.csr_matrix(1.5 * np.eye(12, 9)))


def test_well_formed_request_reaches_the_device_or_fails_loudly():
    """No CPU fallback: without a GPU the call is an error of the library, with one it answers."""
    from nbmf_mm_amd import NBMF, _hip
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    X = r.random((12, 9)) < 0.3
    if _hip.device_count() == 0:
        for call in (lambda: model.score_samples(X), lambda: model.score_samples(X.astype(float), mask=X, axis=1)):
            with pytest.raises(_hip.NBMFHipError, match="no HIP device"):
                call()
    else:
        scores, counts = model.score_samples(X, return_counts=True)
        assert scores.shape == (12,) and np.all(counts == 9) and np.all(scores < 0)
