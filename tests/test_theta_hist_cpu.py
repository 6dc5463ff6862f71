"""Class histograms of Theta on the device (nbmf_theta_hist, Context.theta_hist, NBMF.theta_histogram / roc_auc /
calibration_curve): what can be said without a GPU -- the symbol is declared and exported, a null context is an argument
error, every malformed request raises ValueError BEFORE any device call, ``_metrics`` against scikit-learn and against direct
NumPy computations on Theta -- and the reference ``host_theta_hist`` that tests/test_gpu_theta_hist.py compares the device
against for EQUALITY, checked here on hand-written cases (edges, theta = 1, NaN, a fully masked row).

The AUC inputs (``hist_case``) follow the recipe of tests/test_gpu_score_samples.py::case, with H = uniform(0, 1) ** 3 and
X ~ Bernoulli(Theta) so that Theta says something about X.  With seed 3000 + K that gives (measured by this file's own host
reference, B = 1024):   K = 5: slack 0.0009, binned and exact AUC 0.70;   K = 130: slack 0.005, AUC 0.55."""
import ctypes
import os

import numpy as np
import pytest


def host_theta_hist(theta, x, mask, bins):
    """The contract of nbmf_theta_hist in NumPy.  ``theta`` is what predict_rows returned with the clip on.  Observed = no
    mask or mask != 0; class = (x != 0); bin = min(int64(theta * bins), bins - 1) over the observed entries whose theta is
    not NaN, counted per class with ``np.bincount``; the NaN ones are counted per class in ``nan_count``.
    Returns ``(hist int64 (2, bins), nan_count int64 (2,))``."""
    theta = np.asarray(theta, dtype=np.float64)
    x = np.asarray(x)
    assert x.shape == theta.shape and (x.dtype == np.bool_ or x.dtype == np.uint8)
    obs = np.ones(theta.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    assert obs.shape == theta.shape
    nan = np.isnan(theta)
    hist = np.zeros((2, bins), dtype=np.int64)
    nan_count = np.zeros(2, dtype=np.int64)
    for c in (0, 1):
        cls = obs & ((x != 0) == bool(c))
        nan_count[c] = np.count_nonzero(cls & nan)
        b = np.minimum((theta[cls & ~nan] * bins).astype(np.int64), bins - 1)
        hist[c] = np.bincount(b, minlength=bins)
    return hist, nan_count


_cases = {}


def hist_case(k, m, n):
    """(W k x m with columns on the simplex, H k x n = uniform(0, 1) ** 3, X bool m x n ~ Bernoulli(W^T H), mask bool at
    about 70 % observed with row m // 3 and column n // 3 fully unobserved) of one shape, made once and shared (read-only)."""
    key = (k, m, n)
    if key not in _cases:
        r = np.random.default_rng(3000 + k)
        W = r.uniform(0.1, 0.9, (k, m))
        W /= W.sum(0)
        H = r.uniform(0.0, 1.0, (k, n)) ** 3
        X = r.random((m, n)) < np.clip(W.T @ H, 0.0, 1.0)
        mask = r.random((m, n)) < 0.7
        mask[m // 3] = False
        mask[:, n // 3] = False
        for a in (W, H, X, mask):
            a.setflags(write=False)
        _cases[key] = (W, H, X, mask)
    return _cases[key]


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_host_theta_hist_edges_the_last_bin_and_nan():
    theta = np.array([[0.0, 0.125, 0.25, 0.999, 1.0, np.nan],
                      [0.5, 0.5, 0.124, 0.126, np.nan, 1.0]])
    x = np.array([[0, 1, 0, 1, 1, 0], [7, 0, 0, 1, 1, 0]], dtype=np.uint8)   # nonzero, not just 1, is class 1
    hist, nan_count = host_theta_hist(theta, x, None, 8)
    assert hist.dtype == np.int64 and hist.shape == (2, 8) and nan_count.tolist() == [1, 1]
    assert hist[0].tolist() == [2, 0, 1, 0, 1, 0, 0, 1]    # 0.0 and 0.124 | 0.25 on its edge: the upper bin | 0.5 | 1.0: the last
    assert hist[1].tolist() == [0, 2, 0, 0, 1, 0, 0, 2]    # 0.125 on its edge and 0.126 | 0.5 | 0.999 and 1.0
    assert hist.sum() + nan_count.sum() == theta.size
    mask = np.array([[1, 1, 0, 0, 5, 1], [0, 0, 0, 0, 0, 0]], dtype=np.uint8)   # nonzero = observed; row 1 fully masked
    hist, nan_count = host_theta_hist(theta, x, mask, 8)
    assert hist[0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and hist[1].tolist() == [0, 1, 0, 0, 0, 0, 0, 1]
    assert nan_count.tolist() == [1, 0]
    one, _ = host_theta_hist(theta, x != 0, None, 1)        # a single bin: the class totals
    assert one.tolist() == [[5], [5]]
    # ... and what _metrics makes of the hand-written histograms is sklearn's AUC of the bin index over the non-NaN entries
    from sklearn.metrics import roc_auc_score
    from nbmf_mm_amd._metrics import auc_from_hist
    ok = ~np.isnan(theta)
    hist, _ = host_theta_hist(theta, x, None, 8)
    assert abs(auc_from_hist(hist)[0] - roc_auc_score(x[ok] != 0, np.minimum((theta[ok] * 8).astype(np.int64), 7))) <= 1e-15


# ---- the C entry point, as far as a host without a GPU reaches it ---------------------------------------------------------
def test_symbol_is_declared_and_exported():
    from nbmf_mm_amd import _hip
    assert "nbmf_theta_hist" in _hip.SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "nbmf_theta_hist")
    # tests/asan_null_calls.py builds its null call from the argtypes: only these kinds
    plain = {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64}
    assert len(lib.nbmf_theta_hist.argtypes) == 10 and set(lib.nbmf_theta_hist.argtypes) <= plain
    assert lib.nbmf_abi_version() == 4
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbmf_hip.h")).read()
    assert "int nbmf_theta_hist(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int bins," in header
    assert "#define NBMF_HIST_MAX_BINS 1024" in header and _hip.HIST_MAX_BINS == 1024


def test_null_context_is_an_argument_error():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    assert lib.nbmf_theta_hist(None, 0, 0, 0, None, 0, None, 0, None, None) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    x = np.zeros((2, 3), dtype=np.uint8)
    hist = np.full((2, 8), -7, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    assert lib.nbmf_theta_hist(None, 0, 2, 8, ptr(x), 3, None, 0, ptr(hist), None) == _hip.NBMF_ERR_ARG
    assert np.all(hist == -7)


# ---- Context.theta_hist: every argument error before any device call -------------------------------------------------------
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


def test_context_refuses_malformed_requests(bare_context):
    ctx, x = bare_context, np.zeros((12, 9), dtype=np.uint8)
    for row0, nrows in ((-1, 2), (12, 1), (11, 2), (0, -1), (0, 13)):
        with pytest.raises(ValueError, match="rows"):
            ctx.theta_hist(np.zeros((max(nrows, 0), 9), dtype=np.uint8), row0=row0, nrows=nrows)
    for bins in (0, 1025, -3, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="bins"):
            ctx.theta_hist(x, bins=bins)
    for shape in ((12, 8), (11, 9), (12 * 9,)):
        with pytest.raises(ValueError, match="x must have shape"):
            ctx.theta_hist(np.zeros(shape, dtype=np.uint8))
    with pytest.raises(ValueError, match="shape"):
        ctx.theta_hist(x, row0=2, nrows=4)                                   # the shape follows the request: (nrows, n)
    for dtype in (np.float64, np.float32, np.int64, np.int8):                # bytes only: there is no float64 form
        with pytest.raises(ValueError, match="x must be a bool or uint8"):
            ctx.theta_hist(np.zeros((12, 9), dtype=dtype))
    with pytest.raises(ValueError, match="stride"):
        ctx.theta_hist(np.zeros((12, 18), dtype=np.uint8)[:, ::2])
    with pytest.raises(ValueError, match="stride"):
        ctx.theta_hist(np.zeros((9, 12), dtype=bool).T)
    for shape in ((12, 8), (11, 9), (9,)):
        with pytest.raises(ValueError, match="mask must have shape"):
            ctx.theta_hist(x, mask=np.ones(shape, dtype=bool))
    for dtype in (np.float64, np.int64):
        with pytest.raises(ValueError, match="mask must be a bool or uint8"):
            ctx.theta_hist(x, mask=np.ones((12, 9), dtype=dtype))
    with pytest.raises(ValueError, match="mask must have unit stride"):
        ctx.theta_hist(x, mask=np.ones((9, 12), dtype=bool).T)


# ---- _metrics --------------------------------------------------------------------------------------------------------------
def theta_and_labels(k, m, n):
    """The observed Thetas (host product, clipped) and their labels of one ``hist_case``."""
    W, H, X, mask = hist_case(k, m, n)
    theta = np.clip(W.T @ H, 0.0, 1.0)
    return theta, theta[mask], X[mask]


@pytest.mark.parametrize("k,m,n", [(5, 37, 297), (130, 53, 297)])
def test_auc_from_hist_is_sklearns_auc_of_the_bin_index_and_within_its_slack_of_the_exact_one(k, m, n):
    from sklearn.metrics import roc_auc_score
    from nbmf_mm_amd._metrics import auc_from_hist
    W, H, X, mask = hist_case(k, m, n)
    theta, t, y = theta_and_labels(k, m, n)
    exact = roc_auc_score(y, t)
    for bins in (1024, 256, 10, 2):
        hist, nan_count = host_theta_hist(theta, X, mask, bins)
        assert not nan_count.any() and hist.sum() == mask.sum()
        auc, slack = auc_from_hist(hist)
        binned = roc_auc_score(y, np.minimum((t * bins).astype(np.int64), bins - 1))
        print(f"K = {k}, B = {bins}: slack {slack:.5f}, binned AUC {auc:.5f} (sklearn {binned:.5f}), exact AUC {exact:.5f}")
        assert abs(auc - binned) <= 1e-15
        assert abs(auc - exact) <= slack + 1e-15
        if bins == 1024:
            assert slack <= 0.01               # the host reference alone: 1024 bins resolve these Thetas
    if k == 5:
        assert exact >= 0.6                    # ... and the model ranks: the bound above is not vacuous


def test_auc_from_hist_all_ties_and_an_empty_class():
    from sklearn.metrics import roc_auc_score
    from nbmf_mm_amd._metrics import auc_from_hist
    theta, t, y = theta_and_labels(5, 37, 297)
    hist, _ = host_theta_hist(theta, *hist_case(5, 37, 297)[2:], 1)
    auc, slack = auc_from_hist(hist)
    assert auc == 0.5 and slack == 0.5                                        # B = 1: every pair is a tie
    assert abs(auc - roc_auc_score(y, np.zeros(y.size))) <= 1e-15
    for empty in (0, 1):
        h = np.array([[3, 1, 0, 2], [0, 5, 1, 1]], dtype=np.int64)
        h[empty] = 0
        assert all(np.isnan(v) for v in auc_from_hist(h))
    # a hand case: zeros in bins 0, 0, 1; ones in bins 1, 2 -> pairs: (0,1) (0,1) tie | (0,2) (0,2) (1,2) = 5.5 of 6
    auc, slack = auc_from_hist(np.array([[2, 1, 0], [0, 1, 1]]))
    assert auc == 5.5 / 6 and slack == 0.5 / 6
    # counts beyond 2^53 in the products: the integer sums stay exact
    big = np.array([[2 ** 40, 2 ** 40], [2 ** 40, 2 ** 40]], dtype=np.int64)
    assert auc_from_hist(big) == (0.5, 0.25)
    for bad in (np.zeros((3, 4), dtype=np.int64), np.zeros((2, 4)), np.array([[1, -1], [0, 2]])):
        with pytest.raises(ValueError, match="hist"):
            auc_from_hist(bad)


@pytest.mark.parametrize("n_bins,resolution", [(10, 100), (10, 1), (4, 256), (1, 8)])
def test_calibration_from_hist_against_numpy_on_theta(n_bins, resolution):
    from nbmf_mm_amd._metrics import calibration_from_hist
    W, H, X, mask = hist_case(5, 37, 297)
    theta, t, y = theta_and_labels(5, 37, 297)
    bins = n_bins * resolution
    hist, _ = host_theta_hist(theta, X, mask, bins)
    prob_true, prob_pred, counts = calibration_from_hist(hist, n_bins)
    # directly on Theta: the coarse bin of an entry is its fine bin // resolution (the definition)
    q = np.minimum((t * bins).astype(np.int64), bins - 1) // resolution
    want_counts = np.bincount(q, minlength=n_bins)
    want_ones = np.bincount(q, weights=y, minlength=n_bins)
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts) and counts.sum() == mask.sum()
    filled = want_counts > 0
    assert filled.any() and np.array_equal(np.isnan(prob_true), ~filled) and np.array_equal(np.isnan(prob_pred), ~filled)
    assert np.array_equal(prob_true[filled], want_ones[filled] / want_counts[filled])          # exact
    want_mean = np.bincount(q, weights=t, minlength=n_bins)[filled] / want_counts[filled]
    worst = float(np.max(np.abs(prob_pred[filled] - want_mean)) * 2 * bins)
    print(f"n_bins = {n_bins}, resolution = {resolution}: worst |prob_pred - mean Theta| = {worst:.3f} / (2 bins)")
    assert np.all(np.abs(prob_pred[filled] - want_mean) <= 1.0 / (2 * bins) + 1e-15)


def test_calibration_from_hist_refuses_a_resolution_that_does_not_divide():
    from nbmf_mm_amd._metrics import calibration_from_hist
    h = np.ones((2, 12), dtype=np.int64)
    for n_bins in (5, 7, 24, 0, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_bins"):
            calibration_from_hist(h, n_bins)
    prob_true, prob_pred, counts = calibration_from_hist(h, 3)
    assert counts.tolist() == [8, 8, 8] and prob_true.tolist() == [0.5] * 3
    assert np.allclose(prob_pred, [1 / 6, 3 / 6, 5 / 6], rtol=0, atol=1e-15)
    # an empty coarse bin is NaN, and a bin's mean follows its counts: 3 entries at centre 5/8, 1 at 7/8
    prob_true, prob_pred, counts = calibration_from_hist(np.array([[0, 0, 2, 1], [0, 0, 1, 0]]), 2)
    assert counts.tolist() == [0, 4] and np.isnan(prob_true[0]) and np.isnan(prob_pred[0])
    assert prob_true[1] == 0.25 and prob_pred[1] == (3 * 5 + 7) / 32


# ---- NBMF.theta_histogram / roc_auc / calibration_curve ---------------------------------------------------------------------
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


def test_not_fitted_is_transforms_error():
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError) as want:
        NBMF().transform(np.zeros((3, 4)))
    for call in (lambda: NBMF().theta_histogram(np.zeros((3, 4))), lambda: NBMF().roc_auc(np.zeros((3, 4))),
                 lambda: NBMF().calibration_curve(np.zeros((3, 4)))):
        with pytest.raises(ValueError) as got:
            call()
        assert str(got.value) == str(want.value)


def test_estimator_refuses_malformed_requests_before_any_device_call(hand_set):
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF
    model = hand_set
    X = np.zeros((12, 9))
    calls = (model.theta_histogram, model.roc_auc, model.calibration_curve)
    for bins in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="bins"):
            model.theta_histogram(X, bins=bins)
        with pytest.raises(ValueError, match="bins"):
            model.roc_auc(X, bins=bins)
    for n_bins, resolution in ((10, 103), (1025, 1), (2, 513), (33, 32)):
        with pytest.raises(ValueError, match="at most 1024|must be in"):
            model.calibration_curve(X, n_bins=n_bins, resolution=resolution)
    for n_bins, resolution in ((0, 10), (10, 0), (2.0, 10), (10, "4")):
        with pytest.raises(ValueError, match="n_bins|resolution"):
            model.calibration_curve(X, n_bins=n_bins, resolution=resolution)
    for call in calls:
        with pytest.raises(ValueError, match="components"):
            call(X[:4], W=np.full((4, 2), 0.5))
        for bad in (np.zeros((12, 8)), np.zeros((9, 12)), sp.csr_matrix((11, 9))):
            with pytest.raises(ValueError, match="shape"):
                call(bad)
        with pytest.raises(ValueError, match="shape"):
            call(X, W=np.full((4, 3), 1 / 3))                               # X follows W, not W_
        for bad in (np.ones((12, 8)), np.ones((9, 12)), np.ones(9), sp.csr_matrix((12, 8))):
            with pytest.raises(ValueError, match="mask has shape"):
                call(X, mask=bad)
        with pytest.raises(ValueError, match="dtype"):
            call(X, mask=np.full((12, 9), "a"))
        # NaN and values outside [0, 1]: the errors fit gives, in fit's order
        for poke in (np.nan, np.inf, 1.5, -0.25):
            bad = X.copy()
            bad[3, 4] = poke
            with pytest.raises(ValueError) as want:
                NBMF(n_components=3).fit(bad)
            with pytest.raises(ValueError) as got:
                call(bad)
            assert str(got.value) == str(want.value)
        # ... and inside [0, 1] but not a class
        bad = X.copy()
        bad[3, 4] = 0.5
        with pytest.raises(ValueError, match="X must be binary"):
            call(bad)
        with pytest.raises(ValueError, match="X must be binary"):
            call(np.full((12, 9), 2, dtype=np.uint8))
        with pytest.raises(ValueError, match="X must be binary"):
            call(sp.csr_matrix(0.5 * np.eye(12, 9)))


def test_well_formed_request_reaches_the_device_or_fails_loudly():
    """No CPU fallback: without a GPU the call is an error of the library, with one it answers."""
    from nbmf_mm_amd import NBMF, _hip
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    X = r.random((12, 9)) < 0.3
    if _hip.device_count() == 0:
        for call in (lambda: model.theta_histogram(X), lambda: model.roc_auc(X.astype(float), mask=X),
                     lambda: model.calibration_curve(X)):
            with pytest.raises(_hip.NBMFHipError, match="no HIP device"):
                call()
    else:
        hist, edges = model.theta_histogram(X, bins=8)
        assert hist.shape == (2, 8) and hist.sum() == X.size and hist[1].sum() == X.sum() and edges.tolist() == [b / 8 for b in range(9)]
