"""Top-N ranking on the device (nbmf_top_n, Context.top_n, NBMF.top_n): everything that can be said without a GPU -- the
symbol is declared and exported, a null context is an argument error, every malformed request raises ValueError BEFORE
any device call -- and the reference ranking ``host_top_n`` that tests/test_gpu_top_n.py compares the device against,
checked here on hand-written cases (ties, NaN, short rows, exclude)."""
import ctypes
import os

import numpy as np
import pytest


def host_top_n(theta, top, exclude=None):
    """The reference ranking: for every row of ``theta`` the ``top`` eligible columns (not NaN, ``exclude`` zero or
    absent) by theta descending, ties by ascending column -- ``np.lexsort((cols, -theta))`` -- and their thetas; rows with
    fewer eligible columns end in -1 / NaN.  Returns ``(cols int64, scores float64)``, both ``(rows, top)``."""
    theta = np.asarray(theta, dtype=np.float64)
    m, n = theta.shape
    if exclude is not None:
        exclude = np.asarray(exclude)
        assert exclude.shape == (m, n)
    cols = np.full((m, top), -1, dtype=np.int64)
    scores = np.full((m, top), np.nan)
    for i in range(m):
        ok = ~np.isnan(theta[i])
        if exclude is not None:
            ok &= exclude[i] == 0
        j = np.nonzero(ok)[0]
        order = j[np.lexsort((j, -theta[i, j]))][:top]
        cols[i, :order.size] = order
        scores[i, :order.size] = theta[i, order]
    return cols, scores


def same_ranking(got, want):
    """Columns equal, scores equal bit for bit, NaN padding compared by isnan: no tolerance."""
    (gc, gs), (wc, ws) = got, want
    assert gc.dtype == np.int64 and gs.dtype == np.float64 and gc.shape == wc.shape and gs.shape == ws.shape
    assert np.array_equal(gc, wc)
    pad = wc < 0
    assert np.all(np.isnan(gs[pad])) and np.all(np.isnan(ws[pad]))
    assert np.array_equal(gs[~pad].view(np.uint64), ws[~pad].view(np.uint64))


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_host_top_n_orders_by_value_then_by_column():
    theta = np.array([[0.2, 0.9, 0.5, 0.9, 0.1],
                      [0.3, 0.3, 0.3, 0.3, 0.3]])
    cols, scores = host_top_n(theta, 3)
    assert cols.tolist() == [[1, 3, 2], [0, 1, 2]]
    assert scores.tolist() == [[0.9, 0.9, 0.5], [0.3, 0.3, 0.3]]
    cols, _ = host_top_n(theta, 1)
    assert cols.tolist() == [[1], [0]]


def test_host_top_n_compares_numerically():
    theta = np.array([[-0.0, 0.0, -1.0, np.inf, -np.inf, 5e-324]])
    cols, scores = host_top_n(theta, 6)
    assert cols.tolist() == [[3, 5, 0, 1, 2, 4]]                  # -0.0 ties with +0.0: the lower column first
    assert np.signbit(scores[0, 2]) and not np.signbit(scores[0, 3])   # ... and each keeps its own bits


def test_host_top_n_skips_nan_and_pads_short_rows():
    nan = np.nan
    theta = np.array([[0.5, nan, 0.7, 0.6],
                      [nan, nan, nan, nan],
                      [0.1, 0.2, 0.3, 0.4]])
    cols, scores = host_top_n(theta, 6)
    assert cols.tolist() == [[2, 3, 0, -1, -1, -1], [-1] * 6, [3, 2, 1, 0, -1, -1]]
    assert np.array_equal(np.isnan(scores), cols < 0)
    assert scores[0, :3].tolist() == [0.7, 0.6, 0.5]


def test_host_top_n_exclude():
    theta = np.array([[0.9, 0.8, 0.7, 0.6],
                      [0.9, 0.8, 0.7, 0.6],
                      [0.5, 0.5, 0.5, np.nan]])
    exclude = np.array([[1, 0, 0, 0],
                        [1, 1, 1, 1],
                        [0, 2, 0, 0]], dtype=np.uint8)                 # nonzero, not just 1, means skip
    cols, scores = host_top_n(theta, 2, exclude)
    assert cols.tolist() == [[1, 2], [-1, -1], [0, 2]]
    assert scores[0].tolist() == [0.8, 0.7] and np.all(np.isnan(scores[1]))
    same_ranking(host_top_n(theta, 2, exclude.astype(bool)), (cols, scores))
    same_ranking(host_top_n(theta, 2, np.zeros((3, 4), dtype=bool)), host_top_n(theta, 2))


# ---- the C entry point, as far as a host without a GPU reaches it ---------------------------------------------------------
def test_symbol_is_declared_and_exported():
    from nbmf_mm_amd import _hip
    assert "nbmf_top_n" in _hip.SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "nbmf_top_n")
    # tests/asan_null_calls.py builds its null call from the argtypes: only these kinds
    plain = {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}
    assert len(lib.nbmf_top_n.argtypes) == 10 and set(lib.nbmf_top_n.argtypes) <= plain
    assert lib.nbmf_abi_version() == 4
    assert _hip.TOP_N_MAX == 256
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbmf_hip.h")).read()
    assert "#define NBMF_TOP_N_MAX 256" in header


def test_null_context_is_an_argument_error():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    assert lib.nbmf_top_n(None, 0, 0, 0, 0, None, 0, None, None, 0) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    cols = np.zeros((2, 3), dtype=np.int64)
    assert lib.nbmf_top_n(None, 0, 2, 3, 1, None, 0, cols.ctypes.data_as(ctypes.c_void_p), None, 3) == _hip.NBMF_ERR_ARG
    assert not cols.any()


# ---- Context.top_n: every argument error before any device call -----------------------------------------------------------
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


@pytest.mark.parametrize("top", [0, -1, 257, 2.0, 2.5, "3", None, True, np.float64(4)])
def test_context_refuses_a_bad_top(bare_context, top):
    with pytest.raises(ValueError, match="top must be"):
        bare_context.top_n(top)


def test_context_takes_numpy_integers_for_top():
    from nbmf_mm_amd import _hip
    assert _hip.top_n_count(np.int32(7)) == 7 and _hip.top_n_count(1) == 1 and _hip.top_n_count(256) == 256


@pytest.mark.parametrize("row0,nrows", [(-1, 2), (12, 1), (11, 2), (0, -1), (0, 13)])
def test_context_refuses_rows_outside_the_matrix(bare_context, row0, nrows):
    with pytest.raises(ValueError, match="rows"):
        bare_context.top_n(3, row0, nrows)


def test_context_refuses_a_bad_exclude(bare_context):
    ctx = bare_context
    with pytest.raises(ValueError, match="shape"):
        ctx.top_n(3, exclude=np.zeros((12, 8), dtype=bool))
    with pytest.raises(ValueError, match="shape"):
        ctx.top_n(3, exclude=np.zeros((11, 9), dtype=bool))
    with pytest.raises(ValueError, match="shape"):
        ctx.top_n(3, 2, 4, exclude=np.zeros((12, 9), dtype=bool))          # the shape follows the request: (nrows, n)
    with pytest.raises(ValueError, match="shape"):
        ctx.top_n(3, exclude=np.zeros(12 * 9, dtype=bool))
    for dtype in (np.float64, np.int64, np.int8, np.float32):
        with pytest.raises(ValueError, match="dtype"):
            ctx.top_n(3, exclude=np.zeros((12, 9), dtype=dtype))
    with pytest.raises(ValueError, match="stride"):
        ctx.top_n(3, exclude=np.zeros((12, 18), dtype=np.uint8)[:, ::2])   # not unit stride along a row
    with pytest.raises(ValueError, match="stride"):
        ctx.top_n(3, exclude=np.zeros((9, 12), dtype=bool).T)              # column-major
    with pytest.raises(ValueError, match="stride"):
        ctx.top_n(3, exclude=np.zeros((12, 9), dtype=bool)[::-1])          # rows run backwards
    with pytest.raises(ValueError, match="stride"):
        ctx.top_n(3, exclude=np.broadcast_to(np.zeros(9, dtype=bool), (12, 9)))


def test_row_array_passes_a_wider_exclude_through():
    from nbmf_mm_amd import _hip
    exclude_bytes = lambda a, nrows, n: _hip.row_array(a, nrows, n, "exclude", _hip.BYTE_KINDS)[::2]   # noqa: E731
    wide = np.zeros((12, 20), dtype=bool)
    view, ldx = exclude_bytes(wide[:, 3:12], 12, 9)
    assert ldx == 20 and view.dtype == np.uint8 and np.shares_memory(view, wide)
    view, ldx = exclude_bytes(np.ones((12, 9), dtype=np.uint8), 12, 9)
    assert ldx == 9
    view, ldx = exclude_bytes(wide[4:5, :9], 1, 9)                         # one row: its stride does not matter
    assert ldx == 9
    view, ldx = exclude_bytes([[True, False]], 1, 2)
    assert view.tolist() == [[1, 0]]


# ---- NBMF.top_n -------------------------------------------------------------------------------------------------------------
def test_not_fitted_is_transforms_error():
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError) as want:
        NBMF().transform(np.zeros((3, 4)))
    with pytest.raises(ValueError) as got:
        NBMF().top_n()
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
    for n in (0, -3, 257, 2.5, 10.0, "5", None, False):
        with pytest.raises(ValueError, match="n must be"):
            model.top_n(n)
    with pytest.raises(ValueError, match="components"):
        model.top_n(3, W=np.full((4, 2), 0.5))
    with pytest.raises(ValueError, match="components"):
        model.top_n(3, W=np.full((4, 5), 0.2))
    with pytest.raises(ValueError, match="shape"):
        model.top_n(3, exclude=np.zeros((12, 8)))
    with pytest.raises(ValueError, match="shape"):
        model.top_n(3, exclude=np.zeros((9, 12)))                          # the other orientation
    with pytest.raises(ValueError, match="shape"):
        model.top_n(3, exclude=np.zeros(9))
    with pytest.raises(ValueError, match="shape"):
        model.top_n(3, W=np.full((4, 3), 1 / 3), exclude=np.zeros((12, 9)))   # exclude follows W, not W_
    with pytest.raises(ValueError, match="shape"):
        model.top_n(3, exclude=sp.csr_matrix((12, 8)))
    with pytest.raises(ValueError, match="dtype"):
        model.top_n(3, exclude=np.full((12, 9), "a"))
    with pytest.raises(ValueError, match="dtype"):
        model.top_n(3, exclude=np.full((12, 9), None, dtype=object))


def test_well_formed_request_reaches_the_device_or_fails_loudly():
    """No CPU fallback: without a GPU the call is an error of the library, with one it answers."""
    from nbmf_mm_amd import NBMF, _hip
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    if _hip.device_count() == 0:
        for call in (lambda: model.top_n(), lambda: model.top_n(3, exclude=np.zeros((12, 9)))):
            with pytest.raises(_hip.NBMFHipError, match="no HIP device"):
                call()
    else:
        cols, scores = model.top_n(3)
        assert cols.shape == (12, 3) and scores.shape == (12, 3)
