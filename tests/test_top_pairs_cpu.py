"""The best entries of Theta over the whole matrix as (row, column) pairs (nbmf_top_pairs, Context.top_pairs,
NBMF.top_pairs, NBMF.least_likely): everything that can be said without a GPU -- the symbol is declared and exported, a null
context is an argument error that leaves the outputs alone, every malformed request raises ValueError BEFORE any device
call -- and the reference selection ``host_top_pairs`` that tests/test_gpu_top_pairs.py compares the device against, checked
here on hand-written cases (order, signed zeros, NaN, short lists, exclude, the likelihood score) and against its own
threshold-predicate restatement and the merge over a row partition."""
import ctypes
import os

import numpy as np
import pytest


def host_top_pairs(score, top, eligible=None, largest=True, row0=0):
    """The reference selection: the first ``top`` entries of ``score`` that are not NaN and that ``eligible`` (nonzero, or
    absent) admits, by score -- descending with ``largest``, else ascending, compared numerically --, then ascending row,
    then ascending column: ``np.lexsort((cols, rows, -+score))``.  Returns ``(rows + row0 int64, cols int64, scores
    float64)``, each ``min(top, eligible entries)`` long; a score keeps its own bits."""
    score = np.asarray(score, dtype=np.float64)
    ok = ~np.isnan(score)
    if eligible is not None:
        eligible = np.asarray(eligible)
        assert eligible.shape == score.shape
        ok &= eligible != 0
    rows, cols = np.nonzero(ok)
    s = score[rows, cols]
    order = np.lexsort((cols, rows, -s if largest else s))[:top]
    return rows[order].astype(np.int64) + row0, cols[order].astype(np.int64), s[order]


def same_pairs(got, want):
    """Rows, columns and count equal, scores equal bit for bit: no tolerance."""
    (gr, gc, gs), (wr, wc, ws) = got, want
    assert gr.dtype == np.int64 and gc.dtype == np.int64 and gs.dtype == np.float64
    assert gr.shape == wr.shape and gc.shape == wc.shape and gs.shape == ws.shape, (gr.shape, wr.shape)
    assert np.array_equal(gr, wr)
    assert np.array_equal(gc, wc)
    assert np.array_equal(gs.view(np.uint64), np.asarray(ws, dtype=np.float64).view(np.uint64))


def merge_pairs(a, b, top, largest=True):
    """The first ``top`` of two results over disjoint row ranges, in the order of ``host_top_pairs``."""
    rows, cols, s = (np.concatenate(p) for p in zip(a, b))
    order = np.lexsort((cols, rows, -s if largest else s))[:top]
    return rows[order], cols[order], s[order]


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_host_top_pairs_orders_by_value_then_row_then_column():
    theta = np.array([[0.2, 0.9, 0.5],
                      [0.9, 0.1, 0.9],
                      [0.5, 0.9, 0.2]])
    rows, cols, scores = host_top_pairs(theta, 6)
    assert list(zip(rows.tolist(), cols.tolist())) == [(0, 1), (1, 0), (1, 2), (2, 1), (0, 2), (2, 0)]
    assert scores.tolist() == [0.9, 0.9, 0.9, 0.9, 0.5, 0.5]
    rows, cols, scores = host_top_pairs(theta, 3, largest=False, row0=10)
    assert list(zip(rows.tolist(), cols.tolist())) == [(11, 1), (10, 0), (12, 2)]
    assert scores.tolist() == [0.1, 0.2, 0.2]


def test_host_top_pairs_compares_numerically_and_keeps_bits():
    theta = np.array([[0.0, -1.0], [-0.0, 5e-324], [np.inf, -np.inf]])
    rows, cols, scores = host_top_pairs(theta, 6)
    assert list(zip(rows.tolist(), cols.tolist())) == [(2, 0), (1, 1), (0, 0), (1, 0), (0, 1), (2, 1)]
    assert not np.signbit(scores[2]) and np.signbit(scores[3])            # -0.0 ties +0.0: row order, own bits
    rows, cols, scores = host_top_pairs(-theta, 6, largest=False)          # the same order from the other end
    assert list(zip(rows.tolist(), cols.tolist())) == [(2, 0), (1, 1), (0, 0), (1, 0), (0, 1), (2, 1)]
    assert np.signbit(scores[2]) and not np.signbit(scores[3])


def test_host_top_pairs_skips_nan_and_shortens_the_list():
    nan = np.nan
    theta = np.array([[0.5, nan], [nan, nan], [0.1, 0.7]])
    rows, cols, scores = host_top_pairs(theta, 10)
    assert rows.tolist() == [2, 0, 2] and cols.tolist() == [1, 0, 0] and scores.tolist() == [0.7, 0.5, 0.1]
    rows, cols, scores = host_top_pairs(np.full((2, 2), nan), 3)
    assert rows.size == cols.size == scores.size == 0


def test_host_top_pairs_exclude_bytes_other_than_one():
    theta = np.array([[0.9, 0.8], [0.7, 0.6]])
    exclude = np.array([[2, 0], [0, 255]], dtype=np.uint8)                # nonzero, not just 1, means skip
    rows, cols, scores = host_top_pairs(theta, 4, eligible=exclude == 0)
    assert rows.tolist() == [0, 1] and cols.tolist() == [1, 0] and scores.tolist() == [0.8, 0.7]
    same_pairs(host_top_pairs(theta, 4, eligible=~exclude.astype(bool)), (rows, cols, scores))
    rows, _, _ = host_top_pairs(theta, 4, eligible=np.zeros((2, 2), dtype=bool))
    assert rows.size == 0


def test_host_top_pairs_likelihood_scores_under_a_mask():
    theta = np.array([[0.9, 0.2, 0.6], [0.3, 0.75, 0.5]])
    x = np.array([[1, 1, 0], [0, 0, 1]], dtype=np.uint8)
    mask = np.array([[1, 1, 1], [1, 0, 1]], dtype=np.uint8)
    prob = np.where(x != 0, theta, 1.0 - theta)                            # [[.9 .2 .4] [.7 .25 .5]]
    rows, cols, scores = host_top_pairs(prob, 3, eligible=mask, largest=False)
    assert list(zip(rows.tolist(), cols.tolist())) == [(0, 1), (0, 2), (1, 2)]   # (1, 1) at 0.25 is not observed
    assert scores.tolist() == [0.2, 1.0 - 0.6, 0.5]


def test_threshold_predicate_and_row_partition_restate_the_reference():
    """What the device does: a threshold value T, everything better than T, and of the entries equal to T the first in
    (row, column) order up to a boundary (r*, c*).  And the call on a row range is the merge of the calls on two ranges
    that partition it.  On a dyadic matrix with 24 distinct values, so nearly every threshold falls inside a tie group."""
    r = np.random.default_rng(3)
    theta = r.integers(0, 24, (23, 41)) / 32.0
    theta[r.random(theta.shape) < 0.05] = np.nan
    eligible = r.random(theta.shape) < 0.8
    for largest in (True, False):
        for top in (1, 5, 100, 400, 2000):
            want = host_top_pairs(theta, top, eligible, largest)
            ok = eligible & ~np.isnan(theta)
            rr, cc = np.nonzero(ok)
            key = theta[rr, cc] if largest else -theta[rr, cc]
            if top >= key.size:
                take = np.ones(key.size, dtype=bool)
            else:
                T = np.sort(key)[::-1][top - 1]
                need = top - int((key > T).sum())
                ties = np.flatnonzero(key == T)                           # (row-major order already)
                rs, cs = rr[ties[need - 1]], cc[ties[need - 1]]
                take = (key > T) | ((key == T) & ((rr < rs) | ((rr == rs) & (cc <= cs))))
            got_set = sorted(zip(rr[take].tolist(), cc[take].tolist()))
            assert got_set == sorted(zip(want[0].tolist(), want[1].tolist()))
            a = host_top_pairs(theta[:9], top, eligible[:9], largest)
            b = host_top_pairs(theta[9:], top, eligible[9:], largest, row0=9)
            same_pairs(merge_pairs(a, b, top, largest), want)


# ---- the C entry point, as far as a host without a GPU reaches it ---------------------------------------------------------
def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbmf_hip.h")).read()


def test_symbol_is_declared_and_exported():
    from nbmf_mm_amd import _hip
    assert "nbmf_top_pairs" in _hip.SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "nbmf_top_pairs")
    # tests/asan_null_calls.py builds its null call from the argtypes: only these kinds
    plain = {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}
    assert len(lib.nbmf_top_pairs.argtypes) == 16 and set(lib.nbmf_top_pairs.argtypes) <= plain
    assert lib.nbmf_abi_version() == 4
    header = _header()
    assert "int nbmf_top_pairs(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int64_t top, int clip_theta, int kind," in header
    assert "#define NBMF_TOP_PAIRS_MAX (1 << 22)" in header and _hip.TOP_PAIRS_MAX == 1 << 22
    assert "#define NBMF_PAIRS_THETA 0" in header and _hip.PAIRS_THETA == 0
    assert "#define NBMF_PAIRS_LIKELIHOOD 1" in header and _hip.PAIRS_LIKELIHOOD == 1


def test_null_context_is_an_argument_error_and_writes_nothing():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    assert lib.nbmf_top_pairs(None, 0, 0, 0, 0, 0, None, 0, 0, None, 0, 0, None, None, None, None) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    rows, cols = np.full(3, 7, dtype=np.int64), np.full(3, 7, dtype=np.int64)
    scores = np.full(3, 7.0)
    count = ctypes.c_int64(7)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    assert lib.nbmf_top_pairs(None, 0, 2, 3, 1, 0, None, _hip.DATA_U8, 0, None, _hip.MASK_NONE, 0, ptr(rows), ptr(cols), ptr(scores),
                              ctypes.cast(ctypes.byref(count), ctypes.c_void_p)) == _hip.NBMF_ERR_ARG
    assert count.value == 7 and np.all(rows == 7) and np.all(cols == 7) and np.all(scores == 7.0)


# ---- Context.top_pairs: every argument error before any device call -------------------------------------------------------
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


@pytest.mark.parametrize("top", [0, -1, (1 << 22) + 1, 2.0, 2.5, "3", None, True, np.float64(4)])
def test_context_refuses_a_bad_top(bare_context, top):
    with pytest.raises(ValueError, match="top must be"):
        bare_context.top_pairs(top)


def test_context_takes_numpy_integers_for_top():
    from nbmf_mm_amd import _hip
    assert _hip.top_pairs_count(np.int32(7)) == 7 and _hip.top_pairs_count(1) == 1
    assert _hip.top_pairs_count(np.int64(1 << 22)) == 1 << 22


@pytest.mark.parametrize("row0,nrows", [(-1, 2), (12, 1), (11, 2), (0, -1), (0, 13)])
def test_context_refuses_rows_outside_the_matrix(bare_context, row0, nrows):
    with pytest.raises(ValueError, match="rows"):
        bare_context.top_pairs(3, row0=row0, nrows=nrows)


def test_context_refuses_a_bad_kind_or_a_misplaced_operand(bare_context):
    ctx = bare_context
    for kind in ("Theta", "loglik", 0, None):
        with pytest.raises(ValueError, match="kind must be"):
            ctx.top_pairs(3, kind=kind)
    with pytest.raises(ValueError, match="not a mask"):
        ctx.top_pairs(3, mask=np.ones((12, 9), dtype=bool))
    with pytest.raises(ValueError, match="needs the data"):
        ctx.top_pairs(3, kind="likelihood")
    with pytest.raises(ValueError, match="needs the data"):
        ctx.top_pairs(3, kind="likelihood", mask=np.ones((12, 9), dtype=bool))


@pytest.mark.parametrize("kind,name", [("theta", "x"), ("likelihood", "x"), ("likelihood", "mask")])
def test_context_refuses_a_bad_operand(bare_context, kind, name):
    from nbmf_mm_amd import PackedBits
    ctx = bare_context
    good = np.zeros((12, 9), dtype=np.uint8)

    def call(a, **kw):
        args = {"x": good} if kind == "likelihood" else {}
        args[name] = a
        return ctx.top_pairs(3, kind=kind, **args, **kw)
    for bad in (np.zeros((12, 8), dtype=bool), np.zeros((11, 9), dtype=bool), np.zeros(12 * 9, dtype=bool)):
        with pytest.raises(ValueError, match="shape"):
            call(bad)
    with pytest.raises(ValueError, match="shape"):
        ctx.top_pairs(3, kind=kind, row0=2, nrows=4, **{**({"x": good[2:6]} if kind == "likelihood" else {}), name: good})
    for dtype in (np.float64, np.int64, np.int8, np.float32):
        with pytest.raises(ValueError, match="dtype"):
            call(np.zeros((12, 9), dtype=dtype))
    with pytest.raises(ValueError, match="stride"):
        call(np.zeros((12, 18), dtype=np.uint8)[:, ::2])
    with pytest.raises(ValueError, match="stride"):
        call(np.zeros((9, 12), dtype=bool).T)
    with pytest.raises(ValueError, match="stride"):
        call(np.zeros((12, 9), dtype=bool)[::-1])
    with pytest.raises(ValueError, match="shape"):
        call(PackedBits.from_dense(np.zeros((12, 10), dtype=bool)))
    with pytest.raises(ValueError, match="shape"):
        call(PackedBits.from_dense(np.zeros((11, 9), dtype=bool)))


# ---- NBMF.top_pairs and NBMF.least_likely ---------------------------------------------------------------------------------
def test_not_fitted_is_transforms_error():
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError) as want:
        NBMF().transform(np.zeros((3, 4)))
    for call in (lambda: NBMF().top_pairs(), lambda: NBMF().least_likely(np.zeros((3, 4)))):
        with pytest.raises(ValueError) as got:
            call()
        assert str(got.value) == str(want.value)


def _hand_set_model():
    from nbmf_mm_amd import NBMF
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    return model


@pytest.fixture
def hand_set(monkeypatch):
    """An estimator with hand-set factors (12 x 9, k = 3), in a process where creating a context is an error of the test."""
    from nbmf_mm_amd import _hip
    model = _hand_set_model()

    def no_device_call(*a, **k):
        raise AssertionError("a context was created for a request that is malformed")
    monkeypatch.setattr(_hip, "Context", no_device_call)
    return model


def test_top_pairs_refuses_malformed_requests_before_any_device_call(hand_set):
    import scipy.sparse as sp
    from nbmf_mm_amd import PackedBits
    model = hand_set
    for n in (0, -3, (1 << 22) + 1, 2.5, 10.0, "5", None, False):
        with pytest.raises(ValueError, match="n must be"):
            model.top_pairs(n)
    with pytest.raises(ValueError, match="components"):
        model.top_pairs(3, W=np.full((4, 2), 0.5))
    for bad in (np.zeros((12, 8)), np.zeros((9, 12)), np.zeros(9), sp.csr_matrix((12, 8)),
                PackedBits.from_dense(np.zeros((12, 8), dtype=bool))):
        with pytest.raises(ValueError, match="shape"):
            model.top_pairs(3, exclude=bad)
    with pytest.raises(ValueError, match="shape"):
        model.top_pairs(3, W=np.full((4, 3), 1 / 3), exclude=np.zeros((12, 9)))   # exclude follows W, not W_
    with pytest.raises(ValueError, match="dtype"):
        model.top_pairs(3, exclude=np.full((12, 9), "a"))


def test_least_likely_refuses_malformed_requests_before_any_device_call(hand_set):
    import scipy.sparse as sp
    from nbmf_mm_amd import PackedBits
    model = hand_set
    X = (np.random.default_rng(1).random((12, 9)) < 0.3).astype(np.float64)
    for n in (0, -3, (1 << 22) + 1, 2.5, 10.0, "5", None, False):
        with pytest.raises(ValueError, match="n must be"):
            model.least_likely(X, n=n)
    with pytest.raises(ValueError, match="components"):
        model.least_likely(X[:4], W=np.full((4, 2), 0.5))
    for bad in (X[:, :8], X.T, sp.csr_matrix(X[:, :8]), PackedBits.from_dense(X[:11])):
        with pytest.raises(ValueError, match="shape"):
            model.least_likely(bad)
    with pytest.raises(ValueError, match="X must be binary"):
        model.least_likely(X * 0.5)                                        # real-valued data is out of scope
    with pytest.raises(ValueError, match="X must be binary"):
        model.least_likely(sp.csr_matrix(X * 0.5))
    with pytest.raises(ValueError, match="X must be binary"):
        model.least_likely(X + 1.0)
    with pytest.raises(ValueError, match="shape"):
        model.least_likely(X, mask=np.ones((12, 8)))
    with pytest.raises(ValueError, match="shape"):
        model.least_likely(X, mask=PackedBits.from_dense(np.ones((11, 9), dtype=bool)))
    with pytest.raises(ValueError, match="dtype"):
        model.least_likely(X, mask=np.full((12, 9), "a"))


def test_one_call_operand_packs_sparse_and_numeric_input_block_by_block(monkeypatch):
    """A sparse or 0/1 numeric operand becomes packed bits without an m x n byte matrix on the host; bool / uint8 and
    PackedBits pass through as they are."""
    import scipy.sparse as sp
    from nbmf_mm_amd import PackedBits, _solver
    r = np.random.default_rng(2)
    A = r.random((50, 21)) < 0.3
    monkeypatch.setattr(_solver, "TOP_N_EXCLUDE_BLOCK_BYTES", 21 * 7)      # 7 rows per block
    for form in (sp.csr_matrix(A.astype(np.float64)), sp.coo_matrix(A.astype(np.int8)), A.astype(np.float64), A.astype(np.int64)):
        for is_mask in (True, False):
            p = _solver._one_call_operand(form, is_mask)
            assert isinstance(p, PackedBits) and p.shape == (50, 21) and np.array_equal(p.toarray(), A)
    assert np.array_equal(_solver._one_call_operand(2.0 * A, True).toarray(), A)   # a mask is != 0
    with pytest.raises(ValueError, match="X must be binary"):
        _solver._one_call_operand(2.0 * A, False)
    byte = A.view(np.uint8)
    assert np.shares_memory(_solver._one_call_operand(byte, True), byte) and np.shares_memory(_solver._one_call_operand(A, False), A)
    packed = PackedBits.from_dense(A)
    assert _solver._one_call_operand(packed, True) is packed and _solver._one_call_operand(None, True) is None


def test_well_formed_request_reaches_the_device_or_fails_loudly():
    """No CPU fallback: without a GPU the call is an error of the library, with one it answers."""
    from nbmf_mm_amd import _hip
    model = _hand_set_model()
    X = np.random.default_rng(1).random((12, 9)) < 0.3
    if _hip.device_count() == 0:
        for call in (lambda: model.top_pairs(), lambda: model.top_pairs(3, exclude=X), lambda: model.least_likely(X, n=5)):
            with pytest.raises(_hip.NBMFHipError, match="no HIP device"):
                call()
    else:
        rows, cols, scores = model.top_pairs(5)
        assert rows.shape == cols.shape == scores.shape == (5,)
        rows, cols, prob = model.least_likely(X, n=5)
        assert rows.shape == cols.shape == prob.shape == (5,)
