"""PackedBits and everything about bit-packed input that needs no GPU: the layout (np.packbits, rows on their own, pad
bits meaningless), what the type offers and what it refuses, the estimator's shape errors and the out-of-scope
combinations -- all raised before any device work (``_hip.Context`` is replaced by a class that fails when constructed)
-- and the argument checks of the new C entry points, which return before the runtime is touched."""
import ctypes

import numpy as np
import pytest

from nbmf_mm_amd import NBMF, PackedBits, _hip, nbmf_mm_solver
from nbmf_mm_amd import _dist, _solver

NEW_SYMBOLS = ("nbmf_top_n_v", "nbmf_score_rows_v", "nbmf_theta_hist_v", "nbmf_rank_rows_v", "nbmf_selftest_unpack_bits")


def dense(rows, n, seed=0, p=0.4):
    return np.random.default_rng(seed).random((rows, n)) < p


# ---- the type ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65])
def test_round_trip(n):
    A = dense(6, n, seed=n)
    P = PackedBits.from_dense(A)
    assert P.shape == (6, n) and P.bits.dtype == np.uint8 and P.bits.shape == (6, (n + 7) // 8)
    assert np.array_equal(P.bits, np.packbits(A, axis=1))
    assert P.nbytes == 6 * ((n + 7) // 8) and len(P) == 6 and P.ndim == 2
    out = P.toarray()
    assert out.dtype == np.bool_ and np.array_equal(out, A)
    assert np.array_equal(PackedBits(np.packbits(A, axis=1), A.shape).toarray(), A)


def test_from_dense_packs_nonzero_of_any_dtype():
    A = dense(5, 19, seed=3)
    for B in (A, A.astype(np.float64) * 0.25, A.astype(np.int32) * -3, A.astype(np.uint8) * 7, A.astype(np.float32)):
        assert np.array_equal(PackedBits.from_dense(B).toarray(), A)
    assert np.array_equal(PackedBits.from_dense(A.tolist()).toarray(), A)
    with pytest.raises(ValueError, match="2-D"):
        PackedBits.from_dense(A[0])


def test_at_reads_index_pairs():
    A = dense(9, 21, seed=4)
    P = PackedBits.from_dense(A)
    r, c = np.divmod(np.random.default_rng(5).permutation(9 * 21), 21)
    got = P.at(r, c)
    assert got.dtype == np.bool_ and np.array_equal(got, A[r, c])
    assert P.at(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)).shape == (0,)
    with pytest.raises(ValueError, match="outside"):
        P.at(np.array([9]), np.array([0]))
    with pytest.raises(ValueError, match="outside"):
        P.at(np.array([0]), np.array([21]))
    with pytest.raises(ValueError, match="outside"):
        P.at(np.array([-1]), np.array([0]))
    with pytest.raises(ValueError, match="integer"):
        P.at(np.array([0.0]), np.array([0]))
    with pytest.raises(ValueError, match="same shape"):
        P.at(np.array([0, 1]), np.array([0]))


def test_row_slices_are_views():
    A = dense(10, 21, seed=6)
    P = PackedBits.from_dense(A)
    S = P[2:7]
    assert S.shape == (5, 21) and np.array_equal(S.toarray(), A[2:7])
    assert np.shares_memory(S.bits, P.bits) and S.bits.strides == P.bits.strides
    assert P[:].shape == P.shape and P[8:100].shape == (2, 21) and P[4:4].shape == (0, 21) and P[7:2].shape == (0, 21)
    assert np.array_equal(P[-3:].toarray(), A[-3:])
    # rows of a wider packed array: 21 entries need 3 bytes, the rows are 8 bytes apart and stay so
    wide = np.full((10, 8), 0xFF, dtype=np.uint8)
    wide[:, :3] = P.bits
    Q = PackedBits(wide[3:9], (6, 21))
    assert np.shares_memory(Q.bits, wide) and Q.bits.strides == (8, 1) and Q.ld == 8 and Q.nbytes == 18
    assert np.array_equal(Q.toarray(), A[3:9])
    assert Q[1:3].bits.strides == (8, 1) and np.shares_memory(Q[1:3].bits, wide)
    assert np.array_equal(Q[1:3].toarray(), A[4:6])
    assert P.ld == 3 and P[0:1].ld == 3                      # (a single row has no stride to speak of)


def test_pad_bits_do_not_show():
    A = dense(4, 13, seed=7)
    bits = np.packbits(A, axis=1)
    bits[:, -1] |= 0x07                                      # the 3 pad bits of the last byte
    P = PackedBits(bits, (4, 13))
    assert np.array_equal(P.toarray(), A)
    r, c = np.nonzero(np.ones_like(A))
    assert np.array_equal(P.at(r, c), A[r, c])


def test_rejected_constructions_and_operations():
    bits = np.zeros((4, 3), dtype=np.uint8)
    with pytest.raises(TypeError, match="uint8"):
        PackedBits(bits.astype(np.int8), (4, 20))
    with pytest.raises(TypeError, match="uint8"):
        PackedBits(bits.astype(bool), (4, 20))
    with pytest.raises(TypeError):
        PackedBits(PackedBits(bits, (4, 20)), (4, 20))
    with pytest.raises(ValueError, match="2-D"):
        PackedBits(bits.ravel(), (4, 20))
    with pytest.raises(ValueError, match="at least 4 bytes"):
        PackedBits(bits, (4, 25))                            # 25 entries need 4 bytes a row
    with pytest.raises(ValueError, match="4 rows"):
        PackedBits(bits[:3], (4, 20))
    with pytest.raises(ValueError, match="shape must be"):
        PackedBits(bits, 20)
    with pytest.raises(ValueError, match="non-negative"):
        PackedBits(bits, (4, -1))
    with pytest.raises(ValueError, match="unit stride"):
        PackedBits(np.zeros((4, 6), dtype=np.uint8)[:, ::2], (4, 20))
    with pytest.raises(ValueError, match="unit stride"):
        PackedBits(np.zeros((3, 4), dtype=np.uint8).T, (4, 20))    # column-major: rows 1 byte apart
    P = PackedBits(bits, (4, 20))
    for key in (1, (slice(None), slice(0, 8)), np.array([0, 1]), (0, 0), Ellipsis):
        with pytest.raises(TypeError, match="row slices"):
            P[key]
    with pytest.raises(ValueError, match="step 1"):
        P[::2]
    with pytest.raises(ValueError, match="transposed"):
        P.T
    with pytest.raises(TypeError):
        P + 1
    with pytest.raises(TypeError):
        np.ones((4, 20)) * P


# ---- the estimator: every error before any device work ----------------------------------------------------------------------
class _NoDevice:
    def __init__(self, *a, **k):
        raise AssertionError("a device context was created before the arguments were checked")


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_hip, "Context", _NoDevice)


def fitted(m=12, n=20, k=3):
    est = NBMF(n_components=k, max_iter=5)
    r = np.random.default_rng(8)
    W = r.uniform(0.1, 0.9, (m, k))
    est.W_ = W / W.sum(1, keepdims=True)
    est.components_ = r.uniform(0.1, 0.9, (k, n))
    return est


def test_estimator_shape_errors_come_before_the_device(no_device):
    X = dense(12, 20, seed=9)
    P, short, narrow = PackedBits.from_dense(X), PackedBits.from_dense(X[:11]), PackedBits.from_dense(X[:, :19])
    est = NBMF(n_components=3, max_iter=5)
    with pytest.raises(ValueError, match=r"mask has shape \(11, 20\)"):
        est.fit(P, mask=short)
    with pytest.raises(ValueError, match=r"mask has shape \(12, 19\)"):
        est.fit(X, mask=narrow)
    with pytest.raises(ValueError, match="at least one sample"):
        est.fit(P[0:0])
    with pytest.raises(ValueError, match="eval_mask has shape"):
        est.fit(P, eval_mask=X[:11])
    est = fitted()
    with pytest.raises(ValueError, match="X has 19 features"):
        est.transform(narrow)
    with pytest.raises(ValueError, match="X has 19 features"):
        est.score(narrow)
    with pytest.raises(ValueError, match=r"mask has shape \(11, 20\)"):
        est.score(P, mask=short)
    for call in (est.score_samples, est.theta_histogram, est.roc_auc, est.calibration_curve):
        with pytest.raises(ValueError, match=r"X has shape \(11, 20\), the request describes \(12, 20\)"):
            call(short)
        with pytest.raises(ValueError, match=r"mask has shape \(12, 19\), the request describes \(12, 20\)"):
            call(P, mask=narrow)
        with pytest.raises(ValueError, match=r"mask has shape \(11, 20\)"):
            call(X, mask=short)
    with pytest.raises(ValueError, match=r"exclude has shape \(11, 20\), the request describes \(12, 20\)"):
        est.top_n(3, exclude=short)
    with pytest.raises(ValueError, match=r"exclude has shape \(12, 19\)"):
        est.rank_of(X, exclude=narrow)
    with pytest.raises(ValueError, match=r"exclude has shape \(12, 19\)"):
        est.ranking_metrics(X, exclude=narrow)


def test_out_of_scope_combinations_raise(no_device):
    X = dense(12, 20, seed=10)
    M = dense(12, 20, seed=11, p=0.9)
    P, PM = PackedBits.from_dense(X), PackedBits.from_dense(M)
    for kw in (dict(n_gpus=2), dict(devices=[0, 1]), dict(devices=[0])):
        with pytest.raises(ValueError, match="one GPU"):
            NBMF(n_components=3, max_iter=5, **kw).fit(P)
        with pytest.raises(ValueError, match="one GPU"):
            NBMF(n_components=3, max_iter=5, **kw).fit(X, mask=PM)
        with pytest.raises(ValueError, match="one GPU"):
            nbmf_mm_solver(P, 3, max_iter=5, **kw)
        with pytest.raises(ValueError, match="one GPU"):
            nbmf_mm_solver(X.astype(float), 3, max_iter=5, mask=PM, **kw)
    with pytest.raises(ValueError, match="sharded fits"):
        _dist.fit_in_process(P, 3, 2)
    with pytest.raises(ValueError, match="sharded fits"):
        _dist.fit_in_process(X.astype(float), 3, 2, mask=PM)
    with pytest.raises(ValueError, match="sharded fits"):
        _dist.fit_sharded(P, (12, 20), 0, 3, group=None)
    with pytest.raises(ValueError, match="sharded fits"):
        _dist.fit_row_sharded(P, 12, 0, 3, group=None)
    est = fitted()
    with pytest.raises(ValueError, match="impute does not take PackedBits"):
        est.impute(P, M)
    with pytest.raises(ValueError, match="impute does not take PackedBits"):
        est.impute(X.astype(float), PM)
    with pytest.raises(ValueError, match="targets as PackedBits is not supported"):
        est.rank_of(P)
    with pytest.raises(ValueError, match="targets as PackedBits is not supported"):
        est.ranking_metrics(P, exclude=P)
    with pytest.raises(ValueError, match="eval_mask as PackedBits is not supported"):
        NBMF(n_components=3, max_iter=5).fit(P, mask=PM, eval_mask=PackedBits.from_dense(~M))
    with pytest.raises(ValueError, match="eval_mask as PackedBits is not supported"):
        nbmf_mm_solver(P, 3, max_iter=5, eval_mask=PackedBits.from_dense(~M))
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(ValueError, match="nbmf_upload_csr"):
        _solver.upload_any(None, sp.csr_matrix(X.astype(float)), mask=PM)
    with pytest.raises(ValueError, match="nbmf_upload_csr"):
        _solver.upload_any(None, P, mask=sp.csr_matrix(M.astype(float)))


def test_eval_pairs_reads_the_truth_of_packed_data():
    X = dense(12, 20, seed=12)
    E = dense(12, 20, seed=13, p=0.2)
    for orientation in ("beta-dir", "dir-beta"):
        want = _solver.eval_pairs(X, E, 5, 0, orientation)
        got = _solver.eval_pairs(PackedBits.from_dense(X), E, 5, 0, orientation)
        assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(want, got))


def test_row_array_takes_packed_operands_where_asked():
    P = PackedBits.from_dense(dense(6, 21, seed=14))
    a, kind, ld = _hip.row_array(P, 6, 21, "x", _hip.BYTE_KINDS, packed=True)
    assert a is P.bits and kind == _hip.DATA_BITS == 3 and ld == 3 and _hip.MASK_BITS == 3
    wide = np.zeros((6, 8), dtype=np.uint8)
    assert _hip.row_array(PackedBits(wide, (6, 21)), 6, 21, "x", _hip.BYTE_KINDS, packed=True)[2] == 8
    with pytest.raises(ValueError, match=r"x must have shape \(5, 21\)"):
        _hip.row_array(P, 5, 21, "x", _hip.BYTE_KINDS, packed=True)
    with pytest.raises(ValueError, match="out must be a NumPy array"):
        _hip.row_array(P, 6, 21, "out", _hip.BYTE_KINDS)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_symbols_hold_the_new_names():
    lib = _hip.load()
    for name in NEW_SYMBOLS:
        assert name in _hip.SYMBOLS and hasattr(lib, name) and getattr(lib, name).argtypes
    assert lib.nbmf_abi_version() == 4


def test_argument_checks_return_before_any_device_call():
    """All of these come back with NBMF_ERR_ARG from argument validation: no runtime call is made, with or without a GPU."""
    lib = _hip.load()
    ERR = _hip.NBMF_ERR_ARG
    bits = np.zeros((2, 2), dtype=np.uint8)
    out = np.zeros((2, 9), dtype=np.uint8)
    pb, po = bits.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    unpack = lib.nbmf_selftest_unpack_bits
    assert unpack(0, None, 0, 0, 0, None, 0) == ERR and b"null" in lib.nbmf_last_error()
    assert unpack(0, None, 2, 2, 9, po, 9) == ERR and b"null" in lib.nbmf_last_error()
    assert unpack(0, pb, 2, 2, 9, None, 9) == ERR and b"null" in lib.nbmf_last_error()
    assert unpack(0, pb, 2, -1, 9, po, 9) == ERR and b">= 0" in lib.nbmf_last_error()
    assert unpack(0, pb, 2, 2, -9, po, 9) == ERR and b">= 0" in lib.nbmf_last_error()
    assert unpack(0, pb, 1, 2, 9, po, 9) == ERR and lib.nbmf_last_error() == b"ldbits 1 is less than ceil(n / 8) = 2"
    assert unpack(0, pb, 1, 0, 9, po, 9) == ERR and b"ldbits" in lib.nbmf_last_error()        # (also with no rows)
    assert unpack(0, pb, 2, 2, 9, po, 8) == ERR and lib.nbmf_last_error() == b"ldout 8 is less than n = 9"
    assert unpack(0, pb, 2, 0, 9, po, 8) == ERR and b"ldout" in lib.nbmf_last_error()
    assert lib.nbmf_top_n_v(None, 0, 0, 0, 0, None, 0, 0, None, None, 0) == ERR and b"null context" in lib.nbmf_last_error()
    assert lib.nbmf_score_rows_v(None, 0, 0, 0, 0.0, None, 0, 0, None, 0, 0, None, None, None, None) == ERR
    assert b"null context" in lib.nbmf_last_error()
    assert lib.nbmf_theta_hist_v(None, 0, 0, 0, None, 0, 0, None, 0, 0, None, None) == ERR
    assert b"null context" in lib.nbmf_last_error()
    assert lib.nbmf_rank_rows_v(None, 0, 0, 0, None, None, None, 0, 0, None, None, None, None, None) == ERR
    assert b"null context" in lib.nbmf_last_error()
    assert lib.nbmf_upload_v(None, pb, _hip.DATA_BITS, 1, 0, None, 0, 0, None) == ERR
