"""Prediction on the device (nbmf_predict_at / nbmf_predict_rows, NBMF.predict_proba / predict / impute): everything that
can be said without a GPU -- the symbols are declared and exported, a null context is an argument error, every malformed
request raises ValueError BEFORE a context is created, and a well-formed one fails loudly where no device is visible
(there is no CPU fallback).  The values are tested on the GPU: tests/test_gpu_predict.py."""
import ctypes

import numpy as np
import pytest


def test_symbols_are_declared():
    from nbmf_mm_amd import _hip
    assert "nbmf_predict_at" in _hip.SYMBOLS and "nbmf_predict_rows" in _hip.SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "nbmf_predict_at") and hasattr(lib, "nbmf_predict_rows")
    # tests/asan_null_calls.py builds its null call from the argtypes: only these four kinds
    plain = {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}
    assert set(lib.nbmf_predict_at.argtypes) <= plain and set(lib.nbmf_predict_rows.argtypes) <= plain


def test_null_context_is_an_argument_error():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    assert lib.nbmf_predict_at(None, None, None, 0, 0, None) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    assert lib.nbmf_predict_rows(None, 0, 0, 0, 0, 0.0, None, 0) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()


def test_not_fitted_is_transforms_error():
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError) as want:
        NBMF().transform(np.zeros((3, 4)))
    for call in (lambda: NBMF().predict_proba(), lambda: NBMF().predict(),
                 lambda: NBMF().impute(np.zeros((3, 4)), np.ones((3, 4)))):
        with pytest.raises(ValueError) as got:
            call()
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


def test_malformed_requests_raise_before_any_device_call(hand_set):
    model = hand_set
    with pytest.raises(ValueError, match="both or neither"):
        model.predict_proba(rows=np.array([0, 1]))
    with pytest.raises(ValueError, match="both or neither"):
        model.predict_proba(cols=np.array([0, 1]))
    with pytest.raises(ValueError, match="equally long"):
        model.predict_proba(rows=np.array([0, 1, 2]), cols=np.array([0, 1]))
    with pytest.raises(ValueError, match="integer"):
        model.predict_proba(rows=np.array([0.0, 1.0]), cols=np.array([0, 1]))
    with pytest.raises(ValueError, match="integer"):
        model.predict_proba(rows=np.array([0, 1]), cols=np.array([0.0, 1.0]))
    with pytest.raises(ValueError, match="1-D"):
        model.predict_proba(rows=np.zeros((2, 2), dtype=np.int64), cols=np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="components"):
        model.predict_proba(W=np.full((4, 2), 0.5))
    with pytest.raises(ValueError, match="components"):
        model.predict(W=np.full((4, 5), 0.2))
    with pytest.raises(ValueError, match="NaN"):
        model.predict(threshold=float("nan"))
    X = np.zeros((12, 9))
    with pytest.raises(ValueError, match="mask"):
        model.impute(X, None)
    with pytest.raises(ValueError, match="shape"):
        model.impute(np.zeros((12, 8)), np.ones((12, 8)))
    with pytest.raises(ValueError, match="shape"):
        model.impute(np.zeros((11, 9)), np.ones((11, 9)))


def test_binding_checks_its_index_arrays_without_a_context():
    from nbmf_mm_amd import _hip
    rows, cols = _hip.index_pairs(np.array([3, 1], dtype=np.int32), [0, 2])
    assert rows.dtype == np.int64 and cols.dtype == np.int64 and rows.flags.c_contiguous
    assert rows.tolist() == [3, 1] and cols.tolist() == [0, 2]
    with pytest.raises(ValueError):
        _hip.index_pairs(np.array([True, False]), np.array([0, 1]))


def test_no_gpu_means_loud_failure_not_fallback():
    from nbmf_mm_amd import NBMF, _hip
    if _hip.device_count() > 0:
        pytest.skip("a GPU is visible here")
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    for call in (lambda: model.predict_proba(), lambda: model.predict_proba(rows=np.array([0]), cols=np.array([1])),
                 lambda: model.predict(), lambda: model.impute(np.zeros((12, 9)), np.zeros((12, 9)))):
        with pytest.raises(_hip.NBMFHipError, match="no HIP device"):
            call()
