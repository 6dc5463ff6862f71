"""What of the bit-decision path (nbmf_theta_bits; predict(packed=True), sample) needs no device: the NumPy regeneration of
the counter-based uniform, the seed rule, the argument errors of the estimator methods, and the declaration."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 7, 2 ** 63 + 5, 2 ** 64 - 1)


def test_hash_uniform_is_the_u_of_synthetic_reference():
    from nbmf_mm_amd import _hip
    rows, cols = np.array([3, 0, 36, 36]), np.array([52, 2, 0])
    for s in SEEDS:
        u = _hip.hash_uniform(37, 53, s)
        assert u.dtype == np.float64 and u.shape == (37, 53)
        for d in (0.0, 0.25, 0.3, 1.0):
            assert np.array_equal(u < d, _hip.synthetic_reference(37, 53, s, density=d)[0] != 0)
        sub = _hip.hash_uniform(37, 53, s, rows=rows, cols=cols)
        assert np.array_equal(sub, u[rows][:, cols])
        assert np.array_equal(sub < 0.3, _hip.synthetic_reference(37, 53, s, density=0.3, rows=rows, cols=cols)[0] != 0)
        assert np.array_equal(_hip.hash_uniform(37, 53, s, rows=rows), u[rows])
    assert not np.array_equal(_hip.hash_uniform(37, 53, 0), _hip.hash_uniform(37, 53, 1))
    # i * n + j: the matrix width enters the counter
    assert np.array_equal(_hip.hash_uniform(4, 6, 9).ravel(), _hip.hash_uniform(1, 24, 9).ravel())


def test_hash_uniform_lies_in_the_half_open_unit_interval():
    from nbmf_mm_amd import _hip
    for s in SEEDS:
        u = _hip.hash_uniform(256, 512, s)
        assert u.min() >= 0.0 and u.max() < 1.0
        assert np.array_equal(u * 2.0 ** 53, np.floor(u * 2.0 ** 53))        # 53-bit integers times 2^-53
        assert abs(u.mean() - 0.5) < 5 * np.sqrt(1 / 12 / u.size)
    # the largest value the construction can give is below 1
    assert float(2 ** 53 - 1) * (1.0 / 9007199254740992.0) < 1.0


def test_synthetic_reference_is_what_it_was():
    """Entries computed with the parent commit's synthetic_reference, before the hash was factored out of it."""
    from nbmf_mm_amd import _hip
    Y, M = _hip.synthetic_reference(37, 53, 12345, 0.25, 0.8)
    assert Y.dtype == np.float64 and M.dtype == np.bool_
    assert Y[:3, :10].astype(int).tolist() == [[0, 0, 0, 0, 0, 1, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0, 0, 1, 1, 0],
                                               [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
    assert int(Y.sum()) == 512 and int(M.sum()) == 1586
    assert M[36, -8:].astype(int).tolist() == [1, 1, 1, 1, 0, 1, 1, 1]
    Y, M = _hip.synthetic_reference(5, 7, 2 ** 64 - 1, 0.5, 0.5)
    assert Y.astype(int).tolist() == [[0, 0, 1, 1, 0, 0, 1], [1, 1, 0, 1, 0, 1, 1], [0, 1, 1, 0, 1, 0, 1], [0, 0, 0, 1, 1, 1, 1],
                                      [0, 1, 0, 0, 0, 0, 0]]
    assert M.astype(int).tolist() == [[0, 1, 0, 0, 1, 1, 0], [1, 1, 1, 1, 0, 1, 0], [0, 0, 0, 0, 1, 1, 0], [0, 0, 1, 0, 0, 0, 0],
                                      [1, 1, 0, 1, 1, 0, 0]]
    Ys, Ms = _hip.synthetic_reference(5, 7, 2 ** 64 - 1, 0.5, 0.5, rows=[4, 1], cols=[6, 0, 3])
    assert np.array_equal(Ys, Y[[4, 1]][:, [6, 0, 3]]) and np.array_equal(Ms, M[[4, 1]][:, [6, 0, 3]])
    u = _hip.hash_uniform(2, 3, 1)
    assert [x.hex() for x in u.ravel()] == ["0x1.ffb8ee2564b44p-2", "0x1.af3fe3a733e3fp-1", "0x1.fe4b4f5bdad54p-3",
                                            "0x1.db74b25dbcca4p-2", "0x1.3c7c2f7fe3e8cp-1", "0x1.0228e52a16258p-1"]


def test_sample_seed():
    from nbmf_mm_amd import _hip
    for s in (0, 1, 2 ** 63 + 5, 2 ** 64 - 1):
        assert _hip.sample_seed(s) == s and type(_hip.sample_seed(s)) is int
    assert _hip.sample_seed(np.int64(5)) == 5 and _hip.sample_seed(np.uint64(2 ** 64 - 1)) == 2 ** 64 - 1
    for bad in (-1, 2 ** 64, True, False, np.bool_(True), 1.0, "3", (1,), np.random.default_rng(0), np.random.RandomState(0)):
        with pytest.raises(ValueError, match="random_state"):
            _hip.sample_seed(bad)
    # None: NumPy's global RNG decides, as it does for transform
    np.random.seed(123)
    a, b = _hip.sample_seed(None), _hip.sample_seed(None)
    np.random.seed(123)
    assert _hip.sample_seed(None) == a and a != b and 0 <= a < 2 ** 64


def fitted(n=12, k=3, rows=9):
    """An estimator that looks fitted, made without a device."""
    from nbmf_mm_amd import NBMF
    g = np.random.default_rng(0)
    model = NBMF(n_components=k)
    model.components_ = g.uniform(0.1, 0.9, (k, n))
    W = g.uniform(0.1, 0.9, (rows, k))
    model.W_ = W / W.sum(1, keepdims=True)
    return model


def test_argument_errors_come_before_any_device_work(monkeypatch):
    from nbmf_mm_amd import NBMF, _base

    def no_device(*a, **kw):
        raise AssertionError("device work was started")
    for name in ("device_theta_bits", "device_predict"):
        monkeypatch.setattr(_base, name, no_device)
    model = fitted()
    for call in (lambda: model.predict(packed=1), lambda: model.predict(packed=None), lambda: model.predict(packed="yes"),
                 lambda: model.predict(threshold=float("nan"), packed=True),
                 lambda: model.sample(packed=1), lambda: model.sample(random_state=-1), lambda: model.sample(random_state=2 ** 64),
                 lambda: model.sample(random_state=True), lambda: model.sample(random_state=0.5),
                 lambda: model.sample(W=np.ones((4, 2))), lambda: model.predict(W=np.ones((4, 5)), packed=True),
                 lambda: model.sample(W=np.ones(3))):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: NBMF(n_components=3).sample(), lambda: NBMF(n_components=3).sample(random_state=1, packed=True),
                 lambda: NBMF(n_components=3).predict(packed=True)):
        with pytest.raises(ValueError, match="not fitted"):
            call()
    # ... and good arguments do reach the device path
    with pytest.raises(AssertionError, match="device work"):
        model.sample(random_state=2 ** 64 - 1, packed=True)
    with pytest.raises(AssertionError, match="device work"):
        model.predict(packed=True)


def test_the_symbol_is_declared_and_bound():
    from nbmf_mm_amd import _hip
    text = open(os.path.join(ROOT, "include", "nbmf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+nbmf_theta_bits\s*\(\s*nbmf_ctx\s*\*", code)
    assert re.search(r"#define\s+NBMF_BITS_THRESHOLD\s+0\b", code) and re.search(r"#define\s+NBMF_BITS_SAMPLE\s+1\b", code)
    assert "nbmf_theta_bits" in _hip.SYMBOLS
    assert (_hip.BITS_THRESHOLD, _hip.BITS_SAMPLE) == (0, 1)
    lib = _hip.load()
    assert hasattr(lib, "nbmf_theta_bits") and len(lib.nbmf_theta_bits.argtypes) == 9
    # what can be refused without a device is: a null context
    assert lib.nbmf_theta_bits(None, 0, 0, 1, 0, 0.5, 0, None, 0) == _hip.NBMF_ERR_ARG
    assert hasattr(_hip.Context, "theta_bits")
