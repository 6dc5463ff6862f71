"""The held-out split drawn on the device (nbmf_hold_out, nbmf_hold_out_undo, nbmf_get_eval_pairs; Context.hold_out ...;
NBMF.fit(holdout=...), experiments.cross_validate): what can be said without a GPU.

* ``holdout_interval``: what it accepts and what it refuses;
* ``holdout_reference``, the NumPy statement of the rule the GPU tests compare the device against, in integers: a subset of
  the mask, folds that partition the mask exactly, no symmetry under a transpose of the shape, a salted uniform that is not
  ``hash_uniform``'s, and a held-out share inside 5 binomial standard deviations;
* every ValueError of the fit's hold-out arguments, raised before any device work; the symbols."""
import math
import os

import numpy as np
import pytest

from nbmf_mm_amd import NBMF, _hip, holdout_mask, nbmf_mm_solver
from nbmf_mm_amd._hip import holdout_interval, holdout_reference


def narrow_interval_37x83():
    """An interval on 37 x 83 (seed 3, everything observed) so narrow that several rows hold out nothing while at least one
    entry is held out: shared with the GPU tests, and checked here."""
    return 3, 0.5, 0.5 + 1.0 / 256


def test_interval_accepts_and_refuses():
    assert holdout_interval(0.2) == (0.0, 0.2)
    assert holdout_interval(np.float64(0.5)) == (0.0, 0.5)
    assert holdout_interval((0.4, 0.6)) == (0.4, 0.6)
    assert holdout_interval([0, 0.25]) == (0.0, 0.25)
    assert holdout_interval((0.8, 1)) == (0.8, 1.0)
    assert holdout_interval((0.0, 1.0)) == (0.0, 1.0)          # a pair means itself: the library says what it leaves
    for bad in (True, False, np.True_, (True, 0.5), (0.1, False), float("nan"), (float("nan"), 0.5), (0.1, float("nan")),
                0.0, 1.0, 0, 1, -0.1, 1.5, (0.5, 0.5), (0.6, 0.4), (-0.1, 0.5), (0.0, 1.1), "0.2", None, (0.1,), (0.1, 0.2, 0.3),
                (0.1, "x"), float("inf")):
        with pytest.raises(ValueError, match="holdout"):
            holdout_interval(bad)


def test_reference_is_a_subset_of_the_mask_and_folds_partition_it():
    shape = (37, 83)
    mask = np.random.default_rng(4).random(shape) < 0.7
    for seed in (0, 5, 2 ** 64 - 1):
        folds = [holdout_reference(shape, seed, f / 5, (f + 1) / 5, mask=mask) for f in range(5)]
        for held in folds:
            assert held.dtype == np.bool_ and held.shape == shape
            assert not np.any(held & ~mask)
        assert np.array_equal(np.sum(folds, axis=0, dtype=np.int64), mask.astype(np.int64))   # each observed entry exactly once
        assert all(h.any() for h in folds)
        # no mask: everything is in the pool; a numeric mask counts by != 0
        assert np.array_equal(np.sum([holdout_reference(shape, seed, f / 5, (f + 1) / 5) for f in range(5)], axis=0,
                                     dtype=np.int64), np.ones(shape, dtype=np.int64))
        assert np.array_equal(holdout_reference(shape, seed, 0.2, 0.4, mask=mask * 2.5), folds[1])
    # a slice costs its own size and is the slice
    rows, cols = np.array([36, 0, 7]), np.array([82, 1])
    whole = holdout_reference(shape, 5, 0.1, 0.6)
    assert np.array_equal(holdout_reference(shape, 5, 0.1, 0.6, rows=rows, cols=cols), whole[rows][:, cols])
    assert np.array_equal(holdout_mask(shape, 5, (0.1, 0.6), mask=mask), whole & mask)
    assert np.array_equal(holdout_mask(shape, 5, 0.6), holdout_reference(shape, 5, 0.0, 0.6))


def test_reference_of_the_transposed_shape_is_another_split():
    # the counter is u * V + v of the shape as given: nobody may assume the split of (V, U) is the transpose of (U, V)'s
    a, b = holdout_reference((37, 83), 0, 0.0, 0.25), holdout_reference((83, 37), 0, 0.0, 0.25)
    assert not np.array_equal(b.T, a)
    assert np.count_nonzero(b.T != a) > 100


def test_salted_uniform_is_not_hash_uniform():
    m, n, seed = 37, 83, 11
    u = _hip.hash_uniform(m, n, seed)
    salted = _hip._hash_u01(m, n, seed, None, None, salt=_hip.HOLDOUT_SALT)
    assert _hip.HOLDOUT_SALT == 0xA0761D6478BD642F
    assert np.all((salted >= 0) & (salted < 1))
    assert np.count_nonzero(u == salted) == 0
    assert np.array_equal(holdout_reference((m, n), seed, 0.25, 0.5), (salted >= 0.25) & (salted < 0.5))
    assert not np.array_equal(holdout_reference((m, n), seed, 0.25, 0.5), (u >= 0.25) & (u < 0.5))
    # the rule by hand for one entry, in Python integers
    i, j, M64 = 36, 82, (1 << 64) - 1
    x = (((seed * 0x100000001B3 + i * n + j) & M64) ^ 0xA0761D6478BD642F)
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    assert salted[i, j] == (x >> 11) * 2.0 ** -53


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_held_out_share(seed):
    # 65536 entries at f = 0.1: mean 6553.6, standard deviation sqrt(65536 x 0.1 x 0.9) = 76.8; 5 of them = 384
    count = int(np.count_nonzero(holdout_reference((256, 256), seed, 0.0, 0.1)))
    print(f"seed {seed}: {count} held out of 65536 (mean 6553.6, 5 sigma = {5 * math.sqrt(65536 * 0.1 * 0.9):.1f})")
    assert abs(count - 6553.6) <= 384


def test_the_narrow_interval_of_the_gpu_tests():
    seed, lo, hi = narrow_interval_37x83()
    held = holdout_reference((37, 83), seed, lo, hi)
    per_row = held.sum(axis=1)
    assert held.sum() >= 1 and np.count_nonzero(per_row == 0) >= 3 and np.count_nonzero(per_row) >= 3
    per_row_t = holdout_reference((83, 37), seed, lo, hi).sum(axis=0)     # dir-beta: the internal rows are the user's columns
    assert per_row_t.sum() >= 1 and np.count_nonzero(per_row_t == 0) >= 3


def test_argument_errors_come_before_any_device_work(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a context was created before the arguments were checked")
    monkeypatch.setattr(_hip, "Context", no_device)
    X = (np.random.default_rng(0).random((20, 30)) < 0.3).astype(np.float64)
    E = np.zeros(X.shape, dtype=bool)
    E[0, 0] = True
    for fit in (lambda **kw: NBMF(n_components=3, max_iter=5, **kw.pop("ctor", {})).fit(X, **kw),
                lambda **kw: nbmf_mm_solver(X, 3, max_iter=5, **kw.pop("ctor", {}), **kw)):
        with pytest.raises(ValueError, match="eval_mask"):
            fit(holdout=0.2, eval_mask=E)
        with pytest.raises(ValueError, match="n_gpus"):
            fit(holdout=0.2, ctor=dict(n_gpus=2))
        with pytest.raises(ValueError, match="n_gpus"):
            fit(holdout=0.2, ctor=dict(devices=[0]))
        for bad in (0.0, 1.0, True, float("nan"), (0.5, 0.5), (0.6, 0.4), (-0.1, 0.5), (0.0, 1.5), "x"):
            with pytest.raises(ValueError, match="holdout"):
                fit(holdout=bad)
        for bad in (-1, 2 ** 64, 1.5, True, "7"):
            with pytest.raises(ValueError, match="holdout_seed"):
                fit(holdout=0.2, holdout_seed=bad)
        with pytest.raises(ValueError, match="holdout_seed needs a holdout"):
            fit(holdout_seed=3)
        with pytest.raises(ValueError, match="eval_every"):
            fit(holdout=0.2, eval_every=0)
        with pytest.raises(ValueError, match="patience"):
            fit(holdout=0.2, patience=-1)
    from nbmf_mm_amd.experiments import cross_validate
    for bad in (1, 0, True, 2.0):
        with pytest.raises(ValueError, match="n_folds"):
            cross_validate(X, 3, n_folds=bad)
    with pytest.raises(ValueError, match="orientation"):
        cross_validate(X, 3, orientation="sideways")


def test_signatures_and_symbols():
    import inspect
    p = inspect.signature(NBMF.fit).parameters
    assert list(p)[-2:] == ["holdout", "holdout_seed"] and p["holdout"].default is None and p["holdout_seed"].default is None
    p = inspect.signature(nbmf_mm_solver).parameters
    assert p["holdout"].default is None and p["holdout_seed"].default is None
    p = inspect.signature(_hip.Context.hold_out).parameters
    assert list(p) == ["self", "seed", "lo", "hi", "transposed", "every", "patience"]
    assert (p["transposed"].default, p["every"].default, p["patience"].default) == (False, 10, 0)
    for name in ("nbmf_hold_out", "nbmf_hold_out_undo", "nbmf_get_eval_pairs"):
        assert name in _hip.SYMBOLS
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nbmf_hip.h")).read()
    for decl in ("int nbmf_hold_out(nbmf_ctx* ctx, uint64_t seed, int transposed, double lo, double hi, int every, int patience, "
                 "int64_t* count);", "int nbmf_hold_out_undo(nbmf_ctx* ctx);",
                 "int nbmf_get_eval_pairs(nbmf_ctx* ctx, int64_t cap, int64_t* count, int64_t* rows, int64_t* cols, uint8_t* x);"):
        assert decl in header
