"""Held-out log-likelihood curve and early stopping inside fit (nbmf_set_eval, nbmf_eval_loglik, nbmf_get_eval,
nbmf_get_best_factors; Context.set_eval ...; NBMF.fit(eval_mask=...)): what can be said without a GPU.

* ``host_eval_loglik``, the reference tests/test_gpu_eval_curve.py compares the device's sum against, on hand cases;
* ``stop_rule``, a restatement of the patience rule as a pure function, on hand cases;
* the planted case (``planted_case``, ``oracle_curve``: made once, shared with the GPU tests) and that the ORACLE's curve on
  it has what the GPU test of early stopping needs: a peak inside the run, a stop before the last iteration, and no
  comparison of the rule closer than 1e-6 in the mean -- the fit's pinned parity with the oracle (factors to 1e-9) then
  cannot flip one;
* every ValueError of the estimator's eval arguments, raised before any device work; the symbols."""
import ctypes
import math
import os

import numpy as np
import pytest


def host_eval_loglik(theta_at_pairs, x, eps=1e-8):
    """The semantics of nbmf_eval_loglik in NumPy: ``t = log(where(x != 0, theta + eps, (1 - theta) + eps))`` at every
    pair, ``theta_at_pairs`` being what predict_at returned for them without the clip.  Returns ``(fsum(t), fsum(|t|))``:
    exactly rounded sums, so the reference's own summation error is nil."""
    theta = np.asarray(theta_at_pairs, dtype=np.float64)
    x = np.asarray(x)
    assert theta.ndim == 1 and x.shape == theta.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.log(np.where(x != 0, theta + eps, (1.0 - theta) + eps))
    return math.fsum(t), math.fsum(np.abs(t))


def eval_bound(count, abs_sum):
    """\\|got - want\\| <= (count + 8) 2^-52 sum\\|t\\|: the bound of test_score_samples_cpu.assert_sums_within_bound with the
    same derivation -- both logarithms within 1 ulp of the same argument and at most two roundings to form a term
    (8 2^-52 \\|t\\| in all, generously), and at most count - 1 roundings of 2^-53 sum\\|t\\| for ANY summation order."""
    return (count + 8) * 2.0 ** -52 * abs_sum


def stop_rule(labels, values, every, patience):
    """The stop rule of nbmf_run with an eval set, restated: ``(stop_s, best_s, stopped_early)`` for a curve given as
    ascending labels s and the sums at them.  An evaluation improves if its value is strictly greater than the best so
    far; the first always improves.  With ``patience = p > 0`` the run ends at the p-th consecutive evaluation on a
    multiple of ``every`` that does not improve; otherwise (and with ``patience = 0``) at the last label.  ``best_s`` is
    the label of the best evaluation up to the stop."""
    assert len(labels) == len(values) >= 1
    best_s, best_v, since = None, None, 0
    for s, v in zip(labels, values):
        if best_s is None or v > best_v:
            best_s, best_v, since = s, v, 0
        elif s % every == 0:
            since += 1
        if patience > 0 and since >= patience:
            return s, best_s, True
    return labels[-1], best_s, False


def rule_gaps(labels, values, every, patience):
    """\\|value - best so far\\| of every comparison ``stop_rule`` makes up to its stop."""
    stop_s = stop_rule(labels, values, every, patience)[0]
    gaps, best = [], None
    for s, v in zip(labels, values):
        if best is not None:
            gaps.append(abs(v - best))
        if best is None or v > best:
            best = v
        if s == stop_s:
            break
    return gaps


# ---- the planted case: made once, shared (read-only) with tests/test_gpu_eval_curve.py -----------------------------------
PLANTED = dict(K=6, alpha=1.0, beta=1.0, random_state=0, max_iter=120, every=5, patience=3)
_planted = {}


def planted_case():
    """``(X float64 100 x 500, train bool, ev bool)``: V ~ Bernoulli(Wt Ht) from three planted components, 70 % of the
    entries for training and 20 % held out, everything drawn from one generator in a fixed order."""
    if "case" not in _planted:
        g = np.random.default_rng(0)
        Wt = g.dirichlet(np.full(3, 0.3), 100)
        Ht = g.beta(0.5, 0.5, (3, 500))
        X = (g.random((100, 500)) < Wt @ Ht).astype(np.float64)
        u = g.random((100, 500))
        train, ev = u < 0.7, (u >= 0.7) & (u < 0.9)
        for a in (X, train, ev):
            a.setflags(write=False)
        _planted["case"] = (X, train, ev)
    return _planted["case"]


def planted_init(m, k, n, random_state):
    """The init oracle.solve draws for ``random_state``: ``(W k x m on the simplex, H k x n)``."""
    rs = np.random.RandomState(random_state)
    W0 = rs.uniform(0.1, 0.9, (m, k))
    H0 = rs.uniform(0.1, 0.9, (k, n))
    W = W0.T
    return np.ascontiguousarray(W / W.sum(axis=0, keepdims=True)), H0


def oracle_curve():
    """``(labels, sums, count)``: the held-out log-likelihood SUM of the oracle's factors after s = 5, 10, ..., 120 of its
    own MM steps from solve's own init, over the planted case's held-out entries in row-major order."""
    if "curve" not in _planted:
        from oracle import nbmf_oracle as orc
        X, train, ev = planted_case()
        p = PLANTED
        W, H = planted_init(100, p["K"], 500, p["random_state"])
        r, c = np.nonzero(ev)
        x = X[r, c]
        labels, sums = [], []
        for s in range(1, p["max_iter"] + 1):
            W, H = orc.mm_step(X, W, H, train, p["alpha"], p["beta"], 1e-8)
            if s % p["every"] == 0:
                labels.append(s)
                sums.append(host_eval_loglik(np.einsum("kt,kt->t", W[:, r], H[:, c]), x, 1e-8)[0])
        _planted["curve"] = (labels, sums, int(r.size))
    return _planted["curve"]


# ---- the reference itself ---------------------------------------------------------------------------------------------------
def near(got, want, ulps=4):
    return abs(got - want) <= ulps * 2.0 ** -52 * abs(want)


def test_host_eval_loglik_hand_cases():
    eps = 1e-8
    theta = np.array([0.25, 0.5, 0.75, 0.1])
    x = np.array([1, 0, 7, 0], dtype=np.uint8)                                # nonzero, not just 1, means x = 1
    t = [math.log(0.25 + eps), math.log((1 - 0.5) + eps), math.log(0.75 + eps), math.log((1 - 0.1) + eps)]
    s, a = host_eval_loglik(theta, x, eps)
    assert near(s, math.fsum(t)) and near(a, -math.fsum(t))                   # every term is negative here
    # bool truth is the same as bytes; a repeated pair counts twice; the order does not matter to fsum
    assert host_eval_loglik(theta, x != 0, eps) == (s, a)
    s2, a2 = host_eval_loglik(np.concatenate([theta, theta[:1]]), np.concatenate([x, x[:1]]), eps)
    assert near(s2, math.fsum(t + t[:1])) and near(a2, -math.fsum(t + t[:1]))
    assert host_eval_loglik(theta[::-1], x[::-1], eps) == (s, a)
    # another eps enters the argument
    assert near(host_eval_loglik(theta[:1], x[:1], 1e-3)[0], math.log(0.25 + 1e-3))


def test_host_eval_loglik_at_the_ends_of_theta():
    eps = 1e-8
    lo, hi = math.log(eps), math.log(1.0 + eps)
    theta = np.array([0.0, 1.0, 0.0, 1.0])
    s, a = host_eval_loglik(theta, np.array([1, 1, 0, 0], dtype=np.uint8), eps)
    assert near(s, math.fsum([lo, hi, hi, lo])) and near(a, math.fsum([-lo, hi, hi, -lo])) and hi > 0.0
    # unclipped: a theta beyond 1 + eps has no likelihood where x = 0
    assert math.isnan(host_eval_loglik(np.array([1.5]), np.array([0], dtype=np.uint8), eps)[0])
    assert near(host_eval_loglik(np.array([1.5]), np.array([1], dtype=np.uint8), eps)[0], math.log(1.5 + eps))


def test_the_bound_is_the_score_samples_bound():
    from test_score_samples_cpu import assert_sums_within_bound
    edge = eval_bound(3, 10.0)
    assert edge == 11 * 2.0 ** -52 * 10.0
    obs = np.array([3], dtype=np.int64)
    assert_sums_within_bound(np.array([-10.0 + 0.9 * edge]), obs, np.array([-10.0]), obs, np.array([10.0]))
    with pytest.raises(AssertionError):
        assert_sums_within_bound(np.array([-10.0 + 1.2 * edge]), obs, np.array([-10.0]), obs, np.array([10.0]))


# ---- the stop rule ----------------------------------------------------------------------------------------------------------
def test_stop_rule_hand_cases():
    lab = [5, 10, 15, 20, 25, 30]
    # rises, peaks at 10, falls: patience 3 stops at the third non-improving evaluation
    assert stop_rule(lab, [-3.0, -2.0, -2.5, -2.4, -2.3, -2.2], 5, 3) == (25, 10, True)
    assert stop_rule(lab, [-3.0, -2.0, -2.5, -2.4, -2.3, -2.2], 5, 1) == (15, 10, True)
    # patience 0 records the curve and never stops
    assert stop_rule(lab, [-3.0, -2.0, -2.5, -2.4, -2.3, -2.2], 5, 0) == (30, 10, False)
    # an improvement resets the count
    assert stop_rule(lab, [-3.0, -3.5, -3.4, -2.0, -2.1, -2.2], 5, 3) == (30, 20, False)
    assert stop_rule(lab, [-3.0, -3.5, -3.4, -2.0, -2.1, -2.2], 5, 2) == (15, 5, True)
    # ties do not improve: the best stays the FIRST of equal values
    assert stop_rule(lab, [-2.0, -2.0, -2.0, -2.0, -2.0, -2.0], 5, 2) == (15, 5, True)
    assert stop_rule(lab, [-2.0, -2.0, -2.0, -2.0, -2.0, -2.0], 5, 0) == (30, 5, False)
    # the first evaluation is always the best so far, whatever its value -- also a NaN, which nothing then exceeds
    assert stop_rule([5], [-1e300], 5, 1) == (5, 5, False)
    assert stop_rule(lab[:3], [math.nan, -1.0, -0.5], 5, 2) == (15, 5, True)
    # a monotone rise never stops
    assert stop_rule(lab, [-6.0, -5.0, -4.0, -3.0, -2.0, -1.0], 5, 1) == (30, 30, False)
    # a last evaluation off the multiples (max_iter = 23, or a tol stop) can improve but does not count against patience
    assert stop_rule([5, 10, 15, 20, 23], [-2.0, -2.1, -2.2, -2.3, -2.4], 5, 4) == (23, 5, False)
    assert stop_rule([5, 10, 15, 20, 23], [-2.0, -2.1, -2.2, -2.3, -1.0], 5, 4) == (23, 23, False)


def test_rule_gaps_are_the_comparisons_up_to_the_stop():
    lab = [5, 10, 15, 20, 25, 30]
    gaps = rule_gaps(lab, [-3.0, -2.0, -2.5, -2.4, -2.3, -2.2], 5, 3)
    assert np.allclose(gaps, [1.0, 0.5, 0.4, 0.3]) and len(gaps) == 4          # 10 v 5, then 15, 20, 25 v the best (10)


# ---- the planted case can show what the GPU test needs ---------------------------------------------------------------------
def test_planted_case_draws():
    X, train, ev = planted_case()
    assert X.shape == train.shape == ev.shape == (100, 500)
    assert not np.any(train & ev)
    assert abs(train.mean() - 0.7) < 0.01 and abs(ev.mean() - 0.2) < 0.01
    assert set(np.unique(X)) == {0.0, 1.0}


def test_oracle_curve_peaks_inside_the_run_and_the_rule_stops_on_clear_gaps():
    p = PLANTED
    labels, sums, count = oracle_curve()
    assert labels == list(range(p["every"], p["max_iter"] + 1, p["every"]))
    mean = np.asarray(sums) / count
    print("oracle mean held-out log-likelihood:", dict(zip(labels, np.round(mean, 5))))
    best = int(np.argmax(mean))
    assert 0 < best < len(labels) - 1, "the best evaluation must be neither the first nor the last"
    stop_s, best_s, early = stop_rule(labels, sums, p["every"], p["patience"])
    assert early and stop_s < p["max_iter"]
    assert best_s == labels[best]
    gaps = np.asarray(rule_gaps(labels, sums, p["every"], p["patience"])) / count
    print(f"stop at {stop_s}, best at {best_s}, smallest gap of a comparison {gaps.min():.3e}")
    assert gaps.min() >= 1e-6


# ---- the estimator: every error of the eval arguments before any device work ------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called for a request that is malformed")


@pytest.fixture
def no_device(monkeypatch):
    from nbmf_mm_amd import _hip
    monkeypatch.setattr(_hip, "_lib", _NoDevice())
    monkeypatch.setattr(_hip, "Context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("a context was created")))


def small():
    g = np.random.default_rng(5)
    X = (g.random((12, 9)) < 0.4).astype(np.float64)
    ev = g.random((12, 9)) < 0.2
    return X, ~ev, ev


@pytest.mark.parametrize("entry", ["estimator", "solver"])
def test_eval_argument_errors_before_any_device_work(no_device, entry):
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF, nbmf_mm_solver
    X, train, ev = small()

    def fit(X=X, n_gpus=1, devices=None, **kw):
        if entry == "estimator":
            return NBMF(n_components=2, max_iter=5, n_gpus=n_gpus, devices=devices).fit(X, mask=train, **kw)
        return nbmf_mm_solver(X, 2, max_iter=5, mask=train, n_gpus=n_gpus, devices=devices, **kw)

    with pytest.raises(ValueError, match="eval_mask has shape"):
        fit(eval_mask=ev[:, :-1])
    with pytest.raises(ValueError, match="eval_mask has shape"):
        fit(eval_mask=sp.csr_matrix(ev.T))
    with pytest.raises(ValueError, match="eval_mask has shape"):
        fit(eval_mask=ev.ravel())
    with pytest.raises(ValueError, match="eval set is empty"):
        fit(eval_mask=np.zeros_like(ev))
    with pytest.raises(ValueError, match="eval set is empty"):
        fit(eval_mask=sp.csr_matrix(ev.shape))
    with pytest.raises(ValueError, match="bool or numeric"):
        fit(eval_mask=np.full(ev.shape, "x"))
    half = X.copy()
    half[np.nonzero(ev)[0][0], np.nonzero(ev)[1][0]] = 0.5
    with pytest.raises(ValueError, match="0 or 1 at the entries eval_mask marks"):
        fit(X=half, eval_mask=ev)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="eval_every"):
            fit(eval_mask=ev, eval_every=bad)
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError, match="patience"):
            fit(eval_mask=ev, patience=bad)
    with pytest.raises(ValueError, match="patience > 0 needs an eval_mask"):
        fit(patience=2)
    with pytest.raises(ValueError, match="n_gpus > 1 or devices"):
        fit(eval_mask=ev, n_gpus=2)
    with pytest.raises(ValueError, match="n_gpus > 1 or devices"):
        fit(eval_mask=ev, devices=[0])


def test_eval_pairs_are_row_major_in_the_internal_layout():
    import scipy.sparse as sp
    from nbmf_mm_amd._solver import eval_pairs
    X, _, ev = small()
    r, c, x = eval_pairs(X, ev)
    want_r, want_c = np.nonzero(ev)
    assert r.dtype == c.dtype == np.int64 and x.dtype == np.uint8
    assert np.array_equal(r, want_r) and np.array_equal(c, want_c) and np.array_equal(x, X[want_r, want_c].astype(np.uint8))
    # a 0/1 numeric mask and a sparse one mark the same entries, in the same order
    for form in (ev.astype(np.float64), sp.csr_matrix(ev), sp.coo_matrix(ev.astype(np.int8)).tocsc()):
        got = eval_pairs(X, form)
        assert all(np.array_equal(a, b) for a, b in zip(got, (r, c, x)))
    assert all(np.array_equal(a, b) for a, b in zip(eval_pairs(sp.csr_matrix(X), ev), (r, c, x)))
    # dir-beta: the internal matrix is X^T, so the pairs are those of ev^T in ITS row-major order
    rt, ct, xt = eval_pairs(X, ev, orientation="dir-beta")
    want_r, want_c = np.nonzero(ev.T)
    assert np.array_equal(rt, want_r) and np.array_equal(ct, want_c) and np.array_equal(xt, X.T[want_r, want_c].astype(np.uint8))
    assert eval_pairs(X, None) is None


def test_set_eval_refuses_malformed_arrays():
    from nbmf_mm_amd import _hip
    ctx = object.__new__(_hip.Context)
    ctx._lib, ctx._h, ctx.m, ctx.n, ctx.k = _NoDevice(), None, 4, 5, 2
    with pytest.raises(ValueError, match="integer array"):
        ctx.set_eval(np.zeros(3), np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.uint8))
    with pytest.raises(ValueError, match="equally long"):
        ctx.set_eval(np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.int64), np.zeros(3, dtype=np.uint8))
    with pytest.raises(ValueError, match="as long as rows and cols"):
        ctx.set_eval(np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), np.zeros(2, dtype=np.uint8))
    ctx._h = None                              # (nothing to destroy)


# ---- the symbols --------------------------------------------------------------------------------------------------------------
NEW = {"nbmf_set_eval": 7, "nbmf_eval_loglik": 2, "nbmf_get_eval": 7, "nbmf_get_best_factors": 3}


def test_symbols_are_declared_and_exported():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbmf_hip.h")).read()
    for name, nargs in NEW.items():
        assert name in _hip.SYMBOLS
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs
        assert f"int {name}(nbmf_ctx* ctx" in header
    assert "int nbmf_set_eval(nbmf_ctx* ctx, const int64_t* rows, const int64_t* cols, const uint8_t* x, int64_t count," in header
    assert lib.nbmf_abi_version() == 4
    for method in ("set_eval", "eval_loglik", "eval_curve", "best_factors"):
        assert callable(getattr(_hip.Context, method))


def test_null_context_is_an_argument_error():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    v = ctypes.c_double(-7.25)
    assert lib.nbmf_set_eval(None, None, None, None, 0, 1, 0) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    assert lib.nbmf_eval_loglik(None, ctypes.byref(v)) == _hip.NBMF_ERR_ARG and v.value == -7.25
    assert lib.nbmf_get_eval(None, 0, None, None, None, None, None) == _hip.NBMF_ERR_ARG
    assert lib.nbmf_get_best_factors(None, None, None) == _hip.NBMF_ERR_ARG
