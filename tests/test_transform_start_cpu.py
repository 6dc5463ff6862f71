"""The cases of tests/transform_start.py, on the CPU: the conditions that keep the GPU comparisons honest.  Each case IS off
the simplex where it claims to be (Theta above 1 on step 0, non-positive entries later for real-valued data), the float64
oracle is well conditioned where a kernel is held to it (against the same arithmetic in long double: at most a tenth of every
bound), and the bound bites: the sweeps' plain variant, which a wrong dispatch would run, misses it by three orders of
magnitude.  A case that missed a condition would get another seed or shape -- never a wider tolerance or a row left out.
No GPU.
"""
import numpy as np
import pytest

import planted as pl
import transform_start as ts
from oracle import nbmf_oracle as orc

needs_long_double = pytest.mark.skipif(not pl.have_long_double(), reason="np.longdouble is no wider than float64 here")
L = np.longdouble
STEP_CASES = ts.A_CASES + tuple(c for c in ts.NAMED_CASES if c not in ts.A_CASES)


def test_cases_are_the_stated_ones():
    assert len(ts.A_CASES) == 54 and len(set(ts.A_CASES)) == 54
    for cid, c in ts.CONFIGS.items():
        X, mask, H, W0 = ts.problem(64, cid)
        assert X.shape == (ts.M, ts.N) and H.shape == (64, ts.N) and W0.shape == (ts.M, 64)
        assert (set(np.unique(X)) == {0.0, 1.0}) == (c.data == "binary")
        assert 0.0 <= X.min() and X.max() <= 1.0
        assert 0.02 <= H.min() and H.max() <= 0.98 and 0.1 <= W0.min() and W0.max() <= 0.9
        if c.mask == "bool":
            assert mask.dtype == np.bool_ and mask.mean() == pytest.approx(ts.OBSERVED_SHARE, abs=0.02)
        elif c.mask == "weights":
            assert mask.dtype == np.float64 and 0.05 < mask.min() and mask.max() <= 1.0 and len(np.unique(mask)) > 1000
        else:
            assert mask is None
        if c.data == "binary":
            assert X.mean() == pytest.approx(ts.ONES_SHARE, abs=0.02)
        assert np.array_equal(X, ts.problem(64, cid)[0]) and not X.flags.writeable
    X, mask, _, _ = ts.problem(17, "binary-mask", ts.N, 37)
    assert not mask[37].any() and mask[36].any() and mask[38].any()
    assert ts.problem(17, "binary", ts.N_NO_PAD)[0].shape == (ts.M, ts.N_NO_PAD)
    # the oracle's step here is the one the suite already compares with (orc.w_only_transform minus its final clip)
    X, mask, H, W0 = ts.problem(24, "binary-mask")
    W = W0
    for _ in range(4):
        W = ts.w_step(X, H, ts.as_float(mask), W)
    want = orc.w_only_transform(X, H, ts.as_float(mask), W0=W0, n_iter=4)
    Wc = np.clip(W, 1e-8, 1.0)
    np.testing.assert_array_equal(Wc / Wc.sum(axis=1, keepdims=True), want)


@pytest.mark.parametrize("k,cid", STEP_CASES, ids=lambda v: str(v))
def test_step_cases_start_off_the_simplex(k, cid):
    """Step 0 of every case has Theta above 1 (so its ratios are negative); the real-valued cases are still off at step 1 or
    2 (a non-positive entry in the state the step starts from), the binary ones at 17 <= K <= 130 -- the range of the loop
    and estimator cases -- are back in range at step 1 (at K = 300 the unmasked case keeps an entry of -6e-4)."""
    states = ts.a_states(k, cid)
    t0 = ts.theta_max(k, cid, 0)
    print(k, cid, "Theta max at steps 0-2: %.3g %.3g %.3g" % tuple(ts.theta_max(k, cid, j) for j in range(3)),
          "| smallest entry of states 1, 2: %.3g %.3g" % (states[1].min(), states[2].min()),
          "| largest |entry| of states 1-3: %.3g" % max(np.abs(s).max() for s in states[1:]))
    assert t0 > 1.0
    assert all(np.isfinite(s).all() for s in states)
    if ts.config(cid).data == "real":
        assert min(states[1].min(), states[2].min()) <= 0.0
    elif 17 <= k <= 130:
        _, _, H, _ = ts.problem(k, cid)
        for s in states[1:]:
            assert (s > 0).all() and (s @ H).max() < 1.0


@needs_long_double
@pytest.mark.parametrize("k,cid", STEP_CASES, ids=lambda v: str(v))
def test_one_step_is_well_conditioned_and_the_plain_variant_misses_it(k, cid):
    """From each of the three float64 states: the step in long double stands within 0.1 of ``step_bound`` of the float64
    step on EVERY row; and the same step with the plain variant's |Theta - z| denominators misses the bound by at least
    1000 x at step 0 -- a W sweep dispatched to the wrong variant cannot pass."""
    X, mask, H, _ = ts.problem(k, cid)
    states = ts.a_states(k, cid)
    maskf, Xl, Hl, maskl = ts.as_float(mask), X.astype(L), H.astype(L), ts.as_float(mask, L)
    worst = 0.0
    for j in range(ts.A_STEPS):
        bound = ts.step_bound(states[j + 1])
        ext = ts.w_step(Xl, Hl, maskl, states[j].astype(L))
        gap = float(np.max(np.abs(ext - states[j + 1]) / bound))
        worst = max(worst, gap)
        assert gap <= 0.1, f"step {j}: float64 / long double gap is {gap:.3f} of the bound"
    with np.errstate(all="ignore"):
        plain = ts.w_step(X, H, maskf, states[0], denominators="plain")
    miss = float(np.max(np.abs(plain - states[1]) / ts.step_bound(states[1])))
    print(k, cid, "gap %.3f of the bound; the plain variant misses it by %.3g x" % (worst, miss))
    assert miss >= 1000.0


@needs_long_double
@pytest.mark.parametrize("k,lid", ts.B_CASES, ids=lambda v: str(v))
def test_loop_is_stable_on_binary_data(k, lid):
    """Binary data, K >= 17: every row is positive with Theta < 1 from the first step on (except a row observed nowhere,
    NaN in both) and float64 and long double end within 1e-10 of each other -- a tenth of the 1e-9 a kernel is held to."""
    lp = ts.LOOPS[lid]
    W, positive = ts.loop_reference(k, lid)
    ext = ts.loop_extended(k, lid)
    assert positive
    nan = np.isnan(W)
    assert np.array_equal(nan, np.isnan(ext.astype(np.float64)))
    if lp.dead_row is None:
        assert not nan.any()
    else:
        assert nan[lp.dead_row].all() and nan.sum() == k
    gap = float(np.max(np.abs(ext - W)[~nan]))
    print(k, lid, "end gap %.2e" % gap)
    assert gap <= ts.FACTOR_ATOL / 10
    assert np.max(np.abs(W[~nan.any(axis=1)].sum(axis=1) - 1.0)) <= 1e-12


@needs_long_double
@pytest.mark.parametrize("k", ts.C_KS)
@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_estimator_calls_are_stable(k, orientation):
    """transform(X), transform(X, mask) and score(X, mask) from the seeded global draw, on the oracle's fitted components:
    positive from the first step, both transforms within 1e-10 of their long-double evaluation, the score within 1e-11
    relative."""
    X, mask = ts.estimator_data(k)
    H = ts.oracle_components(k, orientation)
    Wp, Wm, sc, ok = ts.estimator_reference(X, H, mask)
    Wpx, Wmx, scx, _ = ts.estimator_reference(X, H, mask, dtype=L)
    gaps = (float(np.max(np.abs(Wpx - Wp))), float(np.max(np.abs(Wmx - Wm))), float(abs(scx - sc) / abs(sc)))
    print(k, orientation, "transform gaps %.2e (plain) %.2e (masked), score gap %.2e relative" % gaps)
    assert ok and np.isfinite(Wp).all() and np.isfinite(Wm).all() and np.isfinite(sc)
    assert gaps[0] <= ts.FACTOR_ATOL / 10 and gaps[1] <= ts.FACTOR_ATOL / 10
    assert gaps[2] <= ts.LOSS_RTOL / 10
