"""GPU parity from transform()'s UN-NORMALISED start, W ~ U(0.1, 0.9) (tests/transform_start.py): Theta = W H stands far
above 1 on the first W-only step, the ratios (1 - Y) / (1 - Theta + eps) are negative and the W sweep must run its select
(TINY) variant -- at every K layout, in the sliced sweeps above 128 components and on all three storage paths -- then switch
back to the plain / two-state variant once ``nbmf_w_only_steps`` has seen the factors in range.

  A  one step from the oracle's own state, steps 0-2, every entry of every row against ``transform_start.step_bound``;
  B  the chained loop on binary data, 1e-9 on ALL rows, with the launch counters showing which variant served;
  C  the estimator's transform / score / perplexity from the seeded global draw, both orientations, dense and CSR.

tests/test_transform_start_cpu.py shows on the CPU that the oracle is well conditioned wherever a kernel is held to it here
(float64 against long double: at most a tenth of every bound) and that the sweeps' plain variant misses the bound of A by
more than 1000 x.
"""
import os

import numpy as np
import pytest

import transform_start as ts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


def _check_steps(hip, k, cid, tag):
    c = ts.config(cid)
    X, mask, H, _ = ts.problem(k, cid)
    states = ts.a_states(k, cid)
    worst = 0.0
    with hip.Context(ts.M, ts.N, k) as ctx:
        ctx.set_hyper(1.2, 1.2, ts.EPS)
        ctx.set_storage(c.storage)
        assert ctx.upload(X, mask=mask) == c.binary_path
        for j in range(ts.A_STEPS):
            ctx.set_factors(np.ascontiguousarray(states[j].T), H)
            ctx.w_only_steps(1)
            Wk, Hk = ctx.get_factors()
            np.testing.assert_array_equal(Hk, H)
            ratio = np.abs(Wk.T - states[j + 1]) / ts.step_bound(states[j + 1])
            print(tag, k, cid, "step", j, "largest deviation %.3f of the bound" % np.nanmax(ratio))
            assert np.isfinite(Wk).all(), f"step {j}"
            assert (ratio <= 1.0).all(), f"step {j}: {np.max(ratio):.3g} of the bound at row {int(np.argmax(ratio.max(axis=1)))}"
            worst = max(worst, float(ratio.max()))
    print(tag, k, cid, "worst %.3f of the bound" % worst)


@pytest.mark.parametrize("k,cid", ts.A_CASES, ids=lambda v: str(v))
def test_one_step_from_the_unnormalised_start(hip, k, cid):
    """One context; before each of three steps the oracle's float64 state goes in (step 0: W0 itself), ``w_only_steps(1)``
    runs -- always in the select variant -- and every entry of every row must stand within the bound of the oracle's step
    from that same state; H comes back bit for bit."""
    _check_steps(hip, k, cid, "A")


@pytest.mark.parametrize("k,cid", ts.NAMED_CASES, ids=lambda v: str(v))
def test_real_valued_observed_zeros_keep_their_sign_above_theta_1(hip, k, cid):
    """What the step cases found, at its smallest: real-valued data on the 8-byte path without weight tiles (bool mask
    folded in, or no mask).  Its W sweep formed (1 - y) / (1 - Theta + eps) as max(it2 - y it2, 0), the max being there to
    turn an unobserved entry's NaN into the zero the reference has -- and with it every NEGATIVE quotient, which is every
    observed entry's once Theta stands above 1 + eps: the step from transform's start came out as W * S1 instead of
    W * (S1 - S2), 1e9 ... 1e11 bounds away (1e-2 absolute), in every layout; byte codes and weight tiles were right.  The
    select variant now clips 1 - y and keeps the quotient's sign."""
    _check_steps(hip, k, cid, "named")


_loops = {}


def _device_loop(hip, k, lid):
    """Each loop case runs once per session; the variant comparison below reads the same results."""
    if (k, lid) not in _loops:
        _loops[k, lid] = ts.device_loop(hip, k, lid)
    return _loops[k, lid]


@pytest.mark.parametrize("k,lid", ts.B_CASES, ids=lambda v: str(v))
def test_loop_from_the_unnormalised_start(hip, k, lid):
    """``w_only_steps(50)`` from W0 against 50 oracle steps: 1e-9 on ALL rows.  Which variant served shows in the launch
    counters: after step 0 the range check finds the factors in range, so steps 1-49 run the two-state W sweep on data
    observed everywhere (one layout's worth of components: the sliced sweeps of K > 128 have no such form and must not count
    one) and the ragged-K variant at K = 17 and 40 -- neither exists in the select variant; a row observed nowhere is NaN
    from step 0 on, which the range check sees, and ``w_only_steps(2)`` makes no check: both stay in the select variant."""
    lp = ts.LOOPS[lid]
    want, _ = ts.loop_reference(k, lid)
    W, Hk, full_w, ragged = _device_loop(hip, k, lid)
    H = ts.problem(k, lp.config, lp.n, lp.dead_row)[2]
    np.testing.assert_array_equal(Hk, H)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(W), nan), "NaN pattern"
    if lp.dead_row is None:
        assert not nan.any()
    else:
        assert nan[lp.dead_row].all() and nan.sum() == k
    dev = float(np.max(np.abs(W - want)[~nan]))
    print("B", k, lid, "largest deviation %.3e = %.2e of the bound; full-W launches %d, ragged-K launches %d"
          % (dev, dev / ts.FACTOR_ATOL, full_w, ragged))
    assert dev <= ts.FACTOR_ATOL
    live = ~nan.any(axis=1)
    assert (W[live] >= 0).all() and np.max(np.abs(W[live].sum(axis=1) - 1.0)) <= 1e-12
    back_in_range = lp.steps > 2 and lp.dead_row is None
    after_first = lp.steps - 1 if back_in_range else 0
    two_state = lid in ts.UNMASKED_LOOPS and k <= 128
    assert full_w == (after_first if two_state else 0)
    if k in (17, 40):                         # 17 in the K = 32 layout, 40 in the K = 64 one
        assert ragged == after_first


_NO_FULL_W_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import transform_start as ts
from nbmf_mm_amd import _hip
out = {}
for k in ts.B_KS:
    for lid in ts.UNMASKED_LOOPS:
        W, _, full_w, _ = ts.device_loop(_hip, k, lid)
        assert full_w == 0, (k, lid, full_w)
        out["%d %s" % (k, lid)] = W
np.savez(sys.argv[2], **out)
"""


def test_loop_on_the_three_state_sweep_gives_the_same(hip, tmp_path):
    """The unmasked loops once more with NBMF_NO_FULL_W=1 -- the three-state kernels from step 1 on (the switch is read once
    per process, hence a child process): the same W to 1e-12, and still within 1e-9 of the oracle."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path / "three_state.npz")
    env = dict(os.environ, NBMF_NO_FULL_W="1")
    r = subprocess.run([sys.executable, "-c", _NO_FULL_W_SCRIPT, root, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    three = np.load(path)
    assert len(three.files) == len(ts.B_KS) * len(ts.UNMASKED_LOOPS)
    for k in ts.B_KS:
        for lid in ts.UNMASKED_LOOPS:
            W = _device_loop(hip, k, lid)[0]
            W3 = three["%d %s" % (k, lid)]
            print("B", k, lid, "two-state against three-state: %.3e" % np.max(np.abs(W - W3)))
            np.testing.assert_allclose(W3, W, rtol=0, atol=1e-12, err_msg=f"{k} {lid}")
            np.testing.assert_allclose(W3, ts.loop_reference(k, lid)[0], rtol=0, atol=ts.FACTOR_ATOL, err_msg=f"{k} {lid}")


@pytest.mark.parametrize("k,orientation,storage", ts.C_CASES, ids=lambda v: str(v))
def test_estimator_from_the_seeded_draw(hip, k, orientation, storage):
    """A model fitted for a few iterations, then ``np.random.seed(s)`` before each call: ``transform(X)`` and
    ``transform(X, mask)`` against ``orc.w_only_transform`` under the same seed on the model's own components -- 1e-9 on ALL
    rows, row sums 1 to 1e-12 --, ``score(X, mask)`` against ``orc.score`` on the oracle's UNMASKED transform to 1e-10
    relative, ``perplexity`` = exp(-score) likewise.  CSR: data and mask go up as sparse patterns."""
    from nbmf_mm_amd import NBMF
    X, mask = ts.estimator_data(k)
    Xin, maskin = X, mask
    if storage == "csr":
        import scipy.sparse as sp
        Xin, maskin = sp.csr_matrix(X), sp.csr_matrix(mask.astype(np.float64))
    mdl = NBMF(n_components=k, orientation=orientation, random_state=ts.C_FIT_SEED, max_iter=ts.C_FIT_ITERS, tol=0)
    mdl.fit(Xin, mask=maskin)
    H = np.array(mdl.components_)
    assert H.shape == (k, ts.N) and mdl.n_iter_ == ts.C_FIT_ITERS
    np.testing.assert_allclose(H, ts.oracle_components(k, orientation), rtol=0, atol=ts.FACTOR_ATOL)
    W_plain, W_masked, score, positive = ts.estimator_reference(X, H, mask)
    assert positive                           # (the CPU gate, on the components this model actually has)
    for name, want, kw in (("transform(X)", W_plain, {}), ("transform(X, mask)", W_masked, {"mask": maskin})):
        np.random.seed(ts.C_DRAW_SEED)
        got = mdl.transform(Xin, **kw)
        dev = float(np.max(np.abs(got - want)))
        print("C", k, orientation, storage, name, "largest deviation %.3e = %.2e of the bound" % (dev, dev / ts.FACTOR_ATOL))
        assert got.shape == (ts.M, k) and np.isfinite(got).all()
        assert dev <= ts.FACTOR_ATOL
        assert np.max(np.abs(got.sum(axis=1) - 1.0)) <= 1e-12
    np.random.seed(ts.C_DRAW_SEED)
    got = mdl.score(Xin, mask=maskin)
    assert isinstance(got, float)
    print("C", k, orientation, storage, "score %.17g, oracle %.17g: %.2e of the bound"
          % (got, score, abs(got - score) / (ts.LOSS_RTOL * abs(score))))
    assert abs(got - score) <= ts.LOSS_RTOL * abs(score)
    np.random.seed(ts.C_DRAW_SEED)
    got = mdl.perplexity(Xin, mask=maskin)
    print("C", k, orientation, storage, "perplexity: %.2e of the bound" % (abs(got - np.exp(-score)) / (ts.LOSS_RTOL * np.exp(-score))))
    assert abs(got - np.exp(-score)) <= ts.LOSS_RTOL * np.exp(-score)
