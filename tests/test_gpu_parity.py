"""GPU parity: libnbmf_hip (through the C ABI) against the CPU oracle and the reference's golden
vectors, same seeded inputs.  Tolerances: loss curve <= 1e-10 relative per point,
factors <= 1e-9 absolute, final NLL <= 1e-8 relative (north star), monotone within 1e-12.
"""
import os

import numpy as np
import pytest

from conftest import config1_X, config1_mask, midsize_XM, rank_threads_fit_on_one_gpu
from oracle import nbmf_oracle as orc

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-10
FACTOR_ATOL = 1e-9


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


def _one_step(hip, Y, W, H, mask, al, be, projection=0):
    k, m = W.shape
    n = H.shape[1]
    with hip.Context(m, n, k) as ctx:
        ctx.set_hyper(al, be, 1e-8, projection)
        ctx.upload(Y, mask=mask)
        ctx.set_factors(W, H)
        losses, n_iter = ctx.run(1, 0.0)
        Wn, Hn = ctx.get_factors()
        return Wn, Hn, losses[0], ctx.binary_path


def test_reciprocal_accuracy(hip):
    # Newton reciprocal used on the binary path: <= 1 ulp of the IEEE quotient over the denominator
    # range [eps, 1+eps] (log-uniform), plus negative / >1 denominators that transform() can produce
    r = np.random.default_rng(0)
    d = np.concatenate([np.exp(r.uniform(np.log(1e-8), 0.0, 1 << 20)) + 1e-8, -r.uniform(1e-8, 3.0, 1 << 16),
                        r.uniform(1.0, 50.0, 1 << 16), [1e-8, 1.0 + 1e-8, 2e-8]])
    got = hip.selftest_unary(0, d)
    want = 1.0 / d
    ulp = np.abs(got - want) / np.spacing(np.abs(want))
    assert ulp.max() <= 1.0, ulp.max()
    assert (ulp == 0).mean() > 0.9


def test_quotient_accuracy(hip):
    # quotient of the general (real-valued / weighted) path: numerator times the Newton reciprocal -- two roundings,
    # so within 1.5 ulp of the IEEE quotient and the correctly rounded one for most arguments; exact zeros stay exact
    r = np.random.default_rng(2)
    d = np.concatenate([np.exp(r.uniform(np.log(1e-8), 0.0, 1 << 20)) + 1e-8, r.uniform(0.0, 1.0, 1 << 18) + 1e-8,
                        [1e-8, 1.0 + 1e-8, 0.5, 4.0 / 3.0]])
    got = hip.selftest_unary(2, d)
    want = (1.0 - 0.75 * d) / d
    ulp = np.abs(got - want) / np.maximum(np.spacing(np.abs(want)), 5e-324)
    assert ulp.max() <= 1.5, ulp.max()
    assert (ulp == 0).mean() > 0.6
    assert hip.selftest_unary(2, np.array([4.0 / 3.0]))[0] == 0.0


def test_shared_reciprocal_accuracy(hip):
    """The product sweeps take several quotients from ONE reciprocal: the binary path the four reciprocals of
    a lane's entries from that of their product, the general path the two quotients of an entry from the reciprocal
    of the product of their denominators.  A few more roundings than a reciprocal of its own: within 3 ulp."""
    r = np.random.default_rng(4)
    d = np.concatenate([np.exp(r.uniform(np.log(1e-8), 0.0, 1 << 20)) + 1e-8, r.uniform(0.0, 1.0, 1 << 18) + 1e-8])
    d = d[: len(d) // 4 * 4]
    got = hip.selftest_unary(5, d)                      # groups of four consecutive arguments share a reciprocal
    ulp = np.abs(got - 1.0 / d) / np.spacing(1.0 / d)
    assert ulp.max() <= 3.0, ulp.max()
    t2 = (1.0 - (d - 1e-8)) + 1e-8
    for op, want in ((3, (1.0 - 0.75 * d) / d), (4, (0.75 * d) / t2)):
        got = hip.selftest_unary(op, d)
        ulp = np.abs(got - want) / np.maximum(np.spacing(np.abs(want)), 5e-324)
        assert ulp.max() <= 3.0, (op, ulp.max())


@pytest.mark.parametrize("op", [1, 6, 7], ids=["256-entries-degree-5", "1024-entries-degree-4", "table-free-for-the-running-product"])
def test_log_accuracy(hip, op):
    # logarithm of the general path (table + series; the product sweeps use the 1024-entry table, whose series is a term
    # shorter, on t1 / t2 in [1e-8, 1e8]): absolute error <= 2.5e-16 + 1 ulp of the result -- the loss sums millions of
    # such terms of size ~0.5 -- and the same special values as NumPy elsewhere
    r = np.random.default_rng(1)
    x = np.concatenate([np.exp(r.uniform(np.log(1e-8), np.log(2.0), 1 << 20)), r.uniform(0.5, 1.5, 1 << 18),
                        np.exp(r.uniform(np.log(1e-8), np.log(1e8), 1 << 20)),
                        1.0 + r.uniform(-1e-6, 1e-6, 1 << 16),
                        [1.0, 1e-8, 1.0 + 1e-8, 0.5, 2.0, np.nextafter(1.0, 0), np.nextafter(1.0, 2), 1e-300, 1e300]])
    got = hip.selftest_unary(op, x)
    want = np.log(x)
    err = np.abs(got - want)
    assert (err <= 2.5e-16 + np.spacing(np.abs(want))).all(), (err - np.spacing(np.abs(want))).max()
    with np.errstate(all="ignore"):
        sp = np.array([0.0, -1.0, np.inf, np.nan, 5e-324, -0.0, -np.inf])
        np.testing.assert_array_equal(hip.selftest_unary(op, sp), np.log(sp))


def test_one_step_golden_vectors(hip, golden, both_small_paths):
    g = golden("one_step")
    for i in range(int(g["n_cases"])):
        p = f"c{i}_"
        mask = g[p + "mask"]
        mask = None if mask.size == 0 else mask
        al, be = g[p + "ab"]
        Wn, Hn, loss, binpath = _one_step(hip, g[p + "Y"], g[p + "W"], g[p + "H"], mask, al, be)
        np.testing.assert_allclose(Hn, g[p + "H_new"], rtol=0, atol=1e-13, err_msg=f"case {i} H")
        np.testing.assert_allclose(Wn, g[p + "W_new"], rtol=0, atol=1e-13, err_msg=f"case {i} W")
        ref_loss = orc.mm_loss(g[p + "Y"], g[p + "W_new"], g[p + "H_new"], mask, al, be)
        assert abs(loss - ref_loss) <= 1e-12 * abs(ref_loss), f"case {i} loss"
        assert binpath == (i < 18)          # the last vector is real-valued with a weight mask


def test_column_without_an_observed_one_under_a_flat_prior(hip, both_small_paths):
    """alpha = 1 (a = 0) and a column of V with no observed one: the reference's numerator H * P1 + a is an exact 0 there
    and its update lands on the lower clip, eps.  The binary path's H sweep leaves P1 as a DIFFERENCE of all-entry sums
    (P1' - P2' / (1 + 2 eps), round 4) -- a rounding residue of either sign instead of the exact 0 -- which the clip to
    [eps, 1 - eps] must absorb: the same H', to 1e-13 everywhere and exactly eps in that column, masked and not."""
    g = np.random.default_rng(12)
    m, n, k = 96, 70, 7
    Y = (g.random((m, n)) < 0.3).astype(np.float64)
    Y[:, 5] = 0.0                                   # nobody has a one here
    Y[:, 11] = 0.0
    W = g.uniform(0.1, 0.9, (k, m))
    W /= W.sum(axis=0, keepdims=True)
    H = g.uniform(0.1, 0.9, (k, n))
    for mask in (None, g.random((m, n)) < 0.8):
        Wn, Hn, loss, binpath = _one_step(hip, Y, W, H, mask, 1.0, 1.3)
        Wr, Hr = orc.mm_step(Y, W, H, None if mask is None else mask.astype(np.float64), 1.0, 1.3)
        assert binpath
        np.testing.assert_allclose(Hn, Hr, rtol=0, atol=1e-13)
        np.testing.assert_allclose(Wn, Wr, rtol=0, atol=1e-13)
        assert (Hr[:, [5, 11]] == 1e-8).all() and (Hn[:, [5, 11]] == 1e-8).all()


def test_config1_curve(hip, golden, both_small_paths):
    from nbmf_mm_amd import NBMF
    g = golden("config1")
    mdl = NBMF(n_components=6, orientation="beta-dir", alpha=1.2, beta=1.2, random_state=0,
               max_iter=200, tol=0).fit(config1_X())
    np.testing.assert_allclose(mdl.loss_curve_, g["losses"], rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(mdl.W_, g["W"], rtol=0, atol=FACTOR_ATOL)
    np.testing.assert_allclose(mdl.components_, g["H"], rtol=0, atol=FACTOR_ATOL)
    assert mdl.n_iter_ == 200 and len(mdl.loss_curve_) == 200
    # default stop rule: same iteration count and loss as the reference
    mdl = NBMF(n_components=6, random_state=0).fit(config1_X())
    assert mdl.n_iter_ == int(g["default_n_iter"])
    assert abs(mdl.loss_ - float(g["default_loss"])) <= 1e-10 * float(g["default_loss"])
    # both fits qualify for the single-launch engine: the engine this case names served them, the other none
    assert both_small_paths.served() == ((2, 0, 0) if both_small_paths == "single-launch" else (0, 0, 2))


def test_dir_beta(hip, golden, both_small_paths):
    from nbmf_mm_amd import NBMF
    g = golden("dir_beta")
    X = config1_X()
    mdl = NBMF(n_components=6, orientation="dir-beta", random_state=0, max_iter=50, tol=0).fit(X)
    np.testing.assert_allclose(mdl.loss_curve_, g["losses"], rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(mdl.W_, g["W"], rtol=0, atol=FACTOR_ATOL)
    np.testing.assert_allclose(mdl.components_, g["H"], rtol=0, atol=FACTOR_ATOL)
    # the transpose identity is bitwise: dir-beta(X).W_ == beta-dir(X.T).components_.T
    mdlT = NBMF(n_components=6, orientation="beta-dir", random_state=0, max_iter=50, tol=0).fit(X.T)
    np.testing.assert_array_equal(mdl.W_, mdlT.components_.T)
    np.testing.assert_array_equal(mdl.loss_curve_, mdlT.loss_curve_)


def test_masked_float_and_bool(hip, golden, both_small_paths):
    from nbmf_mm_amd import NBMF
    g = golden("masked")
    X, mask = config1_X(), config1_mask()
    curves = []
    for mk, key in [(mask.astype(np.float64), "losses_float"), (mask, "losses_bool")]:
        mdl = NBMF(n_components=6, random_state=0, max_iter=100, tol=0).fit(X, mask=mk)
        np.testing.assert_allclose(mdl.loss_curve_, g[key], rtol=LOSS_RTOL, atol=0)
        curves.append(np.array(mdl.loss_curve_))
    np.testing.assert_array_equal(curves[0], curves[1])
    np.testing.assert_allclose(mdl.W_, g["W"], rtol=0, atol=FACTOR_ATOL)
    l = curves[0]
    assert all(l[i] <= l[i - 1] + 1e-12 for i in range(1, len(l)))


def test_real_valued(hip, golden, both_small_paths):
    from nbmf_mm_amd import NBMF
    g = golden("real_valued")
    Xr = np.random.default_rng(3).random((50, 30))
    mdl = NBMF(n_components=5, random_state=1, max_iter=30, tol=0).fit(Xr)
    np.testing.assert_allclose(mdl.loss_curve_, g["losses"], rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(mdl.W_, g["W"], rtol=0, atol=FACTOR_ATOL)
    np.testing.assert_allclose(mdl.components_, g["H"], rtol=0, atol=FACTOR_ATOL)


def test_custom_init_both_orientations(hip, golden, both_small_paths):
    from nbmf_mm_amd import NBMF
    g = golden("custom_init")
    mdl = NBMF(n_components=4, random_state=123, max_iter=50, tol=1e-8, W_init=g["W0"], H_init=g["H0"]).fit(g["Y"])
    assert mdl.n_iter_ == int(g["n_iter"])
    np.testing.assert_allclose(mdl.loss_curve_, g["losses"], rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(mdl.W_, g["W"], rtol=0, atol=FACTOR_ATOL)
    mdl = NBMF(n_components=4, orientation="dir-beta", random_state=123, max_iter=20, tol=0,
               W_init=g["Wd0"], H_init=g["Hd0"]).fit(g["Y"])
    np.testing.assert_allclose(mdl.loss_curve_, g["d_losses"], rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(mdl.W_, g["dW"], rtol=0, atol=FACTOR_ATOL)
    np.testing.assert_allclose(mdl.components_, g["dH"], rtol=0, atol=FACTOR_ATOL)
    with pytest.raises(ValueError):     # only one init under dir-beta on non-square V
        NBMF(n_components=4, orientation="dir-beta", max_iter=2, W_init=g["Wd0"]).fit(g["Y"])


def test_stop_rule_counts(hip, golden, both_small_paths):
    from nbmf_mm_amd import NBMF
    g = golden("stop_rule")
    hi = NBMF(n_components=5, tol=0.1, max_iter=1000, random_state=42).fit(g["X"])
    lo = NBMF(n_components=5, tol=1e-8, max_iter=1000, random_state=42).fit(g["X"])
    assert hi.n_iter_ == int(g["n_iter_hi"]) and lo.n_iter_ == int(g["n_iter_lo"])
    assert len(lo.loss_curve_) == lo.n_iter_
    np.testing.assert_allclose(lo.loss_curve_, g["losses_lo"], rtol=LOSS_RTOL, atol=0)


def _oracle_w_step(X, H, mask, W):
    """One iteration of the transform loop (src/nbmf_mm/_base.py:180-193), no final clip."""
    Wt = W.T
    th = H.T @ Wt
    Wt = Wt * (H @ ((X.T * mask.T) / (th + 1e-8)) + (1 - H) @ (((1 - X).T * mask.T) / (1 - th + 1e-8)))
    Wt = Wt / X.shape[1]
    Wt = Wt / Wt.sum(axis=0, keepdims=True)
    return Wt.T


def test_transform_score_perplexity(hip, golden):
    from nbmf_mm_amd import NBMF
    g = golden("transform")
    X, mask = config1_X(), config1_mask()
    mdl = NBMF(n_components=6, random_state=0, max_iter=60, tol=0).fit(X, mask=mask)
    np.testing.assert_allclose(mdl.components_, g["H"], rtol=0, atol=FACTOR_ATOL)
    mdl.components_ = g["H"]            # continue from the reference's H so only transform is compared
    Xn = (np.random.default_rng(9).random((10, 500)) < 0.25).astype(np.float64)
    np.random.seed(5)
    np.testing.assert_allclose(mdl.transform(Xn), g["W_new"], rtol=0, atol=FACTOR_ATOL)
    # Masked transform: the reference starts from an UN-normalised W ~ U(0.1,0.9) (_base.py:175), so
    # W@H can exceed 1 on the first steps, ratios turn negative and a few rows follow a chaotic
    # trajectory in the reference itself (rounding-level differences grow to O(1)).  Parity is
    # therefore asserted (a) on every row that stays positive in the oracle and (b) step by step
    # from identical states on ALL rows.
    maskf = mask.astype(np.float64)
    np.random.seed(5)
    W0 = np.random.uniform(0.1, 0.9, (100, 6))
    stable = np.ones(100, dtype=bool)
    Wr = W0
    for _ in range(50):
        Wr = _oracle_w_step(X, g["H"], maskf, Wr)
        stable &= (Wr > 0).all(axis=1)
    assert stable.sum() >= 90
    np.random.seed(5)
    got = mdl.transform(X, mask=maskf)
    np.testing.assert_allclose(got[stable], g["W_masked"][stable], rtol=0, atol=FACTOR_ATOL)
    np.testing.assert_allclose(got.sum(axis=1), 1.0, atol=1e-12)
    Wr = W0
    with hip.Context(100, 500, 6) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X, mask=maskf)
        for _ in range(8):
            ctx.set_factors(np.ascontiguousarray(Wr.T), g["H"])
            ctx.w_only_steps(1)
            Wk, _ = ctx.get_factors()
            Wr = _oracle_w_step(X, g["H"], maskf, Wr)
            # a row whose column-sum nearly cancels amplifies rounding: scale the bound by its magnitude
            bound = 1e-11 * np.maximum(1.0, np.abs(Wr).max(axis=1, keepdims=True)) ** 2
            assert (np.abs(Wk.T - Wr) <= bound).all()
    # score/perplexity: the inner transform is UNMASKED and from the same un-normalised start, so a few rows are chaotic
    # in the reference itself -- tests/test_oracle_golden.py::test_transform_start_is_chaotic_on_a_few_rows moves the
    # reference's own start by one ulp and sees its score move by 1.5e-3 ... 4e-3 -- which is what bounds the END-TO-END
    # comparison at 5e-3.  On the rows that stay positive the same test finds the reference stable to 1e-12, and there
    # the device meets it: their transform to 1e-9 and THEIR share of the score to 1e-10.
    np.random.seed(6)
    sc = mdl.score(X, mask=maskf)
    assert isinstance(sc, float)
    assert abs(sc - float(g["score"])) <= 5e-3 * abs(float(g["score"]))
    np.random.seed(6)
    W0s = np.random.uniform(0.1, 0.9, (100, 6))
    Wo, keep = orc.w_only_transform(X, g["H"], W0=W0s, track_positive=True)
    assert 90 <= keep.sum() < 100
    np.random.seed(6)
    Wg = mdl.transform(X)                                  # what score() runs inside: no mask (_base.py:235)
    np.testing.assert_allclose(Wg[keep], Wo[keep], rtol=0, atol=FACTOR_ATOL)
    with hip.Context(int(keep.sum()), 500, 6) as ctx:      # the stable rows' share of the score, from the DEVICE's transform
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X[keep], mask=maskf[keep])
        ctx.set_factors(np.ascontiguousarray(Wg[keep].T), g["H"])
        dev = ctx.loglik(clip_theta=True) / ctx.n_obs()
    want = orc.score_rows(X, Wo, g["H"], maskf)[keep].sum() / np.count_nonzero(maskf[keep])
    assert abs(dev - want) <= 1e-10 * abs(want)
    np.random.seed(6)
    W_pin = orc.w_only_transform(X, g["H"])
    for mk, key in [(maskf, "score"), (None, "score_nomask")]:
        with hip.Context(100, 500, 6) as ctx:
            ctx.set_hyper(1.2, 1.2)
            ctx.upload(X, mask=mk)
            ctx.set_factors(np.ascontiguousarray(W_pin.T), g["H"])
            dev = ctx.loglik() / ctx.n_obs()
        assert abs(dev - float(g[key])) <= 1e-12 * abs(float(g[key]))
    np.random.seed(6)
    assert abs(mdl.perplexity(X, mask=maskf) - float(g["perplexity"])) <= 5e-3 * float(g["perplexity"])
    # the reference clips W @ H to [0, 1] before the logs (_base.py:210): with components_ pushed outside
    # [0, 1] by hand the clipped device sweep still agrees with the oracle's formula on pinned W
    Hbig = np.clip(g["H"] * 1.6, 0, None)
    with hip.Context(100, 500, 6) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X, mask=maskf)
        ctx.set_factors(np.ascontiguousarray(W_pin.T), Hbig)
        dev = ctx.loglik(clip_theta=True) / ctx.n_obs()
    want = orc.score(X, W_pin, Hbig, maskf)
    assert (W_pin @ Hbig).max() > 1.0 and abs(dev - want) <= 1e-12 * abs(want)


def test_midsize_curves(hip, golden, both_small_paths):
    """512x512 (K=32, 500 its), masked (300 its), dir-beta masked K=64, real-valued weighted K=16."""
    from nbmf_mm_amd import nbmf_mm_solver
    g = golden("midsize")
    X, M = midsize_XM()
    _, _, l, t, n_it = nbmf_mm_solver(X, 32, max_iter=500, tol=0, random_state=0)
    assert t == 0.0 and n_it == 500
    np.testing.assert_allclose(l, g["unmasked"], rtol=LOSS_RTOL, atol=0)
    assert abs(l[-1] - 0.5264565431072413) <= 1e-10
    _, _, l, _, _ = nbmf_mm_solver(X, 32, max_iter=300, tol=0, random_state=0, mask=M)
    np.testing.assert_allclose(l, g["masked"], rtol=LOSS_RTOL, atol=0)
    assert all(l[i] <= l[i - 1] + 1e-12 for i in range(1, len(l)))
    _, _, l, _, _ = nbmf_mm_solver(X[:, :384], 64, max_iter=100, tol=0, random_state=0, orientation="dir-beta",
                                   mask=M[:, :384])
    np.testing.assert_allclose(l, g["dir_beta_masked"], rtol=LOSS_RTOL, atol=0)
    g2 = np.random.default_rng(4)
    Xrv, Wts = g2.random((300, 200)), g2.random((300, 200))
    _, _, l, _, _ = nbmf_mm_solver(Xrv, 16, max_iter=60, tol=0, random_state=2, mask=Wts)
    np.testing.assert_allclose(l, g["real_weighted"], rtol=LOSS_RTOL, atol=0)
    # the K = 64 fit does not qualify for the single-launch engine (K <= 32), the other three do
    assert both_small_paths.served() == ((3, 0, 1) if both_small_paths == "single-launch" else (0, 0, 4))


@pytest.mark.parametrize("m,n,k", [(1, 1, 1), (17, 5, 3), (130, 257, 17), (200, 129, 33), (64, 300, 100),
                                   (129, 128, 128), (16, 16, 16),
                                   (150, 200, 129), (257, 190, 256), (40, 333, 300)])   # > 128: slices sharing a stored Theta
def test_ragged_shapes_vs_oracle(hip, m, n, k, both_small_paths):
    """Edge shapes: not multiples of the 16x16 tile or the 128 padding; every K template."""
    r = np.random.default_rng(m * 1000 + n)
    Y = (r.random((m, n)) < 0.4).astype(np.float64)
    mask = (r.random((m, n)) < 0.85) if (m + n) % 2 else None
    W0 = r.uniform(0.1, 0.9, (m, k))
    H0 = r.uniform(0.1, 0.9, (k, n))
    from nbmf_mm_amd import nbmf_mm_solver
    W, H, l, _, _ = nbmf_mm_solver(Y, k, max_iter=12, tol=0, W_init=W0, H_init=H0, mask=mask, alpha=1.3, beta=1.1)
    Wr, Hr, lr, _, _ = orc.solve(Y, k, max_iter=12, tol=0, W_init=W0, H_init=H0, mask=mask, alpha=1.3, beta=1.1)
    np.testing.assert_allclose(l, lr, rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(W, Wr, rtol=0, atol=FACTOR_ATOL)
    np.testing.assert_allclose(H, Hr, rtol=0, atol=FACTOR_ATOL)


@pytest.mark.parametrize("case", ["H_above_1", "H_exactly_1", "tiny_eps", "W_negative", "eps_2e-7", "eps_3e-7", "eps_1e-4", "eps_1e-12"])
def test_factors_out_of_the_fits_range_follow_the_reference(hip, case, both_small_paths):
    """The H sweep's plain variant forms its ratios from |Theta - z|, which is the reference's arithmetic while
    0 <= Theta < 1 -- what a fit keeps once it starts in range.  Starts that are NOT in range (H_init above or at 1: the
    reference uses H_init as given, _solver.py:133; an eps so small that 1 - eps is 1; negative entries) are detected
    when the factors are set and take the variant with the reference's own selects: same losses -- NaNs included,
    where the reference's log meets a negative number -- and same factors as the oracle."""
    from nbmf_mm_amd import nbmf_mm_solver
    r = np.random.default_rng(5)
    m, n, k = 130, 190, 9
    Y = (r.random((m, n)) < 0.4).astype(np.float64)
    mask = r.random((m, n)) < 0.9
    W0 = r.uniform(0.1, 0.9, (m, k))
    H0 = r.uniform(0.1, 0.9, (k, n))
    kw = dict(max_iter=10, tol=0, mask=mask, alpha=1.2, beta=1.3)
    if case == "H_above_1":
        H0 = r.uniform(0.1, 1.6, (k, n))
    elif case == "H_exactly_1":
        H0[r.random((k, n)) < 0.3] = 1.0
    elif case == "tiny_eps":
        kw["eps"] = 1e-30
    elif case.startswith("eps_"):
        # the plain variant's eps range is [1e-12, 2^-22): z = 1 + 2 eps must share its high word with 1.0.  2e-7 is
        # inside, 3e-7 and 1e-4 outside (the select variant), 1e-12 the lower end
        kw["eps"] = float(case[4:])
    else:
        W0[r.random((m, k)) < 0.05] *= -0.2
    with np.errstate(all="ignore"):
        Wr, Hr, lr, _, _ = orc.solve(Y, k, W_init=W0, H_init=H0, **kw)
    W, H, l, _, _ = nbmf_mm_solver(Y, k, W_init=W0, H_init=H0, **kw)
    lr = np.asarray(lr)
    assert np.array_equal(np.isnan(l), np.isnan(lr))
    ok = ~np.isnan(lr)
    np.testing.assert_allclose(np.asarray(l)[ok], lr[ok], rtol=1e-9, atol=0)
    if np.all(np.isfinite(Wr)) and np.all(np.isfinite(Hr)):
        np.testing.assert_allclose(W, Wr, rtol=0, atol=1e-8)
        np.testing.assert_allclose(H, Hr, rtol=0, atol=1e-8)


def test_more_than_128_components(hip):
    """n_components > 128 runs as slices of 128 (Theta kept in memory between the slices' sweeps): every storage
    path, both orientations, the stop rule, transform / score, and the Duchi extension."""
    from nbmf_mm_amd import NBMF, nbmf_mm_solver
    r = np.random.default_rng(77)
    m, n, k = 210, 301, 200
    Y = (r.random((m, n)) < 0.35).astype(np.float64)
    mask = r.random((m, n)) < 0.9
    for kw in [dict(), dict(mask=mask), dict(orientation="dir-beta", mask=mask.astype(np.float64))]:
        W, H, l, _, it = nbmf_mm_solver(Y, k, max_iter=15, tol=0, random_state=3, **kw)
        Wr, Hr, lr, _, _ = orc.solve(Y, k, max_iter=15, tol=0, random_state=3, **kw)
        np.testing.assert_allclose(l, lr, rtol=LOSS_RTOL, atol=0)
        np.testing.assert_allclose(W, Wr, rtol=0, atol=FACTOR_ATOL)
        np.testing.assert_allclose(H, Hr, rtol=0, atol=FACTOR_ATOL)
    # real-valued data with weights (8-byte path)
    Yr, Wt = r.random((m, n)), r.random((m, n))
    W, H, l, _, _ = nbmf_mm_solver(Yr, 130, max_iter=10, tol=0, random_state=1, mask=Wt)
    Wr, Hr, lr, _, _ = orc.solve(Yr, 130, max_iter=10, tol=0, random_state=1, mask=Wt)
    np.testing.assert_allclose(l, lr, rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(H, Hr, rtol=0, atol=FACTOR_ATOL)
    # stop rule, bitwise repeatability, estimator surface
    a = NBMF(n_components=k, random_state=5, max_iter=300, tol=1e-3).fit(Y, mask=mask)
    _, _, lr, _, itr = orc.solve(Y, k, max_iter=300, tol=1e-3, random_state=5, mask=mask)
    assert a.n_iter_ == itr and 2 < itr < 300
    np.testing.assert_allclose(a.loss_curve_, lr, rtol=LOSS_RTOL, atol=0)
    b = NBMF(n_components=k, random_state=5, max_iter=300, tol=1e-3).fit(Y, mask=mask)
    np.testing.assert_array_equal(a.components_, b.components_)
    # evaluation sweeps and the W-only step on pinned factors (transform()'s own un-normalised start is chaotic at a handful
    # of components only; from it, at every layout: tests/test_gpu_transform_start.py)
    maskf = mask.astype(np.float64)
    with hip.Context(m, n, k) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(Y, mask=maskf)
        ctx.set_factors(np.ascontiguousarray(a.W_.T), a.components_)
        want = orc.score(Y, a.W_, a.components_, maskf)
        assert abs(ctx.loglik(clip_theta=True) / ctx.n_obs() - want) <= 1e-12 * abs(want)
        assert abs(ctx.loss() - orc.mm_loss(Y, a.W_.T, a.components_, maskf, 1.2, 1.2)) <= 1e-12
        ctx.w_only_steps(2)
        Wk, _ = ctx.get_factors()
    # strictly masked held-out log-likelihood (examples/reproduce_magron2022.py:40-47) through the slices
    from nbmf_mm_amd.experiments import heldout_perplexity
    held = ~mask
    with hip.Context(m, n, k) as ev:
        ev.set_hyper(1.0, 1.0)
        ev.upload(Y, mask=held)
        got = heldout_perplexity(ev, np.ascontiguousarray(a.W_.T), a.components_)
    want = orc.heldout_perplexity(Y, a.W_ @ a.components_, held.astype(np.float64))
    assert abs(got - want) <= 1e-12 * want
    Wr = _oracle_w_step(Y, a.components_, maskf, _oracle_w_step(Y, a.components_, maskf, a.W_))
    np.testing.assert_allclose(Wk.T, Wr, rtol=0, atol=1e-11)
    assert isinstance(a.score(Y, mask=mask), float) and a.transform(Y[:40]).shape == (40, k)
    d = NBMF(n_components=k, random_state=5, max_iter=12, tol=0, projection="duchi").fit(Y, mask=mask)
    _, _, ld, _, _ = orc.solve(Y, k, max_iter=12, tol=0, random_state=5, mask=mask, step=orc.mm_step_duchi)
    np.testing.assert_allclose(d.loss_curve_, ld, rtol=1e-9, atol=0)
    np.testing.assert_allclose(d.W_.sum(axis=1), 1.0, atol=1e-12)


def test_bitwise_run_to_run(hip, both_small_paths):
    from nbmf_mm_amd import NBMF
    X, M = midsize_XM()
    a = NBMF(n_components=32, random_state=7, max_iter=40, tol=0).fit(X[:300, :411], mask=M[:300, :411])
    b = NBMF(n_components=32, random_state=7, max_iter=40, tol=0).fit(X[:300, :411], mask=M[:300, :411])
    np.testing.assert_array_equal(a.components_, b.components_)
    np.testing.assert_array_equal(a.W_, b.W_)
    np.testing.assert_array_equal(a.loss_curve_, b.loss_curve_)
    # ... and on the 8-byte storage paths (real-valued data; bool mask folded in / real weights), a size the launches
    # serve with several chunks and rounds of workgroups: partial slabs and the loss slots are summed in a fixed order
    r = np.random.default_rng(3)
    Xr = r.random((1500, 700))
    for mk in (r.random((1500, 700)) < 0.8, r.random((1500, 700))):
        fits = [NBMF(n_components=48, random_state=7, max_iter=12, tol=0).fit(Xr, mask=mk) for _ in range(2)]
        np.testing.assert_array_equal(fits[0].components_, fits[1].components_)
        np.testing.assert_array_equal(fits[0].W_, fits[1].W_)
        np.testing.assert_array_equal(fits[0].loss_curve_, fits[1].loss_curve_)
        # the run of k iterations is a prefix of the run of k + 1: the last loss comes from the Theta-only sweep, the others
        # from the next iteration's H sweep, and the two must give the same bits
        shorter = NBMF(n_components=48, random_state=7, max_iter=11, tol=0).fit(Xr, mask=mk)
        np.testing.assert_array_equal(shorter.loss_curve_, fits[0].loss_curve_[:11])


def test_duchi_extension_properties(hip, both_small_paths):
    """projection='duchi' (README.md:27-35) through the estimator, from its own start ON the simplex, where the projection
    is the identity to within eps: simplex exact, tracks the CPU restatement of the same extension, near-identical to
    'normalize' when unmasked.  Where the projection DROPS components -- starts off the simplex, every K layout and
    storage path, both kernels, factor by factor and the support exactly -- it is pinned by test_gpu_duchi_start.py."""
    from nbmf_mm_amd import NBMF
    X, mask = config1_X(), config1_mask()
    d = NBMF(n_components=6, random_state=0, max_iter=40, tol=0, projection="duchi").fit(X, mask=mask)
    np.testing.assert_allclose(d.W_.sum(axis=1), 1.0, atol=1e-12)
    assert (d.W_ >= 0).all()
    _, _, lr, _, _ = orc.solve(X, 6, max_iter=40, tol=0, random_state=0, mask=mask, step=orc.mm_step_duchi)
    np.testing.assert_allclose(d.loss_curve_, lr, rtol=1e-9, atol=0)
    nrm = NBMF(n_components=6, random_state=0, max_iter=40, tol=0).fit(X)
    du = NBMF(n_components=6, random_state=0, max_iter=40, tol=0, projection_method="duchi").fit(X)
    np.testing.assert_allclose(du.loss_curve_, nrm.loss_curve_, rtol=1e-6)


def test_loss_entry_point_matches_oracle(hip, both_small_paths):
    r = np.random.default_rng(5)
    Y = (r.random((90, 70)) < 0.3).astype(np.float64)
    W = r.uniform(0.1, 0.9, (7, 90)); W /= W.sum(axis=0, keepdims=True)
    H = r.uniform(0.1, 0.9, (7, 70))
    with hip.Context(90, 70, 7) as ctx:
        ctx.set_hyper(1.4, 1.1)
        ctx.upload(Y)
        ctx.set_factors(W, H)
        got = ctx.loss()
        assert ctx.n_obs() == 90 * 70
    want = orc.mm_loss(Y, W, H, None, 1.4, 1.1)
    assert abs(got - want) <= 1e-12 * abs(want)


def test_out_of_range_raises(hip):
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError, match="must be binary"):
        NBMF(n_components=3, max_iter=2).fit(np.random.default_rng(0).normal(size=(20, 10)))
    with pytest.raises(ValueError):
        from nbmf_mm_amd import nbmf_mm_solver
        nbmf_mm_solver(np.full((20, 10), 1.5), 3, max_iter=2)       # solver-level range check is on the device


def test_perplexity_grid_matches_reference_driver(hip):
    """The experiment driver (examples/reproduce_magron2022.py:40-73 of the reference): train on a
    train mask, strictly masked held-out perplexity on validation/test masks, over an (alpha, beta, K) grid."""
    from nbmf_mm_amd.experiments import perplexity_grid
    r = np.random.default_rng(12)
    Y = (r.random((253, 302)) < 0.2).astype(np.float64)
    u = r.random(Y.shape)
    train, val, test = (u < 0.7).astype(np.float64), ((u >= 0.7) & (u < 0.85)).astype(np.float64), (u >= 0.85).astype(np.float64)
    rows = perplexity_grid(Y, train, {"val": val, "test": test}, [4, 20], [0.5, 1.5], [1.0, 2.5], max_iter=60, tol=1e-5)
    assert len(rows) == 8
    for row in rows:
        W, H, losses, _, n_iter = orc.solve(Y, row["K"], max_iter=60, tol=1e-5, alpha=row["alpha"], beta=row["beta"],
                                            mask=train, random_state=12345)
        assert row["n_iter"] == n_iter
        assert abs(row["loss"] - losses[-1]) <= 1e-10 * abs(losses[-1])
        for name, mk in [("val", val), ("test", test)]:
            want = orc.heldout_perplexity(Y, W @ H, mk)
            assert abs(row[name + "_perplexity"] - want) <= 1e-9 * want
    # several grid points at once (threads, one stream each): same rows
    conc = perplexity_grid(Y, train, {"val": val, "test": test}, [4, 20], [0.5, 1.5], [1.0, 2.5], max_iter=60, tol=1e-5,
                           concurrency=4)
    for a, b in zip(rows, conc):
        assert {k: v for k, v in a.items() if k != "time"} == {k: v for k, v in b.items() if k != "time"}
    # real-valued data with a weight mask goes through the f64 variant of the same sweep
    Yr, wts = r.random((40, 70)), r.random((40, 70))
    Wf = r.uniform(0.1, 0.9, (5, 40)); Wf /= Wf.sum(axis=0, keepdims=True)
    Hf = r.uniform(0.1, 0.9, (5, 70))
    with hip.Context(40, 70, 5) as ctx:
        ctx.upload(Yr, mask=wts)
        ctx.set_factors(Wf, Hf)
        got = np.exp(-ctx.loglik_strict() / ctx.n_obs())
    want = orc.heldout_perplexity(Yr, Wf.T @ Hf, wts)
    assert abs(got - want) <= 1e-12 * want


def test_heldout_perplexity_against_the_reference_drivers_own_value(hip, golden, both_small_paths):
    """tests/golden/heldout.npz: the reference's fit on the training entries of a seeded 40 x 70 problem and its driver's
    `compute_perplexity` (examples/reproduce_magron2022.py:40-47, run in the build container) on validation / test /
    real-weight / no mask.  The device's strictly masked sweep on the REFERENCE's factors: <= 1e-12; the whole pipeline of
    `perplexity_grid` (fit on train, evaluate on val and test): the reference's iteration count, loss <= 1e-10,
    perplexities <= 1e-9 (200 ulp of accumulated fit difference at most)."""
    from nbmf_mm_amd.experiments import heldout_perplexity, perplexity_grid
    g = golden("heldout")
    Y = g["Y"].astype(np.float64)
    Wk, H = np.ascontiguousarray(g["W"].T), g["H"]
    for name, mk in (("val", g["val"]), ("test", g["test"]), ("val_float", g["val"].astype(np.float64)),
                     ("weights", g["weights"]), ("nomask", None)):
        with hip.Context(40, 70, 5) as ev:
            ev.set_hyper(1.0, 1.0)
            ev.upload(Y, mask=mk)
            got = heldout_perplexity(ev, Wk, H)
        want = float(g["perp_" + name])
        assert abs(got - want) <= 1e-12 * want, (name, got, want)
    rows = perplexity_grid(Y, g["train"], {"val": g["val"], "test": g["test"]}, 5, [1.2], [1.2], max_iter=60, tol=1e-5)
    assert len(rows) == 1 and rows[0]["n_iter"] == int(g["n_iter"])
    assert abs(rows[0]["loss"] - g["losses"][-1]) <= 1e-10 * g["losses"][-1]
    assert abs(rows[0]["val_perplexity"] - float(g["perp_val"])) <= 1e-9 * float(g["perp_val"])
    assert abs(rows[0]["test_perplexity"] - float(g["perp_test"])) <= 1e-9 * float(g["perp_test"])


@pytest.mark.parametrize("k", [5, 24, 40, 100])
@pytest.mark.parametrize("masked", [False, True])
def test_real_valued_data_with_a_binary_mask_every_sweep_variant(hip, k, masked):
    """The 8-byte storage path whose mask (if any) is folded into the data (DATA_F64): image A keeps an unobserved entry as
    -0.0, so the strictly masked likelihood tells "unobserved" from an OBSERVED zero by the sign bit -- checked here with
    exact zeros (+0.0 and -0.0) among the observed data.  Every sweep variant against the oracle: the fit (H, W and
    likelihood sweeps), nbmf_loss, nbmf_loglik with and without clipping, nbmf_loglik_strict; K = 5 / 24 / 40 / 100 are
    the four register layouts (the last one with the 256-entry logarithm table)."""
    r = np.random.default_rng(100 + k)
    m, n = 77, 150
    Y = r.random((m, n))
    Y[r.random((m, n)) < 0.1] = 0.0                      # observed exact zeros ...
    Y[3, 5], Y[4, 6] = -0.0, 1.0                         # ... one of them negative zero; an exact one
    mask = (r.random((m, n)) < 0.8) if masked else None
    if masked:
        mask[3, 5] = mask[4, 6] = True
    from nbmf_mm_amd import nbmf_mm_solver
    W, H, l, _, _ = nbmf_mm_solver(Y, k, max_iter=8, tol=0, random_state=3, mask=mask, alpha=1.3, beta=1.1)
    Wr, Hr, lr, _, _ = orc.solve(Y, k, max_iter=8, tol=0, random_state=3, mask=mask, alpha=1.3, beta=1.1)
    np.testing.assert_allclose(l, lr, rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(W, Wr, rtol=0, atol=FACTOR_ATOL)
    np.testing.assert_allclose(H, Hr, rtol=0, atol=FACTOR_ATOL)
    mf = None if mask is None else mask.astype(np.float64)
    with hip.Context(m, n, k) as ctx:
        ctx.set_hyper(1.3, 1.1)
        assert ctx.upload(Y, mask=mask) is False          # doubles, not byte codes
        ctx.set_factors(np.ascontiguousarray(Wr.T), Hr)
        want = orc.mm_loss(Y, Wr.T, Hr, mf, 1.3, 1.1)
        assert abs(ctx.loss() - want) <= 1e-12 * abs(want)
        want = orc.score(Y, Wr, Hr, mf)
        assert abs(ctx.loglik(clip_theta=True) / ctx.n_obs() - want) <= 1e-12 * abs(want)
        assert abs(ctx.loglik() / ctx.n_obs() - want) <= 1e-12 * abs(want)      # (W @ H <= 1 here: clipping changes nothing)
        want = orc.heldout_perplexity(Y, Wr @ Hr, mf)
        got = np.exp(-ctx.loglik_strict() / ctx.n_obs())
        assert abs(got - want) <= 1e-12 * want
        assert ctx.n_obs() == (m * n if mask is None else np.count_nonzero(mask))
        # factors pushed off the simplex by hand (W @ H above 1 in places): the clipped sweep is the reference's score
        # (_base.py:210: clip first, then the logarithms)
        Hbig = np.clip(Hr * 3.0, 0, None)
        ctx.set_factors(np.ascontiguousarray(Wr.T), Hbig)
        want = orc.score(Y, Wr, Hbig, mf)
        assert (Wr @ Hbig).max() > 1.0 and abs(ctx.loglik(clip_theta=True) / ctx.n_obs() - want) <= 1e-12 * abs(want)


def test_round4_reference_fixtures(hip, golden, both_small_paths):
    """The reference's own outputs (tests/golden/round4.npz, written by oracle/make_golden.py from the imported reference) for
    real-valued data with real weights and with a bool mask under both orientations -- factors included --, for CSR / bool +
    int / float32 inputs, for a row nobody observes, and for transform after a dir-beta fit."""
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF
    g = golden("round4")
    g3 = np.random.default_rng(41)
    Xq, Wq = g3.random((90, 130)), g3.random((90, 130))
    Bq = g3.random((90, 130)) < 0.8
    Xb = (g3.random((70, 110)) < 0.2)
    Mb = (g3.random((70, 110)) < 0.85)
    for name, orient, mk in (("rw_bd", "beta-dir", Wq), ("rw_db", "dir-beta", Wq), ("rb_bd", "beta-dir", Bq), ("rb_db", "dir-beta", Bq)):
        m = NBMF(n_components=7, alpha=1.3, beta=1.1, random_state=3, max_iter=25, tol=0, orientation=orient).fit(Xq, mask=mk)
        np.testing.assert_allclose(m.loss_curve_, g[name + "_losses"], rtol=LOSS_RTOL, atol=0, err_msg=name)
        np.testing.assert_allclose(m.W_, g[name + "_W"], rtol=0, atol=FACTOR_ATOL, err_msg=name)
        np.testing.assert_allclose(m.components_, g[name + "_H"], rtol=0, atol=FACTOR_ATOL, err_msg=name)
    Xf, Mf = Xb.astype(np.float64), Mb.astype(np.float64)
    for Xv, mv in ((Xf, Mf), (sp.csr_matrix(Xf), sp.csr_matrix(Mf)), (Xb, Mb.astype(np.int32)), (Xb.astype(np.float32), Mb.astype(np.float32))):
        m = NBMF(n_components=5, random_state=4, max_iter=20, tol=0).fit(Xv, mask=mv)
        np.testing.assert_allclose(m.loss_curve_, g["kinds_losses"], rtol=LOSS_RTOL, atol=0)
        np.testing.assert_allclose(m.W_, g["kinds_W"], rtol=0, atol=FACTOR_ATOL)
        np.testing.assert_allclose(m.components_, g["kinds_H"], rtol=0, atol=FACTOR_ATOL)
    Mn = Mf.copy()
    Mn[9, :] = 0.0
    m = NBMF(n_components=5, random_state=4, max_iter=6, tol=0).fit(Xf, mask=Mn)
    assert np.isnan(m.loss_curve_).all() and np.isnan(g["nanrow_losses"]).all()      # 0 / 0 in row 9 of W, NaN from then on (:57)
    assert np.array_equal(np.isnan(m.W_), np.isnan(g["nanrow_W"]))
    md = NBMF(n_components=5, random_state=4, max_iter=30, tol=0, orientation="dir-beta").fit(Xf)
    np.testing.assert_allclose(md.components_, g["dirbeta_H"], rtol=0, atol=FACTOR_ATOL)
    md.components_ = g["dirbeta_H"]
    np.random.seed(8)
    Wo, keep = orc.w_only_transform(Xf[:12], g["dirbeta_H"], W0=np.random.uniform(0.1, 0.9, (12, 5)), track_positive=True)
    np.testing.assert_array_equal(Wo, g["dirbeta_transform"])
    np.random.seed(8)
    got = md.transform(Xf[:12])          # always the simplex-W form, whatever the fitted orientation (_base.py:178-193)
    assert keep.sum() >= 10              # (rows that go through negative ratios are chaotic in the reference itself)
    np.testing.assert_allclose(got[keep], g["dirbeta_transform"][keep], rtol=0, atol=FACTOR_ATOL)


def test_round5_reference_fixtures(hip, golden, both_small_paths):
    """The reference's own outputs (tests/golden/round5.npz) for real-valued data at K = 16 / 32 / 64 -- the register layouts
    of the general path's sweeps round 5 touched: the shared reciprocal at K = 16, the range check left to the TINY variant
    -- plain, with a bool mask under dir-beta, with real weights; and its one-step update of a matrix with columns nobody
    has a one in under a flat prior (binary path: the H sweep's P1 is a difference of all-entry sums there)."""
    from nbmf_mm_amd import NBMF
    g = golden("round5")
    g5 = np.random.default_rng(55)
    Xr5 = g5.random((150, 170))
    Br5 = g5.random((150, 170)) < 0.85
    Wt5 = g5.random((150, 170))
    for name, K, orient, mk, its in (("k16_plain", 16, "beta-dir", None, 40), ("k16_mask_db", 16, "dir-beta", Br5, 40),
                                     ("k32_weights", 32, "beta-dir", Wt5, 30), ("k64_mask", 64, "beta-dir", Br5, 20)):
        m = NBMF(n_components=K, alpha=1.2, beta=1.4, random_state=9, max_iter=its, tol=0, orientation=orient).fit(Xr5, mask=mk)
        np.testing.assert_allclose(m.loss_curve_, g[name + "_losses"], rtol=LOSS_RTOL, atol=0, err_msg=name)
        if K <= 32:
            np.testing.assert_allclose(m.W_, g[name + "_W"], rtol=0, atol=FACTOR_ATOL, err_msg=name)
            np.testing.assert_allclose(m.components_, g[name + "_H"], rtol=0, atol=FACTOR_ATOL, err_msg=name)
    for tag, mk in (("plain", None), ("masked", g["zc_mask"])):
        Wn, Hn, loss, binpath = _one_step(hip, g["zc_Y"], g["zc_W"], g["zc_H"], mk, 1.0, 1.3)
        assert binpath
        np.testing.assert_allclose(Hn, g["zc_H_new_" + tag], rtol=0, atol=1e-13)
        np.testing.assert_allclose(Wn, g["zc_W_new_" + tag], rtol=0, atol=1e-13)
        assert (Hn[:, [5, 11]] == 1e-8).all()


def test_estimator_random_reference_fixtures(hip, golden, both_small_paths):
    """The reference's own outputs (tests/golden/estimator_random.npz, item 12 of oracle/make_golden.py) for twenty random
    fits through its estimator: every orientation alias, the data handed over as the fixture says (float64 / int / bool /
    float32 / CSR), masks of every kind, seeded and custom inits (on the simplex or not), stop rules that fire or not --
    `NBMF(...)` here must give the same W_, components_, loss curve, n_iter_ and normalised `orientation`."""
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF
    from test_oracle_golden import estimator_random_cases
    n = 0
    for c in estimator_random_cases(golden("estimator_random")):
        par = dict(c["par"])
        form, init, mkind = par.pop("form"), par.pop("init"), par.pop("mask")
        X = {"f64": c["X"], "int": c["X"].astype(np.int64), "bool": c["X"].astype(bool), "f32": c["X"].astype(np.float32),
             "csr": sp.csr_matrix(c["X"])}[form]
        m = NBMF(W_init=c["W0"], H_init=c["H0"], **par).fit(X, mask=c["mask"])
        tag = f"case {n}: {c['par']}"
        assert m.n_iter_ == c["n_iter"], tag
        assert m.orientation == c["orientation_after"], tag
        np.testing.assert_allclose(m.loss_curve_, c["losses"], rtol=LOSS_RTOL, atol=0, err_msg=tag)
        np.testing.assert_allclose(m.W_, c["W"], rtol=0, atol=FACTOR_ATOL, err_msg=tag)
        np.testing.assert_allclose(m.components_, c["H"], rtol=0, atol=FACTOR_ATOL, err_msg=tag)
        assert m.loss_ == m.loss_curve_[-1] == m.reconstruction_err_ and m.objective_history_ is m.loss_curve_
        n += 1
    assert n == 20


_RAGGED_SCRIPT = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from nbmf_mm_amd import nbmf_mm_solver
g = np.random.default_rng(33)
Xb = (g.random((700, 520)) < 0.3).astype(np.float64)
Xr = g.random((700, 520))
mk = g.random((700, 520)) < 0.85
out = {}
for name, X, K in (("bin5", Xb, 5), ("bin8", Xb, 8), ("bin10", Xb, 10), ("bin20", Xb, 20), ("bin40", Xb, 40), ("bin48", Xb, 48),
                   ("real20", Xr, 20), ("real40", Xr, 40)):
    W, H, l, _, _ = nbmf_mm_solver(X, K, max_iter=12, tol=0, random_state=1, mask=mk, alpha=1.2, beta=1.3)
    out[name] = [np.asarray(l).tobytes().hex(), W.tobytes().hex()[:4096], H.tobytes().hex()[:4096], float(l[-1])]
# ... real weights (the third storage path), the other orientation, the evaluation-time calls (transform = the W sweep with
# H frozen, score / perplexity = the likelihood sweep, clipped and strict) and a four-rank fit (rank threads on device 0)
import hashlib
from nbmf_mm_amd import NBMF
wts = g.uniform(0.2, 1.0, (700, 520)) * mk
for name, X, K in (("realw20", Xr, 20), ("realw40", Xr, 40)):
    W, H, l, _, _ = nbmf_mm_solver(X, K, max_iter=10, tol=0, random_state=2, mask=wts, orientation="dir-beta")
    out[name] = [np.asarray(l).tobytes().hex(), hashlib.sha1(W.tobytes()).hexdigest(), hashlib.sha1(H.tobytes()).hexdigest(), float(l[-1])]
for name, X, K in (("est_bin10", Xb, 10), ("est_bin40", Xb, 40), ("est_real24", Xr, 24)):
    est = NBMF(n_components=K, max_iter=15, tol=0, random_state=3).fit(X, mask=mk)
    T = est.transform(X[:130], mask=mk[:130])
    out[name] = [hashlib.sha1(T.tobytes()).hexdigest(), repr(est.score(X, mask=mk)), repr(est.perplexity(X, mask=mk)),
                 float(est.score(X[:64]))]
if sys.argv[2] == "1":
    est = NBMF(n_components=40, max_iter=10, tol=0, random_state=4, n_gpus=4, devices=[0] * 4).fit(Xb, mask=mk)
    out["four_ranks_bin40"] = [hashlib.sha1(est.W_.tobytes()).hexdigest(), hashlib.sha1(est.components_.tobytes()).hexdigest(),
                               repr(est.reconstruction_err_), float(est.reconstruction_err_)]
print("RESULT " + json.dumps(out))
"""


def test_ragged_k_variant_gives_the_full_kernels_bits(hip):
    """Fewer components than the layout holds (k = 10 in the K = 16 layout, 40 in the K = 64 one): the sweeps' RAG variant
    skips the Theta k-steps and the 16-blocks of components that hold nothing but padding.  The padding is exact zeros in both
    factors, so the skipped MFMAs would have added zeros: the fit must be the full kernels' (NBMF_NO_RAGGED_K=1) BIT FOR
    BIT -- losses, W, H -- on byte-code and real-valued data (folded mask, real weights), where the variant is used and where it
    is not; and so must transform, score and perplexity (the W sweep with H frozen, the likelihood sweep) and a four-rank fit
    (its four rank threads share device 0: part of the comparison wherever the environment gives them the hardware queues
    they need, see conftest.rank_threads_fit_on_one_gpu)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    four_ranks = rank_threads_fit_on_one_gpu(4)
    res = []
    for no_rag in (False, True):
        env = dict(os.environ, NBMF_PERSISTENT="0", NBMF_PEER_TIMEOUT_MS="20000")
        env.pop("NBMF_NO_RAGGED_K", None)
        if no_rag:
            env["NBMF_NO_RAGGED_K"] = "1"
        r = subprocess.run([sys.executable, "-c", _RAGGED_SCRIPT, root, "1" if four_ranks else "0"], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        res.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    assert res[0].keys() == res[1].keys() and len(res[0]) == (14 if four_ranks else 13)
    for name in res[0]:
        assert res[0][name] == res[1][name], name
        assert np.isfinite(res[0][name][3])


def _vs_oracle(Y, k, mask=None, iters=15, **kw):
    from nbmf_mm_amd import nbmf_mm_solver
    W, H, l, _, n1 = nbmf_mm_solver(Y, k, max_iter=iters, tol=0, mask=mask, **kw)
    Wr, Hr, lr, _, n2 = orc.solve(np.asarray(_dense_any(Y), dtype=np.float64), k, max_iter=iters, tol=0,
                                  mask=mask, **kw)
    assert n1 == n2
    np.testing.assert_allclose(l, lr, rtol=LOSS_RTOL, atol=0)
    np.testing.assert_allclose(W, Wr, rtol=0, atol=FACTOR_ATOL)
    np.testing.assert_allclose(H, Hr, rtol=0, atol=FACTOR_ATOL)
    return W, H, l


def _dense_any(a):
    return a.toarray() if hasattr(a, "toarray") else a


def test_edge_cases_vs_oracle(hip, both_small_paths):
    """Degenerate and boundary inputs the domain offers: constant matrices, K larger than the matrix,
    priors below 1 (negative a, b: the clip is what keeps H in range), rows/columns with nothing
    observed, a mask observing almost nothing, single row / single column."""
    r = np.random.default_rng(33)
    Y = (r.random((37, 53)) < 0.3).astype(np.float64)
    _vs_oracle(np.zeros((20, 31)), 3, random_state=1)
    _vs_oracle(np.ones((20, 31)), 3, random_state=1)
    _vs_oracle(Y[:5, :7], 12, random_state=2)                      # K > min(m, n)
    _vs_oracle(Y, 4, random_state=3, alpha=0.5, beta=2.0)          # a = -0.5
    _vs_oracle(Y, 4, random_state=3, alpha=0.3, beta=0.4)          # both negative
    _vs_oracle(Y[:1, :], 2, random_state=4)                        # one row
    _vs_oracle(Y[:, :1], 2, random_state=4)                        # one column
    mask = (r.random(Y.shape) < 0.7).astype(np.float64)
    mask[5, :] = 0.0                                               # a row never observed
    mask[:, 11] = 0.0                                              # a column never observed
    _vs_oracle(Y, 5, mask=mask, random_state=5)
    _vs_oracle(Y, 5, mask=mask, random_state=5, orientation="dir-beta")
    sparse_mask = np.zeros_like(Y); sparse_mask[3, 4] = 1.0; sparse_mask[30, 50] = 1.0
    _vs_oracle(Y, 3, mask=sparse_mask, random_state=6, iters=6)
    # probabilities exactly at the ends of [0, 1] mixed with interior values -> general path
    Yp = r.random((30, 40)); Yp[0, :5] = 0.0; Yp[1, :5] = 1.0
    _vs_oracle(Yp, 4, random_state=7)
    # ... and with a row nobody observed: 0/0 in the simplex factor, NaN losses from then on, as in the reference
    mp = (r.random(Yp.shape) < 0.8).astype(np.float64); mp[7, :] = 0.0
    _vs_oracle(Yp, 4, mask=mp, random_state=8)
    _vs_oracle(Yp, 4, mask=mp * r.uniform(0.5, 1.5, Yp.shape), random_state=8)      # weights: the other general path


def test_input_types_accepted_like_the_reference(hip):
    """scipy CSR data and masks, bool / int data, Fortran-ordered and strided arrays
    (tests/test_api.py:111-123 and tests/test_public_api.py:125-134 of the reference)."""
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF
    r = np.random.default_rng(8)
    X = (r.random((40, 60)) < 0.25).astype(np.float64)
    mask = r.random((40, 60)) < 0.8
    base = NBMF(n_components=5, random_state=0, max_iter=12, tol=0).fit(X, mask=mask)
    for Xv, mv in [(sp.csr_matrix(X), sp.csr_matrix(mask.astype(np.float64))), (X.astype(bool), mask),
                   (X.astype(np.int64), mask.astype(np.int32)), (np.asfortranarray(X), np.asfortranarray(mask)),
                   (np.repeat(X, 2, axis=1)[:, ::2], mask.astype(np.float32))]:
        got = NBMF(n_components=5, random_state=0, max_iter=12, tol=0).fit(Xv, mask=mv)
        np.testing.assert_array_equal(got.components_, base.components_)
        np.testing.assert_array_equal(got.loss_curve_, base.loss_curve_)
    # dir-beta with a strided (transposed-view) input
    a = NBMF(n_components=5, random_state=0, max_iter=8, tol=0, orientation="dir-beta").fit(X.T.copy().T)
    b = NBMF(n_components=5, random_state=0, max_iter=8, tol=0, orientation="dir-beta").fit(X)
    np.testing.assert_array_equal(a.W_, b.W_)


def test_last_loss_sweep_is_bitwise_the_fused_one(hip, both_small_paths):
    """The loss of the final iteration comes from the Theta-only sweep, every earlier one from the fused
    H-pass of the following iteration; both must give the same bits (so a run of k iterations is a prefix
    of a run of k+1), on the binary and on the general storage path, K = 64 and K = 128."""
    r = np.random.default_rng(3)
    for (m, n, k, real) in [(300, 260, 64, False), (150, 140, 128, False), (90, 200, 20, True)]:
        Y = r.random((m, n)) if real else (r.random((m, n)) < 0.3).astype(np.float64)
        mask = r.random((m, n)) < 0.9
        W0 = r.uniform(0.1, 0.9, (k, m)); W0 /= W0.sum(axis=0, keepdims=True)
        H0 = r.uniform(0.1, 0.9, (k, n))
        with hip.Context(m, n, k) as ctx:
            ctx.set_hyper(1.2, 1.2)
            ctx.upload(Y, mask=mask)
            ctx.set_factors(W0, H0)
            a, _ = ctx.run(5, 0.0)
            if both_small_paths == "single-launch":      # (nbmf_loss is a sweep of the five-kernel engine)
                assert abs(a[-1] - ctx.loss()) <= 1e-13 * abs(a[-1])
            else:
                assert a[-1] == ctx.loss()
            ctx.set_factors(W0, H0)
            b, _ = ctx.run(6, 0.0)
        np.testing.assert_array_equal(a, b[:5])


def test_plain_c_consumer_of_the_abi(hip):
    """tests/c/abi_smoke.c: a C99 program (no Python, no C++) driving libnbmf_hip.so end to end."""
    import os, shutil, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if shutil.which("gcc") is None:
        pytest.skip("no gcc on this box")
    exe = os.path.join(root, "build", "abi_smoke_test")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "c", "abi_smoke.c"), "-L", os.path.join(root, "nbmf_mm_amd"),
                           "-lnbmf_hip", "-Wl,-rpath," + os.path.join(root, "nbmf_mm_amd"), "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "abi_smoke ok" in out.stdout


def test_graph_replay_matches_eager(hip, monkeypatch):
    """Opt-in hipGraph replay of the iteration (device-side loss index): same bits, same stop iteration."""
    from nbmf_mm_amd import nbmf_mm_solver
    X, M = midsize_XM()
    X, M = X[:200, :333], M[:200, :333]
    monkeypatch.setenv("NBMF_PERSISTENT", "0")       # (a problem of this size would otherwise never reach the launches)
    monkeypatch.delenv("NBMF_USE_GRAPH", raising=False)
    W0, H0, l0, _, n0 = nbmf_mm_solver(X, 12, max_iter=300, tol=1e-4, random_state=3, mask=M)
    Wf, Hf, lf, _, nf = nbmf_mm_solver(X, 12, max_iter=40, tol=0, random_state=3, mask=M)
    monkeypatch.setenv("NBMF_USE_GRAPH", "1")
    W1, H1, l1, _, n1 = nbmf_mm_solver(X, 12, max_iter=300, tol=1e-4, random_state=3, mask=M)
    Wg, Hg, lg, _, ng = nbmf_mm_solver(X, 12, max_iter=40, tol=0, random_state=3, mask=M)
    assert 8 < n0 < 300 and n1 == n0 and ng == nf == 40
    np.testing.assert_array_equal(l1, l0)
    np.testing.assert_array_equal(W1, W0)
    np.testing.assert_array_equal(H1, H0)
    np.testing.assert_array_equal(lg, lf)
    np.testing.assert_array_equal(Wg, Wf)


def test_storage_path_is_decided_by_the_whole_matrix(hip):
    """The host samples a few rows to guess the storage path; the device pack checks every entry and the
    upload falls back to the 8-byte path when the guess was wrong (data or mask)."""
    r = np.random.default_rng(17)
    Y = (r.random((100, 50)) < 0.3).astype(np.float64)
    mask = (r.random((100, 50)) < 0.8).astype(np.float64)
    W = r.uniform(0.1, 0.9, (4, 100)); W /= W.sum(axis=0, keepdims=True)
    H = r.uniform(0.1, 0.9, (4, 50))
    for Yv, mv, want_bin in [(Y, mask, True), (Y, None, True), (Y, mask.astype(bool), True)]:
        with hip.Context(100, 50, 4) as ctx:
            assert ctx.upload(Yv, mask=mv) is want_bin
    Y2 = Y.copy(); Y2[37, 3] = 0.5                       # one non-binary entry in a row the sample skips
    m2 = mask.copy(); m2[41, 7] = 0.25                   # one weight in the mask
    for Yv, mv in [(Y2, mask), (Y, m2), (Y2, None)]:
        with hip.Context(100, 50, 4) as ctx:
            ctx.set_hyper(1.2, 1.2)
            assert ctx.upload(Yv, mask=mv) is False
            ctx.set_factors(W, H)
            losses, _ = ctx.run(3, 0.0)
            Wn, Hn = ctx.get_factors()
        Wr, Hr = W, H
        for _ in range(3):
            Wr, Hr = orc.mm_step(Yv, Wr, Hr, mv, 1.2, 1.2)
        np.testing.assert_allclose(Wn, Wr, rtol=0, atol=1e-13)
        np.testing.assert_allclose(Hn, Hr, rtol=0, atol=1e-13)
        assert abs(losses[-1] - orc.mm_loss(Yv, Wr, Hr, mv, 1.2, 1.2)) <= 1e-12
    # re-upload on the same context switches paths cleanly
    with hip.Context(100, 50, 4) as ctx:
        assert ctx.upload(Y2, mask=mask) is False
        assert ctx.upload(Y, mask=mask) is True
        ctx.set_factors(W, H)
        a = ctx.loss()
    assert abs(a - orc.mm_loss(Y, W, H, mask, 1.2, 1.2)) <= 1e-12


def test_fuzz_against_oracle(hip, both_small_paths):
    """Seeded random configurations: shapes straddling the 16 / 128 padding units, every K template,
    both orientations, mask kinds (none / bool / float 0-1 / weights), real-valued data, priors on both
    sides of 1, both projections (the Duchi extension against the oracle's restatement of it)."""
    from nbmf_mm_amd import nbmf_mm_solver
    r = np.random.default_rng(2024)
    shapes = [(1, 17), (15, 16), (16, 129), (127, 128), (128, 127), (129, 255), (257, 31), (300, 513), (640, 65)]
    for case in range(36):
        m, n = shapes[case % len(shapes)]
        if case % 7 == 3:
            m, n = int(r.integers(1, 400)), int(r.integers(1, 400))
        k = int(r.choice([1, 2, 7, 16, 17, 31, 32, 33, 48, 64, 65, 100, 128]))
        real = case % 5 == 4
        Y = r.random((m, n)) if real else (r.random((m, n)) < r.uniform(0.05, 0.6)).astype(np.float64)
        mk = case % 4
        mask = None if mk == 0 else (r.random((m, n)) < 0.8) if mk == 1 else \
            (r.random((m, n)) < 0.7).astype(np.float64) if mk == 2 else r.random((m, n))
        orient = "dir-beta" if case % 3 == 1 else "beta-dir"
        al, be = float(r.uniform(0.6, 2.5)), float(r.uniform(0.6, 2.5))
        duchi = case % 6 == 5
        kw = dict(max_iter=8, tol=0, alpha=al, beta=be, mask=mask, random_state=int(case), orientation=orient)
        W, H, l, _, _ = nbmf_mm_solver(Y, k, projection="duchi" if duchi else "normalize", **kw)
        Wr, Hr, lr, _, _ = orc.solve(Y, k, step=orc.mm_step_duchi if duchi else None, **kw)
        tag = f"case {case}: {m}x{n} k={k} real={real} mask={mk} {orient} duchi={duchi}"
        if duchi:
            print(tag, "loss %.3g of LOSS_RTOL, W %.3g and H %.3g of FACTOR_ATOL" % (
                np.max(np.abs(np.asarray(l) - lr) / np.abs(lr)) / LOSS_RTOL, np.max(np.abs(W - Wr)) / FACTOR_ATOL,
                np.max(np.abs(H - Hr)) / FACTOR_ATOL))
        np.testing.assert_allclose(l, lr, rtol=LOSS_RTOL, atol=0, err_msg=tag)
        np.testing.assert_allclose(W, Wr, rtol=0, atol=FACTOR_ATOL, err_msg=tag)
        np.testing.assert_allclose(H, Hr, rtol=0, atol=FACTOR_ATOL, err_msg=tag)


def test_on_device_synthetic_data_matches_its_numpy_twin(hip):
    """Context.generate (measurement helper): the device-generated matrix equals the NumPy regeneration,
    checked through everything the context computes from it."""
    m, n, k = 203, 310, 9
    Y, mask = hip.synthetic_reference(m, n, seed=77, density=0.3, observed=0.85)
    assert 0.25 < Y.mean() < 0.35 and 0.8 < mask.mean() < 0.9
    r = np.random.default_rng(0)
    W = r.uniform(0.1, 0.9, (k, m)); W /= W.sum(axis=0, keepdims=True)
    H = r.uniform(0.1, 0.9, (k, n))
    with hip.Context(m, n, k) as gen, hip.Context(m, n, k) as up:
        gen.set_hyper(1.2, 1.2); up.set_hyper(1.2, 1.2)
        gen.generate(77, density=0.3, observed=0.85)
        up.upload(Y, mask=mask)
        assert gen.n_obs() == up.n_obs() == float(mask.sum())
        outs = []
        for ctx in (gen, up):
            ctx.set_factors(W, H)
            losses, _ = ctx.run(6, 0.0)
            outs.append((losses,) + ctx.get_factors())
    for a, b in zip(*outs):
        np.testing.assert_array_equal(a, b)


def test_seeded_sweep_of_configurations_vs_oracle(hip, both_small_paths):
    """Forty pseudo-random small problems (shape, K from 1 to 200, density, mask kind, orientation, priors,
    real-valued or binary data, projection) against the oracle: the parity net under the hand-picked cases."""
    from nbmf_mm_amd import nbmf_mm_solver
    r = np.random.default_rng(20260101)
    for case in range(40):
        m, n = int(r.integers(1, 260)), int(r.integers(1, 300))
        k = int(r.choice([1, 2, 5, 16, 17, 31, 48, 64, 65, 100, 128, 129, 200]))
        binary = bool(r.integers(0, 4))                       # one in four real-valued
        Y = (r.random((m, n)) < r.uniform(0.05, 0.6)).astype(np.float64) if binary else r.random((m, n))
        mk = int(r.integers(0, 4))
        mask = [None, r.random((m, n)) < 0.8, (r.random((m, n)) < 0.7).astype(np.float64), r.random((m, n))][mk]
        orientation = "dir-beta" if r.integers(0, 2) else "beta-dir"
        alpha, beta = float(r.uniform(1.0, 2.5)), float(r.uniform(1.0, 2.5))
        duchi = bool(r.integers(0, 3) == 0)
        kw = dict(max_iter=8, tol=0, alpha=alpha, beta=beta, mask=mask, random_state=case, orientation=orientation)
        W, H, l, _, _ = nbmf_mm_solver(Y, k, projection="duchi" if duchi else "normalize", **kw)
        Wr, Hr, lr, _, _ = orc.solve(Y, k, step=orc.mm_step_duchi if duchi else None, **kw)
        tag = f"case {case}: {m}x{n} k={k} binary={binary} mask={mk} {orientation} duchi={duchi}"
        if duchi:
            print(tag, "loss %.3g of LOSS_RTOL, W %.3g and H %.3g of FACTOR_ATOL" % (
                np.max(np.abs(np.asarray(l) - lr) / np.abs(lr)) / LOSS_RTOL, np.max(np.abs(W - Wr)) / FACTOR_ATOL,
                np.max(np.abs(H - Hr)) / FACTOR_ATOL))
        np.testing.assert_allclose(l, lr, rtol=LOSS_RTOL, atol=0, err_msg=tag)
        np.testing.assert_allclose(W, Wr, rtol=0, atol=FACTOR_ATOL, err_msg=tag)
        np.testing.assert_allclose(H, Hr, rtol=0, atol=FACTOR_ATOL, err_msg=tag)


_FULL_W_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from nbmf_mm_amd import _hip, nbmf_mm_solver
g = np.random.default_rng(61)
out = {}
for name, (m, n), K in (("k8", (700, 512), 8), ("k10", (700, 512), 10), ("k16", (333, 256), 16), ("k32", (700, 512), 32), ("k40", (520, 384), 40),
                        ("k64", (700, 512), 64), ("k100", (300, 256), 100), ("padded_n", (700, 500), 32)):
    X = (g.random((m, n)) < 0.3).astype(np.float64)
    before = _hip.variant_stats()[0]
    W, H, l, _, _ = nbmf_mm_solver(X, K, max_iter=12, tol=0, random_state=1, alpha=1.2, beta=1.3)
    one = nbmf_mm_solver(X, K, max_iter=1, tol=0, random_state=1, alpha=1.2, beta=1.3)
    out[name] = {"losses": [float(v) for v in l], "W": W.ravel()[::7].tolist(), "H": H.ravel()[::7].tolist(),
                 "W1": one[0].ravel()[::5].tolist(), "full_launches": _hip.variant_stats()[0] - before}
# a mask of ones is no mask (observed everywhere); a mask with ONE unobserved entry keeps the three-state sweep
X = (g.random((300, 500)) < 0.3).astype(np.float64)
for name, mk in (("mask_of_ones", np.ones((300, 500), dtype=bool)), ("one_unobserved", np.ones((300, 500), dtype=bool))):
    if name == "one_unobserved":
        mk[7, 11] = False
    before = _hip.variant_stats()[0]
    W, H, l, _, _ = nbmf_mm_solver(X, 12, max_iter=6, tol=0, random_state=3, mask=mk)
    out[name] = {"losses": [float(v) for v in l], "W": W.ravel()[::7].tolist(), "H": H.ravel()[::7].tolist(), "W1": [],
                 "full_launches": _hip.variant_stats()[0] - before}
# dir-beta: the W sweep walks the ROWS of V
X = (g.random((512, 300)) < 0.3).astype(np.float64)
before = _hip.variant_stats()[0]
W, H, l, _, _ = nbmf_mm_solver(X, 24, max_iter=8, tol=0, random_state=2, orientation="dir-beta")
out["dir_beta"] = {"losses": [float(v) for v in l], "W": W.ravel()[::7].tolist(), "H": H.ravel()[::7].tolist(), "W1": [],
                   "full_launches": _hip.variant_stats()[0] - before}
print("RESULT " + json.dumps(out))
"""


def test_two_state_w_sweep_on_fully_observed_data_equals_the_three_state_sweep(hip):
    """Binary data observed everywhere: the W sweeps run in the two-state (FULL) variant -- an entry that is not a one IS an
    observed zero, no "observed" factor, four words of lane masks per tile.  Against the three-state kernels on the same
    data (NBMF_NO_FULL_W=1): one step's W <= 1e-13, twelve iterations' losses <= 1e-12 relative, factors <= 1e-11; the
    variant is used wherever nothing is masked -- every layout, ragged K, dir-beta, a mask of ones, and shapes whose swept
    dimension is padded (500 columns: the pad rows are "ones" in that image's lane masks, whose ratios only ever meet the
    zero pad columns of the factor) -- and NOT as soon as one entry is unobserved.  Both runs against the oracle are covered
    by every other test of this file (unmasked data takes the variant by default)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = []
    for no_full in (False, True):
        env = dict(os.environ, NBMF_PERSISTENT="0")
        env.pop("NBMF_NO_FULL_W", None)
        if no_full:
            env["NBMF_NO_FULL_W"] = "1"
        r = subprocess.run([sys.executable, "-c", _FULL_W_SCRIPT, root], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
        res.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    full, three = res
    assert full.keys() == three.keys() and len(full) == 11
    for name in full:
        assert three[name]["full_launches"] == 0
        assert (full[name]["full_launches"] == 0) == (name == "one_unobserved"), name
        np.testing.assert_allclose(full[name]["losses"], three[name]["losses"], rtol=1e-12, atol=0, err_msg=name)
        np.testing.assert_allclose(full[name]["W1"], three[name]["W1"], rtol=0, atol=1e-13, err_msg=name)
        np.testing.assert_allclose(full[name]["W"], three[name]["W"], rtol=0, atol=1e-11, err_msg=name)
        np.testing.assert_allclose(full[name]["H"], three[name]["H"], rtol=0, atol=1e-11, err_msg=name)
