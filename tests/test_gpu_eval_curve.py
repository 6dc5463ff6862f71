"""Held-out log-likelihood on the device and early stopping inside a run: nbmf_set_eval, nbmf_eval_loglik, nbmf_get_eval,
nbmf_get_best_factors (Context.set_eval, eval_loglik, eval_curve, best_factors) and NBMF.fit(eval_mask=...).

REFERENCE.  The sum is always compared with ``host_eval_loglik(ctx.predict_at(rows, cols, clip_theta=False), x, eps)``
(tests/test_eval_curve_cpu.py: NumPy's logarithm, ``math.fsum``).  The device scores the very Theta predict_at returns and
forms the logarithm's argument in the same order, so what separates the two is the logarithm (both within 1 ulp), the
roundings of a term and the summation order:

    |got - want| <= (count + 8) 2^-52 sum|t|                                   (eval_bound)

Wherever two device results are compared with each other (repeats, another every / patience, a value recorded inside a run
against the same factors evaluated on their own, runs with and without an eval set) they are equal BIT FOR BIT.

SHAPES.  37 x 297 with K = 5 (a ragged count of k per lane), 64 (a full layout) and 130 (the sliced factor layout); pair
counts 1, 31, 33, 2049 and m n: below, across and far beyond the 32 pairs of one workgroup, so that the fold has many
partials.  Runs: 100 x 500, K = 6 (the single-launch engine would serve it, and must not) and 512 x 512, K = 64 (never
qualifies for it).  Every fit here takes milliseconds."""
import numpy as np
import pytest

from conftest import config1_X, config1_mask, midsize_XM
from test_eval_curve_cpu import PLANTED, eval_bound, host_eval_loglik, oracle_curve, planted_case, planted_init, stop_rule
from test_gpu_score_samples import case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def pairs_of(m, n, count, seed):
    """``count`` unsorted pairs with repeats and their truth as bytes (nonzero, not just 1, means 1)."""
    r = np.random.default_rng(seed)
    x = (r.random(count) < 0.3).astype(np.uint8) * r.integers(1, 256, count, dtype=np.uint8)
    return r.integers(0, m, count), r.integers(0, n, count), x


# ---- 1. the kernel against the host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 64, 130])
def test_sum_against_the_host(hip, k):
    m, n = 37, 297
    W, H, _, _ = case(k, m, n)
    with hip.Context(m, n, k) as ctx:
        ctx.set_factors(W, H)
        for count in (1, 31, 33, 2049, m * n):
            rows, cols, x = pairs_of(m, n, count, 100 + count)
            if count == m * n:                       # every entry once, shuffled, and then some of them again
                p = np.random.default_rng(7).permutation(m * n)
                rows, cols = p // n, p % n
            ctx.set_eval(rows, cols, x, every=10, patience=0)
            got = ctx.eval_loglik()
            want, abs_sum = host_eval_loglik(ctx.predict_at(rows, cols, clip_theta=False), x, 1e-8)
            bound = eval_bound(count, abs_sum)
            print(f"K={k} count={count}: got {got!r} want {want!r} error / bound = {abs(got - want) / bound:.3f}")
            assert abs(got - want) <= bound
            assert same_bits(ctx.eval_loglik(), got)                       # the same call twice
            ctx.set_eval(rows, cols, x, every=3, patience=7)                # every / patience do not enter the sum
            assert same_bits(ctx.eval_loglik(), got)
            ctx.set_eval(rows, cols, (x != 0), every=1, patience=0)         # bool truth is the same as bytes
            assert same_bits(ctx.eval_loglik(), got)
            p = np.random.default_rng(count).permutation(count)            # another order: another sum, inside the bound
            ctx.set_eval(rows[p], cols[p], x[p])
            assert abs(ctx.eval_loglik() - want) <= bound


def test_eps_of_set_hyper_enters_the_term(hip):
    m, n, k = 37, 297, 5
    W, H, _, _ = case(k, m, n)
    rows, cols, x = pairs_of(m, n, 333, 5)
    with hip.Context(m, n, k) as ctx:
        ctx.set_hyper(1.2, 1.2, 1e-3)
        ctx.set_factors(W, H)
        ctx.set_eval(rows, cols, x)
        theta = ctx.predict_at(rows, cols, clip_theta=False)
        want, abs_sum = host_eval_loglik(theta, x, 1e-3)
        assert abs(ctx.eval_loglik() - want) <= eval_bound(333, abs_sum)
        assert abs(ctx.eval_loglik() - host_eval_loglik(theta, x, 1e-8)[0]) > eval_bound(333, abs_sum)


# ---- 2. errors ---------------------------------------------------------------------------------------------------------------
def test_errors_and_what_they_leave_in_place(hip):
    m, n, k = 37, 297, 5
    W, H, X, mask = case(k, m, n)
    rows, cols, x = pairs_of(m, n, 100, 1)
    none = np.zeros(0, dtype=np.int64)
    with hip.Context(m, n, k) as ctx:
        ctx.set_eval(rows, cols, x)
        with pytest.raises(hip.NBMFHipError, match="no factors"):          # an eval set, no factors
            ctx.eval_loglik()
        ctx.set_factors(W, H)
        got = ctx.eval_loglik()
        # a pair out of range names the LOWEST offending position and leaves the eval set in place working
        for bad_r, bad_c in ((m, 0), (-1, 0), (0, n), (0, -1)):
            r2, c2 = rows.copy(), cols.copy()
            r2[[41, 77]], c2[[41, 77]] = bad_r, bad_c
            with pytest.raises(ValueError, match=r"position 41 is outside \[0, 37\) x \[0, 297\)"):
                ctx.set_eval(r2, c2, x)
            assert same_bits(ctx.eval_loglik(), got)
        for every, patience in ((0, 0), (-2, 0), (1, -1)):
            with pytest.raises(ValueError, match="every|patience"):
                ctx.set_eval(rows, cols, x, every=every, patience=patience)
        assert same_bits(ctx.eval_loglik(), got)
        # count = 0 switches evaluation off
        ctx.set_eval(none, none, np.zeros(0, dtype=np.uint8))
        with pytest.raises(hip.NBMFHipError, match="no eval set"):
            ctx.eval_loglik()
        with pytest.raises(hip.NBMFHipError, match="no evaluation"):      # no run has made one
            ctx.best_factors()
        assert ctx.eval_curve()[0].size == 0
        # a communicator and an eval set do not go together, either way round (one rank is enough to attach one)
        ctx.upload(X, mask=mask)
        ctx.comm_init_host(lambda arr: None, 1, 0, 0)
        with pytest.raises(hip.NBMFHipError, match="unsharded"):
            ctx.set_eval(rows, cols, x)
        ctx.comm_detach()
        ctx.set_eval(rows, cols, x)
        with pytest.raises(hip.NBMFHipError, match="eval set"):
            ctx.comm_init_host(lambda arr: None, 1, 0, 0)
        assert same_bits(ctx.eval_loglik(), got)
        with pytest.raises(hip.NBMFHipError, match="eval set"):           # nbmf_run_batch does not evaluate
            ctx.run_batch([1.2], [1.2], W, H, 3, 0.0)


# ---- 3. the curve inside a run ---------------------------------------------------------------------------------------------
def problem(hip, X, mask, k, alpha=1.2, beta=1.2):
    ctx = hip.Context(X.shape[0], X.shape[1], k)
    ctx.set_hyper(alpha, beta, 1e-8)
    ctx.upload(X, mask=mask)
    W0, H0 = planted_init(X.shape[0], k, X.shape[1], 0)
    ctx.set_factors(W0, H0)
    return ctx


def heldout(X, ev):
    r, c = np.nonzero(ev)
    return r, c, (X[r, c] != 0).astype(np.uint8)


@pytest.mark.parametrize("shape", ["config1", "midsize"])
def test_curve_inside_a_run(hip, monkeypatch, shape):
    if shape == "config1":
        X, mask, k, max_iter, every = config1_X(), config1_mask(), 6, 23, 5
        labels = [5, 10, 15, 20, 23]
    else:
        X, mask = midsize_XM()
        k, max_iter, every = 64, 7, 3
        labels = [3, 6, 7]
    mask = np.asarray(mask) != 0
    pairs = heldout(X, ~mask)
    monkeypatch.delenv("NBMF_PERSISTENT", raising=False)
    monkeypatch.delenv("NBMF_USE_GRAPH", raising=False)
    s0 = hip.engine_stats()
    with problem(hip, X, mask, k) as ctx:
        ctx.set_eval(*pairs, every=every, patience=0)
        losses, n_iter = ctx.run(max_iter, 0.0)
        iters, lls, best_iter, early = ctx.eval_curve()
        Wf, Hf = ctx.get_factors()
        Wb, Hb = ctx.best_factors()
        last = ctx.eval_loglik()
    s1 = hip.engine_stats()
    assert (s1[0] - s0[0], s1[2] - s0[2]) == (0, 1), "a run with an eval set is served by the launch engine"
    assert n_iter == max_iter and iters.tolist() == labels and not early
    assert best_iter == iters[int(np.argmax(lls))]
    assert same_bits(lls[-1], last)
    # without an eval set: the single-launch engine still serves the small shape ...
    with problem(hip, X, mask, k) as ctx:
        ctx.run(max_iter, 0.0)
        assert ctx.eval_curve()[0].size == 0
    s2 = hip.engine_stats()
    assert (s2[0] - s1[0], s2[2] - s1[2]) == ((1, 0) if shape == "config1" else (0, 1))
    # ... and under the launch engine the losses and the factors are those of the run with the eval set, bit for bit
    monkeypatch.setenv("NBMF_PERSISTENT", "0")
    with problem(hip, X, mask, k) as ctx:
        plain_losses, plain_n = ctx.run(max_iter, 0.0)
        Wp, Hp = ctx.get_factors()
    assert plain_n == n_iter and same_bits(plain_losses, losses) and same_bits(Wp, Wf) and same_bits(Hp, Hf)
    # the entry at label s is eval_loglik() of a fresh context after run(s, 0.0) from the same init; the snapshot is the
    # factors of run(best_iter, 0.0)
    for s, ll in zip(labels, lls):
        with problem(hip, X, mask, k) as ctx:
            ctx.run(s, 0.0)
            ctx.set_eval(*pairs, every=1, patience=0)
            assert same_bits(ctx.eval_loglik(), ll), f"label {s}"
            if s == best_iter:
                Ws, Hs = ctx.get_factors()
                assert same_bits(Ws, Wb) and same_bits(Hs, Hb)


def test_progress_reports_are_delivered_at_the_looks(hip):
    X, mask = config1_X(), config1_mask()
    with problem(hip, X, mask, 6) as ctx:
        ctx.set_eval(*heldout(X, ~mask), every=5, patience=0)
        calls = []
        ctx.set_progress(lambda first, vals: calls.append((first, list(vals))), every=10)
        losses, n_iter = ctx.run(23, 0.0)
        ctx.set_progress(None)
    assert [f for f, _ in calls] == sorted(f for f, _ in calls)
    assert [v for _, vals in calls for v in vals] == list(losses) and n_iter == 23
    assert len(calls) >= 5                                                   # a look behind every batch of 5


# ---- 4. a tol stop between two multiples ----------------------------------------------------------------------------------
@pytest.mark.parametrize("on_a_multiple", [False, True])
def test_tol_stop_is_recorded_under_n_iter(hip, monkeypatch, on_a_multiple):
    X, mask = config1_X(), config1_mask()
    pairs = heldout(X, ~mask)
    monkeypatch.setenv("NBMF_PERSISTENT", "0")
    with problem(hip, X, mask, 6) as ctx:
        curve, _ = ctx.run(40, 0.0)
    rel = np.abs(curve[:-1] - curve[1:]) / np.abs(curve[:-1])                 # rel[i - 1]: the stop test of iteration i
    # the first i >= 6 (n_iter = i + 1 off / on a multiple of 5) whose test value lies below every earlier one: a tol
    # between the two stops the plain run exactly there
    want = next(i for i in range(6, 39)
                if ((i + 1) % 5 == 0) == on_a_multiple and rel[i - 1] < 0.99 * rel[:i - 1].min())
    tol = float(np.sqrt(rel[want - 1] * rel[:want - 1].min()))
    with problem(hip, X, mask, 6) as ctx:
        plain_losses, n_iter = ctx.run(40, tol)
        Wp, Hp = ctx.get_factors()
    assert n_iter == want + 1 and ((n_iter % 5 == 0) == on_a_multiple)
    with problem(hip, X, mask, 6) as ctx:
        ctx.set_eval(*pairs, every=5, patience=0)
        losses, got_n = ctx.run(40, tol)
        iters, lls, _, early = ctx.eval_curve()
        W, H = ctx.get_factors()
        last = ctx.eval_loglik()
    assert got_n == n_iter and same_bits(losses, plain_losses) and same_bits(W, Wp) and same_bits(H, Hp)
    assert iters.tolist() == [s for s in range(5, n_iter, 5)] + [n_iter] and not early
    assert same_bits(lls[-1], last)


# ---- 5. early stopping ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_run(hip):
    """The planted case on the device with patience 3, once: what the run and the context hold afterwards."""
    import os
    p = PLANTED
    X, train, ev = planted_case()
    with problem(hip, X, train, p["K"], p["alpha"], p["beta"]) as ctx:
        ctx.set_eval(*heldout(X, ev), every=p["every"], patience=p["patience"])
        losses, n_iter = ctx.run(p["max_iter"], 0.0)
        out = dict(losses=losses, n_iter=n_iter, curve=ctx.eval_curve(), final=ctx.get_factors(), best=ctx.best_factors(),
                   last=ctx.eval_loglik())
    old = os.environ.get("NBMF_PERSISTENT")
    os.environ["NBMF_PERSISTENT"] = "0"
    try:
        for name, s in (("at_best", out["curve"][2]), ("at_stop", n_iter)):
            with problem(hip, X, train, p["K"], p["alpha"], p["beta"]) as ctx:
                out[name + "_losses"] = ctx.run(int(s), 0.0)[0]
                out[name] = ctx.get_factors()
    finally:
        if old is None:
            del os.environ["NBMF_PERSISTENT"]
        else:
            os.environ["NBMF_PERSISTENT"] = old
    return out


def test_early_stop_follows_the_rule_on_the_oracles_curve(planted_run):
    p = PLANTED
    labels, sums, count = oracle_curve()
    stop_s, best_s, early = stop_rule(labels, sums, p["every"], p["patience"])
    iters, lls, best_iter, stopped = planted_run["curve"]
    print("device mean held-out log-likelihood:", dict(zip(iters.tolist(), np.round(lls / count, 5))))
    assert early and stopped
    assert planted_run["n_iter"] == stop_s and best_iter == best_s
    assert iters.tolist() == [s for s in labels if s <= stop_s]
    assert stop_rule(iters.tolist(), lls.tolist(), p["every"], p["patience"]) == (stop_s, best_s, True)
    # the run ended as one with max_iter = n_iter would: its losses and factors, and the last value is of those factors
    assert len(planted_run["losses"]) == stop_s and same_bits(planted_run["losses"], planted_run["at_stop_losses"])
    assert all(same_bits(a, b) for a, b in zip(planted_run["final"], planted_run["at_stop"]))
    assert same_bits(lls[-1], planted_run["last"])
    # the snapshot is the factors of run(best_iter, 0.0) from the same init
    assert all(same_bits(a, b) for a, b in zip(planted_run["best"], planted_run["at_best"]))


def fit_planted(transposed=False, **kw):
    from nbmf_mm_amd import NBMF
    p = PLANTED
    X, train, ev = planted_case()
    t = (lambda a: np.ascontiguousarray(a.T)) if transposed else (lambda a: a)
    model = NBMF(n_components=p["K"], alpha=p["alpha"], beta=p["beta"], random_state=p["random_state"], tol=0,
                 max_iter=p["max_iter"], orientation="dir-beta" if transposed else "beta-dir")
    return model.fit(t(X), mask=t(train), eval_mask=t(ev), eval_every=p["every"], patience=p["patience"], **kw)


def test_estimator_restores_the_best_factors(hip, planted_run):
    from nbmf_mm_amd._solver import _touch_up
    iters, lls, best_iter, _ = planted_run["curve"]
    count = int(planted_case()[2].sum())
    model = fit_planted()
    assert model.n_iter_ == planted_run["n_iter"] and model.best_iter_ == best_iter and model.stopped_early_ is True
    assert np.array_equal(model.eval_iters_, iters) and same_bits(model.eval_loglik_, lls / count)
    assert same_bits(model.eval_perplexity_, np.exp(-(lls / count)))
    assert same_bits(model.loss_curve_, planted_run["losses"])               # the run's own, not the restored factors'
    Wb, Hb = planted_run["best"]
    W_want, H_want = _touch_up(Wb.T, Hb, "beta-dir")
    assert same_bits(model.W_, W_want) and same_bits(model.components_, H_want)
    # restore_best=False: the factors after n_iter_
    plain = fit_planted(restore_best=False)
    Wf, Hf = planted_run["final"]
    W_want, H_want = _touch_up(Wf.T, Hf, "beta-dir")
    assert same_bits(plain.W_, W_want) and same_bits(plain.components_, H_want)
    assert plain.best_iter_ == best_iter and same_bits(plain.eval_loglik_, model.eval_loglik_)
    # a fit without an eval set has none of the attributes
    X, train, _ = planted_case()
    model.set_params(max_iter=3).fit(X, mask=train)
    assert not any(hasattr(model, a) for a in ("eval_iters_", "eval_loglik_", "eval_perplexity_", "best_iter_", "stopped_early_"))


def test_last_perplexity_agrees_with_the_second_context_route(hip, planted_run):
    from nbmf_mm_amd import experiments
    X, train, ev = planted_case()
    iters, lls, _, _ = planted_run["curve"]
    count = int(ev.sum())
    got = float(np.exp(-lls[-1] / count))
    Wf, Hf = planted_run["final"]
    with hip.Context(100, 500, PLANTED["K"]) as second:
        second.set_hyper(1.0, 1.0, 1e-8)
        second.upload(X, mask=ev)
        want = experiments.heldout_perplexity(second, Wf, Hf)
        r, c, x = heldout(X, ev)
        abs_sum = host_eval_loglik(second.predict_at(r, c, clip_theta=False), x, 1e-8)[1]
    # the kernel's bound on the sum, through exp(-sum / count): d exp(-s / c) = p ds / c, plus the roundings of the
    # division and of exp on either side
    tol = want * np.expm1(eval_bound(count, abs_sum) / count) + 8 * 2.0 ** -52 * want
    print(f"perplexity: eval curve {got!r}, second context {want!r}, difference / tolerance = {abs(got - want) / tol:.3f}")
    assert abs(got - want) <= tol


def test_dir_beta_gives_the_same_curve(hip, planted_run):
    iters, lls, best_iter, _ = planted_run["curve"]
    count = int(planted_case()[2].sum())
    model = fit_planted(transposed=True)
    assert np.array_equal(model.eval_iters_, iters) and same_bits(model.eval_loglik_, lls / count)
    assert model.best_iter_ == best_iter and model.n_iter_ == planted_run["n_iter"] and model.stopped_early_
    Wb, Hb = planted_run["best"]
    assert np.allclose(model.W_, Hb.T, rtol=0, atol=1e-12) and np.allclose(model.components_, Wb, rtol=0, atol=1e-12)


def test_restarts_with_an_eval_set_run_one_after_the_other(hip):
    from nbmf_mm_amd import NBMF
    X, train, ev = planted_case()
    kw = dict(n_components=4, alpha=1.0, beta=1.0, tol=0, max_iter=12)
    fits = [NBMF(random_state=s, **kw).fit(X, mask=train, eval_mask=ev, eval_every=4) for s in (3, 4)]
    both = NBMF(random_state=3, n_init=2, **kw).fit(X, mask=train, eval_mask=ev, eval_every=4)
    keep = min(fits, key=lambda f: f.loss_curve_[-1])                        # the lowest final TRAINING loss, as without
    assert same_bits(both.loss_curve_, keep.loss_curve_) and same_bits(both.eval_loglik_, keep.eval_loglik_)
    assert both.eval_iters_.tolist() == [4, 8, 12] and both.stopped_early_ is False
    assert same_bits(both.W_, keep.W_) and same_bits(both.components_, keep.components_)
