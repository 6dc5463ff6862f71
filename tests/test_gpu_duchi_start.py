"""GPU parity of ``projection="duchi"`` from starts OFF the simplex (tests/duchi_start.py), where the projection drops most
components and Michelot's iteration takes 3 to 8 rounds -- from a start on the simplex it is the identity to within eps and
ends in its first round, so no fit that starts there shows whether the later rounds, the ``(s - 1) / c2`` divisor, the
``c2 == 0`` exit or the LDS tile above one layout's worth of components are right.

  A  one step at K = 1 ... 512 on the three storage paths: every entry of W and H to 1e-9 of the float64 oracle, the loss to
     1e-10, the SUPPORT (exact 0.0 where the long-double v - tau is below -1e-9, positive where it is above +1e-9), column
     sums, the row observed nowhere at exactly 1 / K; K <= 32 on the persistent kernel's epilogue AND on w_update_kernel, the
     two against each other at 1e-12;
  B  three chained iterations from S = 3 and 12: iteration 2 starts from a W that is mostly exact zeros;
  C  33000 rows: the 8-group instantiation of w_update_kernel (derived from the device's compute units);
  D  three starts and three priors in one ``run_batch`` call, bit for bit the sequential runs, on the persistent launch;
  E  two identical components stay identical, kept together or dropped together.

tests/test_duchi_start_cpu.py shows on the CPU that the oracle is well conditioned on every case (float64 against long double:
1e-6 of each bound), that five planted defects of the projection miss these bounds by more than 1000 x, and that the one-round
and K-divisor defects pass on the S = 1 control.

Measured on an MI355X, 256 compute units (largest deviation per group as a fraction of its bound; every test prints its own):
  A  persistent kernel (50 cases)   W 1.8e-6  H 3.3e-7  loss 5.0e-6  column sums 1.8e-3
     w_update_kernel<32>, K <= 32   W 1.8e-6  H 2.8e-6  loss 5.3e-6  column sums 1.3e-3;  the two engines' W 8.9e-4 of 1e-12
     w_update_kernel<32>, K >= 40   W 1.8e-6  H 2.2e-7  loss 3.5e-6  column sums 2.7e-3
  B  after 1 / 2 / 3 iterations     W 1.4e-6  H 1.5e-6  loss 3.8e-6  column sums 6.0e-3  (K = 17 persistent, 40 and 130 launches)
  C  w_update_kernel<8>, 33000 rows W 6.7e-7  H 1.1e-7  loss 4.5e-6  column sums 5.6e-4
  D  one persistent launch, 3 fits  bit for bit; against the oracle W 4.4e-7  H 3.3e-7  loss 2.5e-6
  E  rows 1 and 2 of W              bit for bit equal on every engine (bound 1e-12)
"""
import ctypes

import numpy as np
import pytest

import duchi_start as ds

pytestmark = pytest.mark.gpu

SMALL_CASES = tuple(c for c in ds.A_CASES if c.k <= ds.SMALL_ENGINE_MAX_K)
LARGE_CASES = tuple(c for c in ds.A_CASES if c.k > ds.SMALL_ENGINE_MAX_K)
DUP_CASES = tuple(c for c in ds.A_CASES if c.dup)


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


_runs = {}
PERSISTENT_FLAG = {"single-launch": "1", "five-kernels": "0"}


def _device_run(hip, case, engine):
    """One step of the case on the named engine, once per session (the engine comparison and the duplicate check read the
    same results): ``(W, H, losses)``, after the engine counters have shown that the named engine served it."""
    if (case, engine) not in _runs:
        before = hip.engine_stats()
        out = ds.device_run(hip, case)
        served = tuple(a - b for a, b in zip(hip.engine_stats(), before))
        assert served == ((1, 0, 0) if engine == "single-launch" else (0, 0, 1)), f"{engine}: served {served}"
        _runs[case, engine] = out
    return _runs[case, engine]


@pytest.mark.parametrize("case", SMALL_CASES, ids=ds.case_id)
def test_one_step_off_the_simplex_on_both_engines(hip, both_small_paths, case):
    """K <= 32: ``run(1)`` on the persistent kernel (its W epilogue projects) and on the launches (``w_update_kernel``, 32
    groups), each against the oracle's step; the engine counters show that the named engine ran."""
    W, H, losses = _device_run(hip, case, str(both_small_paths))
    ds.check_against_oracle("A " + both_small_paths, case, W, H, losses)


@pytest.mark.parametrize("case", SMALL_CASES, ids=ds.case_id)
def test_the_two_engines_project_alike(hip, monkeypatch, case):
    """The persistent kernel's epilogue and ``w_update_kernel`` face the same numbers: W within 1e-12 of each other, the same
    zeros outside the support band."""
    out = {}
    for engine, flag in PERSISTENT_FLAG.items():
        monkeypatch.setenv("NBMF_PERSISTENT", flag)
        out[engine] = _device_run(hip, case, engine)
    (Wp, Hp, lp), (Wl, Hl, ll) = out["single-launch"], out["five-kernels"]
    dev = float(np.max(np.abs(Wp - Wl)))
    print("A engines %s: W apart by %.3g = %.3g of the bound, H by %.3g, loss by %.3g relative"
          % (ds.case_id(case), dev, dev / ds.ENGINES_ATOL, np.max(np.abs(Hp - Hl)), abs(lp[0] - ll[0]) / abs(ll[0])))
    assert dev <= ds.ENGINES_ATOL
    _, _, band = ds.support(case)
    assert np.array_equal((Wp == 0)[~band], (Wl == 0)[~band])


@pytest.mark.parametrize("case", LARGE_CASES, ids=ds.case_id)
def test_one_step_off_the_simplex_above_32_components(hip, case):
    """K = 40 ... 512 on the launches: the K = 64 and 128 layouts, and two and four slices of 128 -- above 128 components the
    tile of ``w_update_kernel`` ((KP + 2) x 32 doubles, KP = 256 or 512) needs the raised dynamic-LDS attribute."""
    W, H, losses = _device_run(hip, case, "launches")
    if case.k > 128:
        assert (-(-case.k // 128) * 128 + 2) * ds.WU_COLS * 8 > 65536
    ds.check_against_oracle("A launches", case, W, H, losses)


@pytest.mark.parametrize("case", ds.B_CASES, ids=ds.case_id)
def test_three_chained_iterations(hip, monkeypatch, case):
    """``run(3)`` against three oracle steps: all three losses, the final factors, the support of the last projection.
    Iteration 2 starts from a W on the simplex that is mostly exact zeros; its pre-projection column sums to 1 - O(eps), so
    tau is negative and the projection lifts every entry by -tau, the zeros included (in the oracle too:
    test_duchi_start_cpu.py::test_on_the_simplex_the_projection_lifts_the_zeros) -- so what is held exactly is: an entry the
    oracle has at 0 after step 1 is 0.0 on the device after step 1, and after step 2 all such entries of a column carry ONE
    value, bit for bit, which is -tau of the oracle to 1e-9."""
    monkeypatch.setenv("NBMF_PERSISTENT", "1")
    Y, mask, W0, H0 = ds.problem(case)
    out = []
    before = hip.engine_stats()
    with hip.Context(case.m, case.n, case.k) as ctx:
        ctx.set_hyper(ds.ALPHA, ds.BETA, ds.EPS, hip.PROJ_DUCHI)
        assert ctx.upload(Y, mask=mask) is True
        for steps in (1, 2, ds.B_STEPS):
            ctx.set_factors(W0, H0)
            losses, n_iter = ctx.run(steps, 0.0)
            assert n_iter == steps
            out.append(ctx.get_factors() + (losses,))
    served = tuple(a - b for a, b in zip(hip.engine_stats(), before))
    assert served == ((3, 0, 0) if case.k <= ds.SMALL_ENGINE_MAX_K else (0, 0, 3))
    for steps, (W, H, losses) in zip((1, 2, ds.B_STEPS), out):
        ds.check_against_oracle("B %d step(s)" % steps, case, W, H, losses, steps)
    zero = ds.reference(case).zero_after_first
    _, _, band = ds.support(case)
    assert (out[0][0][zero & ~band] == 0.0).all()
    W2, tau2 = out[1][0], ds.reference(case, 2).tau
    for i in range(case.m):
        z = zero[:, i] & ~band[:, i]
        if z.any():
            assert (W2[z, i] == W2[z, i][0]).all() and abs(W2[z, i][0] + tau2[i]) <= ds.FACTOR_ATOL


def _compute_units(hip):
    """``multiProcessorCount`` of device 0, the figure ``enqueue_w_update`` goes by, asked of the HIP runtime this process has
    loaded (hipDeviceGetAttribute, hipDeviceAttributeMultiprocessorCount = 63 in hip_runtime_api.h)."""
    value = ctypes.c_int(0)
    rc = hip.load().hipDeviceGetAttribute(ctypes.byref(value), 63, 0)     # (resolved through the library's own dependency)
    assert rc == 0 and 0 < value.value <= 4096, (rc, value.value)
    return value.value


def test_tall_case_takes_the_8_group_kernel(hip):
    """More than 4 x CUs blocks of 32 rows: ``w_update_kernel<8>``.  The row count follows from the device's compute units
    (256 on an MI355X: 33000 rows are 1032 blocks against 1024); the data are binary with a mask, K = 3, S = 3."""
    cus = _compute_units(hip)
    m = ds.tall_rows(cus)
    if m > ds.TALL_MAX_M:
        pytest.skip(f"{cus} compute units: the 8-group kernel needs {m} rows, more than {ds.TALL_MAX_M}")
    case = ds.tall_case(m)
    assert ds.w_update_blocks(m) > 4 * cus and ds.w_update_groups(m, cus) == 8 and ds.w_update_groups(ds.M, cus) == 32
    before = hip.engine_stats()
    W, H, losses = ds.device_run(hip, case)
    assert tuple(a - b for a, b in zip(hip.engine_stats(), before)) == (0, 0, 1)
    print("C %d compute units, %d rows, %d blocks of 32 > %d: 8 groups" % (cus, m, ds.w_update_blocks(m), 4 * cus))
    ds.check_against_oracle("C", case, W, H, losses)


def test_run_batch_of_three_starts_and_priors(hip, monkeypatch):
    """One K = 17 context: starts with column sums 0.25, 1.6 and 12 under the priors (1, 1), (1.2, 1.2), (2, 1.5), three
    iterations, in ONE ``run_batch`` call -- bit for bit the three sequential runs, served by one persistent launch; the
    (1.2, 1.2) problem also against the oracle."""
    monkeypatch.setenv("NBMF_PERSISTENT", "1")
    cases = [ds.Case(ds.D_K, S, True, "auto", False, ds.M, ds.N) for S in ds.D_STARTS]
    Y, mask = ds.problem(cases[0])[:2]
    W0 = np.stack([ds.problem(c)[2] for c in cases])
    H0 = np.stack([ds.problem(c)[3] for c in cases])
    alphas, betas = (np.array(v) for v in zip(*ds.D_PRIORS))
    with hip.Context(ds.M, ds.N, ds.D_K) as ctx:
        ctx.set_hyper(ds.ALPHA, ds.BETA, ds.EPS, hip.PROJ_DUCHI)
        assert ctx.upload(Y, mask=mask) is True
        curves, n_iters, Ws, Hs = ctx.run_batch(alphas, betas, W0, H0, ds.D_STEPS, 0.0)
        launches, served = ctx.batch_stats()
        seq = []
        for p in range(3):
            ctx.set_hyper(alphas[p], betas[p], ds.EPS, hip.PROJ_DUCHI)
            ctx.set_factors(W0[p], H0[p])
            losses, n_iter = ctx.run(ds.D_STEPS, 0.0)
            seq.append((losses, n_iter) + ctx.get_factors())
    print("D persistent launches %d, problems served %d" % (launches, served))
    assert (launches, served) == (1, 3)
    for p in range(3):
        losses, n_iter, W, H = seq[p]
        assert n_iters[p] == n_iter == ds.D_STEPS
        np.testing.assert_array_equal(curves[p], losses)
        np.testing.assert_array_equal(Ws[p], W)
        np.testing.assert_array_equal(Hs[p], H)
        assert (Ws[p] >= 0).all() and np.max(np.abs(Ws[p].sum(axis=0) - 1.0)) <= ds.SIMPLEX_ATOL
        assert (Ws[p][:, ds.DEAD_ROW] == 1.0 / ds.D_K).all()
    ds.check_against_oracle("D", cases[1], Ws[1], Hs[1], curves[1], ds.D_STEPS)


@pytest.mark.parametrize("case", DUP_CASES, ids=ds.case_id)
def test_identical_components_stay_identical(hip, monkeypatch, case):
    """Components 1 and 2 start identical (rows of W and of H): they tie in every pre-projection column.  After the step the
    device's two rows of W agree to 1e-12 and are kept together or dropped together outside the support band -- on both
    engines where K <= 32."""
    _, _, band = ds.support(case)
    clear = ~(band[1] | band[2])
    for engine in PERSISTENT_FLAG if case.k <= ds.SMALL_ENGINE_MAX_K else ("launches",):
        if engine in PERSISTENT_FLAG:
            monkeypatch.setenv("NBMF_PERSISTENT", PERSISTENT_FLAG[engine])
        W, H, _ = _device_run(hip, case, engine)
        dev = float(np.max(np.abs(W[1] - W[2])))
        print("E %s %s: rows 1 and 2 of W apart by %.3g (%.3g of the bound), of H by %.3g; %d of %d columns drop both"
              % (engine, ds.case_id(case), dev, dev / ds.ENGINES_ATOL, np.max(np.abs(H[1] - H[2])), int((W[1] == 0).sum()), case.m))
        assert dev <= ds.ENGINES_ATOL
        assert np.array_equal((W[1] == 0)[clear], (W[2] == 0)[clear])
