"""The cases of tests/duchi_start.py, on the CPU: the conditions that keep the GPU comparisons honest.  The float64 oracle is
well conditioned on every case (against the same arithmetic in long double: at most a tenth of every bound), the cases are
where they claim to be (the control drops nothing, the starts above the simplex drop most components over several rounds of
the active-set iteration, S = 0.25 has a negative tau, the row observed nowhere projects to 1 / K), the bounds bite (five
defects planted in a NumPy transcription of the kernels' loop all miss them by more than 1000 x -- two of them ONLY off the
simplex, which is the reason these cases exist), the transcription and the oracle's sort-based algorithm agree, and the band in
which the support rule is silent holds next to nothing.  A case that missed a condition would get another seed
(``duchi_start.SEED_SALT``) -- never a wider tolerance.  No GPU.
"""
import numpy as np
import pytest

import duchi_start as ds
from oracle import nbmf_oracle as orc

needs_long_double = pytest.mark.skipif(not ds.have_long_double(), reason="np.longdouble is no wider than float64 here")
ALL_CASES = ds.A_CASES + (ds.tall_case(),)
ids = ds.case_id


def _gaps(case, steps):
    ref, ext = ds.reference(case, steps), ds.extended(case, steps)
    return {"W": float(np.max(np.abs(ext.W - ref.W))) / ds.FACTOR_ATOL, "H": float(np.max(np.abs(ext.H - ref.H))) / ds.FACTOR_ATOL,
            "loss": float(np.max(np.abs(ext.losses - ref.losses) / np.abs(ref.losses))) / ds.LOSS_RTOL}


def test_cases_are_the_stated_ones():
    assert len(set(ds.A_CASES)) == len(ds.A_CASES) == 96 and len(set(map(ids, ds.A_CASES))) == 96 and len(ds.B_CASES) == 12
    assert {c.k for c in ds.A_CASES} == set(ds.KS) and {c.S for c in ds.A_CASES} == set(ds.STARTS)
    for k in ds.FULL_CROSS_KS:
        assert {(c.S, c.masked) for c in ds.A_CASES if c.k == k and c.storage == "auto" and not c.dup} == \
            {(S, mk) for S in ds.STARTS for mk in (False, True)}
    for storage in ds.STORAGE_BINARY_PATH:
        assert {c.k for c in ds.A_CASES if c.storage == storage and c.S == 12.0 and c.masked} == set(ds.KS)
    for c in ALL_CASES + ds.B_CASES:
        Y, mask, W0, H0 = ds.problem(c)
        assert Y.shape == (c.m, c.n) and W0.shape == (c.k, c.m) and H0.shape == (c.k, c.n) and not W0.flags.writeable
        assert set(np.unique(Y)) == {0.0, 1.0} and Y.mean() == pytest.approx(ds.ONES_SHARE, abs=0.03)
        np.testing.assert_allclose(W0.sum(axis=0), c.S, rtol=1e-14)          # dup or not: the S = 1 control is on the simplex
        assert W0.min() > 0 and (c.k == 1 or (W0.max(axis=0) / W0.min(axis=0)).max() > 20)     # spiky
        assert 0.02 <= H0.min() and H0.max() <= min(0.9, 0.9 / c.S) and (W0.T @ H0).max() < 0.9
        if c.masked:
            assert mask.dtype == np.bool_ and mask.mean() == pytest.approx(ds.OBSERVED_SHARE, abs=0.05)
            small = (c.m, c.n) == (ds.M, ds.N)
            assert not mask[ds.dead_row(c)].any() and mask[ds.SINGLE_ROW if small else ds.TALL_SINGLE_ROW].sum() == 1
        else:
            assert mask is None
        if c.dup:
            assert np.array_equal(W0[1], W0[2]) and np.array_equal(H0[1], H0[2])
        else:
            assert c.k < 3 or not np.array_equal(W0[1], W0[2])
    # one K, one mask setting: one data set (the batched case needs it)
    a, b = (ds.problem(ds.Case(ds.D_K, S, True, "auto", False, ds.M, ds.N)) for S in (0.25, 12.0))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[2], b[2])
    # 70 rows: 6 live columns in the last block of 32 and in the last tile of 16
    assert ds.M % 32 == 6 and ds.M % 16 == 6 and ds.DEAD_ROW >= ds.M - 6
    # the tall case: on 256 compute units 33000 rows are 1032 blocks against 4 x 256, one more row block than the bound
    assert ds.w_update_groups(ds.TALL_M, 256) == 8 and ds.w_update_groups(32768, 256) == 32 and ds.tall_rows(256) == ds.TALL_M
    assert ds.tall_rows(304) == 4 * 304 * 32 + 1 <= ds.TALL_MAX_M and ds.tall_rows(1024) > ds.TALL_MAX_M
    assert ds.w_update_groups(ds.M, 256) == 32


@pytest.mark.parametrize("case", ALL_CASES + ds.B_CASES, ids=ids)
def test_reference_is_the_oracles_step(case):
    """The helper's pre-projection column and tau ARE the oracle's: max(v - tau, 0) is ``orc.mm_step_duchi``'s W bit for
    bit, and ``pre_projection``'s H its H."""
    Y, mask, W0, H0 = ds.problem(case)
    ref = ds.reference(case)
    v, H1, counts = ds.pre_projection(Y, W0, H0, mask, ds.ALPHA, ds.BETA, ds.EPS)
    np.testing.assert_array_equal(v / counts, ref.v)
    np.testing.assert_array_equal(H1, ref.H)
    np.testing.assert_array_equal(np.maximum(ref.v - ref.tau[None, :], 0.0), ref.W)
    W1, H1o = orc.mm_step_duchi(Y, W0, H0, mask, ds.ALPHA, ds.BETA, ds.EPS)
    np.testing.assert_array_equal(W1, ref.W)
    np.testing.assert_array_equal(H1o, ref.H)
    assert ref.losses[0] == orc.mm_loss(Y, W1, H1o, mask, ds.ALPHA, ds.BETA, ds.EPS)
    np.testing.assert_allclose(ref.W.sum(axis=0), 1.0, rtol=0, atol=ds.SIMPLEX_ATOL / 100)


@needs_long_double
@pytest.mark.parametrize("case", ALL_CASES, ids=ids)
def test_one_step_is_well_conditioned(case):
    """Float64 against long double: W, H and the loss within a tenth of the bound a kernel is held to (measured: 1e-6 of it,
    absolute 1e-15)."""
    g = _gaps(case, 1)
    print(ids(case), "float64 / long double gap: W %.2g, H %.2g, loss %.2g of the bounds" % (g["W"], g["H"], g["loss"]))
    assert ds.extended(case).W.dtype == np.longdouble
    assert max(g.values()) <= 0.1, g


@needs_long_double
@pytest.mark.parametrize("case", ds.B_CASES, ids=ids)
def test_chained_steps_are_well_conditioned(case):
    g = _gaps(case, ds.B_STEPS)
    print(ids(case), "after %d steps: W %.2g, H %.2g, losses %.2g of the bounds" % (ds.B_STEPS, g["W"], g["H"], g["loss"]))
    assert max(g.values()) <= 0.1, g


@pytest.mark.parametrize("case", ds.B_CASES, ids=ids)
def test_on_the_simplex_the_projection_lifts_the_zeros(case):
    """What the chained cases can and cannot ask.  Step 1 drops most components: W is then on the simplex and mostly exact
    zeros.  From a column that sums to 1 the pre-projection column sums to 1 - O(eps) -- each term of the sum over j is
    Theta / (Theta + eps) or (1 - Theta) / (1 - Theta + eps) --, so tau is NEGATIVE (-1e-10 ... -1e-9) and the Euclidean
    projection adds -tau to every entry, the zeros included: in the oracle (float64 and long double alike) NONE of the zeros of
    step 1 is a zero after step 2 or 3.  "Zeros stay exact zeros" is therefore not a property of this projection; what holds,
    exactly, is that the zeros of a column leave step 2 with ONE common value, -tau of that column (max(0 - tau, 0) for each of
    them), and that is what the GPU test asks bit for bit."""
    refs = [ds.reference(case, s) for s in (1, 2, 3)]
    zero = refs[0].zero_after_first
    assert 0.7 < zero.mean() < 0.99                                    # the sparse regime iteration 2 starts from
    for ref in refs[1:]:
        live = np.ones(case.m, dtype=bool)
        if case.masked:
            live[ds.dead_row(case)] = False
        assert (ref.tau[live] < 0).all() and ref.tau[live].min() > -1e-6
        assert (ref.W[zero] > 0).all()
    if ds.have_long_double():
        assert (ds.extended(case, 3).W[zero] > 0).all()
    W2, tau2 = refs[1].W, refs[1].tau
    for i in range(case.m):
        z = zero[:, i]
        if z.any():
            assert (W2[z, i] == -tau2[i]).all()


@pytest.mark.parametrize("case", ALL_CASES, ids=ids)
def test_cases_are_what_they_claim(case):
    """The control drops nothing and its pre-projection columns sum to 1 within 1e-6; S >= 1.6 at K >= 17 drops more than half
    of the components and takes at least 3 rounds in some column; S = 0.25 has a negative tau everywhere; the row observed
    nowhere projects to exactly 1 / K; and the transcription of the kernels' loop agrees with the oracle's sort-based
    algorithm to 1e-14 (W and tau)."""
    ref = ds.reference(case)
    w, tau, rounds = ds.michelot(ref.v)
    live = np.ones(case.m, dtype=bool)
    if case.masked:
        dead = ds.dead_row(case)
        live[dead] = False
        assert (ref.v[:, dead] == 0).all() and (ref.W[:, dead] == 1.0 / case.k).all() and (w[:, dead] == 1.0 / case.k).all()
    dropped = float((ref.W[:, live] == 0).mean())
    print(ids(case), "dropped %.2f of the entries, rounds %d ... %d, tau %.3g ... %.3g, transcription off by %.1e"
          % (dropped, rounds[live].min(), rounds[live].max(), ref.tau[live].min(), ref.tau[live].max(), np.max(np.abs(w - ref.W))))
    assert np.max(np.abs(w - ref.W)) <= 1e-14 and np.max(np.abs(tau - ref.tau)) <= 1e-14
    assert np.array_equal(w == 0, ref.W == 0)
    assert rounds.min() >= 1 and rounds.max() <= case.k
    if case.S == 1.0:
        assert dropped == 0.0 and (rounds == 1).all()
        assert np.max(np.abs(ref.v[:, live].sum(axis=0) - 1.0)) <= 1e-6
    if case.S == 0.25:
        assert (ref.tau < 0).all() and ref.tau[live].max() < -1e-3 and dropped == 0.0 and (rounds == 1).all()
    if case.S >= 1.6 and case.k >= 17:
        assert dropped > 0.5 and rounds.max() >= 3


@pytest.mark.parametrize("case", ALL_CASES, ids=ids)
def test_support_band_holds_at_most_one_percent(case):
    dropped, kept, band = ds.support(case)
    print(ids(case), "band share %.4f, dropped %.3f, kept %.3f" % (band.mean(), dropped.mean(), kept.mean()))
    assert band.mean() <= ds.BAND_SHARE_MAX
    ref = ds.reference(case)                                 # outside the band the float64 oracle is on the stated side
    assert (ref.W[dropped] == 0).all() and (ref.W[kept] > 0).all()


def _miss(case, name):
    d = np.abs(ds.mutant_step(case, name) - ds.reference(case).W)
    return float("inf") if np.isnan(d).any() else float(d.max()) / ds.FACTOR_ATOL


@pytest.mark.parametrize("name", ds.MUTANTS)
def test_bounds_bite(name):
    """Each planted defect misses the W bound of the GPU test by more than 1000 x on at least one case; leaving the loop
    after one round, or dividing by K instead of the active count, stays WITHIN the bound on every S = 1 control -- so no
    assertion from an on-simplex start could have caught either."""
    miss = {c: _miss(c, name) for c in ds.A_CASES}
    worst = max(miss, key=miss.get)
    control = max(v for c, v in miss.items() if c.S == 1.0)
    print(name, "misses the bound by %.3g x on %s (%d of %d cases beyond 1000 x); on the controls %.3g of the bound"
          % (miss[worst], ids(worst), sum(v > 1000 for v in miss.values()), len(miss), control))
    assert miss[worst] > 1000.0
    if name in ("one-round", "K-divisor"):
        assert control <= 1.0
        off = [v for c, v in miss.items() if c.S >= 1.6 and c.k >= 17]
        assert min(off) > 1000.0                              # ... and every case above the simplex at K >= 17 catches it
    if name == "N-count":
        # (K = 1 projects any positive number to 1: only the NaN of a zero count shows there)
        assert all(v > 1000.0 for c, v in miss.items() if c.masked and c.k >= 2)
        assert all(v <= 1e-5 for c, v in miss.items() if not c.masked or c.k == 1)      # (nothing to get wrong there)
    if name == "no-max-count":
        assert all(v == float("inf") for c, v in miss.items() if c.masked)


def test_the_unmutated_transcription_passes():
    """The harness of the teeth test itself: with no defect planted the same comparison stands at 1e-5 of the bound."""
    for c in ds.A_CASES:
        assert np.max(np.abs(ds.michelot(ds.reference(c).v)[0] - ds.reference(c).W)) <= 1e-5 * ds.FACTOR_ATOL
