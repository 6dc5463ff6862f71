"""Expected counts by sample, feature and group on the device (nbmf_moment_rows_v, Context.moments, NBMF.expected_counts,
_metrics.Moments): what can be said without a GPU -- the symbol is declared and exported, a null context is an argument
error, every malformed request raises ValueError BEFORE any device call, ``Moments`` against direct float computations on
Theta -- and the reference ``host_moments`` that tests/test_gpu_moments.py compares the device against for EQUALITY, checked
here on hand-written cases (theta = 0, 1, 0.5, the tie 2^-33, a NaN, a nonzero byte that is not 1, a fully masked row, an
empty group, label -1).

THE BOUNDS of the float properties, per slot, from the rounding of ONE entry (nothing here comes from what the code gives):
  q1 / Q is within 2^-33 of theta (rint of an exact product, Q = 2^32);
  q2 / Q is within 2^-33 + 2^-54 of theta^2 (the product theta * theta is rounded first: half an ulp of a value <= 1);
so, against ``math.fsum`` over the slot's entries (whose own terms carry at most 2^-52 each, allowed for as n_obs * 2^-50),
  |expected - fsum(theta)|               <= n_obs * 2^-33                                   (the issue's bound)
  |variance - fsum(theta * (1 - theta))| <= n_obs * (2^-32 + 2^-50)                          (q1 and q2, one each)
  |brier - fsum((x - theta)^2) / n_obs|  <= ((3 n_ones + n_zeros) * 2^-33 + n_obs * 2^-50) / n_obs
                                            (a one: 1 - 2 q1 / Q + q2 / Q, three roundings; a zero: q2 / Q, one)."""
import ctypes
import math
import os

import numpy as np
import pytest

from test_theta_hist_cpu import hist_case


def host_moments(theta, x, mask, groups, G):
    """The contract of nbmf_moment_rows_v in NumPy.  ``theta`` is what predict_rows returned with the clip on.  Observed = no
    mask or mask != 0; one = (x != 0); q1 = rint(theta * 2^32), q2 = rint((theta * theta) * 2^32) as int64.  An observed
    entry whose theta is not NaN adds (1, one, q1, q2, one ? q1 : 0) to row_tab[row, groups[col]] where the label is not -1
    and to col_tab[col]; a NaN one adds 1 to nan_count[one].  ``groups`` None: every column in group 0.
    Returns ``(row_tab int64 (rows, G, 5), col_tab int64 (cols, 5), nan_count int64 (2,))``."""
    theta = np.asarray(theta, dtype=np.float64)
    x = np.asarray(x)
    assert theta.ndim == 2 and x.shape == theta.shape and (x.dtype == np.bool_ or x.dtype == np.uint8)
    obs = np.ones(theta.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    assert obs.shape == theta.shape
    groups = np.zeros(theta.shape[1], dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64)
    assert groups.shape == (theta.shape[1],) and groups.min(initial=0) >= -1 and groups.max(initial=0) < G
    nan = np.isnan(theta)
    one = x != 0
    nan_count = np.array([np.count_nonzero(obs & nan & ~one), np.count_nonzero(obs & nan & one)], dtype=np.int64)
    live = obs & ~nan
    t = np.where(live, theta, 0.0)
    q1 = np.rint(t * 2.0 ** 32).astype(np.int64)
    q2 = np.rint((t * t) * 2.0 ** 32).astype(np.int64)
    terms = np.stack([live.astype(np.int64), (live & one).astype(np.int64), np.where(live, q1, 0), np.where(live, q2, 0),
                      np.where(live & one, q1, 0)], axis=-1)                    # (rows, cols, 5)
    col_tab = terms.sum(axis=0)
    row_tab = np.zeros((theta.shape[0], G, 5), dtype=np.int64)
    for g in range(G):
        row_tab[:, g] = terms[:, groups == g].sum(axis=1)
    return row_tab, col_tab, nan_count


# ---- the reference itself -------------------------------------------------------------------------------------------------
def test_host_moments_on_hand_written_cases():
    tie = 2.0 ** -33                                                             # theta * Q = 0.5: rounds to even, 0
    theta = np.array([[0.0, 1.0, 0.5, tie, np.nan, 0.25],
                      [0.5, 3 * tie, 1.0, 0.75, np.nan, 0.0],
                      [0.5, 0.5, 0.5, 0.5, 0.5, 0.5]])
    x = np.array([[0, 1, 7, 1, 0, 0], [1, 0, 0, 255, 1, 1], [1, 1, 1, 1, 1, 1]], dtype=np.uint8)   # nonzero, not just 1, is a one
    groups = np.array([0, 0, 2, 2, 2, -1])                                       # group 1 is empty, the last column in none
    row_tab, col_tab, nan_count = host_moments(theta, x, None, groups, 3)
    assert row_tab.dtype == col_tab.dtype == nan_count.dtype == np.int64
    assert row_tab.shape == (3, 3, 5) and col_tab.shape == (6, 5) and nan_count.tolist() == [1, 1]
    H, F = 2 ** 31, 2 ** 32                                                      # 0.5 and 1 in fixed point
    assert row_tab[0, 0].tolist() == [2, 1, F, F, F]                             # theta 0 (a zero) and 1 (a one)
    assert row_tab[0, 2].tolist() == [2, 2, H, H // 2, H]                        # 0.5 and the tie (-> 0); the NaN is not here
    assert not row_tab[:, 1].any()                                               # the empty group
    # 3 * 2^-33 * Q = 1.5 -> 2 (half to even goes UP here); its square is far below 2^-33: 0
    assert row_tab[1, 0].tolist() == [2, 1, H + 2, H // 2, H]
    assert row_tab[1, 2].tolist() == [2, 1, F + 3 * 2 ** 30, F + 9 * 2 ** 28, 3 * 2 ** 30]
    assert row_tab[2].tolist() == [[2, 2, F, H, F], [0] * 5, [3, 3, 3 * H, 3 * H // 2, 3 * H]]
    assert col_tab[5].tolist() == [3, 2, 2 ** 30 + H, 2 ** 28 + H // 2, H]       # label -1 still counts per column
    assert col_tab[4].tolist() == [1, 1, H, H // 2, H]                           # two NaNs are in no sum
    assert col_tab[:, 0].sum() + nan_count.sum() == theta.size
    assert np.array_equal(col_tab[:5].sum(0), row_tab.sum((0, 1)))              # the grouped columns: the same entries
    # a mask: nonzero = observed; row 2 fully masked
    mask = np.array([[1, 1, 0, 0, 9, 1], [0, 1, 1, 0, 0, 0], [0, 0, 0, 0, 0, 0]], dtype=np.uint8)
    row_tab, col_tab, nan_count = host_moments(theta, x, mask, groups, 3)
    assert nan_count.tolist() == [1, 0] and not row_tab[2].any()
    assert row_tab[0, 0].tolist() == [2, 1, F, F, F] and not row_tab[0, 2].any()
    assert row_tab[1].tolist() == [[1, 0, 2, 0, 0], [0] * 5, [1, 0, F, F, 0]]
    assert col_tab[5].tolist() == [1, 0, 2 ** 30, 2 ** 28, 0]
    # groups=None: one group of every column
    row_tab, col_tab, _ = host_moments(theta, x, mask, None, 1)
    assert np.array_equal(row_tab[:, 0], host_moments(theta, x, mask, np.zeros(6, dtype=int), 1)[0][:, 0])
    assert np.array_equal(row_tab.sum((0, 1)), col_tab.sum(0))


# ---- the C entry point, as far as a host without a GPU reaches it ---------------------------------------------------------
def test_symbol_is_declared_and_exported():
    from nbmf_mm_amd import _hip
    assert "nbmf_moment_rows_v" in _hip.SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "nbmf_moment_rows_v")
    plain = {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64}                      # tests/asan_null_calls.py: only these kinds
    assert len(lib.nbmf_moment_rows_v.argtypes) == 14 and set(lib.nbmf_moment_rows_v.argtypes) <= plain
    assert lib.nbmf_abi_version() == 4
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbmf_hip.h")).read()
    assert "int nbmf_moment_rows_v(nbmf_ctx* ctx, int64_t row0, int64_t nrows," in header
    assert "#define NBMF_MOMENT_MAX_GROUPS 16" in header and _hip.MOMENT_MAX_GROUPS == 16
    assert "#define NBMF_MOMENT_FRAC_BITS 32" in header and _hip.MOMENT_FRAC_BITS == 32
    assert "#define NBMF_MOMENT_FIELDS 5" in header and len(_hip.MOMENT_FIELDS) == 5
    assert _hip.MOMENT_FIELDS == ("n_obs", "n_ones", "s1", "s2", "s1_ones")


def test_null_context_is_an_argument_error():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    assert lib.nbmf_moment_rows_v(None, 0, 0, None, 0, 0, None, 0, 0, None, 0, None, None, None) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    x = np.zeros((2, 3), dtype=np.uint8)
    row_tab = np.full((2, 1, 5), -7, dtype=np.int64)
    col_tab = np.full((3, 5), -7, dtype=np.int64)
    nan_count = np.full(2, -7, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    rc = lib.nbmf_moment_rows_v(None, 0, 2, ptr(x), _hip.DATA_U8, 3, None, _hip.MASK_NONE, 0, None, 1, ptr(row_tab), ptr(col_tab),
                                ptr(nan_count))
    assert rc == _hip.NBMF_ERR_ARG
    assert np.all(row_tab == -7) and np.all(col_tab == -7) and np.all(nan_count == -7)


# ---- Context.moments: every argument error before any device call -----------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called for a request that is malformed")


@pytest.fixture
def bare_context():
    """A Context of a 12 x 9 problem that has no library behind it: touching the device is an error of the test."""
    from nbmf_mm_amd import _hip
    ctx = object.__new__(_hip.Context)
    ctx._lib, ctx._h = _NoDevice(), None
    ctx.m, ctx.n, ctx.k = 12, 9, 3
    return ctx


def test_context_refuses_malformed_requests(bare_context):
    ctx, x = bare_context, np.zeros((12, 9), dtype=np.uint8)
    for row0, nrows in ((-1, 2), (12, 1), (11, 2), (0, -1), (0, 13)):
        with pytest.raises(ValueError, match="rows"):
            ctx.moments(np.zeros((max(nrows, 0), 9), dtype=np.uint8), row0=row0, nrows=nrows)
    with pytest.raises(ValueError, match="nothing requested"):
        ctx.moments(x, rows=False, cols=False)
    for groups in (np.zeros(8, dtype=int), np.zeros(10, dtype=int), np.zeros((9, 1), dtype=int), 3):
        with pytest.raises(ValueError, match="groups must have shape"):
            ctx.moments(x, groups=groups)
    for groups in (np.zeros(9), np.zeros(9, dtype=bool), np.array(["a"] * 9)):
        with pytest.raises(ValueError, match="groups must be an integer array"):
            ctx.moments(x, groups=groups)
    bad = np.zeros(9, dtype=int)
    bad[4] = -2
    with pytest.raises(ValueError, match="position 4 is below -1"):
        ctx.moments(x, groups=bad)
    bad[4] = 16
    with pytest.raises(ValueError, match="n_groups must be at most 16"):        # 17 groups: passes are _solver's business
        ctx.moments(x, groups=bad)
    bad[4] = 3
    with pytest.raises(ValueError, match=r"label 3 at position 4 is outside \[-1, 3\)"):
        ctx.moments(x, groups=bad, n_groups=3)
    for n_groups in (0, -1, 17, 2.0, "4", True):
        with pytest.raises(ValueError, match="n_groups"):
            ctx.moments(x, n_groups=n_groups)
    for shape in ((12, 8), (11, 9), (12 * 9,)):
        with pytest.raises(ValueError, match="x must have shape"):
            ctx.moments(np.zeros(shape, dtype=np.uint8))
    with pytest.raises(ValueError, match="shape"):
        ctx.moments(x, row0=2, nrows=4)                                      # the shape follows the request: (nrows, n)
    for dtype in (np.float64, np.float32, np.int64, np.int8):                # bytes only
        with pytest.raises(ValueError, match="x must be a bool or uint8"):
            ctx.moments(np.zeros((12, 9), dtype=dtype))
    with pytest.raises(ValueError, match="stride"):
        ctx.moments(np.zeros((12, 18), dtype=np.uint8)[:, ::2])
    with pytest.raises(ValueError, match="stride"):
        ctx.moments(np.zeros((9, 12), dtype=bool).T)
    for shape in ((12, 8), (11, 9), (9,)):
        with pytest.raises(ValueError, match="mask must have shape"):
            ctx.moments(x, mask=np.ones(shape, dtype=bool))
    for dtype in (np.float64, np.int64):
        with pytest.raises(ValueError, match="mask must be a bool or uint8"):
            ctx.moments(x, mask=np.ones((12, 9), dtype=dtype))
    with pytest.raises(ValueError, match="mask must have unit stride"):
        ctx.moments(x, mask=np.ones((9, 12), dtype=bool).T)


# ---- _metrics.Moments -------------------------------------------------------------------------------------------------------
def slot_sums(theta, X, mask, f):
    """math.fsum of f(theta, x) over the observed entries of every column: the direct float computation."""
    return np.array([math.fsum(f(theta[i, j], X[i, j]) for i in np.flatnonzero(mask[:, j])) for j in range(theta.shape[1])])


def test_moments_properties_against_direct_float_computations_on_theta():
    from nbmf_mm_amd import Moments
    W, H, X, mask = hist_case(5, 37, 297)
    theta = np.clip(W.T @ H, 0.0, 1.0)
    row_tab, col_tab, nan_count = host_moments(theta, X, mask, None, 1)
    assert not nan_count.any()
    for mo, th, x, mk in ((Moments.from_table(col_tab), theta, X, mask), (Moments.from_table(row_tab[:, 0]), theta.T, X.T, mask.T)):
        n_obs, n_ones = mo.n_obs.astype(np.float64), mo.n_ones.astype(np.float64)
        assert np.array_equal(mo.n_obs, mk.sum(0)) and np.array_equal(mo.n_ones, (x & mk).sum(0)) and (mo.n_obs == 0).any()
        seen = n_obs > 0
        err = np.abs(mo.expected - slot_sums(th, x, mk, lambda t, v: t))
        print(f"expected: worst slot at {np.max(err[seen] / (n_obs[seen] * 2.0 ** -33)):.3f} of n_obs * 2^-33")
        assert np.all(err <= n_obs * 2.0 ** -33)
        err = np.abs(mo.variance - slot_sums(th, x, mk, lambda t, v: t * (1.0 - t)))
        print(f"variance: worst slot at {np.max(err[seen] / (n_obs[seen] * (2.0 ** -32 + 2.0 ** -50))):.3f} of its bound")
        assert np.all(err <= n_obs * (2.0 ** -32 + 2.0 ** -50))
        direct = slot_sums(th, x, mk, lambda t, v: (float(v) - t) ** 2)[seen] / n_obs[seen]
        bound = ((3 * n_ones + (n_obs - n_ones)) * 2.0 ** -33 + n_obs * 2.0 ** -50)[seen] / n_obs[seen]
        err = np.abs(mo.brier[seen] - direct)
        print(f"brier: worst slot at {np.max(err / bound):.3f} of its bound")
        assert np.all(err <= bound)
        assert np.array_equal(np.isnan(mo.brier), ~seen) and np.array_equal(np.isnan(mo.mean_theta), ~seen)
        assert np.allclose(mo.mean_theta[seen], slot_sums(th, x, mk, lambda t, v: t)[seen] / n_obs[seen], rtol=0, atol=2.0 ** -33 + 2.0 ** -50)
        # tjur: the mean theta of the ones less that of the zeros, NaN where a class is empty
        both = (n_ones > 0) & (n_obs > n_ones)
        assert np.array_equal(np.isnan(mo.tjur), ~both) and both.any()
        want = np.array([th[mk[:, j] & x[:, j], j].mean() - th[mk[:, j] & ~x[:, j], j].mean() for j in np.flatnonzero(both)])
        assert np.allclose(mo.tjur[both], want, rtol=0, atol=2.0 ** -32)
        # z: defined where something is observed and the variance is positive
        z = mo.z
        assert np.array_equal(np.isnan(z), ~(seen & (mo.variance > 0)))
        ok = ~np.isnan(z)
        assert np.allclose(z[ok], (n_ones[ok] - mo.expected[ok]) / np.sqrt(mo.variance[ok]), rtol=1e-15, atol=0)


@pytest.mark.parametrize("k,m,n", [(5, 37, 297), (130, 20, 130), (5, 37, 100), (130, 53, 297)])
def test_z_of_planted_data_is_standard_on_the_host_reference(k, m, n):
    """X ~ Bernoulli(Theta): the per-feature z-scores have mean square about 1.  The reference alone: this guards the
    formulae, not the device."""
    from nbmf_mm_amd import Moments
    W, H, X, mask = hist_case(k, m, n)
    theta = np.clip(W.T @ H, 0.0, 1.0)
    z = Moments.from_table(host_moments(theta, X, mask, None, 1)[1]).z
    z = z[~np.isnan(z)]
    rms, worst = float(np.sqrt(np.mean(z ** 2))), float(np.max(np.abs(z)))
    print(f"K = {k}, {m} x {n}: rms z = {rms:.3f}, max |z| = {worst:.3f} over {z.size} features")
    assert z.size >= n - 2 and 0.8 <= rms <= 1.25 and worst <= 4.5


def test_moments_is_an_immutable_holder_of_equally_shaped_integer_arrays():
    from nbmf_mm_amd import Moments, _metrics
    assert Moments is _metrics.Moments
    tab = np.arange(4 * 3 * 5, dtype=np.int64).reshape(4, 3, 5)
    mo = Moments.from_table(tab)
    assert mo.shape == (4, 3) and mo._fields == ("n_obs", "n_ones", "s1", "s2", "s1_ones")
    for f, a in enumerate(mo):
        assert a.dtype == np.int64 and np.array_equal(a, tab[..., f]) and not a.flags.writeable
        with pytest.raises(ValueError):
            a[0, 0] = 1
    tab[0, 0, 0] = 99                                                            # the holder's arrays are its own
    assert mo.n_obs[0, 0] == 0
    with pytest.raises(AttributeError):
        mo.s1 = tab[..., 2]
    with pytest.raises(ValueError, match="shape"):
        Moments(tab[..., 0], tab[..., 1], tab[..., 2], tab[..., 3], tab[:2, :, 4])
    with pytest.raises(ValueError, match="integer"):
        Moments(*(tab[..., f].astype(np.float64) for f in range(5)))
    with pytest.raises(ValueError, match="last axis"):
        Moments.from_table(tab[..., :4])
    # nothing observed: every float property is NaN or 0, none raises
    empty = Moments.from_table(np.zeros((2, 5), dtype=np.int64))
    assert empty.expected.tolist() == [0.0, 0.0] and empty.variance.tolist() == [0.0, 0.0]
    assert all(np.isnan(getattr(empty, p)).all() for p in ("z", "mean_theta", "brier", "tjur"))


def test_grouped_equals_the_reference_over_the_merged_rows():
    from nbmf_mm_amd import Moments
    W, H, X, mask = hist_case(5, 37, 297)
    theta = np.clip(W.T @ H, 0.0, 1.0)
    r = np.random.default_rng(12)
    fgroups = r.integers(-1, 7, 297)
    sgroups = r.integers(-1, 4, 37)
    sgroups[sgroups == 2] = 0                                                    # sample group 2 is empty
    row_tab = host_moments(theta, X, mask, fgroups, 7)[0]
    got = Moments.from_table(row_tab).grouped(sgroups, 4)
    assert got.shape == (4, 7) and all(a.dtype == np.int64 for a in got)
    for s in range(4):
        rows = sgroups == s
        # the rows of a group as ONE row: its entries side by side, the feature labels repeated
        merged = host_moments(theta[rows].reshape(1, -1), X[rows].reshape(1, -1), mask[rows].reshape(1, -1),
                              np.tile(fgroups, int(rows.sum())), 7)[0][0]
        for f, a in enumerate(got):
            assert np.array_equal(a[s], merged[:, f])
    assert not got.n_obs[2].any()
    assert np.array_equal(Moments.from_table(row_tab).grouped(sgroups).n_obs, got.n_obs)      # n_groups: max label + 1
    assert Moments.from_table(row_tab).grouped(np.zeros(37, dtype=int), 3).shape == (3, 7)
    for bad in (sgroups[:-1], sgroups.astype(float), np.where(sgroups == 1, -2, sgroups)):
        with pytest.raises(ValueError, match="labels"):
            Moments.from_table(row_tab).grouped(bad)
    with pytest.raises(ValueError, match="outside"):
        Moments.from_table(row_tab).grouped(sgroups, 3)


def test_grouped_is_exact_beyond_int64():
    from nbmf_mm_amd import Moments
    big = 2 ** 62 + 12345                                                        # what a slot of 2^30 entries may hold
    tab = np.zeros((5, 2, 5), dtype=np.int64)
    tab[:, 0, 2] = [big, big - 1, big + 7, 5, big]                               # s1 of feature group 0
    tab[:, 0, 3] = [big // 2, 3, 4, 5, 6]
    tab[:, :, 0] = 2 ** 30
    tab[:, 1, 2] = [1, 2, 3, 4, 5]
    got = Moments.from_table(tab).grouped([0, 0, 0, 1, -1], 2)
    assert got.s1.dtype == object and got.s1.shape == (2, 2)
    assert got.s1[0, 0] == 3 * big + 6 and got.s1[0, 0] > 2 ** 63 and got.s1[1, 0] == 5 and got.s1[0, 1] == 6 and got.s1[1, 1] == 4
    assert got.s2.dtype == np.int64 and got.s2[0, 0] == big // 2 + 7
    assert got.n_obs.dtype == np.int64 and got.n_obs.tolist() == [[3 * 2 ** 30] * 2, [2 ** 30] * 2]
    # the float properties come from the exact sums: one rounding of the exact integer
    assert got.expected[0, 0] == (3 * big + 6) / 2 ** 32 and got.variance[0, 0] == (3 * big + 6 - (big // 2 + 7)) / 2 ** 32
    # ... also where every FIELD still fits int64 and only the Brier numerator n_ones Q - 2 s1_ones + s2 does not:
    # 2^30 ones of theta = 0 and as many zeros of theta = 1 -- every entry is off by 1, the Brier score is exactly 1
    n = 2 ** 30
    off = Moments([2 * n], [n], [n * 2 ** 32], [n * 2 ** 32], [0])
    assert all(a.dtype == np.int64 for a in off) and off.brier.tolist() == [1.0] and off.tjur.tolist() == [-1.0]
    assert off.expected.tolist() == [float(n)] and off.variance.tolist() == [0.0] and np.isnan(off.z).all()
    half = Moments([2 * n], [n], [n * 2 ** 32], [n * 2 ** 31], [n * 2 ** 31])    # theta = 1/2 everywhere: (x - theta)^2 = 1/4
    assert half.brier.tolist() == [0.25] and half.tjur.tolist() == [0.0]
    again = got.grouped([0, 0], 1)                                               # Python ints all the way
    assert again.s1[0, 0] == 3 * big + 11 and again.s1[0, 1] == 10


# ---- NBMF.expected_counts ---------------------------------------------------------------------------------------------------
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


def test_not_fitted_is_transforms_error():
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError) as want:
        NBMF().transform(np.zeros((3, 4)))
    with pytest.raises(ValueError) as got:
        NBMF().expected_counts(np.zeros((3, 4)))
    assert str(got.value) == str(want.value)


def test_estimator_refuses_malformed_requests_before_any_device_call(hand_set):
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF
    model = hand_set
    X = np.zeros((12, 9))
    call = model.expected_counts
    for name, length in (("feature_groups", 9), ("sample_groups", 12)):
        for bad in (np.zeros(length - 1, dtype=int), np.zeros((length, 1), dtype=int), 2):
            with pytest.raises(ValueError, match=f"{name} must have shape"):
                call(X, **{name: bad})
        for bad in (np.zeros(length), np.zeros(length, dtype=bool)):
            with pytest.raises(ValueError, match=f"{name} must be an integer array"):
                call(X, **{name: bad})
        bad = np.zeros(length, dtype=int)
        bad[2] = -2
        with pytest.raises(ValueError, match=f"{name} label -2 at position 2 is below -1"):
            call(X, **{name: bad})
    with pytest.raises(ValueError, match="sample_groups must have shape"):
        call(X[:4], W=np.full((4, 3), 1 / 3), sample_groups=np.zeros(12, dtype=int))   # the labels follow W, not W_
    with pytest.raises(ValueError, match="components"):
        call(X[:4], W=np.full((4, 2), 0.5))
    for bad in (np.zeros((12, 8)), np.zeros((9, 12)), sp.csr_matrix((11, 9))):
        with pytest.raises(ValueError, match="shape"):
            call(bad)
    for bad in (np.ones((12, 8)), np.ones((9, 12)), np.ones(9), sp.csr_matrix((12, 8))):
        with pytest.raises(ValueError, match="mask has shape"):
            call(X, mask=bad)
    with pytest.raises(ValueError, match="dtype"):
        call(X, mask=np.full((12, 9), "a"))
    for poke in (np.nan, np.inf, 1.5, -0.25):                                    # the errors fit gives, in fit's order
        bad = X.copy()
        bad[3, 4] = poke
        with pytest.raises(ValueError) as want:
            NBMF(n_components=3).fit(bad)
        with pytest.raises(ValueError) as got:
            call(bad)
        assert str(got.value) == str(want.value)
    bad = X.copy()
    bad[3, 4] = 0.5                                                              # inside [0, 1] but not a class
    with pytest.raises(ValueError, match="X must be binary"):
        call(bad)
    with pytest.raises(ValueError, match="X must be binary"):
        call(np.full((12, 9), 2, dtype=np.uint8))
    with pytest.raises(ValueError, match="X must be binary"):
        call(sp.csr_matrix(0.5 * np.eye(12, 9)))


def test_well_formed_request_reaches_the_device_or_fails_loudly():
    """No CPU fallback: without a GPU the call is an error of the library, with one it answers."""
    from nbmf_mm_amd import NBMF, _hip
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    X = r.random((12, 9)) < 0.3
    groups = np.array([0, 0, 1, 1, -1, 2, 2, 2, 0])
    if _hip.device_count() == 0:
        for call in (lambda: model.expected_counts(X), lambda: model.expected_counts(X.astype(float), mask=X, feature_groups=groups),
                     lambda: model.expected_counts(X, sample_groups=np.arange(12) % 3)):
            with pytest.raises(_hip.NBMFHipError, match="no HIP device"):
                call()
    else:
        by_sample, by_feature = model.expected_counts(X, feature_groups=groups)
        assert by_sample.shape == (12, 3) and by_feature.shape == (9,)
        assert by_feature.n_obs.sum() == X.size and by_feature.n_ones.sum() == X.sum()
        assert np.array_equal(by_sample.n_ones.sum(0), [X[:, groups == g].sum() for g in range(3)])
