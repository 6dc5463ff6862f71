"""Expected counts summed on the device: nbmf_moment_rows_v, Context.moments, NBMF.expected_counts.

REFERENCE.  Always ``host_moments(ctx.predict_rows(row0, nrows, clip_theta=True), x, mask, groups, G)``
(tests/test_moments_cpu.py: the contract in NumPy).  The device rounds the very Theta predict_rows returns to the same
fixed-point integers NumPy's ``rint`` gives and adds integers: every comparison in this file is for EQUALITY of int64 arrays.
There is no tolerance anywhere.

SHAPES.  The smallest at which each path runs, those of tests/test_gpu_theta_hist.py: n = 297 (staged width 300: three pad
columns inside one lane's four, a ragged last strip, five strips over two workgroups), n = 130 (nA = 256: a workgroup with
one whole pad strip), n = 100 (nA = 128: a workgroup two of whose waves leave before the k loop), m = 37 / 53 (pad rows in
the last 16-row tile, several tiles, an offset inside a tile), K = 5 (a ragged k block) and K = 130 (the sliced factor
layout); G = 1, 2, 7, 16 (the smallest and the largest table a wave keeps)."""
import ctypes

import numpy as np
import pytest

from conftest import config1_X, config1_mask
from test_moments_cpu import host_moments
from test_theta_hist_cpu import hist_case

pytestmark = pytest.mark.gpu

ALL_G = (1, 2, 7, 16)


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


def context(hip, W, H):
    ctx = hip.Context(W.shape[1], H.shape[1], W.shape[0])
    ctx.set_factors(W, H)
    return ctx


def same(got, want):
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and w.dtype == np.int64 and g.shape == w.shape
        assert np.array_equal(g, w)


def label_patterns(n, G, seed=0):
    """The label layouts of one (n, G): contiguous runs, random, all in one group, one group empty, some -1."""
    r = np.random.default_rng(100 * G + seed)
    runs = np.minimum(np.arange(n) * G // n, G - 1)
    rand = r.integers(0, G, n)
    one = np.full(n, G - 1)
    hole = np.where(rand == G // 2, (G // 2 + 1) % G, rand) if G > 1 else np.full(n, -1)    # G = 1: the one group is empty
    some = np.where(r.random(n) < 0.2, -1, rand)
    return {"runs": runs, "random": rand, "one": one, "hole": hole, "some": some}


def all_tables(ctx, X, mask, groups, G, **kw):
    return ctx.moments(X, mask, groups=groups, n_groups=G, rows=True, cols=True, **kw)


# ---- 1. ragged tile: every group count, every label layout, bytes ------------------------------------------------------------
@pytest.mark.parametrize("G", ALL_G)
def test_ragged_tile_every_label_layout_and_byte_kind(hip, G):
    m, n = 37, 297
    W, H, X, mask = hist_case(5, m, n)
    assert not mask[m // 3].any() and not mask[:, n // 3].any()             # a fully masked row and column are in it
    r = np.random.default_rng(9)
    xb = X.astype(np.uint8) * r.integers(1, 256, (m, n), dtype=np.uint8)    # bytes: any nonzero value is a one / observed
    mb = mask.astype(np.uint8) * r.integers(1, 256, (m, n), dtype=np.uint8)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        for name, groups in label_patterns(n, G).items():
            for mk, mk_bytes in ((None, None), (mask, mb)):
                got = all_tables(ctx, X, mk, groups, G)
                assert got[0].shape == (m, G, 5) and got[1].shape == (n, 5) and got[2].shape == (2,), name
                same(got, host_moments(theta, X, mk, groups, G))
                obs = np.ones((m, n), dtype=bool) if mk is None else mask
                assert got[1][:, 0].sum() == obs.sum() and got[1][:, 1].sum() == (X & obs).sum() and not got[2].any()
                assert got[0][:, :, 0].sum() == obs[:, groups >= 0].sum()
                same(all_tables(ctx, xb, mk_bytes, groups, G), got)
        if G == 1:                                                           # groups=None: every column in group 0
            for mk in (None, mask):
                got = ctx.moments(X, mk, rows=True, cols=True)
                same(got, host_moments(theta, X, mk, None, 1))
                same(got, all_tables(ctx, X, mk, np.zeros(n, dtype=np.int64), 1))
        # one table at a time: the same arrays, None for the other
        groups = label_patterns(n, G)["some"]
        both = all_tables(ctx, X, mask, groups, G)
        rows_only = ctx.moments(X, mask, groups=groups, n_groups=G)          # the default: rows
        cols_only = ctx.moments(X, mask, groups=groups, n_groups=G, rows=False, cols=True)
        assert rows_only[1] is None and cols_only[0] is None
        assert np.array_equal(rows_only[0], both[0]) and np.array_equal(cols_only[1], both[1])
        assert np.array_equal(rows_only[2], both[2]) and np.array_equal(cols_only[2], both[2])


@pytest.mark.parametrize("k,m,n", [(130, 20, 130), (5, 37, 100), (130, 53, 297)])
def test_pad_strips_and_the_sliced_layout(hip, k, m, n):
    W, H, X, mask = hist_case(k, m, n)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        for G in ALL_G:
            pats = label_patterns(n, G)
            same(all_tables(ctx, X, mask, pats["some"], G), host_moments(theta, X, mask, pats["some"], G))
            same(all_tables(ctx, X, None, pats["runs"], G), host_moments(theta, X, None, pats["runs"], G))


# ---- 2. packed operands ----------------------------------------------------------------------------------------------------------
def test_packed_bits_equal_bytes(hip):
    from nbmf_mm_amd import PackedBits
    m, n = 53, 297
    W, H, X, mask = hist_case(5, m, n)
    groups = label_patterns(n, 7)["some"]
    Xp, Mp = PackedBits.from_dense(X), PackedBits.from_dense(mask)
    with context(hip, W, H) as ctx:
        want = all_tables(ctx, X, mask, groups, 7)
        same(want, host_moments(ctx.predict_rows(), X, mask, groups, 7))
        same(all_tables(ctx, Xp, Mp, groups, 7), want)
        same(all_tables(ctx, Xp, mask, groups, 7), want)
        same(all_tables(ctx, X, Mp, groups, 7), want)
        same(all_tables(ctx, Xp, None, groups, 7), all_tables(ctx, X, None, groups, 7))
        same(all_tables(ctx, Xp[5:25], Mp[5:25], groups, 7, row0=5, nrows=20), all_tables(ctx, X[5:25], mask[5:25], groups, 7, row0=5, nrows=20))


# ---- 3. offsets and panels ---------------------------------------------------------------------------------------------------------
def test_row_offsets_panels_and_repeats(hip, monkeypatch):
    m, n = 53, 297
    W, H, X, mask = hist_case(5, m, n)
    g16, g7, g2 = (label_patterns(n, G)[name] for G, name in ((16, "random"), (7, "some"), (2, "runs")))
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        calls = [lambda: all_tables(ctx, X, mask, g16, 16),
                 lambda: all_tables(ctx, X, None, g7, 7),
                 lambda: all_tables(ctx, X[5:25], mask[5:25], g7, 7, row0=5, nrows=20),
                 lambda: all_tables(ctx, X[48:], None, g16, 16, row0=48),
                 lambda: all_tables(ctx, X[20:], mask[20:], g2, 2, row0=20)]
        wants = [host_moments(theta, X, mask, g16, 16), host_moments(theta, X, None, g7, 7),
                 host_moments(theta[5:25], X[5:25], mask[5:25], g7, 7),       # slices of the whole-matrix reference
                 host_moments(theta[48:], X[48:], None, g16, 16),              # the last, ragged 16-row tile alone
                 host_moments(theta[20:], X[20:], mask[20:], g2, 2)]
        unset = [call() for call in calls]
        for got, want in zip(unset, wants):
            same(got, want)
        # the reference of a row range is also what predict_rows gives for that range
        same(unset[2], host_moments(ctx.predict_rows(5, 20), X[5:25], mask[5:25], g7, 7))
        # disjoint row ranges: the column tables and the NaN counts add up, the row tables lie end to end
        parts = [all_tables(ctx, X[a:b], mask[a:b], g16, 16, row0=a, nrows=b - a) for a, b in ((0, 5), (5, 25), (25, 48), (48, m))]
        same((np.concatenate([p[0] for p in parts]), sum(p[1] for p in parts), sum(p[2] for p in parts)), wants[0])
        # no rows: an empty row table, zeros, and nothing is read
        empty = all_tables(ctx, X[7:7], mask[7:7], g7, 7, row0=7, nrows=0)
        assert empty[0].shape == (0, 7, 5) and empty[1].shape == (n, 5) and not empty[1].any() and not empty[2].any()
        # the same call twice, and every panel height: identical arrays
        for call, want in zip(calls, unset):
            same(call(), want)
        for rows_per_panel in ("1", "7", "16", "21"):
            monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", rows_per_panel)
            for call, want in zip(calls, unset):
                same(call(), want)
        monkeypatch.delenv("NBMF_PREDICT_PANEL_ROWS")
        # ... and however many copies of the column table the device spreads its adds over
        for copies in ("1", "3"):
            monkeypatch.setenv("NBMF_MOMENT_COPIES", copies)
            same(calls[0](), unset[0])
    with context(hip, W, H) as ctx:                                          # another context, the same factors
        same(all_tables(ctx, X, mask, g16, 16), unset[0])


# ---- 4. strided input ----------------------------------------------------------------------------------------------------------------
def test_strided_inputs_and_nothing_beside_the_slice_is_read(hip):
    m, n = 37, 297
    W, H, X, mask = hist_case(5, m, n)
    groups = label_patterns(n, 7)["random"]
    wide_x = np.ones((m + 2, n + 40), dtype=bool)                            # what lies beside the slices would change the sums
    wide_m = np.ones((m + 3, n + 9), dtype=np.uint8)
    wide_x[1:m + 1, 7:7 + n] = X
    wide_m[2:m + 2, 0:n] = mask
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        want = host_moments(theta, X, mask, groups, 7)
        same(all_tables(ctx, wide_x[1:m + 1, 7:7 + n], wide_m[2:m + 2, 0:n], groups, 7), want)
        same(all_tables(ctx, wide_x[1:m + 1, 7:7 + n], None, groups, 7), host_moments(theta, X, None, groups, 7))
        same(all_tables(ctx, wide_x[6:26, 7:7 + n], wide_m[7:27, 0:n], groups, 7, row0=5, nrows=20),
             host_moments(theta[5:25], X[5:25], mask[5:25], groups, 7))
        m2 = np.zeros((m, n), dtype=bool)                                    # the last columns count: nothing stops short of n - 1
        m2[:, n - 3:] = True
        got = all_tables(ctx, X, m2, groups, 7)
        assert got[1][:, 0].sum() == 3 * m and got[1][n - 3:, 0].tolist() == [m] * 3
        same(got, host_moments(theta, X, m2, groups, 7))


# ---- 5. exact values: ties, 0 and 1 ---------------------------------------------------------------------------------------------------
def test_thetas_on_ties_zero_and_one(hip):
    k, m, n = 5, 37, 297
    r = np.random.default_rng(31)
    W = np.zeros((k, m))
    W[r.integers(0, k, m), np.arange(m)] = 1.0                               # one-hot columns: Theta[i, j] = H[k_i, j] exactly
    H = r.choice([0.0, 1.0, 0.5, 2.0 ** -33, 3 * 2.0 ** -33, 5 * 2.0 ** -34, 0.75, 1.0 - 2.0 ** -53], (k, n))
    X = r.random((m, n)) < 0.4
    mask = r.random((m, n)) < 0.7
    groups = label_patterns(n, 7)["some"]
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        assert np.array_equal(theta, W.T @ H) and (theta == 2.0 ** -33).any() and (theta == 1.0).any()
        got = all_tables(ctx, X, mask, groups, 7)
        same(got, host_moments(theta, X, mask, groups, 7))
        # by hand for one feature: q1 of the tie 2^-33 is 0 (half to even), of 3 * 2^-33 is 2, of 5 * 2^-34 (1.25) is 1
        q1 = {0.0: 0, 1.0: 2 ** 32, 0.5: 2 ** 31, 2.0 ** -33: 0, 3 * 2.0 ** -33: 2, 5 * 2.0 ** -34: 1, 0.75: 3 * 2 ** 30,
              1.0 - 2.0 ** -53: 2 ** 32}
        for j in (0, 131, n - 1):
            assert got[1][j, 2] == sum(q1[t] for t in theta[mask[:, j], j])
    # an un-normalised W: every raw Theta is beyond 1, the clip is always on: every q1 and q2 is Q
    with context(hip, 3.0 * W, 0.5 + H / 2.0) as ctx:
        assert ctx.predict_rows(clip_theta=False).min() >= 1.5
        row_tab, col_tab, nan_count = all_tables(ctx, X, mask, None, 1)
        assert not nan_count.any()
        assert np.array_equal(col_tab[:, 2], col_tab[:, 0] << 32) and np.array_equal(col_tab[:, 3], col_tab[:, 0] << 32)
        assert np.array_equal(col_tab[:, 4], col_tab[:, 1] << 32) and np.array_equal(row_tab[:, 0, 0], mask.sum(1))


# ---- 6. NaN --------------------------------------------------------------------------------------------------------------------------
def test_a_nan_theta_is_in_no_sum(hip):
    m, n = 37, 297
    W, H, X, mask = hist_case(5, m, n)
    groups = label_patterns(n, 7)["random"]
    j = 131
    Hn = H.copy()
    Hn[2, j] = np.nan                                                        # W > 0: all of column j of Theta is NaN
    with context(hip, W, Hn) as ctx, context(hip, W, H) as clean:
        theta = ctx.predict_rows()
        assert np.isnan(theta[:, j]).all() and np.isnan(theta).sum() == m
        for mk in (mask, None):
            obs = np.ones(m, dtype=bool) if mk is None else mk[:, j]
            got = all_tables(ctx, X, mk, groups, 7)
            assert got[2].tolist() == [int((obs & ~X[:, j]).sum()), int((obs & X[:, j]).sum())] and got[2].sum() > 0
            same(got, host_moments(theta, X, mk, groups, 7))
            # the other slots: those without that column
            without = np.ones((m, n), dtype=bool) if mk is None else mk.copy()
            without[:, j] = False
            want = all_tables(clean, X, without, groups, 7)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and not got[1][j].any()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_and_the_context_as_they_were(hip):
    m, n = 37, 53
    W, H, X, mask = hist_case(4, m, n)
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    xb = np.ascontiguousarray(X).view(np.uint8)
    mb = np.ascontiguousarray(mask).view(np.uint8)
    groups = np.ascontiguousarray(label_patterns(n, 3)["some"], dtype=np.int32)
    row_tab = np.full((m, 3, 5), -7, dtype=np.int64)
    col_tab = np.full((n, 5), -7, dtype=np.int64)
    nan_count = np.full(2, -7, dtype=np.int64)
    untouched = lambda: np.all(row_tab == -7) and np.all(col_tab == -7) and np.all(nan_count == -7)   # noqa: E731
    U8, NONE = hip.DATA_U8, hip.MASK_NONE
    with hip.Context(m, n, 4) as ctx:
        args = (0, m, ptr(xb), U8, n, None, NONE, 0, ptr(groups), 3, ptr(row_tab), ptr(col_tab), ptr(nan_count))
        assert lib.nbmf_moment_rows_v(ctx._h, *args) == hip.NBMF_ERR_STATE    # no factors
        assert b"no factors" in lib.nbmf_last_error() and untouched()
        with pytest.raises(hip.NBMFHipError, match="no factors"):
            ctx.moments(X)
        ctx.set_factors(W, H)
        theta = ctx.predict_rows()
        want = host_moments(theta, X, mask, groups, 3)
        same(ctx.moments(X, mask, groups=groups, n_groups=3, cols=True), want)
        low, high = groups.copy(), groups.copy()
        low[n - 1], high[0] = -2, 3
        bad = [(-1, 2) + args[2:], (m, 1) + args[2:], (m - 1, 2) + args[2:], (0, -1) + args[2:],     # rows outside [0, m)
               args[:9] + (0,) + args[10:], args[:9] + (17,) + args[10:], args[:9] + (-1,) + args[10:],   # groups outside [1, 16]
               args[:8] + (ptr(low),) + args[9:], args[:8] + (ptr(high),) + args[9:],                # a label outside [-1, groups)
               args[:9] + (2,) + args[10:],                                                          # ... for this group count
               args[:3] + (hip.DATA_F64,) + args[4:], args[:3] + (9,) + args[4:],                    # unknown x_kind
               args[:5] + (ptr(mb), 9, n) + args[8:], args[:5] + (None, hip.MASK_U8, n) + args[8:],  # unknown mask_kind, no mask
               args[:4] + (n - 1,) + args[5:],                                                       # ldx < n
               args[:5] + (ptr(mb), hip.MASK_U8, n - 1) + args[8:],                                  # ldmask < n with a mask
               args[:10] + (None, None, ptr(nan_count)),                                             # no table
               args[:2] + (None,) + args[3:]]                                                        # no data, nrows > 0
        for a in bad:
            assert lib.nbmf_moment_rows_v(ctx._h, *a) == hip.NBMF_ERR_ARG, a
            assert untouched(), a
        # ldmask is not looked at without a mask; nan_count and one of the tables may be null; null labels: one group
        one_tab = np.full((m, 1, 5), -7, dtype=np.int64)
        assert lib.nbmf_moment_rows_v(ctx._h, 0, m, ptr(xb), U8, n, None, NONE, -5, None, 1, ptr(one_tab), None, None) == hip.NBMF_OK
        assert np.array_equal(one_tab, host_moments(theta, X, None, None, 1)[0]) and untouched()
        assert lib.nbmf_moment_rows_v(ctx._h, *(args[:10] + (None, ptr(col_tab), None))) == hip.NBMF_OK
        assert np.array_equal(col_tab, host_moments(theta, X, None, groups, 3)[1]) and np.all(row_tab == -7)
        # no rows: nothing is read (null data), the column table and the NaN counts are zeroed, the row table is left alone
        col_tab[:] = -7
        assert lib.nbmf_moment_rows_v(ctx._h, 5, 0, None, U8, n, None, NONE, 0, ptr(groups), 3, ptr(row_tab), ptr(col_tab),
                                      ptr(nan_count)) == hip.NBMF_OK
        assert not col_tab.any() and not nan_count.any() and np.all(row_tab == -7)
        same(ctx.moments(X, mask, groups=groups, n_groups=3, cols=True), want)   # as usable as before
        # Context.moments: its ValueErrors, with a device behind it
        for call in (lambda: ctx.moments(X, n_groups=0), lambda: ctx.moments(X, groups=high, n_groups=3), lambda: ctx.moments(X[:5]),
                     lambda: ctx.moments(X.astype(np.float64)), lambda: ctx.moments(X, mask.astype(np.float64)),
                     lambda: ctx.moments(X, row0=m, nrows=1), lambda: ctx.moments(np.asfortranarray(X)),
                     lambda: ctx.moments(X, groups=np.arange(n) % 17)):
            with pytest.raises(ValueError):
                call()
        same(ctx.moments(X, mask, groups=groups, n_groups=3, cols=True), want)
    # a sharded context refuses, and answers again once detached
    with hip.Context(m, n, 4) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X, mask=mask)
        ctx.set_factors(W, H)
        ctx.comm_init_host(lambda arr: None, 1, 0)
        assert lib.nbmf_moment_rows_v(ctx._h, *args) == hip.NBMF_ERR_STATE
        assert b"unsharded" in lib.nbmf_last_error()
        ctx.comm_detach()
        same(ctx.moments(X, mask, groups=groups, n_groups=3, cols=True), want)


# ---- 8. the estimator --------------------------------------------------------------------------------------------------------------------
def same_moments(got, want):
    assert type(got) is type(want) and got.shape == want.shape
    for g, w in zip(got, want):
        assert g.dtype == w.dtype == np.int64 and np.array_equal(g, w)


@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_estimator_on_held_out_entries(hip, monkeypatch, orientation):
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF, Moments, PackedBits, _solver
    X, train = config1_X(), config1_mask()
    held = ~train
    model = NBMF(6, random_state=0, max_iter=20, tol=0, orientation=orientation).fit(X, mask=train)
    theta = model.predict_proba()
    Xb = X != 0
    m, n = X.shape
    r = np.random.default_rng(77)
    fgroups = r.integers(-1, 7, n)
    sgroups = r.integers(-1, 4, m)
    # per sample and per feature, no groups
    by_sample, by_feature = model.expected_counts(Xb, mask=held)
    row_tab, col_tab, nan_count = host_moments(theta, Xb, held, None, 1)
    assert not nan_count.any() and isinstance(by_sample, Moments) and by_sample.shape == (m, 1) and by_feature.shape == (n,)
    same_moments(by_sample, Moments.from_table(row_tab))
    same_moments(by_feature, Moments.from_table(col_tab))
    assert np.array_equal(by_feature.n_ones, (Xb & held).sum(0)) and np.array_equal(by_feature.n_obs, held.sum(0))
    assert np.array_equal(by_sample.n_ones[:, 0], (Xb & held).sum(1))
    assert abs(by_feature.expected.sum() - theta[held].sum()) <= held.sum() * 2.0 ** -33 + 1e-9
    print(f"{orientation}: held-out rms z per feature {np.sqrt(np.nanmean(by_feature.z ** 2)):.3f}, per sample "
          f"{np.sqrt(np.nanmean(by_sample.z ** 2)):.3f}")
    # feature groups, sample groups: host_moments on the merged rows
    want_rows, want_cols, _ = host_moments(theta, Xb, held, fgroups, 7)
    by_sample, by_feature = model.expected_counts(Xb, mask=held, feature_groups=fgroups)
    same_moments(by_sample, Moments.from_table(want_rows))
    same_moments(by_feature, Moments.from_table(want_cols))
    grouped, by_feature = model.expected_counts(Xb, mask=held, feature_groups=fgroups, sample_groups=sgroups)
    assert grouped.shape == (4, 7)
    for s in range(4):
        rows = sgroups == s
        merged = host_moments(theta[rows].reshape(1, -1), Xb[rows].reshape(1, -1), held[rows].reshape(1, -1),
                              np.tile(fgroups, int(rows.sum())), 7)[0][0]
        for f, a in enumerate(grouped):
            assert np.array_equal(a[s], merged[:, f])
    kept = sgroups >= 0                                                      # by_feature: the rows whose label is not -1
    same_moments(by_feature, Moments.from_table(host_moments(theta[kept], Xb[kept], held[kept], None, 1)[1]))
    only_samples, by_feature = model.expected_counts(Xb, sample_groups=sgroups)      # no mask at all
    same_moments(by_feature, Moments.from_table(host_moments(theta[kept], Xb[kept], None, None, 1)[1]))
    assert only_samples.shape == (4, 1) and np.array_equal(only_samples.n_obs[:, 0], np.bincount(sgroups[kept], minlength=4) * n)
    # seven feature groups in passes of 3 equal one pass
    one_pass = _solver.device_moments(model.W_, model.components_, Xb, mask=held, groups=fgroups, n_groups=7)
    same(_solver.device_moments(model.W_, model.components_, Xb, mask=held, groups=fgroups, n_groups=7, _pass_groups=3), one_pass)
    same(one_pass, host_moments(theta, Xb, held, fgroups, 7))
    g40 = r.integers(-1, 40, n)                                              # more than 16 groups: three passes by themselves
    by_sample, _ = model.expected_counts(Xb, mask=held, feature_groups=g40)
    same_moments(by_sample, Moments.from_table(host_moments(theta, Xb, held, g40, 40)[0]))
    # the same data in other clothes -- float64, uint8 with a float mask, CSR, COO, packed bits -- in one call or in row
    # blocks of 16: integers, so exactly the dense bool arrays
    want = model.expected_counts(Xb, mask=held, feature_groups=fgroups, sample_groups=sgroups)
    others = ((X, held), (Xb.astype(np.uint8), 2.5 * held), (sp.csr_matrix(X), sp.csr_matrix(held)), (sp.coo_matrix(X), held),
              (Xb, sp.csr_matrix(held)), (PackedBits.from_dense(Xb), PackedBits.from_dense(held)), (PackedBits.from_dense(Xb), held))
    for block_bytes in (None, 16 * 8 * 500):
        if block_bytes:
            monkeypatch.setattr(_solver, "SCORE_SAMPLES_BLOCK_BYTES", block_bytes)
        for Xo, mo in others:
            got = model.expected_counts(Xo, mask=mo, feature_groups=fgroups, sample_groups=sgroups)
            same_moments(got[0], want[0])
            same_moments(got[1], want[1])
            got = model.expected_counts(Xo, mask=mo, feature_groups=fgroups)
            same_moments(got[0], Moments.from_table(want_rows))
    monkeypatch.undo()
    # new rows: transform first, then judge them with W=
    Wnew = model.transform(X[:7])
    got = model.expected_counts(X[:7], mask=held[:7], W=Wnew, feature_groups=fgroups)
    want = host_moments(model.predict_proba(W=Wnew), Xb[:7], held[:7], fgroups, 7)
    same_moments(got[0], Moments.from_table(want[0]))
    same_moments(got[1], Moments.from_table(want[1]))


def test_estimator_refuses_factors_that_give_nan(hip):
    from nbmf_mm_amd import NBMF
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    X = r.random((12, 9)) < 0.3
    assert model.expected_counts(X)[1].n_obs.sum() == X.size
    model.components_[1, 4] = np.nan
    with pytest.raises(ValueError, match="Theta has NaN entries"):
        model.expected_counts(X)
    mask = np.ones((12, 9), dtype=bool)
    mask[:, 4] = False                                                        # the NaN column unobserved: nothing to refuse
    assert model.expected_counts(X, mask=mask)[1].n_obs.sum() == mask.sum()
