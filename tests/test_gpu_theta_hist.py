"""Class histograms of Theta counted on the device: nbmf_theta_hist, Context.theta_hist, NBMF.theta_histogram / roc_auc /
calibration_curve.

REFERENCE.  Always ``host_theta_hist(ctx.predict_rows(row0, nrows, clip_theta=True), x, mask, bins)``
(tests/test_theta_hist_cpu.py: the contract in NumPy, ``np.bincount`` per class).  The device bins the very Theta
predict_rows returns, with one rounded multiplication as NumPy's, and counts in integers: every comparison in this file is
for EQUALITY of int64 arrays.  There is no tolerance anywhere.

SHAPES.  The smallest at which each path runs (those of tests/test_gpu_score_samples.py): n = 297 (staged width 300: three
pad columns inside one lane's four, a ragged last strip, five strips over two workgroups), n = 130 (nA = 256: a workgroup
with one whole pad strip), n = 100 (nA = 128: a workgroup two of whose waves leave before the k loop), m = 37 / 53 (pad rows
in the last 16-row tile, several tiles, an offset inside a tile), K = 5 (a ragged k block) and K = 130 (the sliced factor
layout)."""
import ctypes

import numpy as np
import pytest

from conftest import config1_X, config1_mask
from test_theta_hist_cpu import hist_case, host_theta_hist

pytestmark = pytest.mark.gpu

ALL_BINS = (1, 2, 10, 256, 1000, 1024)


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
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and w.dtype == np.int64 and g.shape == w.shape
        assert np.array_equal(g, w)


# ---- 1. ragged tile ----------------------------------------------------------------------------------------------------------
def test_ragged_tile_every_bin_count_and_byte_kind(hip):
    m, n = 37, 297
    W, H, X, mask = hist_case(5, m, n)
    assert not mask[m // 3].any() and not mask[:, n // 3].any()             # a fully masked row and column are in it
    r = np.random.default_rng(9)
    xb = X.astype(np.uint8) * r.integers(1, 256, (m, n), dtype=np.uint8)    # bytes: any nonzero value is class 1 / observed
    mb = mask.astype(np.uint8) * r.integers(1, 256, (m, n), dtype=np.uint8)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        for bins in ALL_BINS:
            for mk, mk_bytes, observed in ((None, None, m * n), (mask, mb, int(mask.sum()))):
                got = ctx.theta_hist(X, mk, bins=bins)
                assert got[0].shape == (2, bins) and got[1].shape == (2,)
                same(got, host_theta_hist(theta, X, mk, bins))
                assert got[0].sum() == observed and not got[1].any()
                assert got[0][1].sum() == (X.sum() if mk is None else (X & mask).sum())
                same(ctx.theta_hist(X.astype(np.uint8), mk, bins=bins), got)
                same(ctx.theta_hist(xb, mk_bytes, bins=bins), got)
        assert ctx.theta_hist(X, mask)[0].shape == (2, 256)                  # the default


@pytest.mark.parametrize("k,m,n", [(130, 20, 130), (5, 37, 100), (130, 53, 297)])
def test_pad_strips_and_the_sliced_layout(hip, k, m, n):
    W, H, X, mask = hist_case(k, m, n)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        for bins in (10, 1024):
            same(ctx.theta_hist(X, mask, bins=bins), host_theta_hist(theta, X, mask, bins))
            same(ctx.theta_hist(X, bins=bins), host_theta_hist(theta, X, None, bins))


# ---- 2. offsets and panels ------------------------------------------------------------------------------------------------------
def test_row_offsets_panels_and_repeats(hip, monkeypatch):
    m, n = 53, 297
    W, H, X, mask = hist_case(5, m, n)
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        calls = [(lambda b=b: ctx.theta_hist(X, mask, bins=b)) for b in (10, 1024)]
        calls += [lambda: ctx.theta_hist(X, bins=256),
                  lambda: ctx.theta_hist(X[5:25], mask[5:25], 5, 20, bins=1000),
                  lambda: ctx.theta_hist(X[48:], None, 48, bins=256),
                  lambda: ctx.theta_hist(X[20:], mask[20:], 20, bins=2)]
        wants = [host_theta_hist(theta, X, mask, 10), host_theta_hist(theta, X, mask, 1024), host_theta_hist(theta, X, None, 256),
                 host_theta_hist(theta[5:25], X[5:25], mask[5:25], 1000),   # slices of the whole-matrix reference
                 host_theta_hist(theta[48:], X[48:], None, 256),             # the last, ragged 16-row tile alone
                 host_theta_hist(theta[20:], X[20:], mask[20:], 2)]
        unset = [call() for call in calls]
        for got, want in zip(unset, wants):
            same(got, want)
        # the reference of a row range is also what predict_rows gives for that range
        same(unset[3], host_theta_hist(ctx.predict_rows(5, 20), X[5:25], mask[5:25], 1000))
        # disjoint row ranges add up
        parts = [ctx.theta_hist(X[a:b], mask[a:b], a, b - a, bins=1024) for a, b in ((0, 5), (5, 25), (25, 48), (48, m))]
        same((sum(p[0] for p in parts), sum(p[1] for p in parts)), wants[1])
        # no rows: zeros, and nothing is read
        empty = ctx.theta_hist(X[7:7], mask[7:7], 7, 0, bins=16)
        assert empty[0].shape == (2, 16) and not empty[0].any() and not empty[1].any()
        # the same call twice, and every panel height: identical arrays
        for call, want in zip(calls, unset):
            same(call(), want)
        for rows_per_panel in ("1", "7", "16", "21"):
            monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", rows_per_panel)
            for call, want in zip(calls, unset):
                same(call(), want)
    with context(hip, W, H) as ctx:                                          # another context, the same factors
        same(ctx.theta_hist(X, mask, bins=10), unset[0])


# ---- 3. strided input ---------------------------------------------------------------------------------------------------------------
def test_strided_inputs_and_nothing_beside_the_slice_is_read(hip):
    m, n = 37, 297
    W, H, X, mask = hist_case(5, m, n)
    # what lies beside the slices would change the counts if it were read: ones and "observed"
    wide_x = np.ones((m + 2, n + 40), dtype=bool)
    wide_m = np.ones((m + 3, n + 9), dtype=np.uint8)
    wide_x[1:m + 1, 7:7 + n] = X
    wide_m[2:m + 2, 0:n] = mask
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        for bins in (10, 1024):
            want = host_theta_hist(theta, X, mask, bins)
            same(ctx.theta_hist(wide_x[1:m + 1, 7:7 + n], wide_m[2:m + 2, 0:n], bins=bins), want)
            same(ctx.theta_hist(wide_x[1:m + 1, 7:7 + n], mask, bins=bins), want)
            same(ctx.theta_hist(wide_x[1:m + 1, 7:7 + n], bins=bins), host_theta_hist(theta, X, None, bins))
            same(ctx.theta_hist(wide_x[6:26, 7:7 + n], wide_m[7:27, 0:n], 5, 20, bins=bins),
                 host_theta_hist(theta[5:25], X[5:25], mask[5:25], bins))
        # the last columns count: nothing stops short of column n - 1
        m2 = np.zeros((m, n), dtype=bool)
        m2[:, n - 3:] = True
        got = ctx.theta_hist(X, m2, bins=256)
        assert got[0].sum() == 3 * m
        same(got, host_theta_hist(theta, X, m2, 256))


# ---- 4. edges -----------------------------------------------------------------------------------------------------------------------
def test_a_theta_on_an_edge_is_in_the_upper_bin_and_one_in_the_last(hip):
    k, m, n = 5, 37, 297
    r = np.random.default_rng(31)
    W = np.zeros((k, m))
    W[r.integers(0, k, m), np.arange(m)] = 1.0                               # one-hot columns: Theta[i, j] = H[k_i, j] exactly
    H = r.integers(0, 9, (k, n)) / 8.0                                       # {0, 1/8, ..., 1}
    X = r.random((m, n)) < 0.4
    mask = r.random((m, n)) < 0.7
    eighths = np.rint(8.0 * (W.T @ H)).astype(np.int64)                      # which multiple of 1/8 each Theta is
    with context(hip, W, H) as ctx:
        theta = ctx.predict_rows()
        assert np.array_equal(theta, eighths / 8.0) and (theta == 1.0).any() and (theta == 0.0).any()
        for bins in (8, 1024):
            got = ctx.theta_hist(X, mask, bins=bins)
            same(got, host_theta_hist(theta, X, mask, bins))
            want = np.zeros((2, bins), dtype=np.int64)
            edge_bin = np.minimum(eighths * (bins // 8), bins - 1)           # the bin whose LOWER edge Theta is; 1 -> the last
            for c in (0, 1):
                want[c] = np.bincount(edge_bin[mask & (X == bool(c))], minlength=bins)
            assert np.array_equal(got[0], want)
            in_last = eighths >= (7 if bins == 8 else 8)                     # B = 8: [7/8, 1]; B = 1024: theta = 1 alone
            assert got[0][:, bins - 1].sum() == (mask & in_last).sum()
    # an un-normalised W: every raw Theta is beyond 1, the clip is always on, everything lands in the last bin
    with context(hip, 3.0 * W, 0.5 + H / 2.0) as ctx:
        assert ctx.predict_rows(clip_theta=False).min() >= 1.5
        for bins in (8, 1000):
            hist, nan_count = ctx.theta_hist(X, mask, bins=bins)
            assert not hist[:, :bins - 1].any() and not nan_count.any()
            assert hist[:, bins - 1].tolist() == [int((mask & ~X).sum()), int((mask & X).sum())]
            same((hist, nan_count), host_theta_hist(ctx.predict_rows(), X, mask, bins))


# ---- 5. NaN ---------------------------------------------------------------------------------------------------------------------------
def test_a_nan_theta_is_in_no_bin(hip):
    m, n = 37, 297
    W, H, X, mask = hist_case(5, m, n)
    j = 131
    Hn = H.copy()
    Hn[2, j] = np.nan                                                        # W > 0: all of column j of Theta is NaN
    with context(hip, W, Hn) as ctx:
        theta = ctx.predict_rows()
        assert np.isnan(theta[:, j]).all() and np.isnan(theta).sum() == m
        for mk in (mask, None):
            obs = np.ones(m, dtype=bool) if mk is None else mk[:, j]
            hist, nan_count = ctx.theta_hist(X, mk, bins=256)
            assert nan_count.tolist() == [int((obs & ~X[:, j]).sum()), int((obs & X[:, j]).sum())] and nan_count.sum() > 0
            same((hist, nan_count), host_theta_hist(theta, X, mk, 256))
            # the histograms: those without that column
            without = np.ones((m, n), dtype=bool) if mk is None else mk.copy()
            without[:, j] = False
            with context(hip, W, H) as clean:
                assert np.array_equal(hist, clean.theta_hist(X, without, bins=256)[0])


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_outputs_and_the_context_as_they_were(hip):
    m, n = 37, 53
    W, H, X, mask = hist_case(4, m, n)
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    xb = np.ascontiguousarray(X).view(np.uint8)
    mb = np.ascontiguousarray(mask).view(np.uint8)
    hist = np.full((2, 8), -7, dtype=np.int64)
    nan_count = np.full(2, -7, dtype=np.int64)
    with hip.Context(m, n, 4) as ctx:
        args = (0, m, 8, ptr(xb), n, None, 0, ptr(hist), ptr(nan_count))
        assert lib.nbmf_theta_hist(ctx._h, *args) == hip.NBMF_ERR_STATE       # no factors
        assert b"no factors" in lib.nbmf_last_error()
        with pytest.raises(hip.NBMFHipError, match="no factors"):
            ctx.theta_hist(X)
        ctx.set_factors(W, H)
        theta = ctx.predict_rows()
        want = host_theta_hist(theta, X, mask, 8)
        same(ctx.theta_hist(X, mask, bins=8), want)
        bad = [(-1, 2) + args[2:], (m, 1) + args[2:], (m - 1, 2) + args[2:], (0, -1) + args[2:],     # rows outside [0, m)
               args[:2] + (0,) + args[3:], args[:2] + (1025,) + args[3:], args[:2] + (-1,) + args[3:],   # bins outside [1, 1024]
               args[:4] + (n - 1,) + args[5:],                                                       # ldx < n
               args[:5] + (ptr(mb), n - 1) + args[7:],                                               # ldmask < n with a mask
               args[:7] + (None, ptr(nan_count)),                                                    # no hist
               args[:3] + (None,) + args[4:]]                                                        # no data, nrows > 0
        for a in bad:
            assert lib.nbmf_theta_hist(ctx._h, *a) == hip.NBMF_ERR_ARG, a
            assert np.all(hist == -7) and np.all(nan_count == -7)
        # ldmask is not looked at without a mask; nan_count may be null
        assert lib.nbmf_theta_hist(ctx._h, *(args[:6] + (-5, ptr(hist), None))) == hip.NBMF_OK
        assert np.array_equal(hist, host_theta_hist(theta, X, None, 8)[0]) and np.all(nan_count == -7)
        # no rows: nothing is read (null data), the outputs are zeroed
        hist[:] = -7
        assert lib.nbmf_theta_hist(ctx._h, 5, 0, 8, None, n, None, 0, ptr(hist), ptr(nan_count)) == hip.NBMF_OK
        assert not hist.any() and not nan_count.any()
        same(ctx.theta_hist(X, mask, bins=8), want)                          # as usable as before
        # Context.theta_hist: its ValueErrors, with a device behind it
        for call in (lambda: ctx.theta_hist(X, bins=0), lambda: ctx.theta_hist(X, bins=1025), lambda: ctx.theta_hist(X[:5]),
                     lambda: ctx.theta_hist(X.astype(np.float64)), lambda: ctx.theta_hist(X, mask.astype(np.float64)),
                     lambda: ctx.theta_hist(X, row0=m, nrows=1), lambda: ctx.theta_hist(np.asfortranarray(X))):
            with pytest.raises(ValueError):
                call()
        same(ctx.theta_hist(X, mask, bins=8), want)
    # a sharded context refuses, and answers again once detached
    with hip.Context(m, n, 4) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X, mask=mask)
        ctx.set_factors(W, H)
        ctx.comm_init_host(lambda arr: None, 1, 0)
        assert lib.nbmf_theta_hist(ctx._h, *args) == hip.NBMF_ERR_STATE
        assert b"unsharded" in lib.nbmf_last_error()
        ctx.comm_detach()
        same(ctx.theta_hist(X, mask, bins=8), want)


# ---- 7. the estimator --------------------------------------------------------------------------------------------------------------------
def test_estimator_on_held_out_entries(hip, monkeypatch):
    import scipy.sparse as sp
    from sklearn.metrics import roc_auc_score
    from nbmf_mm_amd import NBMF, _metrics, _solver
    X, train = config1_X(), config1_mask()
    held = ~train
    model = NBMF(6, random_state=0, max_iter=20, tol=0).fit(X, mask=train)
    theta = model.predict_proba()
    Xb = X != 0
    # theta_histogram
    for bins in (256, 1000):
        want, want_nan = host_theta_hist(theta, Xb, held, bins)
        assert not want_nan.any()
        hist, edges = model.theta_histogram(Xb, mask=held, bins=bins)
        assert hist.dtype == np.int64 and np.array_equal(hist, want) and hist.sum() == held.sum()
        assert np.array_equal(edges, np.arange(bins + 1) / bins)
    assert np.array_equal(model.theta_histogram(Xb, mask=held)[0], host_theta_hist(theta, Xb, held, 256)[0])
    assert np.array_equal(model.theta_histogram(Xb)[0], host_theta_hist(theta, Xb, None, 256)[0])
    # roc_auc: _metrics on the host histogram, and within its slack of the exact AUC
    want = host_theta_hist(theta, Xb, held, 1024)[0]
    auc, slack = model.roc_auc(Xb, mask=held, return_slack=True)
    assert (auc, slack) == _metrics.auc_from_hist(want) and model.roc_auc(Xb, mask=held) == auc
    exact = roc_auc_score(Xb[held], theta[held])
    print(f"held-out AUC {auc:.5f} +- {slack:.5f} (exact {exact:.5f})")
    assert abs(auc - exact) <= slack + 1e-15
    assert model.roc_auc(Xb, mask=held, bins=16) == _metrics.auc_from_hist(host_theta_hist(theta, Xb, held, 16)[0])[0]
    # calibration_curve
    for n_bins, resolution in ((10, 100), (4, 256), (5, 1)):
        got = model.calibration_curve(Xb, mask=held, n_bins=n_bins, resolution=resolution)
        want = _metrics.calibration_from_hist(host_theta_hist(theta, Xb, held, n_bins * resolution)[0], n_bins)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True)
        assert got[2].sum() == held.sum()
    # the same data in other clothes -- float64, uint8, a float mask, CSR, COO -- in one call or in row blocks of 16:
    # integers, so exactly the dense bool arrays
    want = model.theta_histogram(Xb, mask=held, bins=1000)[0]
    others = ((X, held), (Xb.astype(np.uint8), 2.5 * held), (sp.csr_matrix(X), sp.csr_matrix(held)), (sp.coo_matrix(X), held),
              (Xb, sp.csr_matrix(held)))
    for Xo, mo in others:
        assert np.array_equal(model.theta_histogram(Xo, mask=mo, bins=1000)[0], want)
    monkeypatch.setattr(_solver, "SCORE_SAMPLES_BLOCK_BYTES", 16 * 8 * 500)
    for Xo, mo in others:
        assert np.array_equal(model.theta_histogram(Xo, mask=mo, bins=1000)[0], want)
    assert model.roc_auc(sp.csr_matrix(X), mask=sp.csr_matrix(held)) == auc
    hist, nan_count = _solver.device_theta_hist(model.W_, model.components_, sp.csr_matrix(X), mask=sp.csr_matrix(held), bins=1000)
    assert np.array_equal(hist, want) and not nan_count.any()
    monkeypatch.undo()
    # new rows: transform first, then judge them with W=
    Wnew = model.transform(X[:7])
    got = model.theta_histogram(X[:7], mask=held[:7], W=Wnew, bins=64)[0]
    assert np.array_equal(got, host_theta_hist(model.predict_proba(W=Wnew), Xb[:7], held[:7], 64)[0])


def test_estimator_refuses_factors_that_give_nan(hip):
    from nbmf_mm_amd import NBMF
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    X = r.random((12, 9)) < 0.3
    assert model.theta_histogram(X, bins=4)[0].sum() == X.size
    model.components_[1, 4] = np.nan
    for call in (lambda: model.theta_histogram(X), lambda: model.roc_auc(X), lambda: model.calibration_curve(X)):
        with pytest.raises(ValueError, match="Theta has NaN entries"):
            call()
    mask = np.ones((12, 9), dtype=bool)
    mask[:, 4] = False                                                        # the NaN column unobserved: nothing to refuse
    assert model.theta_histogram(X, mask=mask, bins=4)[0].sum() == mask.sum()
