"""Theta = W^T H handed back by the device: nbmf_predict_at (index pairs), nbmf_predict_rows (row slabs as float64 or as
thresholded bytes) and the estimator methods on top of them (predict_proba, predict, impute).

TOLERANCE (derived, not measured).  A float64 dot product of length K, summed in any order, with or without FMA, errs by
at most gamma_K * sum_k |w_k h_k| with gamma_K ~ K * 2^-53.  The device value and NumPy's ``W.T @ H`` each obey it, so per
entry            tol[i, j] = 2.1 * K * 2^-53 * (|W|.T @ |H|)[i, j],
and clipping to [0, 1] is 1-Lipschitz, so the bound survives it.  The byte slabs are compared EXACTLY, after asserting
that no reference entry lies within tol of the threshold (true for these seeds; the assertion keeps it honest).

CASES.  "case k": default_rng(1000 + k), W k x m uniform(0.1, 0.9) with columns normalised, H k x n uniform(0.1, 0.9),
m x n = 37 x 53 (odd, several 16-row tiles, less than one 64-column strip plus the pad), for k in 1, 3, 4, 5, 16, 17, 40,
130: below, at and above a multiple of 4 (the MFMA's k block), every register layout of the context (16, 32, 64, 128),
one sliced K.  130 x 257 at k = 5 and 40 crosses the 128 padding in both dimensions and fills several strips."""
import numpy as np
import pytest

from conftest import config1_X, config1_mask

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 5, 16, 17, 40, 130)
WIDE = ((5, 130, 257), (40, 130, 257))
SENTINEL = -7.25


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


_cases = {}


def case(k, m=37, n=53):
    """(W k x m, H k x n, ref = W.T @ H, tol) of case k, computed once and shared (read-only)."""
    key = (k, m, n)
    if key not in _cases:
        r = np.random.default_rng(1000 + k)
        W = r.uniform(0.1, 0.9, (k, m))
        W /= W.sum(0)
        H = r.uniform(0.1, 0.9, (k, n))
        ref = W.T @ H
        for a in (W, H, ref):
            a.setflags(write=False)
        _cases[key] = (W, H, ref, bound(W, H))
    return _cases[key]


def bound(W, H):
    return 2.1 * W.shape[0] * 2.0 ** -53 * (np.abs(W).T @ np.abs(H))


def all_pairs(m, n, seed, duplicates=100):
    r = np.random.default_rng(seed)
    flat = r.permutation(m * n)
    flat = np.concatenate([flat, r.choice(flat, duplicates)])
    return flat // n, flat % n


def context(hip, W, H):
    ctx = hip.Context(W.shape[1], H.shape[1], W.shape[0])
    ctx.set_factors(W, H)
    return ctx


def report(tag, got, ref, tol):
    with np.errstate(divide="ignore", invalid="ignore"):
        print(tag, "max |got - ref| / tol = %.3f" % float(np.max(np.abs(got - ref) / tol)) if ref.size else "empty")


# ---- 1. predict_at: parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_predict_at_matches_the_host_product(hip, k):
    W, H, ref, tol = case(k)
    rows, cols = all_pairs(37, 53, seed=k)
    with context(hip, W, H) as ctx:
        for clip in (True, False):
            got = ctx.predict_at(rows, cols, clip_theta=clip)
            assert got.dtype == np.float64 and got.shape == rows.shape
            report(f"k={k} clip={clip}", got, ref[rows, cols], tol[rows, cols])
            assert np.all(np.abs(got - ref[rows, cols]) <= tol[rows, cols])      # Theta is inside (0, 1): the clip is idle
    H2 = 2.0 * H
    ref2, tol2 = W.T @ H2, bound(W, H2)
    over = ref2[rows, cols] > 1.0 + tol2[rows, cols]
    assert over.any() and not over.all()
    with context(hip, W, H2) as ctx:
        got = ctx.predict_at(rows, cols, clip_theta=True)
        assert np.all(got[over] == 1.0)
        assert np.all(np.abs(got - np.clip(ref2, 0, 1)[rows, cols]) <= tol2[rows, cols])
        got = ctx.predict_at(rows, cols, clip_theta=False)
        report(f"k={k} 2H unclipped", got, ref2[rows, cols], tol2[rows, cols])
        assert np.all(np.abs(got - ref2[rows, cols]) <= tol2[rows, cols])


# ---- 2. predict_at: determinism ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (5, 40, 130))
def test_predict_at_depends_on_the_pair_only(hip, k, monkeypatch):
    W, H, _, _ = case(k)
    rows, cols = all_pairs(37, 53, seed=50 + k, duplicates=0)
    assert rows.size == 1961
    with context(hip, W, H) as ctx:
        first = ctx.predict_at(rows, cols)
        assert np.array_equal(first, ctx.predict_at(rows, cols))
        p = np.random.default_rng(3).permutation(rows.size)
        assert np.array_equal(first[p], ctx.predict_at(rows[p], cols[p]))
        monkeypatch.setenv("NBMF_PREDICT_PAIRS", "256")          # 8 chunks, the last one ragged
        assert np.array_equal(first, ctx.predict_at(rows, cols))
        monkeypatch.setenv("NBMF_PREDICT_PAIRS", "1")
        assert np.array_equal(first[:40], ctx.predict_at(rows[:40], cols[:40]))


# ---- 3. predict_at: index checks --------------------------------------------------------------------------------------------
def test_predict_at_refuses_indices_outside_the_matrix(hip, monkeypatch):
    W, H, ref, tol = case(5)
    rows, cols = all_pairs(37, 53, seed=9, duplicates=0)
    with context(hip, W, H) as ctx:
        for pos, (i, j) in ((700, (37, 0)), (3, (-1, 5)), (1960, (0, 53)), (0, (2 ** 40, 1))):
            r, c = rows.copy(), cols.copy()
            r[pos], c[pos] = i, j
            r[1200], c[1200] = (37, 53) if pos < 1200 else (r[1200], c[1200])      # a later offender: the LOWEST is named
            with pytest.raises(ValueError, match=rf"position {pos}\b"):
                ctx.predict_at(r, c)
        monkeypatch.setenv("NBMF_PREDICT_PAIRS", "256")
        r = rows.copy()
        r[1500] = 99
        with pytest.raises(ValueError, match=r"position 1500\b"):
            ctx.predict_at(r, cols)
        monkeypatch.delenv("NBMF_PREDICT_PAIRS")
        with pytest.raises(ValueError):
            ctx.predict_at(rows[:5], cols[:4])
        with pytest.raises(ValueError):
            ctx.predict_at(rows.astype(np.float64), cols)
        assert ctx.predict_at(rows[:0], cols[:0]).shape == (0,)
        got = ctx.predict_at(rows, cols)                            # the context is as usable as before
        assert np.all(np.abs(got - ref[rows, cols]) <= tol[rows, cols])


# ---- 4. predict_rows: float64 ------------------------------------------------------------------------------------------------
def slab_requests(m):
    return ((0, m), (5, 1), (15, 18), (m - 1, 1), (3, 0))


@pytest.mark.parametrize("k,m,n", [(k, 37, 53) for k in KS] + list(WIDE))
def test_predict_rows_float64(hip, k, m, n):
    W, H, ref, tol = case(k, m, n)
    with context(hip, W, H) as ctx:
        for row0, nrows in slab_requests(m):
            buf = np.full((m + 2, n + 3), SENTINEL)
            out = buf[1 + row0:1 + row0 + nrows, :n]
            got = ctx.predict_rows(row0, nrows, out=out)
            assert got is out
            report(f"k={k} {m}x{n} rows {row0}+{nrows}", out, ref[row0:row0 + nrows], tol[row0:row0 + nrows])
            assert np.all(np.abs(out - ref[row0:row0 + nrows]) <= tol[row0:row0 + nrows])
            untouched = np.ones(buf.shape, dtype=bool)
            untouched[1 + row0:1 + row0 + nrows, :n] = False
            assert np.all(buf[untouched] == SENTINEL), "something outside the request was written"
        fresh = ctx.predict_rows()
        assert fresh.shape == (m, n) and fresh.dtype == np.float64 and np.all(np.abs(fresh - ref) <= tol)
        assert np.array_equal(fresh[15:33], ctx.predict_rows(15, 18))            # a slab is the same bits as the whole
        for bad in ((-1, 2), (m, 1), (m - 1, 2), (0, -1)):
            with pytest.raises(ValueError):
                ctx.predict_rows(*bad)
        assert np.all(np.abs(ctx.predict_rows() - ref) <= tol)


# ---- 5. predict_rows: bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,n", [(k, 37, 53) for k in KS] + list(WIDE))
def test_predict_rows_bytes(hip, k, m, n):
    W, H, ref, tol = case(k, m, n)
    thr = 0.5
    for scale, clip in ((1.0, True), (1.0, False), (2.0, True)):
        Hs = scale * H
        refs, tols = W.T @ Hs, bound(W, Hs)
        want = np.clip(refs, 0, 1) if clip else refs
        assert np.all(np.abs(want - thr) > tols), "a reference entry is within tol of the threshold: the case proves nothing"
        want = want > thr
        assert 0.2 < want.mean() < 0.8 or scale == 2.0
        with context(hip, W, Hs) as ctx:
            got = ctx.predict_rows(clip_theta=clip, threshold=thr)
            assert got.dtype == np.bool_ and got.shape == (m, n)
            assert np.array_equal(got, want)
            for row0, nrows in slab_requests(m):
                buf = np.full((m + 2, n + 3), 9, dtype=np.uint8)
                out = buf[1 + row0:1 + row0 + nrows, :n]
                ctx.predict_rows(row0, nrows, clip_theta=clip, threshold=thr, out=out)
                assert np.array_equal(out, want[row0:row0 + nrows].astype(np.uint8))
                buf[1 + row0:1 + row0 + nrows, :n] = 9
                assert np.all(buf == 9), "something outside the request was written"
            if scale == 2.0:
                # every Theta above 1 is clipped to exactly 1, which is NOT > 1: the comparison sees theta AFTER the clip
                assert not ctx.predict_rows(clip_theta=True, threshold=1.0).any()
                assert np.all(np.abs(refs - 1.0) > tols)
                assert np.array_equal(ctx.predict_rows(clip_theta=False, threshold=1.0), refs > 1.0)
            with pytest.raises(ValueError, match="NaN"):
                ctx.predict_rows(threshold=float("nan"))


def test_threshold_is_strict_and_one_hot_rows_are_exact(hip):
    """W one-hot per column: Theta[i, j] = H[c(i), j] exactly, whatever the order (all other terms are 0 * h = 0)."""
    k, m, n = 5, 37, 53
    comp = np.arange(m) % k
    W = np.zeros((k, m))
    W[comp, np.arange(m)] = 1.0
    H = np.random.default_rng(77).uniform(0.1, 0.9, (k, n))
    up, down = np.nextafter(0.5, 1), np.nextafter(0.5, 0)
    H[0, 3], H[1, 20], H[2, 52] = 0.5, up, down
    H[4, 0], H[3, 17], H[0, 36] = down, 0.5, up
    want = H[comp]
    with context(hip, W, H) as ctx:
        dense = ctx.predict_rows()
        assert np.array_equal(dense, want)
        rows, cols = all_pairs(m, n, seed=1)
        assert np.array_equal(ctx.predict_at(rows, cols), want[rows, cols])
        got = ctx.predict_rows(threshold=0.5)
        assert np.array_equal(got, want > 0.5)
        for c, j, bit in ((0, 3, False), (1, 20, True), (2, 52, False), (4, 0, False), (3, 17, False), (0, 36, True)):
            assert np.all(got[comp == c, j] == bit)


# ---- 6. panels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,m,n", WIDE)
def test_panels_do_not_change_a_bit(hip, k, m, n, monkeypatch):
    W, H, ref, tol = case(k, m, n)
    with context(hip, W, H) as ctx:
        whole, whole_b = ctx.predict_rows(), ctx.predict_rows(threshold=0.5)
        part, part_b = ctx.predict_rows(5, 100), ctx.predict_rows(5, 100, threshold=0.5)
        assert np.all(np.abs(whole - ref) <= tol)
        for rows_per_panel in ("16", "7"):
            monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", rows_per_panel)
            assert np.array_equal(whole, ctx.predict_rows())
            assert np.array_equal(whole_b, ctx.predict_rows(threshold=0.5))
            assert np.array_equal(part, ctx.predict_rows(5, 100))
            assert np.array_equal(part_b, ctx.predict_rows(5, 100, threshold=0.5))
        assert np.array_equal(whole[5:105], part)


# ---- 7. after a fit -----------------------------------------------------------------------------------------------------------------
def test_prediction_follows_a_fit(hip, both_small_paths):
    X, mask = config1_X(), config1_mask()
    r = np.random.default_rng(21)
    W0 = r.uniform(0.1, 0.9, (6, 100))
    W0 /= W0.sum(0)
    H0 = r.uniform(0.1, 0.9, (6, 500))
    with hip.Context(100, 500, 6) as ctx:
        ctx.set_hyper(1.2, 1.2)
        ctx.upload(X, mask=mask)
        ctx.set_factors(W0, H0)
        ctx.run(5, 0.0)
        W, H = ctx.get_factors()
        assert not np.array_equal(W, W0)
        ref, tol = np.clip(W.T @ H, 0, 1), bound(W, H)
        rows, cols = r.integers(0, 100, 500), r.integers(0, 500, 500)
        got = ctx.predict_at(rows, cols)
        report(f"after a fit ({both_small_paths}), pairs", got, ref[rows, cols], tol[rows, cols])
        assert np.all(np.abs(got - ref[rows, cols]) <= tol[rows, cols])
        slab = ctx.predict_rows(0, 100)
        report(f"after a fit ({both_small_paths}), slab", slab, ref, tol)
        assert np.all(np.abs(slab - ref) <= tol)
        ctx.w_only_steps(2)                                           # ... and after transform's loop
        W, H = ctx.get_factors()
        assert np.all(np.abs(ctx.predict_rows() - np.clip(W.T @ H, 0, 1)) <= bound(W, H))
    assert both_small_paths.served() == ((1, 0, 0) if both_small_paths == "single-launch" else (0, 0, 1))


def test_prediction_needs_factors_not_data(hip):
    W, H, ref, tol = case(4)
    with hip.Context(37, 53, 4) as ctx:
        with pytest.raises(hip.NBMFHipError, match="no factors"):
            ctx.predict_rows()
        with pytest.raises(hip.NBMFHipError, match="no factors"):
            ctx.predict_at(np.array([0]), np.array([0]))
        ctx.set_factors(W, H)
        assert np.all(np.abs(ctx.predict_rows() - ref) <= tol)


# ---- 8. estimator ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_estimator_methods(hip, orientation):
    from nbmf_mm_amd import NBMF
    g = np.random.default_rng(11)
    X = (g.random((60, 80)) < 0.3).astype(np.float64)
    mask = g.random((60, 80)) < 0.9
    model = NBMF(4, random_state=0, max_iter=30, tol=0, orientation=orientation).fit(X, mask=mask)
    W, H = model.W_, model.components_
    assert W.shape == (60, 4) and H.shape == (4, 80)
    ref, tol = model.inverse_transform(W), bound(np.ascontiguousarray(W.T), H)

    dense = model.predict_proba()
    assert dense.shape == (60, 80) and dense.dtype == np.float64
    report(f"{orientation} predict_proba", dense, ref, tol)
    assert np.all(np.abs(dense - ref) <= tol)

    rows, cols = g.integers(0, 60, 300), g.integers(0, 80, 300)
    at = model.predict_proba(rows=rows, cols=cols)
    assert at.shape == (300,)
    assert np.all(np.abs(at - dense[rows, cols]) <= 2 * tol[rows, cols])

    assert np.all(np.abs(ref - 0.3) > tol), "an entry is within tol of the threshold: the comparison proves nothing"
    labels = model.predict(threshold=0.3)
    assert labels.dtype == np.bool_ and labels.shape == (60, 80)
    assert np.array_equal(labels, ref > 0.3)
    assert 0.1 < labels.mean() < 0.9

    filled = model.impute(X, mask)
    assert filled.dtype == np.float64 and filled is not X
    assert np.array_equal(filled[mask], X[mask])
    hr, hc = np.nonzero(~mask)
    assert hr.size > 0 and np.array_equal(filled[hr, hc], model.predict_proba(rows=hr, cols=hc))
    assert np.array_equal(model.impute(X, mask.astype(np.float64)), filled)

    Wnew = model.transform(X[:7])
    assert model.predict_proba(W=Wnew).shape == (7, 80)
    assert model.predict(W=Wnew).shape == (7, 80)
    with pytest.raises(ValueError, match="position 1"):
        model.predict_proba(rows=np.array([0, 60]), cols=np.array([0, 0]))
