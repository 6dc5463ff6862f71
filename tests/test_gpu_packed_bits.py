"""Bit-packed input on the device: the unpack kernel entry for entry, and every call that takes packed data, masks or
exclude matrices against the same call fed the unpacked bytes.

NO TOLERANCE ANYWHERE.  A packed operand is expanded on the device into the byte staging the uint8 operand is copied into,
and everything behind that staging is the code the uint8 operand runs: every comparison below is ``np.array_equal``.  The
oracle of the unpack kernel is ``np.unpackbits(bits[:, :ceil(n / 8)], axis=1, count=n)``; the oracle of everything else is
the existing byte path fed ``P.toarray()``.

SHAPES.  The kernel: n below, at and above 8 (a source byte), 32 and 64 (a wave's worth of 4- and 1-byte stores), 100 and
257 (several waves, a second workgroup at 1-byte stores), 1, 3 and 17 rows, every store width (ldout = n: whatever n allows;
n + 1 and n + 13: mostly odd, single bytes; round_up(n, 4): the row panels' pitch, 4 or 8 bytes).  The fit: 300 x 70 (three
upload chunks of 128 rows at NBMF_UPLOAD_CHUNK_ROWS=128, the last one partial; 9 bytes a row, 2 pad bits) and
512 x 520 at K = 64.  The row-slab calls: 50 x 70 and 50 x 64 from row 5 on, in one panel and in panels of 16 rows."""
import ctypes

import numpy as np
import pytest

from nbmf_mm_amd import NBMF, PackedBits, _solver

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


def bernoulli(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


def in_wider_array(P, seed, before=7, after=13, extra=5):
    """The same packed matrix as rows [before, before + rows) of a wider, taller packed array full of other bits."""
    rows, nb = P.bits.shape
    wide = np.random.default_rng(seed).integers(0, 256, (before + rows + after, nb + extra), dtype=np.uint8)
    wide[before:before + rows, :nb] = P.bits
    Q = PackedBits(wide[before:before + rows], P.shape)
    assert Q.ld == nb + extra and np.shares_memory(Q.bits, wide)
    return Q


# ---- 1. the unpack kernel, entry for entry -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 100, 257])
def test_unpack_kernel_entry_for_entry(hip, n):
    nb = (n + 7) // 8
    for rows in (1, 3, 17):
        A = bernoulli((rows, n), 0.5, 100 * n + rows)
        tight = np.packbits(A, axis=1)
        surplus = np.full((rows, nb + 3), 0xFF, dtype=np.uint8)
        surplus[:, :nb] = tight
        padded = tight.copy()
        padded[:, -1] |= (1 << (8 * nb - n)) - 1                # every pad bit of the last byte set
        for form, bits in (("tight", tight), ("surplus bytes", surplus), ("pad bits set", padded)):
            want = np.unpackbits(bits[:, :nb], axis=1, count=n)
            assert np.array_equal(want, A)
            for ldout in (n, n + 1, (n + 3) // 4 * 4, n + 13):
                out = np.full((rows, ldout), 0xAA, dtype=np.uint8)
                hip.selftest_unpack_bits(np.ascontiguousarray(bits), n, out)
                where = f"n={n} rows={rows} {form} ldout={ldout}"
                assert np.array_equal(out[:, :n], want), where
                assert np.all(out[:, n:] == 0xAA), where + ": wrote outside [0, n)"


# ---- 2. the fit --------------------------------------------------------------------------------------------------------------
def fit_outcome(X, mask, orientation, k=5, **fit_kw):
    est = NBMF(n_components=k, max_iter=30, tol=1e-12, random_state=3, orientation=orientation).fit(X, mask=mask, **fit_kw)
    return est


def same_fit(a, b, what):
    assert a.n_iter_ == b.n_iter_, what
    assert np.array_equal(np.asarray(a.loss_curve_), np.asarray(b.loss_curve_)), what
    assert np.array_equal(a.W_, b.W_) and np.array_equal(a.components_, b.components_), what


def fit_operands(shape=(300, 70)):
    X = bernoulli(shape, 0.25, 1)
    M = bernoulli(shape, 0.85, 2)
    weights = np.where(M, np.random.default_rng(3).choice([0.5, 1.0, 2.0], shape), 0.0)     # a float64 WEIGHT mask
    return X, M, weights


@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_fit_parity(hip, both_small_paths, orientation):
    X, M, weights = fit_operands()
    P, PM = PackedBits.from_dense(X), PackedBits.from_dense(M)
    ref = {name: fit_outcome(X, mk, orientation) for name, mk in (("none", None), ("bool", M), ("weights", weights))}
    for what, x, mk, against in (("packed X", P, None, "none"), ("packed X, packed mask", P, PM, "bool"),
                                 ("packed X, bool mask", P, M, "bool"), ("bool X, packed mask", X, PM, "bool"),
                                 ("packed X, weight mask", P, weights, "weights")):
        same_fit(fit_outcome(x, mk, orientation), ref[against], f"{what} ({orientation}, {both_small_paths})")
    assert not np.array_equal(ref["none"].W_, ref["bool"].W_) and not np.array_equal(ref["bool"].W_, ref["weights"].W_)
    # packed arrays that are row slices of wider packed arrays: the rows are further apart, the bytes between them unread
    same_fit(fit_outcome(in_wider_array(P, 11), in_wider_array(PM, 12), orientation), ref["bool"], "row slices of wider arrays")


@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_fit_parity_across_upload_chunks(hip, monkeypatch, both_small_paths, orientation):
    X, M, _ = fit_operands()
    P, PM = PackedBits.from_dense(X), PackedBits.from_dense(M)
    whole = fit_outcome(X, M, orientation)
    monkeypatch.setenv("NBMF_UPLOAD_CHUNK_ROWS", "128")          # 300 rows: chunks of 128, 128 and 44
    chunked = fit_outcome(X, M, orientation)
    same_fit(chunked, whole, "bool input in three chunks against one")
    same_fit(fit_outcome(P, PM, orientation), whole, "packed input in three chunks")
    same_fit(fit_outcome(P, M, orientation), whole, "packed X, bool mask in three chunks")
    same_fit(fit_outcome(in_wider_array(P, 13), in_wider_array(PM, 14), orientation), whole, "row slices in three chunks")
    monkeypatch.setenv("NBMF_UPLOAD_CHUNK_ROWS", "100")          # rounded up to 128: the same chunks
    same_fit(fit_outcome(P, PM, orientation), whole, "chunk height rounded up")


def test_fit_parity_k64_on_the_launches(hip):
    X, M, _ = fit_operands((512, 520))
    s0 = hip.engine_stats()
    ref = fit_outcome(X, M, "beta-dir", k=64)
    got = fit_outcome(PackedBits.from_dense(X), PackedBits.from_dense(M), "beta-dir", k=64)
    s1 = hip.engine_stats()
    same_fit(got, ref, "K = 64, 512 x 520")
    assert s1[0] == s0[0] and s1[2] - s0[2] == 2                 # both ran on the launch-per-kernel engine


def test_solver_and_restarts_take_packed_input(hip):
    X, M, _ = fit_operands()
    P, PM = PackedBits.from_dense(X), PackedBits.from_dense(M)
    a = _solver.nbmf_mm_solver(X, 5, max_iter=20, mask=M, random_state=4)
    b = _solver.nbmf_mm_solver(P, 5, max_iter=20, mask=PM, random_state=4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[4] == b[4]
    (a, ia), (b, ib) = (_solver.nbmf_mm_restarts(x, 5, 3, max_iter=20, mask=mk, random_state=4) for x, mk in ((X, M), (P, PM)))
    assert ia == ib and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    est_a = NBMF(n_components=5, max_iter=20, random_state=4).fit_transform(X)
    est_b = NBMF(n_components=5, max_iter=20, random_state=4).fit_transform(P)
    assert np.array_equal(est_a, est_b)


# ---- 3. the row-slab calls ---------------------------------------------------------------------------------------------------
M_ROWS, K, ROW0 = 50, 5, 5


def slab_case(n):
    r = np.random.default_rng(40 + n)
    W = r.uniform(0.1, 0.9, (K, M_ROWS))
    W /= W.sum(0)
    H = r.uniform(0.1, 0.9, (K, n))
    X = bernoulli((M_ROWS, n), 0.3, 50 + n)
    M = bernoulli((M_ROWS, n), 0.8, 60 + n)
    return W, H, X, M


def same_tuple(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert (g is None and w is None) or np.array_equal(g, w, equal_nan=True), what


@pytest.mark.parametrize("panel_rows", [None, 16])
@pytest.mark.parametrize("n", [70, 64])
def test_row_slab_calls_context_level(hip, monkeypatch, n, panel_rows):
    if panel_rows is None:
        monkeypatch.delenv("NBMF_PREDICT_PANEL_ROWS", raising=False)
    else:
        monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", str(panel_rows))   # several panels; score_rows' first one is cut short by row0
    W, H, X, M = slab_case(n)
    nr = M_ROWS - ROW0
    x, mk = X[ROW0:], M[ROW0:]
    px, pm = PackedBits.from_dense(x), PackedBits.from_dense(mk)
    wx, wm = in_wider_array(px, 21), in_wider_array(pm, 22)
    t = np.random.default_rng(70 + n).random((nr, n)) < 0.1
    rows, cols = np.nonzero(t)
    indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=nr))))
    with hip.Context(M_ROWS, n, K) as ctx:
        ctx.set_factors(W, H)
        want = ctx.score_rows(x, mk, ROW0, nr, rows=True, cols=True)
        want_all = ctx.score_rows(x, None, ROW0, nr, rows=True, cols=True)
        for what, a, b in (("packed, packed", px, pm), ("packed, bytes", px, mk), ("bytes, packed", x, pm), ("wider", wx, wm)):
            same_tuple(ctx.score_rows(a, b, ROW0, nr, rows=True, cols=True), want, f"score_rows {what}")
        same_tuple(ctx.score_rows(px, None, ROW0, nr, rows=True, cols=True), want_all, "score_rows packed, no mask")
        same_tuple(ctx.score_rows(px, pm, ROW0, nr, rows=True, cols=False), want[:2] + (None, None), "score_rows rows only")
        assert want[1].sum() == mk.sum() and want_all[1].sum() == mk.size

        want = ctx.theta_hist(x, mk, ROW0, nr, bins=16)
        for what, a, b in (("packed, packed", px, pm), ("packed, bytes", px, mk), ("bytes, packed", x, pm), ("wider", wx, wm)):
            same_tuple(ctx.theta_hist(a, b, ROW0, nr, bins=16), want, f"theta_hist {what}")
        same_tuple(ctx.theta_hist(px, None, ROW0, nr, bins=16), ctx.theta_hist(x, None, ROW0, nr, bins=16), "theta_hist, no mask")
        assert want[0][1].sum() == (x & mk).sum() and want[0][0].sum() == (~x & mk).sum()

        want = ctx.top_n(5, ROW0, nr, exclude=x)
        same_tuple(ctx.top_n(5, ROW0, nr, exclude=px), want, "top_n packed exclude")
        same_tuple(ctx.top_n(5, ROW0, nr, exclude=wx), want, "top_n packed exclude, wider")
        assert not x[np.arange(nr)[:, None], want[0]].any()

        want = ctx.rank_of(indptr, cols, ROW0, nr, exclude=x)
        same_tuple(ctx.rank_of(indptr, cols, ROW0, nr, exclude=px), want, "rank_of packed exclude")
        same_tuple(ctx.rank_of(indptr, cols, ROW0, nr, exclude=wx), want, "rank_of packed exclude, wider")
        assert np.array_equal(want[4], n - x.sum(1))


def fitted(W, H):
    est = NBMF(n_components=K)
    est.W_, est.components_ = np.ascontiguousarray(W.T), H
    return est


def test_row_slab_calls_estimator_level(hip):
    W, H, X, M = slab_case(70)
    P, PM = PackedBits.from_dense(X), PackedBits.from_dense(M)
    held = bernoulli(X.shape, 0.1, 80) & ~X
    est = fitted(W, H)
    for axis in (0, 1):
        same_tuple(est.score_samples(P, mask=PM, axis=axis, return_counts=True),
                   est.score_samples(X, mask=M, axis=axis, return_counts=True), f"score_samples axis {axis}")
        same_tuple(est.score_samples(P, axis=axis, return_counts=True), est.score_samples(X, axis=axis, return_counts=True),
                   f"score_samples axis {axis}, no mask")
    same_tuple(est.theta_histogram(P, mask=PM, bins=16), est.theta_histogram(X, mask=M, bins=16), "theta_histogram")
    assert est.roc_auc(P, mask=PM) == est.roc_auc(X, mask=M)
    same_tuple(est.calibration_curve(P, mask=PM), est.calibration_curve(X, mask=M), "calibration_curve")
    same_tuple(est.top_n(5, exclude=P), est.top_n(5, exclude=X), "top_n")
    got, want = est.ranking_metrics(held, exclude=P), est.ranking_metrics(held, exclude=X)
    assert list(got) == list(want)
    same_tuple(tuple(got.values()), tuple(want.values()), "ranking_metrics")
    same_tuple(tuple(est.rank_of(held, exclude=P)), tuple(est.rank_of(held, exclude=X)), "rank_of")
    results = []
    for x, mk in ((X, M), (P, PM), (P, M), (X, PM)):
        np.random.seed(5)
        s = est.score(x, mask=mk)
        np.random.seed(5)
        results.append((s, est.perplexity(x, mask=mk), est.transform(x, mask=mk)))
    for s, p, w in results[1:]:
        assert s == results[0][0] and p == results[0][1] and np.array_equal(w, results[0][2])


def test_block_streaming_of_packed_input(hip, monkeypatch):
    """Packed data beside a float mask, and a packed exclude, go to the device in row blocks: at least three here."""
    W, H, X, M = slab_case(70)
    P = PackedBits.from_dense(X)
    fmask = M.astype(np.float64)                                   # not a byte mask: the call streams 16-row blocks
    est = fitted(W, H)
    one_call = [est.score_samples(X, mask=M, axis=axis, return_counts=True) for axis in (0, 1)]
    calls = []
    real = hip.Context.score_rows
    monkeypatch.setattr(hip.Context, "score_rows", lambda self, x, *a, **k: calls.append(type(x)) or real(self, x, *a, **k))
    monkeypatch.setattr(_solver, "SCORE_SAMPLES_BLOCK_BYTES", 8 * 70 * 16)
    for axis in (0, 1):
        del calls[:]
        got = est.score_samples(P, mask=fmask, axis=axis, return_counts=True)
        assert calls == [PackedBits] * 4                           # 50 rows in blocks of 16
        same_tuple(got, est.score_samples(X, mask=fmask, axis=axis, return_counts=True), f"same-blocked byte call, axis {axis}")
        if axis == 0:
            same_tuple(got, one_call[0], "row results do not depend on the blocks")
        else:
            assert np.array_equal(got[1], one_call[1][1])         # (the counts are integers; the sums agree to rounding only)
    same_tuple(est.theta_histogram(P, mask=fmask, bins=16), est.theta_histogram(X, mask=M, bins=16), "theta_histogram in blocks")

    held = bernoulli(X.shape, 0.1, 81) & ~X
    want_top, want_rank = est.top_n(5, exclude=X), tuple(est.rank_of(held, exclude=X))
    calls = []
    real_top, real_rank = hip.Context.top_n, hip.Context.rank_of
    monkeypatch.setattr(hip.Context, "top_n", lambda self, *a, **k: calls.append(type(k["exclude"])) or real_top(self, *a, **k))
    monkeypatch.setattr(hip.Context, "rank_of", lambda self, *a, **k: calls.append(type(k["exclude"])) or real_rank(self, *a, **k))
    monkeypatch.setattr(_solver, "TOP_N_EXCLUDE_BLOCK_BYTES", 9 * 16)     # 16 packed rows of ceil(70 / 8) bytes
    same_tuple(est.top_n(5, exclude=P), want_top, "top_n in blocks")
    assert calls == [PackedBits] * 4
    del calls[:]
    same_tuple(tuple(est.rank_of(held, exclude=P)), want_rank, "rank_of in blocks")
    assert calls == [PackedBits] * 4


# ---- 4. the held-out curve of a fit from packed input ------------------------------------------------------------------------
def test_eval_curve_of_a_packed_fit(hip):
    X, M, _ = fit_operands()
    E = ~M & bernoulli(X.shape, 0.5, 90)
    ref = fit_outcome(X, M, "beta-dir", eval_mask=E, eval_every=5)
    got = fit_outcome(PackedBits.from_dense(X), PackedBits.from_dense(M), "beta-dir", eval_mask=E, eval_every=5)
    same_fit(got, ref, "fit with an eval set")
    assert np.array_equal(got.eval_iters_, ref.eval_iters_) and np.array_equal(got.eval_loglik_, ref.eval_loglik_)
    assert got.best_iter_ == ref.best_iter_ and len(ref.eval_iters_) >= 2 and ref.eval_iters_[0] == 5


# ---- 5. errors: argument checks that return before any launch ----------------------------------------------------------------
def test_argument_errors_leave_the_context_usable(hip):
    n = 70
    W, H, X, M = slab_case(n)
    P, PM = PackedBits.from_dense(X), PackedBits.from_dense(M)
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    ERR = hip.NBMF_ERR_ARG
    BITS, U8 = hip.DATA_BITS, hip.DATA_U8
    out = [np.zeros(M_ROWS), np.zeros(M_ROWS, dtype=np.int64), np.zeros(2 * 16, dtype=np.int64), np.zeros((M_ROWS, 5), dtype=np.int64)]
    short = b"ldx 8 is less than ceil(n / 8) = 9"
    with hip.Context(M_ROWS, n, K) as ctx:
        ctx.set_factors(W, H)
        h = ctx._h
        assert lib.nbmf_upload_v(h, ptr(P.bits), BITS, 8, 0, None, 0, 0, None) == ERR and lib.nbmf_last_error() == short
        assert lib.nbmf_upload_v(h, ptr(P.bits), BITS, 9, 0, ptr(PM.bits), hip.MASK_BITS, 8, None) == ERR
        assert lib.nbmf_last_error() == b"ldmask 8 is less than ceil(n / 8) = 9"
        assert lib.nbmf_upload_v(h, ptr(P.bits), 7, 9, 0, None, 0, 0, None) == ERR and b"x_kind" in lib.nbmf_last_error()
        assert lib.nbmf_upload_v(h, ptr(P.bits), BITS, 9, 0, None, hip.MASK_BITS, 9, None) == ERR
        assert lib.nbmf_last_error() == b"mask_kind set but mask is NULL"

        score = lambda xk, ldx, mp, mkind, ldm: lib.nbmf_score_rows_v(h, 0, M_ROWS, 1, 1e-8, ptr(P.bits), xk, ldx, mp, mkind, ldm,   # noqa: E731
                                                                     ptr(out[0]), ptr(out[1]), None, None)
        assert score(BITS, 8, None, 0, 0) == ERR and lib.nbmf_last_error() == short
        assert score(7, 9, None, 0, 0) == ERR and lib.nbmf_last_error() == b"unknown x_kind 7"
        assert score(BITS, 9, ptr(PM.bits), 7, 9) == ERR and lib.nbmf_last_error() == b"unknown mask_kind 7"
        assert score(BITS, 9, None, hip.MASK_BITS, 9) == ERR and lib.nbmf_last_error() == b"mask_kind set but mask is NULL"
        assert score(BITS, 9, ptr(PM.bits), hip.MASK_BITS, 8) == ERR
        assert lib.nbmf_last_error() == b"ldmask 8 is less than ceil(n / 8) = 9"

        hist = lambda xk, ldx, mp, mkind, ldm: lib.nbmf_theta_hist_v(h, 0, M_ROWS, 16, ptr(P.bits), xk, ldx, mp, mkind, ldm,   # noqa: E731
                                                                    ptr(out[2]), None)
        assert hist(BITS, 8, None, 0, 0) == ERR and lib.nbmf_last_error() == short
        assert hist(hip.DATA_F64, 70, None, 0, 0) == ERR and lib.nbmf_last_error() == b"unknown x_kind 0"
        assert hist(BITS, 9, None, hip.MASK_BITS, 9) == ERR and lib.nbmf_last_error() == b"mask_kind set but mask is NULL"

        top = lambda kind, ldx: lib.nbmf_top_n_v(h, 0, M_ROWS, 5, 1, ptr(P.bits), kind, ldx, ptr(out[3]), None, 5)   # noqa: E731
        assert top(BITS, 8) == ERR and lib.nbmf_last_error() == short
        assert top(7, 9) == ERR and lib.nbmf_last_error() == b"unknown exclude_kind 7"
        indptr = np.zeros(M_ROWS + 1, dtype=np.int64)
        rank = lambda kind, ldx: lib.nbmf_rank_rows_v(h, 0, M_ROWS, 1, ptr(indptr), None, ptr(P.bits), kind, ldx, None, None,   # noqa: E731
                                                      None, None, ptr(out[1]))
        assert rank(BITS, 8) == ERR and lib.nbmf_last_error() == short
        assert rank(7, 9) == ERR and lib.nbmf_last_error() == b"unknown exclude_kind 7"
        with pytest.raises(ValueError, match=r"x must have shape \(50, 70\)"):
            ctx.score_rows(P[1:], None)

        # the old entry points say what they said, and the context works
        assert lib.nbmf_top_n(h, 0, M_ROWS, 5, 1, ptr(X.view(np.uint8)), 69, ptr(out[3]), None, 5) == ERR
        assert lib.nbmf_last_error() == b"ldx 69 is less than n = 70"
        theta = ctx.predict_rows(0, M_ROWS)
        assert theta.shape == (M_ROWS, n) and np.allclose(theta, np.clip(W.T @ H, 0, 1), rtol=0, atol=1e-12)
        same_tuple(ctx.top_n(5, exclude=P), ctx.top_n(5, exclude=X), "after the errors")
