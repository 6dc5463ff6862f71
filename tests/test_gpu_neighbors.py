"""Similar items on the device (nbmf_similarity, nbmf_neighbors) on an MI355X.

Two references.  The RANKING is checked against ``host_neighbors`` (tests/test_neighbors_cpu.py) over the device's own slab,
``Context.similarity``: indices equal and scores equal bit for bit, no tolerance -- a neighbour's score IS the slab's entry.
The SLAB is checked against the float64 NumPy restatement of each metric on non-negative factors within the forward-error
bound of the ordered sums (no cancellation: every term is >= 0), which is derived, not measured:
  DOT, COSINE   8 K u, u = 2^-53: K products and K additions on one chain ((K + 1) u relative), and for COSINE two
                operands each off by the norm's own sum, a square root and a division ((K / 2 + 3) u each); COSINE scores
                are <= 1, DOT's bound is taken relative to sum |f f|.
  PROFILE       4 (len + 4 K) u with len the OTHER factor's length: the Gram sums run over len items, then G F, the
                diagonal and the product add K terms each; scores are <= 1.
One case has dyadic factors whose products are exact in any order: NumPy's ``F.T @ F`` is the truth bit for bit there,
independently of the device's own product."""
import ctypes

import numpy as np
import pytest

from test_neighbors_cpu import host_neighbors, same_ranking

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
METRICS = ("dot", "cosine", "profile")


@pytest.fixture(scope="module")
def hip():
    from nbmf_mm_amd import _hip
    assert _hip.device_count() >= 1, "no MI355X visible: the GPU tests must run on the GPU box"
    return _hip


_cases = {}


def case(k, m, n, seed=0):
    """(W k x m with columns on the simplex, H k x n in (0.1, 0.9)) of one shape, made once and shared (read-only)."""
    key = (k, m, n, seed)
    if key not in _cases:
        r = np.random.default_rng(3000 + 97 * seed + k)
        W = r.uniform(0.1, 0.9, (k, m))
        W /= W.sum(0)
        H = r.uniform(0.1, 0.9, (k, n))
        W.setflags(write=False)
        H.setflags(write=False)
        _cases[key] = (W, H)
    return _cases[key]


def context(hip, W, H):
    ctx = hip.Context(W.shape[1], H.shape[1], W.shape[0])
    ctx.set_factors(W, H)
    return ctx


def numpy_similarity(W, H, axis, metric, query=None):
    """The metric restated in float64 NumPy for the ``query`` items (default: all) against all items: ``(S, bound)`` with
    ``bound`` the absolute tolerance per entry."""
    F, C = (W, H) if axis == 0 else (H, W)
    K = F.shape[0]
    q = slice(None) if query is None else query
    if metric == "dot":
        return F.T[q] @ F, 8 * K * U * (np.abs(F).T[q] @ np.abs(F))
    if metric == "cosine":
        norm = np.sqrt((F * F).sum(0))
        Un = np.divide(F, norm, out=np.zeros_like(F), where=norm != 0)
        return Un.T[q] @ Un, 8 * K * U
    G = C @ C.T
    B = G @ F
    d = (F * B).sum(0)
    root = np.sqrt(d)
    P = np.divide(F, root, out=np.zeros_like(F), where=d != 0)
    Q = np.divide(B, root, out=np.zeros_like(B), where=d != 0)
    return P.T[q] @ Q, 4 * (C.shape[1] + 4 * K) * U


def well_formed(idx, scores, L, top, nq):
    assert idx.shape == (nq, top) and scores.shape == (nq, top)
    assert idx.dtype == np.int64 and scores.dtype == np.float64
    assert np.all((idx >= -1) & (idx < L)), "a pad item or a stray index was returned"
    pad = idx < 0
    assert np.array_equal(pad, np.isnan(scores))
    assert np.all(pad[:, 1:] >= pad[:, :-1]), "a real entry follows a pad"
    for row in idx:
        real = row[row >= 0]
        assert real.size == np.unique(real).size


_slabs = {}


def ragged_slabs(hip):
    """The full slabs of the ragged case (k = 5, m = 37, n = 300) for every axis and metric, from the device, made once."""
    if not _slabs:
        W, H = case(5, 37, 300)
        with context(hip, W, H) as ctx:
            for axis in (0, 1):
                for metric in METRICS:
                    S = ctx.similarity(axis=axis, metric=metric)
                    S.setflags(write=False)
                    _slabs[axis, metric] = S
    return _slabs


# ---- 1. the ranking is the slab's -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("metric", METRICS)
def test_ranking_is_the_slabs(hip, axis, metric):
    """k = 5, m = 37, n = 300: ragged everywhere; two 256-item chunks on the feature axis, the second ragged; top = 256 is
    more than the 36 other samples, so the sample axis pads."""
    W, H = case(5, 37, 300)
    L = (37, 300)[axis]
    S = ragged_slabs(hip)[axis, metric]
    assert S.shape == (L, L)
    with context(hip, W, H) as ctx:
        for top in (1, 7, 256):
            got = ctx.neighbors(top, axis=axis, metric=metric)
            well_formed(*got, L, top, L)
            assert not np.any(got[0] == np.arange(L)[:, None]), "a query was returned as its own neighbour"
            assert np.array_equal((got[0] >= 0).sum(1), np.full(L, min(top, L - 1)))
            same_ranking(got, host_neighbors(S, top, np.arange(L)))
            with_self = ctx.neighbors(top, axis=axis, metric=metric, skip_self=False)
            same_ranking(with_self, host_neighbors(S, top))
        only_idx, none = ctx.neighbors(7, axis=axis, metric=metric, return_scores=False)
        assert none is None and np.array_equal(only_idx, host_neighbors(S, 7, np.arange(L))[0])


# ---- 2. the slab is right --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("metric", METRICS)
def test_slab_against_numpy(hip, axis, metric):
    W, H = case(5, 37, 300)
    S = ragged_slabs(hip)[axis, metric]
    want, bound = numpy_similarity(W, H, axis, metric)
    err = np.abs(S - want)
    print(f"axis {axis} {metric}: max error / bound = {np.max(err / bound):.3f}")
    assert np.all(np.isfinite(S)) and np.all(err <= bound)
    if metric != "dot":
        assert np.all(S <= 1.0 + bound) and np.all(np.abs(np.diag(S) - 1.0) <= bound)


def test_dyadic_factors_against_numpy(hip):
    """Multiples of 2^-6 below 1, K = 8: every product is a multiple of 2^-12 and every partial sum stays below 8 -- exact in
    float64 in any order, with or without FMA -- so NumPy's ``F.T @ F`` is the truth, and it is full of ties."""
    r = np.random.default_rng(41)
    W = r.integers(0, 64, (8, 45)) / 64.0
    H = r.integers(0, 8, (8, 530)) / 64.0
    with context(hip, W, H) as ctx:
        for axis, F in ((0, W), (1, H)):
            truth = F.T @ F
            S = ctx.similarity(axis=axis, metric="dot")
            assert np.array_equal(S, truth)
            L = F.shape[1]
            for top in (10, 256):
                got = ctx.neighbors(top, axis=axis, metric="dot")
                well_formed(*got, L, top, L)
                same_ranking(got, host_neighbors(truth, top, np.arange(L)))


# ---- 3. symmetry -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_symmetry(hip, axis):
    slabs = ragged_slabs(hip)
    for metric in ("dot", "cosine"):                                       # the same operand on both sides, the same k order
        S = slabs[axis, metric]
        assert np.array_equal(S.view(np.uint64), S.T.view(np.uint64)), metric
    W, H = case(5, 37, 300)
    S = slabs[axis, "profile"]
    assert np.all(np.abs(S - S.T) <= numpy_similarity(W, H, axis, "profile")[1])


# ---- 4. self and duplicates --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_self_and_duplicates(hip, metric):
    W, H = case(5, 37, 300)
    H = H.copy()
    H[:, 40] = H[:, 3]
    H[:, 299] = H[:, 3]
    if metric == "dot":
        H[:, 3] = H[:, 40] = H[:, 299] = 0.9                                # the longest vector: its copies lead under DOT too
    with context(hip, W, H) as ctx:
        idx, scores = ctx.neighbors(3, axis=1, metric=metric, query=[40, 3])
        assert idx[0, :2].tolist() == [3, 299] and idx[1, :2].tolist() == [40, 299]
        assert scores[0, 0] == scores[0, 1] == scores[1, 0] == scores[1, 1]
        assert 40 not in idx[0] and 3 not in idx[1]
        idx, scores = ctx.neighbors(4, axis=1, metric=metric, query=[40], skip_self=False)
        assert idx[0, :3].tolist() == [3, 40, 299] and scores[0, 0] == scores[0, 1] == scores[0, 2]
        S = ctx.similarity(axis=1, metric=metric, query=[40, 3])
        same_ranking(ctx.neighbors(256, axis=1, metric=metric, query=[40, 3]), host_neighbors(S, 256, [40, 3]))


# ---- 5. zero vectors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_zero_vector(hip, axis):
    W, H = case(5, 37, 300)
    W, H = W.copy(), H.copy()
    L, z = ((37, 11), (300, 257))[axis]
    (W if axis == 0 else H)[:, z] = 0.0
    with context(hip, W, H) as ctx:
        for metric in ("cosine", "profile"):
            S = ctx.similarity(axis=axis, metric=metric)
            assert not np.any(np.isnan(S))
            assert np.all(S[z] == 0.0) and np.all(S[:, z] == 0.0)
            want, bound = numpy_similarity(W, H, axis, metric)
            assert np.all(np.abs(S - want) <= bound)
            idx, scores = ctx.neighbors(5, axis=axis, metric=metric, query=[z, 0])
            assert idx[0].tolist() == [j for j in range(6) if j != z][:5] and np.all(scores[0] == 0.0)   # all tied: by index
            assert z not in idx[1] and not np.any(np.isnan(scores))
            same_ranking(ctx.neighbors(256, axis=axis, metric=metric), host_neighbors(S, 256, np.arange(L)))


# ---- 6. query lists and panels ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1])
def test_query_lists_and_panels(hip, axis, monkeypatch):
    W, H = case(5, 37, 300)
    L = (37, 300)[axis]
    r = np.random.default_rng(8)
    query = np.concatenate([r.integers(0, L, 40), [L - 1, 0, 5, 5, L - 1]])   # 45: unordered, repeats, not a multiple of 16
    slabs = ragged_slabs(hip)
    with context(hip, W, H) as ctx:
        for metric in METRICS:
            S = slabs[axis, metric]
            full = ctx.neighbors(7, axis=axis, metric=metric)
            same_ranking(full, host_neighbors(S, 7, np.arange(L)))
            part = ctx.neighbors(7, axis=axis, metric=metric, query=query)
            same_ranking(part, tuple(a[query] for a in full))
            Sq = ctx.similarity(axis=axis, metric=metric, query=query)
            assert np.array_equal(Sq.view(np.uint64), S[query].view(np.uint64))
            same_ranking(ctx.neighbors(7, axis=axis, metric=metric, query=query), part)      # twice: the same bits
            first = ctx.neighbors(7, axis=axis, metric=metric, query=np.arange(20))          # a prefix, as a list
            same_ranking(first, tuple(a[:20] for a in full))
            for rows_per_panel in ("16", "7"):
                monkeypatch.setenv("NBMF_PREDICT_PANEL_ROWS", rows_per_panel)
                same_ranking(ctx.neighbors(7, axis=axis, metric=metric, query=query), part)
                same_ranking(ctx.neighbors(7, axis=axis, metric=metric), full)
                assert np.array_equal(ctx.similarity(axis=axis, metric=metric, query=query).view(np.uint64), Sq.view(np.uint64))
            monkeypatch.delenv("NBMF_PREDICT_PANEL_ROWS")
        assert ctx.neighbors(7, axis=axis, query=np.zeros(0, dtype=np.int64))[0].shape == (0, 7)
        assert ctx.similarity(axis=axis, query=np.zeros(0, dtype=np.int64)).shape == (0, L)
        wide = np.full((47, L + 3), -7.25)                                   # a slice of a wider array: nothing outside it
        ctx.similarity(axis=axis, metric="cosine", query=query, out=wide[1:46, :L])
        assert np.array_equal(wide[1:46, :L], slabs[axis, "cosine"][query])
        wide[1:46, :L] = -7.25
        assert np.all(wide == -7.25), "something outside the slab was written"


# ---- 7. sliced K, a row beyond 64 KiB -----------------------------------------------------------------------------------------
def test_sliced_k_and_a_row_larger_than_64_kib(hip):
    """k = 130 runs as two slices of 128 components (KP = 256, ragged K); a row of 8195 scores is 64 KiB + 24 B."""
    m, n = 16, 8192 + 3
    W, H = case(130, m, n)
    query = np.concatenate([np.arange(0, 8195, 480), [8194, 8192]])          # 20 queries, the last items among them
    assert query.size == 20
    with context(hip, W, H) as ctx:
        for metric in ("cosine", "profile"):
            S = ctx.similarity(axis=1, metric=metric, query=query)
            got = ctx.neighbors(10, axis=1, metric=metric, query=query)
            well_formed(*got, n, 10, 20)
            same_ranking(got, host_neighbors(S, 10, query))
            want, bound = numpy_similarity(W, H, 1, metric, query)
            assert np.all(np.abs(S - want) <= bound)


# ---- 8. estimator --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orientation", ["beta-dir", "dir-beta"])
def test_estimator(hip, orientation):
    from nbmf_mm_amd import NBMF
    from nbmf_mm_amd._solver import device_neighbors, device_similarity
    g = np.random.default_rng(11)
    X = (g.random((60, 80)) < 0.3).astype(np.float64)
    model = NBMF(4, random_state=0, max_iter=30, tol=0, orientation=orientation).fit(X)
    W, H = model.W_, model.components_
    assert W.shape == (60, 4) and H.shape == (4, 80)                        # user layout in both orientations
    for metric in METRICS:
        same_ranking(model.similar_features(5, metric=metric), device_neighbors(W, H, 5, axis=1, metric=metric))
        same_ranking(model.similar_samples(5, metric=metric), device_neighbors(W, H, 5, axis=0, metric=metric))
        S = device_similarity(W, H, axis=1, metric=metric)
        same_ranking(model.similar_features(5, metric=metric), host_neighbors(S, 5, np.arange(80)))
        want, bound = numpy_similarity(np.ascontiguousarray(W.T), H, 1, metric)
        assert np.all(np.abs(S - want) <= bound)
    idx, scores = model.similar_features()                                 # n = 10, cosine, every feature
    assert idx.shape == (80, 10) and scores.shape == (80, 10)
    feats = [7, 0, 7]
    same_ranking(model.similar_features(3, features=feats), tuple(a[feats, :3] for a in (idx, scores)))
    Wnew = model.transform(X[:7])                                          # unseen rows: neighbours among themselves
    got = model.similar_samples(3, W=Wnew, rows=[6, 2])
    same_ranking(got, device_neighbors(Wnew, H, 3, axis=0, query=np.array([6, 2])))
    assert got[0].shape == (2, 3) and np.all((got[0] >= 0) & (got[0] < 7)) and 6 not in got[0][0] and 2 not in got[0][1]


# ---- 9. C-level errors -----------------------------------------------------------------------------------------------------------
def test_c_level_errors_leave_the_context_usable(hip):
    m, n, top = 37, 53, 7
    W, H = case(4, m, n)
    lib = hip.load()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    idx = np.full((n, top), -5, dtype=np.int64)
    scores = np.full((n, top), -7.25)
    slab = np.full((n, n), -7.25)
    q_bad = np.array([0, 5, n, -1], dtype=np.int64)
    with hip.Context(m, n, 4) as ctx:
        assert lib.nbmf_neighbors(ctx._h, 1, 1, None, n, top, 1, ptr(idx), ptr(scores), top) == hip.NBMF_ERR_STATE
        assert b"no factors" in lib.nbmf_last_error()
        ctx.set_factors(W, H)
        want = ctx.neighbors(top)
        bad = [(2, 1, None, n, top, 1, ptr(idx), ptr(scores), top),          # axis
               (1, 3, None, n, top, 1, ptr(idx), ptr(scores), top),          # metric
               (1, 1, None, n, 0, 1, ptr(idx), ptr(scores), top),            # top < 1
               (1, 1, None, n, 257, 1, ptr(idx), ptr(scores), 257),          # top > NBMF_TOP_N_MAX
               (1, 1, None, n, top, 1, ptr(idx), ptr(scores), top - 1),      # ldout < top
               (1, 1, None, n + 1, top, 1, ptr(idx), ptr(scores), top),      # more than L items without a list
               (1, 1, None, -1, top, 1, ptr(idx), ptr(scores), top),
               (1, 1, ptr(q_bad), 4, top, 1, ptr(idx), ptr(scores), top),    # an index outside [0, L)
               (1, 1, None, n, top, 1, None, ptr(scores), top)]              # no out_idx
        for args in bad:
            assert lib.nbmf_neighbors(ctx._h, *args) == hip.NBMF_ERR_ARG, args
            assert np.all(idx == -5) and np.all(scores == -7.25)
            same_ranking(ctx.neighbors(top), want)                           # as usable as before
        assert lib.nbmf_neighbors(ctx._h, 1, 1, ptr(q_bad), 4, top, 1, ptr(idx), ptr(scores), top) == hip.NBMF_ERR_ARG
        assert b"position 2 is outside [0, 53)" in lib.nbmf_last_error()    # the lowest offending position
        assert lib.nbmf_similarity(ctx._h, 1, 1, None, n, ptr(slab), n - 1) == hip.NBMF_ERR_ARG   # ldout < L
        assert lib.nbmf_similarity(ctx._h, 1, 1, ptr(q_bad), 4, ptr(slab), n) == hip.NBMF_ERR_ARG
        assert np.all(slab == -7.25)
        assert lib.nbmf_neighbors(ctx._h, 1, 1, None, 0, top, 1, None, None, top) == hip.NBMF_OK   # nothing to do
        assert lib.nbmf_neighbors(ctx._h, 1, 1, None, n, top, 1, ptr(idx), None, top) == hip.NBMF_OK
        assert np.array_equal(idx, want[0]) and np.all(scores == -7.25)     # no scores asked for: none written
