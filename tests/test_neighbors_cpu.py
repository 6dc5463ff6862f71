"""Similar items on the device (nbmf_similarity, nbmf_neighbors, Context.similarity / neighbors, NBMF.similar_features /
similar_samples): everything that can be said without a GPU -- the symbols are declared and exported, a null context is an
argument error, every malformed request raises ValueError BEFORE any device call -- and the reference ranking
``host_neighbors`` that tests/test_gpu_neighbors.py compares the device against, checked here on hand-written cases
(ties, duplicated vectors, NaN, top > L - 1, repeated queries)."""
import ctypes
import os

import numpy as np
import pytest


def host_neighbors(S, top, self_idx=None):
    """The reference ranking over a similarity slab ``S`` (queries x items): for every row the ``top`` eligible items --
    not NaN, and not ``self_idx[t]`` where ``self_idx`` is given (by INDEX: an item with the same score stays) -- by score
    descending, ties by ascending index (``np.lexsort((idx, -score))``), and their scores; rows with fewer eligible items
    end in -1 / NaN.  Returns ``(idx int64, scores float64)``, both ``(queries, top)``."""
    S = np.asarray(S, dtype=np.float64)
    nq, L = S.shape
    idx = np.full((nq, top), -1, dtype=np.int64)
    scores = np.full((nq, top), np.nan)
    for t in range(nq):
        ok = ~np.isnan(S[t])
        if self_idx is not None:
            ok[int(self_idx[t])] = False
        j = np.nonzero(ok)[0]
        order = j[np.lexsort((j, -S[t, j]))][:top]
        idx[t, :order.size] = order
        scores[t, :order.size] = S[t, order]
    return idx, scores


def same_ranking(got, want):
    """Indices equal, scores equal bit for bit, NaN padding compared by isnan: no tolerance."""
    (gc, gs), (wc, ws) = got, want
    assert gc.dtype == np.int64 and gs.dtype == np.float64 and gc.shape == wc.shape and gs.shape == ws.shape
    assert np.array_equal(gc, wc)
    pad = wc < 0
    assert np.all(np.isnan(gs[pad])) and np.all(np.isnan(ws[pad]))
    assert np.array_equal(gs[~pad].view(np.uint64), ws[~pad].view(np.uint64))


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_host_neighbors_ties_go_to_the_lower_index():
    S = np.array([[1.0, 0.5, 0.5, 0.9, 0.5],
                  [0.3, 0.3, 0.3, 0.3, 0.3]])
    idx, scores = host_neighbors(S, 3, [0, 1])
    assert idx.tolist() == [[3, 1, 2], [0, 2, 3]]                          # row 1 skips item 1, not the value 0.3
    assert scores.tolist() == [[0.9, 0.5, 0.5], [0.3, 0.3, 0.3]]
    idx, _ = host_neighbors(S, 3)                                          # without a self: the query leads its own row
    assert idx.tolist() == [[0, 3, 1], [0, 1, 2]]
    idx, _ = host_neighbors(np.array([[-0.0, 0.0, -1.0]]), 3)              # compared numerically: -0.0 ties with +0.0
    assert idx.tolist() == [[0, 1, 2]]


def test_host_neighbors_duplicated_vectors_stay_eligible():
    """Items 1, 3 and 4 carry one vector: each one's neighbours start with the other two at equal scores, by index."""
    F = np.array([[1.0, 0.0], [0.6, 0.8], [0.0, 1.0], [0.6, 0.8], [0.6, 0.8]])
    S = F @ F.T
    everyone = np.arange(5)
    idx, scores = host_neighbors(S, 2, everyone)
    assert idx[1].tolist() == [3, 4] and idx[3].tolist() == [1, 4] and idx[4].tolist() == [1, 3]
    assert scores[3, 0] == scores[3, 1] == S[3, 3]
    idx, _ = host_neighbors(S, 3)
    assert idx[3].tolist() == [1, 3, 4]                                    # with itself: plain index order among equals


def test_host_neighbors_skips_nan_and_pads_short_rows():
    nan = np.nan
    S = np.array([[1.0, nan, 0.7, 0.6],
                  [nan, nan, nan, nan],
                  [0.1, 0.2, 0.3, 0.4]])
    idx, scores = host_neighbors(S, 5, [0, 1, 3])
    assert idx.tolist() == [[2, 3, -1, -1, -1], [-1] * 5, [2, 1, 0, -1, -1]]   # top > L - 1: at most L - 1 real slots
    assert np.array_equal(np.isnan(scores), idx < 0)
    idx, _ = host_neighbors(S, 4)
    assert idx[2].tolist() == [3, 2, 1, 0]


def test_host_neighbors_repeated_queries_give_repeated_rows():
    g = np.random.default_rng(3)
    F = g.random((9, 4))
    S = F @ F.T
    query = np.array([4, 0, 4, 8, 0])
    got = host_neighbors(S[query], 3, query)
    full = host_neighbors(S, 3, np.arange(9))
    same_ranking(got, tuple(a[query] for a in full))
    assert np.array_equal(got[0][0], got[0][2]) and not np.any(got[0] == query[:, None])


# ---- the C entry points, as far as a host without a GPU reaches them ----------------------------------------------------
def test_symbols_are_declared_and_exported():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    plain = {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}   # (tests/asan_null_calls.py: only these kinds)
    for name, nargs in (("nbmf_similarity", 7), ("nbmf_neighbors", 10)):
        assert name in _hip.SYMBOLS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert len(fn.argtypes) == nargs and set(fn.argtypes) <= plain
    assert lib.nbmf_abi_version() == 4                                      # a compatible addition
    assert (_hip.SIM_DOT, _hip.SIM_COSINE, _hip.SIM_PROFILE) == (0, 1, 2)
    assert _hip.SIM_METRICS == {"dot": 0, "cosine": 1, "profile": 2}
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbmf_hip.h")).read()
    for line in ("#define NBMF_SIM_DOT 0", "#define NBMF_SIM_COSINE 1", "#define NBMF_SIM_PROFILE 2", "int nbmf_similarity(",
                 "int nbmf_neighbors("):
        assert line in header


def test_null_context_is_an_argument_error():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    assert lib.nbmf_similarity(None, 1, 1, None, 0, None, 0) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    assert lib.nbmf_neighbors(None, 1, 1, None, 0, 1, 1, None, None, 1) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    idx = np.zeros((2, 3), dtype=np.int64)
    assert lib.nbmf_neighbors(None, 0, 0, None, 2, 3, 1, idx.ctypes.data_as(ctypes.c_void_p), None, 3) == _hip.NBMF_ERR_ARG
    assert not idx.any()


# ---- Context.similarity / neighbors: every argument error before any device call --------------------------------------------
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


@pytest.mark.parametrize("top", [0, -1, 257, 2.0, "3", None, True])
def test_context_refuses_a_bad_top(bare_context, top):
    with pytest.raises(ValueError, match="top must be"):
        bare_context.neighbors(top)


@pytest.mark.parametrize("axis", [2, -1, 0.0, "features", None, True])
def test_context_refuses_an_unknown_axis(bare_context, axis):
    with pytest.raises(ValueError, match="axis must be"):
        bare_context.neighbors(3, axis=axis)
    with pytest.raises(ValueError, match="axis must be"):
        bare_context.similarity(axis=axis)


@pytest.mark.parametrize("metric", ["euclid", "COSINE", 3, -1, None, 1.0, True])
def test_context_refuses_an_unknown_metric(bare_context, metric):
    with pytest.raises(ValueError, match="metric must be"):
        bare_context.neighbors(3, metric=metric)
    with pytest.raises(ValueError, match="metric must be"):
        bare_context.similarity(metric=metric)


def test_context_refuses_a_bad_query(bare_context):
    ctx = bare_context
    for axis, L in ((0, 12), (1, 9)):
        for call in (lambda q: ctx.neighbors(3, axis=axis, query=q), lambda q: ctx.similarity(axis=axis, query=q)):
            with pytest.raises(ValueError, match=r"position 1 is outside \[0, %d\)" % L):
                call([0, -1, L])                                           # the lowest offending position is named
            with pytest.raises(ValueError, match=r"position 2 is outside \[0, %d\)" % L):
                call([0, L - 1, L])
            with pytest.raises(ValueError, match="integer array"):
                call([0.0, 1.0])
            with pytest.raises(ValueError, match="integer array"):
                call(np.array([True, False]))
            with pytest.raises(ValueError, match="1-D"):
                call(np.zeros((2, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="skip_self"):
        ctx.neighbors(3, skip_self=1)


def test_context_refuses_an_out_that_is_too_small(bare_context):
    ctx = bare_context
    with pytest.raises(ValueError, match="shape"):
        ctx.similarity(axis=1, out=np.zeros((9, 8)))                       # a row shorter than the L = 9 items: ldout < L
    with pytest.raises(ValueError, match="shape"):
        ctx.similarity(axis=0, out=np.zeros((12, 9)))                      # axis 0 has L = 12
    with pytest.raises(ValueError, match="shape"):
        ctx.similarity(axis=1, query=[1, 2], out=np.zeros((9, 9)))         # the shape follows the query
    with pytest.raises(ValueError, match="dtype"):
        ctx.similarity(axis=1, out=np.zeros((9, 9), dtype=np.float32))
    with pytest.raises(ValueError, match="stride"):
        ctx.similarity(axis=1, out=np.zeros((9, 18))[:, ::2])
    with pytest.raises(ValueError, match="NumPy array"):
        ctx.similarity(axis=1, out=[[0.0] * 9] * 9)


def test_item_query_passes_a_well_formed_list_through():
    from nbmf_mm_amd import _hip
    q, nq = _hip.item_query(np.array([5, 0, 5, 8], dtype=np.int32), 9)
    assert q.dtype == np.int64 and q.flags.c_contiguous and q.tolist() == [5, 0, 5, 8] and nq == 4
    assert _hip.item_query(None, 9) == (None, 9)
    assert _hip.item_query(np.zeros(0, dtype=np.int64), 9)[1] == 0
    assert _hip.sim_metric("profile") == 2 and _hip.sim_metric(np.int64(1)) == 1 and _hip.sim_axis(np.int32(0)) == 0


# ---- NBMF.similar_features / similar_samples ---------------------------------------------------------------------------------
def test_estimator_has_the_two_methods():
    from nbmf_mm_amd import NBMF
    assert callable(NBMF.similar_features) and callable(NBMF.similar_samples)


def test_not_fitted_is_transforms_error():
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError) as want:
        NBMF().transform(np.zeros((3, 4)))
    for call in (lambda: NBMF().similar_features(), lambda: NBMF().similar_samples()):
        with pytest.raises(ValueError) as got:
            call()
        assert str(got.value) == str(want.value)


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


def test_estimator_refuses_malformed_requests_before_any_device_call(hand_set):
    model = hand_set
    for call in (model.similar_features, model.similar_samples):
        for n in (0, -3, 257, 2.5, "5", None, False):
            with pytest.raises(ValueError, match="n must be"):
                call(n)
        for metric in ("euclid", 7, None):
            with pytest.raises(ValueError, match="metric must be"):
                call(3, metric=metric)
    with pytest.raises(ValueError, match=r"features index at position 0 is outside \[0, 9\)"):
        model.similar_features(3, features=[9])
    with pytest.raises(ValueError, match=r"features index at position 1 is outside \[0, 9\)"):
        model.similar_features(3, features=[8, -1])
    with pytest.raises(ValueError, match=r"rows index at position 0 is outside \[0, 12\)"):
        model.similar_samples(3, rows=[12])
    with pytest.raises(ValueError, match=r"rows index at position 0 is outside \[0, 4\)"):
        model.similar_samples(3, W=np.full((4, 3), 1 / 3), rows=[4])       # the rows follow W, not W_
    with pytest.raises(ValueError, match="integer array"):
        model.similar_features(3, features=[0.5])
    with pytest.raises(ValueError, match="components"):
        model.similar_samples(3, W=np.full((4, 2), 0.5))


def test_well_formed_request_reaches_the_device_or_fails_loudly():
    """No CPU fallback: without a GPU the call is an error of the library, with one it answers."""
    from nbmf_mm_amd import NBMF, _hip
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    if _hip.device_count() == 0:
        for call in (lambda: model.similar_features(3), lambda: model.similar_samples(3, rows=[0, 5], metric="profile")):
            with pytest.raises(_hip.NBMFHipError, match="no HIP device"):
                call()
    else:
        idx, scores = model.similar_features(3)
        assert idx.shape == (9, 3) and scores.shape == (9, 3)
        idx, scores = model.similar_samples(3, rows=[0, 5], metric="profile")
        assert idx.shape == (2, 3) and scores.shape == (2, 3)
