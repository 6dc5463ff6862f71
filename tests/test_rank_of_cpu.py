"""Ranks of given entries on the device (nbmf_rank_rows, Context.rank_of, NBMF.rank_of / ranking_metrics): everything
that can be said without a GPU -- the reference ``host_rank_of`` that tests/test_gpu_rank_of.py compares the device
against, checked here on hand-written cases and against ``host_top_n``; ``_metrics.ranking_from_ranks`` against hand-computed
values and against sklearn's ``roc_auc_score``; the symbol is declared and exported, a null context is an argument error,
and every malformed request raises ValueError BEFORE any device call."""
import ctypes
import os

import numpy as np
import pytest

from test_top_n_cpu import host_top_n


def host_rank_of(theta, indptr, indices, exclude=None):
    """The reference: ``(rank, above, tied, score, eligible)`` of the targets ``indices[indptr[i]:indptr[i + 1]]`` of every
    row i of ``theta``, by plain NumPy comparisons of doubles over the eligible columns (not NaN, ``exclude`` zero or
    absent).  The per-target arrays are ``indptr[-1]`` long; positions below ``indptr[0]`` hold -1 / NaN."""
    theta = np.asarray(theta, dtype=np.float64)
    m, n = theta.shape
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    assert indptr.shape == (m + 1,)
    count = int(indptr[-1])
    rank, above, tied = (np.full(count, -1, dtype=np.int64) for _ in range(3))
    score = np.full(count, np.nan)
    eligible = np.zeros(m, dtype=np.int64)
    for i in range(m):
        ok = ~np.isnan(theta[i])
        if exclude is not None:
            ok &= np.asarray(exclude)[i] == 0
        eligible[i] = ok.sum()
        for p in range(int(indptr[i]), int(indptr[i + 1])):
            j = int(indices[p])
            score[p] = theta[i, j]
            if ok[j]:
                above[p] = np.sum(ok & (theta[i] > theta[i, j]))
                same = ok & (theta[i] == theta[i, j])
                tied[p] = same.sum() - 1
                rank[p] = above[p] + same[:j].sum()
    return rank, above, tied, score, eligible


def same_ranks(got, want):
    """The five arrays equal: integers exactly, scores bit for bit (NaN by isnan).  No tolerance."""
    assert len(got) == len(want) == 5
    for g, w, dtype in zip(got, want, (np.int64, np.int64, np.int64, np.float64, np.int64)):
        assert g.dtype == dtype and g.shape == w.shape
    for k in (0, 1, 2, 4):
        assert np.array_equal(got[k], want[k]), ("rank", "above", "tied", "score", "eligible")[k]
    nan = np.isnan(want[3])
    assert np.array_equal(np.isnan(got[3]), nan)
    assert np.array_equal(got[3][~nan].view(np.uint64), want[3][~nan].view(np.uint64))


def csr_of(lists):
    """``(indptr, indices)`` of a list of per-row target lists, kept in the order given."""
    indptr = np.concatenate(([0], np.cumsum([len(t) for t in lists]))).astype(np.int64)
    return indptr, np.array([j for t in lists for j in t], dtype=np.int32)


# ---- the reference itself -----------------------------------------------------------------------------------------------
def test_host_rank_of_by_hand():
    theta = np.array([[0.2, 0.9, 0.5, 0.9, 0.1],
                      [0.3, 0.3, 0.3, 0.3, 0.3],
                      [0.1, 0.2, 0.3, 0.4, 0.5]])
    indptr, indices = csr_of([[3, 0, 1, 3], [2], []])                     # unsorted, one repeat, an empty row
    rank, above, tied, score, eligible = host_rank_of(theta, indptr, indices)
    assert rank.tolist() == [1, 3, 0, 1, 2]
    assert above.tolist() == [0, 3, 0, 0, 0]
    assert tied.tolist() == [1, 0, 1, 1, 4]
    assert score.tolist() == [0.9, 0.2, 0.9, 0.9, 0.3]
    assert eligible.tolist() == [5, 5, 5]


def test_host_rank_of_compares_numerically():
    theta = np.array([[-0.0, 0.0, -1.0, np.inf, -np.inf, 5e-324, np.nan]])
    indptr, indices = csr_of([[0, 1, 2, 3, 4, 5, 6]])
    rank, above, tied, score, eligible = host_rank_of(theta, indptr, indices)
    assert rank.tolist() == [2, 3, 4, 0, 5, 1, -1]                        # -0.0 ties with +0.0: the lower column first
    assert above.tolist() == [2, 2, 4, 0, 5, 1, -1]
    assert tied.tolist() == [1, 1, 0, 0, 0, 0, -1]
    assert np.signbit(score[0]) and not np.signbit(score[1]) and np.isnan(score[6])
    assert eligible.tolist() == [6]


def test_host_rank_of_exclude_and_nan():
    nan = np.nan
    theta = np.array([[0.9, 0.8, 0.7, 0.6],
                      [0.9, 0.8, 0.7, 0.6],
                      [0.5, 0.5, 0.5, nan]])
    exclude = np.array([[1, 0, 0, 0],
                        [1, 1, 1, 1],
                        [0, 2, 0, 0]], dtype=np.uint8)                     # nonzero, not just 1, means skip
    indptr, indices = csr_of([[0, 3], [1], [2, 1, 3]])
    rank, above, tied, score, eligible = host_rank_of(theta, indptr, indices, exclude)
    assert rank.tolist() == [-1, 2, -1, 1, -1, -1]
    assert above.tolist() == [-1, 2, -1, 0, -1, -1]
    assert tied.tolist() == [-1, 0, -1, 1, -1, -1]
    assert score[:5].tolist() == [0.9, 0.6, 0.8, 0.5, 0.5] and np.isnan(score[5])   # an excluded target keeps its theta
    assert eligible.tolist() == [3, 0, 2]


def test_host_rank_of_leaves_the_positions_below_the_base():
    theta = np.array([[0.1, 0.9, 0.5]])
    rank, above, tied, score, eligible = host_rank_of(theta, np.array([2, 4]), np.array([7, 7, 2, 1]))
    assert rank.tolist() == [-1, -1, 1, 0] and above.tolist() == [-1, -1, 1, 0] and tied.tolist() == [-1, -1, 0, 0]
    assert np.isnan(score[:2]).all() and score[2:].tolist() == [0.5, 0.9]


def tie_heavy_case(m=23, n=300, seed=3):
    """Two-decimal thetas (ties everywhere), NaN, both zeros, an exclude matrix, and unsorted targets in most rows."""
    r = np.random.default_rng(seed)
    theta = np.round(r.random((m, n)), 2)
    theta[r.random((m, n)) < 0.02] = np.nan
    theta[r.random((m, n)) < 0.02] = -0.0
    theta[r.random((m, n)) < 0.02] = 0.0
    exclude = r.random((m, n)) < 0.2
    lists = [r.choice(n, size=int(c), replace=False).tolist() for c in r.integers(0, 40, m)]
    lists[5] = []
    return theta, exclude, lists


def test_rank_is_the_slot_of_host_top_n():
    theta, exclude, lists = tie_heavy_case()
    m, n = theta.shape
    indptr, indices = csr_of(lists)
    rank, above, tied, score, eligible = host_rank_of(theta, indptr, indices, exclude)
    cols, scores = host_top_n(theta, n, exclude)
    rows = np.repeat(np.arange(m), np.diff(indptr))
    assert (rank >= 0).sum() > 300 and (rank < 0).sum() > 50
    for i, j, rk, sc in zip(rows, indices, rank, score):
        if rk >= 0:
            assert cols[i, rk] == j and scores[i, rk].tobytes() == sc.tobytes()
        else:
            assert j not in cols[i]
    assert np.array_equal(eligible, (cols >= 0).sum(1))
    assert np.all(above[rank >= 0] <= rank[rank >= 0]) and np.all(rank[rank >= 0] <= (above + tied)[rank >= 0])


# ---- ranking_from_ranks ---------------------------------------------------------------------------------------------------
def ranks_of(theta, lists, exclude=None):
    from nbmf_mm_amd._metrics import Ranks
    indptr, indices = csr_of(lists)
    rank, above, tied, score, eligible = host_rank_of(theta, indptr, indices, exclude)
    rows = np.repeat(np.arange(theta.shape[0]), np.diff(indptr))
    return Ranks(rows, indices.astype(np.int64), rank, score, above, tied, eligible)


def test_metrics_by_hand():
    from nbmf_mm_amd._metrics import ranking_from_ranks
    theta = np.array([[0.9, 0.8, 0.7, 0.6, 0.5, 0.4],      # targets at ranks 0 and 3
                      [0.9, 0.8, 0.7, 0.6, 0.5, 0.4],      # one target at rank 4
                      [0.9, 0.8, 0.7, 0.6, 0.5, 0.4],      # no target: enters no mean
                      [0.5, 0.5, 0.5, 0.5, 0.9, 0.1]])     # a tie: target column 2 -> rank 3, above 1, tied 3
    got = ranking_from_ranks(ranks_of(theta, [[3, 0], [4], [], [2]]), k=2)
    assert got["rows_scored"] == 3
    assert got["hit_rate@2"] == pytest.approx(1 / 3, abs=1e-15)
    assert got["recall@2"] == pytest.approx((1 / 2 + 0 + 0) / 3, abs=1e-15)
    assert got["precision@2"] == pytest.approx((1 / 2 + 0 + 0) / 3, abs=1e-15)
    assert got["ndcg@2"] == pytest.approx((1.0 / (1.0 + 1.0 / np.log2(3.0)) + 0 + 0) / 3, abs=1e-15)
    assert got["mrr"] == pytest.approx((1 + 1 / 5 + 1 / 4) / 3, abs=1e-15)
    assert got["mean_percentile_rank"] == pytest.approx((0 / 5 + 3 / 5 + 4 / 5 + (1 + 3 / 2) / 5) / 4, abs=1e-15)
    # row 0: targets 0.9 and 0.6 against 4 others: 0.9 beats 4, 0.6 beats 2 -> 6 / 8; row 1: 1 / 5; row 3: (1 + 3 / 2) / 5
    assert got["auc"] == pytest.approx((6 / 8 + 1 / 5 + 2.5 / 5) / 3, abs=1e-15)
    deep = ranking_from_ranks(ranks_of(theta, [[3, 0], [4], [], [2]]), k=1000)       # k is not bounded by anything
    assert deep["recall@1000"] == 1.0 and deep["hit_rate@1000"] == 1.0
    assert deep["precision@1000"] == pytest.approx((2 + 1 + 1) / 3 / 1000, abs=1e-15)
    ideal2 = 1.0 + 1.0 / np.log2(3.0)
    assert deep["ndcg@1000"] == pytest.approx(((1 + 1 / np.log2(5)) / ideal2 + 1 / np.log2(6) + 1 / np.log2(5)) / 3, abs=1e-15)


def test_perfect_and_reversed_rankings():
    from nbmf_mm_amd._metrics import ranking_from_ranks
    theta = np.tile(np.linspace(0.9, 0.1, 9), (4, 1))
    best = ranking_from_ranks(ranks_of(theta, [[0]] * 4), k=3)
    assert best["mean_percentile_rank"] == 0.0 and best["auc"] == 1.0 and best["mrr"] == 1.0
    assert best["ndcg@3"] == 1.0 and best["recall@3"] == 1.0 and best["precision@3"] == pytest.approx(1 / 3, abs=1e-15)
    worst = ranking_from_ranks(ranks_of(theta, [[8]] * 4), k=3)
    assert worst["mean_percentile_rank"] == 1.0 and worst["auc"] == 0.0 and worst["mrr"] == pytest.approx(1 / 9, abs=1e-15)
    assert worst["ndcg@3"] == 0.0 and worst["recall@3"] == 0.0 and worst["hit_rate@3"] == 0.0
    top3 = ranking_from_ranks(ranks_of(theta, [[2, 0, 1]] * 4), k=3)
    assert top3["ndcg@3"] == 1.0 and top3["precision@3"] == 1.0 and top3["auc"] == 1.0


def test_rows_without_eligible_targets_are_left_out():
    from nbmf_mm_amd._metrics import ranking_from_ranks
    theta = np.tile(np.linspace(0.9, 0.1, 9), (3, 1))
    exclude = np.zeros((3, 9), dtype=bool)
    exclude[1, 4] = True                                                   # row 1's only target is excluded
    one = ranking_from_ranks(ranks_of(theta, [[0], [4], []], exclude), k=3)
    assert one["rows_scored"] == 1 and one["mrr"] == 1.0 and one["auc"] == 1.0 and one["mean_percentile_rank"] == 0.0
    none = ranking_from_ranks(ranks_of(theta, [[], [4], []], exclude), k=3)
    assert none["rows_scored"] == 0
    assert all(np.isnan(v) for key, v in none.items() if key != "rows_scored")
    exclude[0, 1:] = True                                                  # E = 1: percentile 0, and no negatives: no AUC
    alone = ranking_from_ranks(ranks_of(theta, [[0], [], []], exclude), k=3)
    assert alone["rows_scored"] == 1 and alone["mean_percentile_rank"] == 0.0 and np.isnan(alone["auc"])


def test_auc_against_sklearn_on_a_tie_heavy_case():
    from sklearn.metrics import roc_auc_score
    from nbmf_mm_amd._metrics import ranking_from_ranks
    theta, exclude, lists = tie_heavy_case()
    m, n = theta.shape
    aucs = []
    for i in range(m):
        one = ranks_of(theta[i:i + 1], [lists[i]], exclude[i:i + 1])
        got = ranking_from_ranks(one, k=5)
        ok = ~np.isnan(theta[i]) & ~exclude[i]
        y = np.zeros(n, dtype=int)
        y[lists[i]] = 1
        if 0 < y[ok].sum() < ok.sum():
            want = roc_auc_score(y[ok], theta[i][ok])
            assert abs(got["auc"] - want) <= 1e-12
            aucs.append(got["auc"])
        else:
            assert np.isnan(got["auc"])
    assert len(aucs) >= 20
    whole = ranking_from_ranks(ranks_of(theta, lists, exclude), k=5)
    assert abs(whole["auc"] - np.mean(aucs)) <= 1e-12


def test_ranking_from_ranks_refuses_bad_input():
    from nbmf_mm_amd._metrics import ranking_from_ranks
    theta = np.tile(np.linspace(0.9, 0.1, 9), (2, 1))
    with pytest.raises(ValueError, match="twice"):
        ranking_from_ranks(ranks_of(theta, [[3, 0, 3], [1]]))
    good = ranks_of(theta, [[3, 0], [1]])
    for k in (0, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="k must be"):
            ranking_from_ranks(good, k=k)
    with pytest.raises(ValueError, match="equally long"):
        ranking_from_ranks(good._replace(rank=good.rank[:2]))
    with pytest.raises(ValueError, match="ascend"):
        ranking_from_ranks(good._replace(rows=good.rows[::-1].copy()))


# ---- the C entry point, as far as a host without a GPU reaches it ---------------------------------------------------------
def test_symbol_is_declared_and_exported():
    from nbmf_mm_amd import _hip
    assert "nbmf_rank_rows" in _hip.SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "nbmf_rank_rows")
    # tests/asan_null_calls.py builds its null call from the argtypes: only these kinds
    plain = {ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double}
    assert len(lib.nbmf_rank_rows.argtypes) == 13 and set(lib.nbmf_rank_rows.argtypes) <= plain
    assert lib.nbmf_abi_version() == 4
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nbmf_hip.h")).read()
    assert "int nbmf_rank_rows(nbmf_ctx* ctx, int64_t row0, int64_t nrows, int clip_theta," in header


def test_null_context_is_an_argument_error():
    from nbmf_mm_amd import _hip
    lib = _hip.load()
    assert lib.nbmf_rank_rows(None, 0, 0, 0, None, None, None, 0, None, None, None, None, None) == _hip.NBMF_ERR_ARG
    assert b"null context" in lib.nbmf_last_error()
    indptr = np.array([0, 1, 2], dtype=np.int64)
    indices = np.array([0, 1], dtype=np.int32)
    rank = np.full(2, -5, dtype=np.int64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    rc = lib.nbmf_rank_rows(None, 0, 2, 1, ptr(indptr), ptr(indices), None, 0, ptr(rank), None, None, None, None)
    assert rc == _hip.NBMF_ERR_ARG and np.all(rank == -5)


# ---- csr_targets ----------------------------------------------------------------------------------------------------------------
def test_csr_targets_passes_good_input_through():
    from nbmf_mm_amd import _hip
    indptr, indices = _hip.csr_targets([0, 2, 2, 3], [4, 0, 8], 3, 9)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32 and indptr.flags.c_contiguous and indices.flags.c_contiguous
    assert indptr.tolist() == [0, 2, 2, 3] and indices.tolist() == [4, 0, 8]
    ip, ix = np.array([0, 2, 2, 3], dtype=np.int64), np.array([4, 0, 8], dtype=np.int32)
    a, b = _hip.csr_targets(ip, ix, 3, 9)
    assert np.shares_memory(a, ip) and np.shares_memory(b, ix)              # nothing is copied when the types fit
    # a slice of a larger CSR: the base is above 0, and what lies outside [indptr[0], indptr[-1]) is not looked at
    a, b = _hip.csr_targets(np.array([2, 3, 4]), np.array([99, -7, 1, 8, 1234]), 2, 9)
    assert a.tolist() == [2, 3, 4] and b[2:4].tolist() == [1, 8] and b.size == 5
    a, b = _hip.csr_targets(np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int64), 0, 9)
    assert a.tolist() == [0] and b.size == 0
    a, b = _hip.csr_targets(np.array([0, 0, 0], dtype=np.uint8), np.zeros(0, dtype=np.int16), 2, 9)
    assert a.dtype == np.int64 and b.dtype == np.int32


def test_csr_targets_refuses_malformed_input():
    from nbmf_mm_amd import _hip
    bad = [(([0.0, 1.0], [0], 1, 9), "indptr must be an integer"),
           (([0, 1], [0.0], 1, 9), "indices must be an integer"),
           (([0, 1], [True], 1, 9), "indices must be an integer"),
           (([[0, 1]], [0], 1, 9), "indptr must be 1-D"),
           (([0, 1], [[0]], 1, 9), "indices must be 1-D"),
           (([0, 1], [0], 2, 9), "nrows \\+ 1 = 3"),
           (([0, 1, 2], [0, 1], 1, 9), "nrows \\+ 1 = 2"),
           (([-1, 1], [0, 0], 1, 9), "negative"),
           (([0, 2, 1], [0, 0], 2, 9), "decreases at row 1"),
           (([0, 2], [0], 1, 9), "indices has 1 entries"),
           (([0, 3], [0, 9, 10], 1, 9), "column 9 at position 1"),
           (([0, 3], [0, 8, -1], 1, 9), "column -1 at position 2"),
           (([1, 3], [77, 8, 9], 1, 9), "column 9 at position 2"),
           (([0, 1], [2 ** 40], 1, 2 ** 41), "position 0")]                # a column int32 cannot carry
    for args, match in bad:
        with pytest.raises(ValueError, match=match):
            _hip.csr_targets(*args)


# ---- Context.rank_of: every argument error before any device call -----------------------------------------------------------
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
    ctx = bare_context
    indptr, indices = csr_of([[1, 2]] * 12)
    for row0, nrows in [(-1, 2), (12, 1), (11, 2), (0, -1), (0, 13)]:
        with pytest.raises(ValueError, match="rows"):
            ctx.rank_of(indptr, indices, row0, nrows)
    with pytest.raises(ValueError, match="nrows \\+ 1 = 5"):
        ctx.rank_of(indptr, indices, 2, 4)                                  # indptr follows the request: nrows + 1 entries
    with pytest.raises(ValueError, match="column 9 at position 3"):
        ctx.rank_of(indptr, np.where(np.arange(24) == 3, 9, indices))
    with pytest.raises(ValueError, match="column -2 at position 23"):
        ctx.rank_of(indptr, np.where(np.arange(24) == 23, -2, indices))
    with pytest.raises(ValueError, match="decreases"):
        ctx.rank_of(indptr[::-1].copy(), indices)
    with pytest.raises(ValueError, match="integer"):
        ctx.rank_of(indptr.astype(np.float64), indices)
    with pytest.raises(ValueError, match="shape"):
        ctx.rank_of(indptr, indices, exclude=np.zeros((12, 8), dtype=bool))
    with pytest.raises(ValueError, match="shape"):
        ctx.rank_of(indptr[2:7], indices, 2, 4, exclude=np.zeros((12, 9), dtype=bool))
    with pytest.raises(ValueError, match="dtype"):
        ctx.rank_of(indptr, indices, exclude=np.zeros((12, 9)))
    with pytest.raises(ValueError, match="stride"):
        ctx.rank_of(indptr, indices, exclude=np.zeros((9, 12), dtype=bool).T)


# ---- NBMF.rank_of / ranking_metrics ---------------------------------------------------------------------------------------------
def test_not_fitted_is_transforms_error():
    from nbmf_mm_amd import NBMF
    with pytest.raises(ValueError) as want:
        NBMF().transform(np.zeros((3, 4)))
    for call in (lambda: NBMF().rank_of(np.eye(3)), lambda: NBMF().ranking_metrics(np.eye(3))):
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
    import scipy.sparse as sp
    model = hand_set
    good = np.zeros((12, 9))
    good[:, 2] = 1
    for name, call in (("targets", lambda t, **k: model.rank_of(t, **k)),
                       ("targets", lambda t, **k: model.ranking_metrics(t, **k))):
        with pytest.raises(ValueError, match="targets"):
            call(None)
        for t in (np.zeros((12, 8)), np.zeros((9, 12)), np.zeros(9), sp.csr_matrix((12, 8))):
            with pytest.raises(ValueError, match="targets has shape"):
                call(t)
        with pytest.raises(ValueError, match="targets has shape"):
            call(good, W=np.full((4, 3), 1 / 3))                            # targets follow W, not W_
        with pytest.raises(ValueError, match="components"):
            call(good, W=np.full((4, 2), 0.5))
        for t in (np.full((12, 9), "a"), np.full((12, 9), None, dtype=object)):
            with pytest.raises(ValueError, match="targets must be a bool or numeric"):
                call(t)
        with pytest.raises(ValueError, match="exclude has shape"):
            call(good, exclude=np.zeros((12, 8)))
        with pytest.raises(ValueError, match="exclude has shape"):
            call(good, exclude=sp.csr_matrix((9, 12)))
        with pytest.raises(ValueError, match="exclude must be a bool or numeric"):
            call(good, exclude=np.full((12, 9), "a"))
    for k in (0, -3, 2.5, 10.0, "5", None, False):
        with pytest.raises(ValueError, match="k must be"):
            model.ranking_metrics(good, k=k)


def test_well_formed_request_reaches_the_device_or_fails_loudly():
    """No CPU fallback: without a GPU the call is an error of the library, with one it answers."""
    import scipy.sparse as sp
    from nbmf_mm_amd import NBMF, _hip
    r = np.random.default_rng(5)
    model = NBMF(n_components=3)
    model.W_ = r.dirichlet(np.ones(3), 12)
    model.components_ = r.uniform(0.1, 0.9, (3, 9))
    held = np.zeros((12, 9))
    held[np.arange(12), np.arange(12) % 9] = 1
    if _hip.device_count() == 0:
        for call in (lambda: model.rank_of(held), lambda: model.rank_of(sp.csr_matrix(held), exclude=np.zeros((12, 9))),
                     lambda: model.ranking_metrics(held, k=1000)):
            with pytest.raises(_hip.NBMFHipError, match="no HIP device"):
                call()
    else:
        ranks = model.rank_of(held)
        assert ranks.rows.tolist() == list(range(12)) and ranks.cols.tolist() == [i % 9 for i in range(12)]
        assert np.all((ranks.rank >= 0) & (ranks.rank < 9)) and np.all(ranks.eligible == 9)
        assert model.ranking_metrics(held, k=1000)["recall@1000"] == 1.0
