"""ROC AUC and calibration from the two class histograms of Theta (``Context.theta_hist``, ``NBMF.theta_histogram``): pure
NumPy on ``2 * bins`` integers, no device.  ``hist`` is int64 of shape ``(2, bins)``: ``hist[0, b]`` the observed zeros and
``hist[1, b]`` the observed ones whose Theta lies in bin b, ``[b / bins, (b + 1) / bins)`` (the last bin closed at 1).
And the ranking metrics of held-out entries from their positions in ``top_n``'s order (``Context.rank_of``,
``NBMF.rank_of``): pure NumPy on a few integers per entry (:class:`Ranks`, :func:`ranking_from_ranks`)."""
from collections import namedtuple

import numpy as np

from ._hip import MOMENT_FIELDS, MOMENT_FRAC_BITS, group_labels


def _hist(hist):
    hist = np.asarray(hist)
    if hist.ndim != 2 or hist.shape[0] != 2 or hist.shape[1] < 1 or not np.issubdtype(hist.dtype, np.integer):
        raise ValueError(f"hist must be an integer array of shape (2, bins) (got {hist.dtype} {hist.shape})")
    if hist.size and hist.min() < 0:
        raise ValueError("hist has negative counts")
    return hist.astype(np.int64, copy=False)


def auc_from_hist(hist):
    """``(auc, slack)``: the ROC AUC of the BINNED scores, ties counted one half, and a bound on its distance from the
    AUC of the unbinned scores.  With ``c0[b]`` the zeros in the bins below b and n0, n1 the class totals,

        auc   = sum_b hist[1][b] (c0[b] + hist[0][b] / 2) / (n0 n1)
        slack = sum_b hist[0][b] hist[1][b] / (2 n0 n1)

    A (zero, one) pair in two different bins is ordered by the bins exactly as by the scores themselves; a pair that
    shares a bin contributes 1/2 here and 0, 1/2 or 1 to the exact AUC: ``|auc - exact AUC| <= slack``.  The sums are
    formed in Python integers (exact whatever the counts) and divided once.  ``(nan, nan)`` where a class is empty."""
    h0, h1 = ([int(v) for v in row] for row in _hist(hist))
    n0, n1 = sum(h0), sum(h1)
    if n0 == 0 or n1 == 0:
        return float("nan"), float("nan")
    below = twice_auc = shared = 0
    for a, b in zip(h0, h1):
        twice_auc += b * (2 * below + a)
        shared += a * b
        below += a
    return twice_auc / (2 * n0 * n1), shared / (2 * n0 * n1)


def calibration_from_hist(hist, n_bins):
    """``(prob_true, prob_pred, counts)`` of a calibration curve over ``n_bins`` equal-width bins of [0, 1], from a
    histogram of ``bins = r * n_bins`` fine bins (``bins % n_bins`` must be 0).  DEFINITION: coarse bin q is the union of
    the fine bins ``q r .. q r + r - 1`` (coarse = fine ``// r``), so it holds the Thetas in ``[q / n_bins, (q + 1) /
    n_bins)`` by the very edge rule of the histogram, the last one closed at 1.

        counts[q]    = the observed entries in coarse bin q (int64)
        prob_true[q] = the ones among them / counts[q]
        prob_pred[q] = the count-weighted mean of the fine-bin centres (b + 1/2) / bins

    ``counts`` and ``prob_true`` are exact; ``prob_pred`` is within ``1 / (2 bins)`` of the bin's true mean Theta (every
    Theta is within half a fine bin of its centre).  NaN where a coarse bin is empty."""
    hist = _hist(hist)
    bins = hist.shape[1]
    if isinstance(n_bins, (bool, np.bool_)) or not isinstance(n_bins, (int, np.integer)) or n_bins < 1:
        raise ValueError(f"n_bins must be a positive integer (got {n_bins!r})")
    n_bins = int(n_bins)
    if bins % n_bins:
        raise ValueError(f"the histogram's {bins} bins are no multiple of n_bins = {n_bins}")
    r = bins // n_bins
    both = (hist[0] + hist[1]).reshape(n_bins, r)
    counts = both.sum(axis=1)
    ones = hist[1].reshape(n_bins, r).sum(axis=1)
    prob_true = np.full(n_bins, np.nan)
    prob_pred = np.full(n_bins, np.nan)
    for q in np.flatnonzero(counts):
        prob_true[q] = int(ones[q]) / int(counts[q])
        # sum_b both[b] (2 b + 1) is an exact integer; one division by 2 bins counts[q]
        odd = sum(int(c) * (2 * (q * r + j) + 1) for j, c in enumerate(both[q]))
        prob_pred[q] = odd / (2 * bins * int(counts[q]))
    return prob_true, prob_pred, counts


#: What ``NBMF.rank_of`` returns.  ``rows`` / ``cols`` are the targets in CSR order (row ascending); ``rank``, ``score``,
#: ``above`` and ``tied`` belong to them one to one (``Context.rank_of``); ``eligible`` is per row of the request.
Ranks = namedtuple("Ranks", ["rows", "cols", "rank", "score", "above", "tied", "eligible"])


def _mean(values):
    return float(np.mean(values)) if len(values) else float("nan")


def ranking_from_ranks(ranks, k=10):
    """The ranking metrics of the targets in ``ranks`` (:class:`Ranks`) -- the held-out ones of each row -- as a dict.
    ``P_i`` is the number of eligible targets of row i (``rank >= 0``: neither excluded nor NaN), ``E_i = eligible[i]``;
    rows with ``P_i = 0`` enter no mean.

        rows_scored           the rows with P_i > 0
        hit_rate@k            the share of them with a target at rank < k
        recall@k              mean of #{rank < k} / P_i
        precision@k           mean of #{rank < k} / k
        ndcg@k                mean of sum_{rank < k} 1 / log2(rank + 2)  over  sum_{s < min(P_i, k)} 1 / log2(s + 2)
        mrr                   mean of 1 / (the row's smallest rank + 1)
        mean_percentile_rank  over ALL eligible targets, pooled: (above + tied / 2) / (E_i - 1), 0 where E_i = 1
        auc                   mean over the rows with 0 < P_i < E_i of the ROC AUC of the row's eligible columns, targets
                              against the rest, ties counted one half

    The ``@k`` metrics and ``mrr`` use ``rank``: the slot ``top_n`` would show the target in, ties broken towards the lower
    column.  ``mean_percentile_rank`` and ``auc`` use MID-RANKS: a tie counts one half, whatever the columns.  The AUC of a
    row is ``1 - sum_t (neg_above_t + neg_tied_t / 2) / (P_i (E_i - P_i))`` with ``neg_above_t`` / ``neg_tied_t`` the
    ``above`` / ``tied`` of target t less the row's own eligible targets above, respectively tied with, t, which are found
    here from the targets' ``score`` compared numerically; the sums are formed in integers and divided once.  ``k`` is any
    positive integer.  A mean over nothing is NaN.  A target listed twice in a row is an error (``ValueError``): every
    metric here counts entries, not mentions."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"k must be a positive integer (got {k!r})")
    k = int(k)
    per_target = (ranks.rows, ranks.cols, ranks.rank, ranks.above, ranks.tied)
    rows, cols, rank, above, tied = (np.asarray(a, dtype=np.int64) for a in per_target)
    score = np.asarray(ranks.score, dtype=np.float64)
    E = np.asarray(ranks.eligible, dtype=np.int64)
    if len({a.shape for a in (rows, cols, rank, above, tied, score)}) != 1 or rows.ndim != 1 or E.ndim != 1:
        raise ValueError("the per-target arrays of ranks must be 1-D and equally long, eligible 1-D")
    m = E.size
    if rows.size and (rows.min() < 0 or rows.max() >= m or np.any(rows[1:] < rows[:-1])):
        raise ValueError("ranks.rows must ascend inside [0, len(eligible))")
    order = np.lexsort((cols, rows))
    if np.any((rows[order][1:] == rows[order][:-1]) & (cols[order][1:] == cols[order][:-1])):
        raise ValueError("a target is listed twice in a row")
    ok = rank >= 0
    r, rk, ab, td, sc = rows[ok], rank[ok], above[ok], tied[ok], score[ok]
    P = np.bincount(r, minlength=m)
    scored = P > 0
    out = {"rows_scored": int(scored.sum())}
    top = rk < k
    hits = np.bincount(r[top], minlength=m)
    out[f"hit_rate@{k}"] = _mean(hits[scored] > 0)
    out[f"recall@{k}"] = _mean(hits[scored] / P[scored])
    out[f"precision@{k}"] = _mean(hits[scored] / k)
    dcg = np.zeros(m)
    np.add.at(dcg, r[top], 1.0 / np.log2(rk[top] + 2.0))
    ideal = np.concatenate(([0.0], np.cumsum(1.0 / np.log2(np.arange(min(k, int(P.max()) if m else 0)) + 2.0))))
    out[f"ndcg@{k}"] = _mean(dcg[scored] / ideal[np.minimum(P[scored], k)])
    best = np.full(m, np.iinfo(np.int64).max)
    np.minimum.at(best, r, rk)
    out["mrr"] = _mean(1.0 / (best[scored] + 1.0))
    Et = E[r]
    out["mean_percentile_rank"] = _mean(np.where(Et > 1, (ab + td / 2.0) / np.maximum(Et - 1, 1), 0.0))
    # the row's own targets above / tied with each target: sort them by (row, score) and read the runs of equal scores
    by = np.lexsort((sc, r))
    rs, ss = r[by], sc[by]
    new_run = np.ones(rs.size, dtype=bool)
    new_run[1:] = (rs[1:] != rs[:-1]) | (ss[1:] != ss[:-1])
    run = np.cumsum(new_run) - 1
    start = np.flatnonzero(new_run)
    length = np.diff(np.append(start, rs.size))
    row_end = np.cumsum(P)[rs]                       # one past the row's last target in the sorted order
    own_above = row_end - (start + length)[run]
    own_tied = length[run] - 1
    twice = np.zeros(m, dtype=np.int64)              # 2 neg_above + neg_tied, summed per row: exact
    np.add.at(twice, rs, 2 * (ab[by] - own_above) + (td[by] - own_tied))
    both = scored & (P < E)
    pairs = (P[both] * (E[both] - P[both])).astype(np.float64)
    out["auc"] = _mean(1.0 - twice[both] / (2.0 * pairs))
    return out


# ---- expected counts: the five integer sums of a slot and what follows from them -----------------------------
def _exact_float(a):
    """An integer array -- int64, or Python ints where a sum has outgrown int64 -- as float64, each entry rounded once."""
    return np.asarray(a).astype(np.float64)


class Moments(namedtuple("Moments", MOMENT_FIELDS)):
    """The five integer sums of ``Context.moments`` / ``NBMF.expected_counts`` over the observed entries of each slot (a
    sample, a feature, a sample group x feature group cell), as read-only arrays of one shape, and what follows from them.
    With ``Q = 2**32`` and Theta the model's clipped probability of an entry:

        n_obs    the observed entries of the slot                 s1       sum of rint(Theta * Q)
        n_ones   the ones among them                              s2       sum of rint((Theta * Theta) * Q)
                                                                  s1_ones  s1 over the ones alone

    The arrays are int64; after :meth:`grouped` a field some sum of which has outgrown int64 is an object array of Python
    ints instead -- the sums stay exact either way, and the float64 properties below are computed from the exact sums,
    every integer difference taken before the one division:

        expected    s1 / Q                     the number of ones the model expects among the slot's observed entries
        variance    (s1 - s2) / Q              its variance: the sum of Theta (1 - Theta)
        z           (n_ones - expected) / sqrt(variance)        NaN where variance <= 0 or n_obs == 0
        mean_theta  expected / n_obs           NaN where nothing is observed
        brier       (n_ones Q - 2 s1_ones + s2) / (Q n_obs)     the mean of (x - Theta)**2; NaN where nothing is observed
        tjur        s1_ones / (Q n_ones) - (s1 - s1_ones) / (Q (n_obs - n_ones))    Tjur's coefficient of discrimination:
                    the mean Theta of the ones less that of the zeros; NaN where a class is empty

    ``expected`` is within ``n_obs * 2**-33`` of the sum of the slot's Thetas (the rounding of one entry's term)."""
    __slots__ = ()
    Q = 1 << MOMENT_FRAC_BITS

    def __new__(cls, n_obs, n_ones, s1, s2, s1_ones):
        fields = []
        for name, a in zip(MOMENT_FIELDS, (n_obs, n_ones, s1, s2, s1_ones)):
            a = np.array(a)                                   # (a copy: the holder's arrays are its own, and read-only)
            if a.dtype != object:
                if not np.issubdtype(a.dtype, np.integer):
                    raise ValueError(f"{name} must be an integer array (got dtype {a.dtype})")
                a = a.astype(object) if a.dtype == np.uint64 and a.size and int(a.max()) >= 1 << 63 else a.astype(np.int64)
            if a.shape != np.shape(fields[0] if fields else a):
                raise ValueError(f"{name} has shape {a.shape}, n_obs has {fields[0].shape}")
            a.setflags(write=False)
            fields.append(a)
        return super().__new__(cls, *fields)

    @classmethod
    def from_table(cls, table):
        """From an integer table whose last axis is the five fields (``Context.moments``' ``row_tab`` / ``col_tab``)."""
        table = np.asarray(table)
        if table.ndim < 1 or table.shape[-1] != len(MOMENT_FIELDS):
            raise ValueError(f"the last axis of a moment table holds {len(MOMENT_FIELDS)} fields (got shape {table.shape})")
        return cls(*(table[..., f] for f in range(len(MOMENT_FIELDS))))

    @property
    def shape(self):
        return self.n_obs.shape

    @property
    def expected(self):
        return _exact_float(self.s1) / self.Q

    @property
    def variance(self):
        return _exact_float(self.s1 - self.s2) / self.Q

    @property
    def z(self):
        var, seen = self.variance, _exact_float(self.n_obs) > 0
        ok = (var > 0) & seen
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(ok, (_exact_float(self.n_ones) - self.expected) / np.sqrt(np.where(ok, var, 1.0)), np.nan)

    @property
    def mean_theta(self):
        n = _exact_float(self.n_obs)
        return np.where(n > 0, self.expected / np.where(n > 0, n, 1.0), np.nan)

    @property
    def brier(self):
        n = _exact_float(self.n_obs)
        # n_ones Q - 2 s1_ones + s2 as ONE exact integer: in int64 where no term or partial sum can leave it (slots of at
        # most 2**29 ones and sums below 2**61: every table that came from the device ungrouped), else in Python ints
        ones, s1o, s2 = (np.asarray(a) for a in (self.n_ones, self.s1_ones, self.s2))
        small = all(a.dtype != object for a in (ones, s1o, s2)) and (
            ones.size == 0 or (int(ones.max()) < (1 << 29) and int(s1o.max()) < (1 << 61) and int(s2.max()) < (1 << 61)))
        if not small:
            ones, s1o, s2 = (a.astype(object) for a in (ones, s1o, s2))
        top = _exact_float(ones * self.Q - 2 * s1o + s2)
        return np.where(n > 0, top / (self.Q * np.where(n > 0, n, 1.0)), np.nan)

    @property
    def tjur(self):
        ones, zeros = _exact_float(self.n_ones), _exact_float(self.n_obs - self.n_ones)
        ok = (ones > 0) & (zeros > 0)
        of_ones = _exact_float(self.s1_ones) / (self.Q * np.where(ok, ones, 1.0))
        of_zeros = _exact_float(self.s1 - self.s1_ones) / (self.Q * np.where(ok, zeros, 1.0))
        return np.where(ok, of_ones - of_zeros, np.nan)

    def grouped(self, labels, n_groups=None):
        """The slots summed along the LEADING axis into groups: ``labels`` holds one integer per leading index, in
        ``[-1, n_groups)``, and -1 drops the slot (``n_groups`` defaults to ``max label + 1``); the result has ``n_groups``
        in place of the leading axis.  Exact whatever the sums reach: every field is split into its high and low 32 bits,
        the halves are summed as int64 (at most 2**31 slots of less than 2**32 each) and put together as Python ints; a
        field all of whose sums fit int64 comes back as int64, another as an object array of Python ints."""
        if not self.shape:
            raise ValueError("grouped needs a leading axis to sum over")
        labels, n_groups = group_labels(labels, self.shape[0], n_groups, name="labels")
        keep = labels >= 0
        out = []
        for a in self:
            if a.dtype == object:                             # (already beyond int64: Python ints all the way)
                total = np.zeros((n_groups,) + a.shape[1:], dtype=object)
                np.add.at(total, labels[keep], a[keep])
            else:
                hi, lo = np.zeros((2, n_groups) + a.shape[1:], dtype=np.int64)
                np.add.at(hi, labels[keep], a[keep] >> 32)
                np.add.at(lo, labels[keep], a[keep] & 0xffffffff)
                if hi.size == 0 or int(hi.max()) < (1 << 30):  # hi * 2**32 + lo < 2**63: int64 holds it
                    total = (hi << 32) + lo
                else:
                    total = hi.astype(object) * (1 << 32) + lo.astype(object)
            out.append(total)
        return Moments(*out)
