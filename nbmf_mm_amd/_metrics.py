"""ROC AUC and calibration from the two class histograms of Theta (``Context.theta_hist``, ``NBMF.theta_histogram``): pure
NumPy on ``2 * bins`` integers, no device.  ``hist`` is int64 of shape ``(2, bins)``: ``hist[0, b]`` the observed zeros and
``hist[1, b]`` the observed ones whose Theta lies in bin b, ``[b / bins, (b + 1) / bins)`` (the last bin closed at 1)."""
import numpy as np


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

