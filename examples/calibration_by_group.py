#!/usr/bin/env python3
"""Does the model reproduce the marginals on entries the fit never saw?  Plant a users x items model with user segments
and item categories, hold 20 % of the entries out, fit on the other 80 %, and compare how many held-out ones there are with
how many `predict_proba` expects -- per (segment, category) cell as a z-score table, and per item: the five most
over-predicted ones.  Every count is an exact integer sum formed on the device (`expected_counts`): no Theta crosses to the
host.  To make the check bite, the held-out entries of one category are thinned for one segment after the fact: that cell
should stand out as over-predicted.  Needs an MI355X and the built library (`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF

rng = np.random.default_rng(0)
k, users, items = 6, 1500, 2000
W_true = rng.dirichlet(np.full(k, 0.2), users)              # planted model: each user mostly in one taste group
H_true = rng.beta(0.15, 0.6, (k, items))                    # each group likes a few items a lot
X = rng.random((users, items)) < W_true @ H_true
train = rng.random((users, items)) < 0.8                    # 80 % of the entries are fitted ...
held_out = ~train                                           # ... and the rest is what the model is judged on

segment = W_true.argmax(1) % 4                              # four user segments, five item categories
category = rng.integers(0, 5, items)
drift = (segment[:, None] == 2) & (category[None, :] == 3) & held_out
X_seen = X & ~(drift & (rng.random((users, items)) < 0.3))  # segment 2 stopped liking category 3: 30 % of those held-out ones are gone

model = NBMF(n_components=k, random_state=0, max_iter=300).fit(X_seen, mask=train)

cells, by_item = model.expected_counts(X_seen, mask=held_out, feature_groups=category, sample_groups=segment)
print(f"{users} users x {items} items, {int(held_out.sum())} held-out entries, {int(cells.n_ones.sum())} of them ones, "
      f"{cells.expected.sum():.1f} expected")
print("held-out ones per (user segment, item category): observed / expected, z = (observed - expected) / sd")
print("  segment " + "".join(f"      category {c}      " for c in range(5)))
for s in range(4):
    print(f"  {s:7d} " + "".join(f" {int(cells.n_ones[s, c]):6d} /{cells.expected[s, c]:8.1f} {cells.z[s, c]:+5.1f}" for c in range(5)))
s, c = np.unravel_index(np.nanargmin(cells.z), cells.shape)   # (a cell without observed entries has no z: NaN)
print(f"most over-predicted cell: segment {s}, category {c} (z = {cells.z[s, c]:+.1f}; mean predicted "
      f"{cells.mean_theta[s, c]:.4f}, share of ones {cells.n_ones[s, c] / cells.n_obs[s, c]:.4f})")

print("the five most over-predicted items on the held-out entries:")
print("     item   category   held-out   ones   expected       z")
for j in np.argsort(np.where(np.isnan(by_item.z), np.inf, by_item.z))[:5]:
    print(f"  {j:7d}   {category[j]:8d}   {int(by_item.n_obs[j]):8d}   {int(by_item.n_ones[j]):4d}   {by_item.expected[j]:8.1f}   {by_item.z[j]:+5.1f}")
z = by_item.z[~np.isnan(by_item.z)]
overall = by_item.grouped(np.zeros(items, dtype=np.int64))  # all items as one slot: exact sums of the exact sums
print(f"root-mean-square z over the items {np.sqrt(np.mean(z ** 2)):.2f} (1 for a calibrated model); over all held-out "
      f"entries: Brier score {overall.brier[0]:.4f}, Tjur's coefficient of discrimination {overall.tjur[0]:.4f}")
