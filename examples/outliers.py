#!/usr/bin/env python3
"""Which rows does the model explain badly?  Fit a planted users x items matrix in which a few users have been replaced by
noise, score every row on the device (`score_samples`: the mean log-likelihood per observed entry of a row under the fitted
model) and print the ten worst-explained rows -- the planted ones -- and the worst-calibrated features.  Only one number
per row (or per feature) crosses to the host, not a row of Theta.  Needs an MI355X and the built library
(`make -C nbmf_mm_amd/csrc`)."""
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
odd = np.sort(rng.choice(users, 10, replace=False))         # ten users who pick items at random, as often as the others do
X[odd] = rng.random((10, items)) < X.mean()
mask = rng.random((users, items)) < 0.9                     # a tenth of the entries is held out of the fit

model = NBMF(n_components=k, random_state=0, max_iter=300).fit(X, mask=mask)

scores, counts = model.score_samples(X, mask=mask, return_counts=True)      # (users,): mean log-likelihood per observed entry
worst = np.argsort(scores)[:10]
print(f"{users} users x {items} items, {int(counts.sum())} observed entries; mean score {scores.mean():.4f}")
print("the ten worst-explained rows:")
for i in worst:
    print(f"  row {i:5d}  score {scores[i]:.4f}  over {counts[i]} entries{'  (planted)' if i in odd else ''}")
print(f"{np.isin(worst, odd).sum()} of the 10 planted rows are among them")

held_out = model.score_samples(X, mask=~mask)               # the same rows judged on the entries the fit never saw
print(f"held-out mean score {held_out.mean():.4f}; worst held-out rows: {np.argsort(held_out)[:5].tolist()}")

by_item = model.score_samples(X, mask=mask, axis=1)         # (items,): which features the model explains badly
print("worst-explained features:", ", ".join(f"{j} ({by_item[j]:.3f})" for j in np.argsort(by_item)[:5]))
