#!/usr/bin/env python3
"""A posterior-predictive check: fit a binary matrix, draw 20 replicates X_rep ~ Bernoulli(Theta) on the device
(``NBMF.sample``: one bit per entry comes back), and see whether the data's row and column sums look like the replicates'.
A model that fits puts most of the data's sums inside the replicates' spread.  Needs an MI355X and the built library
(`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF

rng = np.random.default_rng(0)
k, users, items, replicates = 5, 400, 300, 20
W_true = rng.dirichlet(np.full(k, 0.3), users)
H_true = rng.beta(0.3, 0.8, (k, items))
X = rng.random((users, items)) < W_true @ H_true

model = NBMF(n_components=k, random_state=0, max_iter=500).fit(X)
print(f"fit: {model.n_iter_} iterations, loss {model.loss_:.6f}")

row_sums = np.empty((replicates, users))
col_sums = np.empty((replicates, items))
for s in range(replicates):                                   # the seed names the replicate: any entry can be regenerated
    rep = model.sample(random_state=s)
    row_sums[s], col_sums[s] = rep.sum(1), rep.sum(0)

for name, data, reps in (("row", X.sum(1), row_sums), ("column", X.sum(0), col_sums)):
    lo, hi = reps.min(0), reps.max(0)
    inside = np.mean((data >= lo) & (data <= hi))
    z = (data - reps.mean(0)) / np.maximum(reps.std(0), 1e-12)
    print(f"{name} sums: {100 * inside:.1f} % of the data's lie inside the range of {replicates} replicates "
          f"(19 in 21 expected of an exact model); mean z {z.mean():+.2f}, rms z {np.sqrt(np.mean(z ** 2)):.2f}")
print(f"ones: data {X.mean():.4f}, replicates {row_sums.sum(1).mean() / X.size:.4f}")

# a parametric bootstrap step: refit one replicate, kept as bits all the way
boot = NBMF(n_components=k, random_state=0, max_iter=500).fit(model.sample(random_state=0, packed=True))
print(f"refit of replicate 0: loss {boot.loss_:.6f}")
