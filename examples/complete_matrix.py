#!/usr/bin/env python3
"""Matrix completion end to end: fit with a mask, fill the unobserved entries on the device, compare them with the truth
that was held out.  Needs an MI355X and the built library (`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF

rng = np.random.default_rng(0)
k, m, n = 5, 400, 300
W_true = rng.dirichlet(np.full(k, 0.3), m)                  # planted model: rows on the simplex, H near 0 or 1
H_true = rng.beta(0.3, 0.3, (k, n))
X = (rng.random((m, n)) < W_true @ H_true).astype(float)
mask = rng.random((m, n)) < 0.8                             # 20 % of the entries are held out

model = NBMF(n_components=k, random_state=0, max_iter=500).fit(X, mask=mask)

filled = model.impute(X, mask)                              # X where observed, Theta where not: only those entries are formed
held = ~mask
p = filled[held]
ll = np.mean(X[held] * np.log(p + 1e-8) + (1 - X[held]) * np.log(1 - p + 1e-8))
base = X[mask].mean()
ll0 = np.mean(X[held] * np.log(base) + (1 - X[held]) * np.log(1 - base))
print(f"{held.sum()} held-out entries: mean log-likelihood {ll:.4f} (predicting the observed mean {base:.3f} everywhere: {ll0:.4f})")
print(f"accuracy of filled > 0.5 on them: {np.mean((p > 0.5) == (X[held] > 0.5)):.3f}")

rows, cols = np.nonzero(held)
assert np.array_equal(p, model.predict_proba(rows=rows, cols=cols))    # the same entries, asked for by index
labels = model.predict(threshold=0.5)                       # the whole 0/1 matrix, thresholded on the device
print("predict:", labels.shape, labels.dtype, f"{labels.mean():.3f} ones ({X.mean():.3f} in the data)")
