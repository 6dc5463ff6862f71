#!/usr/bin/env python3
"""Which recorded entries does the model believe least?  Flip a few entries of a planted block-structured matrix, fit, and
ask the device for the observed entries with the lowest probability under the fitted model (`least_likely`): the suspect
CELLS of a data set, where examples/outliers.py finds its suspect rows.  Only the listed entries cross to the host, not a
row of Theta.  Needs an MI355X and the built library (`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF

rng = np.random.default_rng(0)
k, animals, attributes = 4, 400, 600
group = rng.integers(0, k, animals)                          # planted model: four groups of animals ...
H_true = rng.random((k, attributes)) < 0.3                   # ... each with its own attributes
clean = H_true[group]                                        # the table as it should have been recorded
flips = 40
at = rng.choice(animals * attributes, flips, replace=False)
flipped = np.zeros(animals * attributes, dtype=bool)
flipped[at] = True
flipped = flipped.reshape(animals, attributes)
X = clean ^ flipped                                          # 40 entries recorded wrongly

model = NBMF(n_components=k, random_state=0, max_iter=500).fit(X)

N = 200
rows, cols, prob = model.least_likely(X, n=N)
found = flipped[rows, cols]
print(f"{animals} animals x {attributes} attributes, {flips} entries flipped; the {N} least likely recorded entries hold "
      f"{int(found.sum())} of them ({int(found[:flips].sum())} in the first {flips})")
for i, j, p, hit in list(zip(rows, cols, prob, found))[:10]:
    print(f"  animal {i:4d}  attribute {j:4d}  recorded {int(X[i, j])}  p(recorded) = {p:.4f}{'  (flipped)' if hit else ''}")

mask = rng.random(X.shape) < 0.9                             # judged on a subset only: unobserved entries are never listed
rows, cols, prob = model.least_likely(X, mask=mask, n=N)
assert mask[rows, cols].all()
print(f"under a 90 % mask: {int(flipped[rows, cols].sum())} of the {int((flipped & mask).sum())} observed flips are among the {N}")
