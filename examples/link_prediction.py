#!/usr/bin/env python3
"""Which missing links are the most probable?  Hide a tenth of the entries of a planted species x sites matrix from the
fit, then ask the device for the 500 most probable (species, site) pairs that are not recorded presences of the training
data (`top_pairs(exclude=...)`) and count how many of them are hidden presences.  This is ONE list over the whole matrix --
`top_n` gives a list per row -- and only the 500 pairs cross to the host, not a row of Theta.  Needs an MI355X and the built
library (`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF

rng = np.random.default_rng(0)
k, species, sites = 6, 1500, 2000
W_true = rng.dirichlet(np.full(k, 0.2), species)            # planted model: each species mostly in one habitat group
H_true = rng.beta(0.15, 0.6, (k, sites))                    # each group occupies a few sites densely
X = rng.random((species, sites)) < W_true @ H_true
mask = rng.random((species, sites)) < 0.9                   # a tenth of the entries is hidden from the fit
train = X & mask                                            # the presences the fit saw
hidden = X & ~mask                                          # the presences it did not

model = NBMF(n_components=k, random_state=0, max_iter=300).fit(X, mask=mask)

N = 500
rows, cols, prob = model.top_pairs(N, exclude=train | (mask & ~X))   # candidates: the entries the fit never saw
hits = hidden[rows, cols]
base = hidden.sum() / (~mask).sum()
print(f"{species} species x {sites} sites; {int(train.sum())} recorded presences, {int(hidden.sum())} hidden ones "
      f"among {int((~mask).sum())} unseen entries (base rate {base:.3f})")
print(f"the {N} most probable unseen links: probability {prob[0]:.3f} .. {prob[-1]:.3f}, "
      f"{int(hits.sum())} are hidden presences (precision {hits.mean():.3f}, {hits.mean() / base:.1f} x the base rate)")
for i, j, p, hit in list(zip(rows, cols, prob, hits))[:10]:
    print(f"  species {i:5d}  site {j:5d}  p = {p:.4f}{'  (a hidden presence)' if hit else ''}")

rows, cols, prob = model.top_pairs(N, exclude=train)         # the usual query: everything that is not a recorded presence
print(f"excluding only the recorded presences: {int(hidden[rows, cols].sum())} of the {N} pairs are hidden presences, "
      f"{int((mask & ~X)[rows, cols].sum())} are recorded absences the model doubts")
