#!/usr/bin/env python3
"""Similar items end to end: planted data in which two groups of features are near-duplicates of one another (the same
column of the model with a little noise on it -- two spellings of one artist, two probes for one genus), a fit, and the
question "which features are most like this one?" answered on the device from the fitted factors alone.  The neighbours
of a feature of a group are the rest of its group; the feature itself is left out by index.  The same for samples: the
rows most similar to a row, for fitted rows and for rows embedded afterwards.  Needs an MI355X and the built library
(`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF

rng = np.random.default_rng(0)
k, samples, features, size = 6, 3000, 400, 5
W_true = rng.dirichlet(np.full(k, 0.3), samples)
H_true = rng.beta(0.4, 0.8, (k, features))
group_a, group_b = np.arange(10, 10 + size), np.arange(200, 200 + size)
for group in (group_a, group_b):                            # every member: the group's first column, slightly perturbed
    H_true[:, group[1:]] = np.clip(H_true[:, group[:1]] + rng.normal(0, 0.01, (k, size - 1)), 0.0, 1.0)
X = (rng.random((samples, features)) < W_true @ H_true).astype(np.float64)

model = NBMF(n_components=k, random_state=0, max_iter=500).fit(X)

for metric in ("cosine", "profile"):
    idx, scores = model.similar_features(size - 1, features=np.concatenate([group_a, group_b]), metric=metric)
    found = sum(len(set(row) & set(group)) for group, rows in ((group_a, idx[:size]), (group_b, idx[size:])) for row in rows)
    print(f"{metric:8s}: {found} of {2 * size * (size - 1)} neighbour slots of the two groups hold a member of the same group")
    print(f"          feature {group_a[0]}:", ", ".join(f"{j} ({s:.4f})" for j, s in zip(idx[0], scores[0])))
    assert found >= 0.8 * 2 * size * (size - 1), "the planted groups did not come back"

idx, scores = model.similar_samples(5, rows=[0, 1, 2])      # the fitted rows most like rows 0, 1, 2
print("samples most like sample 0:", ", ".join(f"{i} ({s:.4f})" for i, s in zip(idx[0], scores[0])))
main = W_true.argmax(1)                                     # the planted component a sample mostly belongs to
print("  share of them with sample 0's main planted component:", float(np.mean(main[idx[0]] == main[0])))

W_new = model.transform(X[:50])                             # rows embedded afterwards, compared among themselves
idx_new, _ = model.similar_samples(3, W=W_new, rows=[0])
print("among 50 re-embedded samples, most like the first:", idx_new[0].tolist())
