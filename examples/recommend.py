#!/usr/bin/env python3
"""Recommendation end to end: fit a users x items matrix with some of each user's items hidden, rank the ten most
probable items per user on the device without the ones the user is known to have, and count how many of the hidden items
come back.  Only ten numbers per user cross to the host, not a row of Theta.  Needs an MI355X and the built library
(`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF

rng = np.random.default_rng(0)
k, users, items = 6, 1500, 2000                             # a lastfm-sized problem
W_true = rng.dirichlet(np.full(k, 0.2), users)              # planted model: each user mostly in one taste group
H_true = rng.beta(0.15, 0.6, (k, items))                    # each group likes a few items a lot
full = rng.random((users, items)) < W_true @ H_true
hidden = full & (rng.random((users, items)) < 0.2)          # a fifth of every user's items is held back
X = sp.csr_matrix((full & ~hidden).astype(np.float64))      # what the model sees

model = NBMF(n_components=k, random_state=0, max_iter=300).fit(X)

cols, scores = model.top_n(10, exclude=X)                   # (users, 10): items by probability, known items left out
assert not X[np.arange(users)[:, None], cols].toarray().any()
hits = hidden[np.arange(users)[:, None], cols]
chance = hidden.sum() / (users * items - X.nnz)
print(f"{users} users x {items} items, {X.nnz} known and {hidden.sum()} hidden entries")
print(f"precision@10 on the hidden items: {hits.mean():.3f} (picking unknown items at random: {chance:.3f})")
print("user 0:", ", ".join(f"item {j} ({s:.2f})" for j, s in zip(cols[0, :5], scores[0, :5])), "...")

new_users = model.transform(X[:3])                          # rows the model has not been fitted on work the same way
cols_new, _ = model.top_n(5, W=new_users, exclude=X[:3])
print("top 5 for three re-embedded users:", cols_new.tolist())
