#!/usr/bin/env python3
"""Where do the items a user really has, but the fit never saw, land in that user's recommendations?  Plant a users x items
model, hide 20 % of every user's items, fit on the rest, and rank the hidden ones among everything the user does not have
yet -- the order `top_n(exclude=X_train)` would show: recall@10, NDCG@10, MRR, the mean percentile rank and the mean
per-user AUC.  The positions are counted on the device (`rank_of`): a few integers per hidden item come back, no row of
Theta crosses to the host and nothing is sorted.  Needs an MI355X and the built library (`make -C nbmf_mm_amd/csrc`)."""
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
X_heldout = X & (rng.random((users, items)) < 0.2)          # 20 % of what a user has is hidden from the fit ...
X_train = X & ~X_heldout                                    # ... which sees those entries as zeros

model = NBMF(n_components=k, random_state=0, max_iter=300).fit(X_train)

print(f"{users} users x {items} items, {int(X_train.sum())} entries fitted, {int(X_heldout.sum())} hidden")
for name, value in model.ranking_metrics(X_heldout, exclude=X_train, k=10).items():
    print(f"  {name:22s} {value:.4f}" if isinstance(value, float) else f"  {name:22s} {value}")

# the same question for one user, entry by entry: rank 0 is the first recommendation top_n would make
ranks = model.rank_of(X_heldout, exclude=X_train)
user = int(np.argmax(np.bincount(ranks.rows, minlength=users)))
mine = ranks.rows == user
shown = model.top_n(10, exclude=X_train)[0][user]
print(f"user {user}: {int(mine.sum())} hidden items among {int(ranks.eligible[user])} it does not have yet")
for col, rank, score in sorted(zip(ranks.cols[mine], ranks.rank[mine], ranks.score[mine]), key=lambda t: t[1])[:8]:
    print(f"  item {col:5d}   rank {rank:5d}   predicted {score:.4f}{'   (in the top 10)' if col in shown else ''}")
