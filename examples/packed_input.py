#!/usr/bin/env python3
"""Bit-packed input end to end: a users x items matrix and its mask kept as bits on the host (``np.packbits`` layout, an
eighth of a bool array), fitted, scored and ranked without ever being unpacked there -- one bit per entry crosses to the
device, which unpacks it.  Every result is bit for bit that of the bool arrays.  Needs an MI355X and the built library
(`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF, PackedBits

rng = np.random.default_rng(0)
k, users, items = 6, 1500, 2000
W_true = rng.dirichlet(np.full(k, 0.2), users)
H_true = rng.beta(0.15, 0.6, (k, items))
full = rng.random((users, items)) < W_true @ H_true
observed = rng.random((users, items)) < 0.9                 # the fit sees 90 % of the entries

X = PackedBits.from_dense(full)                             # or PackedBits(np.packbits(A, axis=1), A.shape) of bits you hold
mask = PackedBits.from_dense(observed)
print(f"{users} x {items}: {full.nbytes} bytes as bool, {X.nbytes} bytes packed")

model = NBMF(n_components=k, random_state=0, max_iter=300).fit(X, mask=mask)
print(f"fit: {model.n_iter_} iterations, loss {model.loss_:.6f}")

held_out = PackedBits.from_dense(~observed)
per_user = model.score_samples(X, mask=held_out)            # mean held-out log-likelihood of every user, summed on the device
print(f"held-out log-likelihood per entry: mean over users {np.nanmean(per_user):.4f}, worst user {np.nanmin(per_user):.4f}")
print(f"held-out ROC AUC: {model.roc_auc(X, mask=held_out):.4f}")

cols, scores = model.top_n(10, exclude=X)                   # the ten most probable items a user does not have yet
assert not full[np.arange(users)[:, None], cols].any()
print("user 0:", ", ".join(f"item {j} ({s:.2f})" for j, s in zip(cols[0, :5], scores[0, :5])), "...")

same = NBMF(n_components=k, random_state=0, max_iter=300).fit(full, mask=observed)
assert np.array_equal(same.W_, model.W_) and np.array_equal(same.components_, model.components_)
assert np.array_equal(same.top_n(10, exclude=full)[0], cols)
print("the bool arrays give the same fit and the same ranking, bit for bit")
