#!/usr/bin/env python3
"""How good are the predictions on entries the fit never saw?  Plant a users x items model, hold 20 % of the entries out,
fit on the other 80 %, and judge `predict_proba` on the held-out 20 %: the ROC AUC (does Theta rank the held-out ones above
the held-out zeros?) with the slack its binning leaves, and a ten-bin calibration table (is a predicted 0.3 a one 30 % of
the time?).  Both are functions of two integer histograms counted on the device (`theta_histogram`): no Theta crosses to the
host and nothing is sorted.  Needs an MI355X and the built library (`make -C nbmf_mm_amd/csrc`)."""
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

model = NBMF(n_components=k, random_state=0, max_iter=300).fit(X, mask=train)

auc, slack = model.roc_auc(X, mask=held_out, return_slack=True)
auc_train = model.roc_auc(X, mask=train)
print(f"{users} users x {items} items, {int(held_out.sum())} held-out entries, {int((X & held_out).sum())} of them ones")
print(f"held-out ROC AUC {auc:.4f} +- {slack:.4f} (1024 bins; on the fitted entries {auc_train:.4f})")

prob_true, prob_pred, counts = model.calibration_curve(X, mask=held_out, n_bins=10, resolution=100)
print("calibration on the held-out entries:")
print("  predicted in     entries   mean predicted   share of ones")
for q in range(10):
    if counts[q]:
        print(f"  [{q / 10:.1f}, {(q + 1) / 10:.1f}{']' if q == 9 else ')'}   {counts[q]:9d}   {prob_pred[q]:14.4f}   {prob_true[q]:13.4f}")
    else:
        print(f"  [{q / 10:.1f}, {(q + 1) / 10:.1f}{']' if q == 9 else ')'}   {0:9d}                -               -")
gap = np.nansum(counts * np.abs(prob_true - prob_pred)) / counts.sum()
print(f"expected calibration error {gap:.4f}")
