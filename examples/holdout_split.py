#!/usr/bin/env python3
"""Hold out a validation split without building a mask: `fit(holdout=0.2)` draws the split on the device.  The planted
100 x 500 problem of `early_stopping.py` -- a weak prior (alpha = beta = 1) overfits it visibly -- fitted with 20 % of the
observed entries held out by a counter-based hash of `(holdout_seed, entry)`: they leave the fit, their log-likelihood is
summed on the device every `eval_every` iterations, and `patience` ends the fit where the curve peaks.  `mask` is the pool the
split draws from, so the caller's own 10 % test set is never touched; `holdout_mask` names the held-out entries afterwards.
Then `cross_validate`: five folds on ONE upload of X -- each fold is drawn, fitted, evaluated and put back on the device --
to choose the number of components.  Needs an MI355X and the built library (`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF, holdout_mask
from nbmf_mm_amd.experiments import cross_validate

g = np.random.default_rng(0)
Wt = g.dirichlet(np.full(3, 0.3), 100)                      # three planted components
Ht = g.beta(0.5, 0.5, (3, 500))
X = (g.random((100, 500)) < Wt @ Ht).astype(np.float64)
test = g.random((100, 500)) >= 0.9                          # the caller's own test set: 10 %, never fitted, never held out
pool = ~test

kw = dict(n_components=6, alpha=1.0, beta=1.0, random_state=0, tol=0, max_iter=120)
model = NBMF(**kw).fit(X, mask=pool, holdout=0.2, eval_every=5, patience=3)
print(f"held out {model.holdout_count_} of {pool.sum()} observed entries (seed {model.holdout_seed_}, "
      f"uniform in [{model.holdout_interval_[0]}, {model.holdout_interval_[1]}))")
print("iteration   mean held-out log-likelihood   perplexity")
for s, ll, pp in zip(model.eval_iters_, model.eval_loglik_, model.eval_perplexity_):
    print(f"{s:9d}   {ll:28.5f}   {pp:10.5f}{'   <- best' if s == model.best_iter_ else ''}")
print(f"patience = 3: stopped after {model.n_iter_} of {kw['max_iter']} iterations (stopped_early_ = {model.stopped_early_}), "
      f"factors restored from iteration {model.best_iter_}")

held = holdout_mask(X.shape, model.holdout_seed_, model.holdout_interval_, mask=pool)    # the same entries, on the host
assert held.sum() == model.holdout_count_ and not (held & test).any()
for name, mk in (("held-out 20 %", held), ("untouched test set", test)):
    print(f"{name:>20}: mean log-likelihood {np.nansum(model.score_samples(X, mask=mk) * mk.sum(1)) / mk.sum():.5f}, "
          f"ROC AUC {model.roc_auc(X, mask=mk):.4f}")

print("\n5-fold cross-validation, one upload per K:")
for k in (3, 6):
    folds = cross_validate(X, k, n_folds=5, mask=pool, seed=1, alpha=1.0, beta=1.0, max_iter=120, tol=0, eval_every=5, patience=3,
                           random_state=0)
    assert sum(f["count"] for f in folds) == pool.sum()     # the folds partition the pool
    print(f"K = {k}: best held-out perplexity per fold " + " ".join(f"{f['best_perplexity']:.4f}" for f in folds)
          + f"   mean {np.mean([f['best_perplexity'] for f in folds]):.4f}, stopped at "
          + " ".join(str(f["n_iter"]) for f in folds))
