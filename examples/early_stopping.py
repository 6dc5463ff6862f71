#!/usr/bin/env python3
"""Stop a fit where the held-out log-likelihood peaks.  An MM fit with a weak prior (alpha = beta = 1) overfits visibly: on
this planted 100 x 500 problem the held-out score rises for about twenty iterations and falls for good afterwards, while the
training loss keeps improving.  `fit(eval_mask=...)` keeps the held-out entries on the device as index pairs, sums their
log-likelihood there every `eval_every` iterations -- the factors never leave the device -- and with `patience` ends the
fit at the first run of that many evaluations without an improvement; `W_` / `components_` are the factors of the best
evaluation.  Needs an MI355X and the built library (`make -C nbmf_mm_amd/csrc`)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nbmf_mm_amd import NBMF

g = np.random.default_rng(0)
Wt = g.dirichlet(np.full(3, 0.3), 100)                      # three planted components
Ht = g.beta(0.5, 0.5, (3, 500))
X = (g.random((100, 500)) < Wt @ Ht).astype(np.float64)
u = g.random((100, 500))
train, held_out = u < 0.7, (u >= 0.7) & (u < 0.9)           # 70 % fitted, 20 % held out (10 % kept for a final test)

kw = dict(n_components=6, alpha=1.0, beta=1.0, random_state=0, tol=0, max_iter=120)

full = NBMF(**kw).fit(X, mask=train, eval_mask=held_out, eval_every=5)                 # patience = 0: the whole curve
print("iteration   mean held-out log-likelihood   perplexity")
for s, ll, pp in zip(full.eval_iters_, full.eval_loglik_, full.eval_perplexity_):
    print(f"{s:9d}   {ll:28.5f}   {pp:10.5f}{'   <- best' if s == full.best_iter_ else ''}")

early = NBMF(**kw).fit(X, mask=train, eval_mask=held_out, eval_every=5, patience=3)
print(f"patience = 3: stopped after {early.n_iter_} of {kw['max_iter']} iterations (stopped_early_ = {early.stopped_early_}), "
      f"factors restored from iteration {early.best_iter_}")
test = u >= 0.9
for name, model in (("run to max_iter", NBMF(**kw).fit(X, mask=train)), ("early stopping", early)):
    print(f"{name:>16}: training loss {model.loss_:.5f}, mean log-likelihood on the untouched 10 % "
          f"{np.nansum(model.score_samples(X, mask=test) * test.sum(1)) / test.sum():.5f}")
