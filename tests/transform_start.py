"""transform()'s un-normalised start, W ~ U(0.1, 0.9), at every K layout and storage path (TEST INFRASTRUCTURE: no test in
this file).

``transform``, ``score`` and ``perplexity`` all begin with ``nbmf_w_only_steps`` from a W whose rows sum to about K / 2
(src/nbmf_mm/_base.py:175 of the reference), so on the first step Theta = W H is far above 1, the ratios
(1 - Y) / (1 - Theta + eps) are negative and the W sweep must take the variant with the reference's own selects (TINY,
chosen by ``w_free`` in ``w_pass_args``) in every instantiation: the K = 16 / 32 / 64 / 128 layouts, the sliced forms above
128 components, and the three storage paths.  This module holds the deterministic cases, the oracle's step in the dtype it
is given (float64, or ``np.longdouble`` for the conditioning gates) and the bounds; ``test_transform_start_cpu.py`` shows on
the CPU that the cases are where they claim to be and that the bounds bite, ``test_gpu_transform_start.py`` holds the kernels
to them.

What makes tight bounds possible (measured on the CPU, float64 against long double; the CPU test re-measures all of it):
  * binary data, 17 <= K <= 130, with or without a bool mask: after the FIRST step every row is positive and Theta < 1, and
    the 50-step loop is stable (end gap 3-5e-16), so the whole transform is held to 1e-9 on ALL rows and the score to 1e-10;
  * real-valued data, any K (and binary data at K = 6): W keeps negative entries for many steps and Theta reaches the
    hundreds, but ONE step from an identical state is well conditioned -- steps 0, 1, 2 are compared from the oracle's own
    state, against ``step_bound``.

Layouts as in tests/planted.py: X (m, n); W (m, k) in the user layout, (k, m) on the device; H (k, n).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import nbmf_oracle as orc

M, N, N_NO_PAD = 70, 150, 128         # the smallest shapes with a ragged tile and a pad in both dimensions; 128: no pad columns
EPS = 1e-8                            # the transform loop's, hard-coded in the reference (_base.py:190)
KS = (6, 17, 24, 40, 64, 100, 128, 130, 300)    # every layout, ragged and full; two and three slices of 128
FACTOR_ATOL = 1e-9                    # the project's factor tolerance, absolute
LOSS_RTOL = 1e-10                     # the project's loss / score tolerance, relative
ONES_SHARE, OBSERVED_SHARE = 0.3, 0.85
A_STEPS = 3                           # same-state steps compared per case (the gap reached 0.83 of the bound at a fourth)
LOOP_STEPS = 50                       # transform's own count (_base.py:180)

# data: "binary" (30 % ones) or "real" (uniform on [0, 1)); mask: None, "bool" (85 % observed) or "weights" (real, in
# (0.05, 1]); storage: what ``Context.set_storage`` is given before the upload
Config = namedtuple("Config", "id data mask storage binary_path")
CONFIGS = {c.id: c for c in (
    Config("binary", "binary", None, "auto", True),
    Config("binary-mask", "binary", "bool", "auto", True),
    Config("binary-mask-f64", "binary", "bool", "f64", False),
    Config("binary-f64w", "binary", None, "f64w", False),
    Config("real-mask", "real", "bool", "auto", False),
    Config("real-weights", "real", "weights", "auto", False),
)}
A_CASES = tuple((k, cid) for k in KS for cid in CONFIGS)
# What the step cases found (test_real_valued_observed_zeros_keep_their_sign_above_theta_1): the W sweep of the 8-byte path
# WITHOUT weight tiles dropped every negative ratio.  Its smallest cases, kept by name: K = 6, real-valued data with the bool
# mask folded in, and the same path with nothing to fold -- no mask at all, which the six configurations do not have.
EXTRA_CONFIGS = {"real": Config("real", "real", None, "auto", False)}
NAMED_CASES = ((6, "real-mask"), (6, "real"))
# Cases whose first draw (salt 0) missed a condition of test_transform_start_cpu.py and were drawn again -- the tolerance
# stays, the seed moves.  (6, binary), (24, real-mask), (100, real-weights): the float64 / long-double gap of one of their
# three steps stood at 0.10, 0.13 and 0.22 of the bound; (17, real-mask): every entry came out positive after the first step,
# so steps 1 and 2 would not have started off the simplex.
SEED_SALT = {(6, "binary"): 1, (17, "real-mask"): 1, (24, "real-mask"): 1, (100, "real-weights"): 1}

# the chained loop: binary data only, K >= 17
B_KS = (17, 40, 100, 130)
Loop = namedtuple("Loop", "id config n dead_row steps")
LOOPS = {c.id: c for c in (
    Loop("unmasked-n128", "binary", N_NO_PAD, None, LOOP_STEPS),
    Loop("unmasked-n150", "binary", N, None, LOOP_STEPS),
    Loop("mask", "binary-mask", N, None, LOOP_STEPS),
    Loop("mask-one-row-unobserved", "binary-mask", N, 37, LOOP_STEPS),
    Loop("f64", "binary-mask-f64", N, None, LOOP_STEPS),
    Loop("f64w", "binary-f64w", N, None, LOOP_STEPS),
    Loop("two-steps", "binary", N, None, 2),          # no range check after the first step: both steps in the select variant
)}
B_CASES = tuple((k, lid) for k in B_KS for lid in LOOPS)
UNMASKED_LOOPS = ("unmasked-n128", "unmasked-n150")

# the estimator: fit a few iterations, then transform / score / perplexity from the seeded global draw
C_KS = (24, 130)
C_FIT_ITERS, C_FIT_SEED, C_DRAW_SEED = 3, 11, 5
C_CASES = tuple((k, o, s) for k in C_KS for o in ("beta-dir", "dir-beta") for s in ("dense", "csr"))


def config(config_id):
    return CONFIGS[config_id] if config_id in CONFIGS else EXTRA_CONFIGS[config_id]


def _readonly(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def problem(k, config_id, n=N, dead_row=None):
    """``(X, mask, H, W0)``: X (M, n), mask (None, bool or float64 weights), H (k, n) ~ U(0.02, 0.98), W0 (M, k) ~
    U(0.1, 0.9) -- the reference's start, NOT on the simplex.  Seeded per case; read-only, shared."""
    c = config(config_id)
    index = sorted(CONFIGS).index(config_id) if config_id in CONFIGS else 100 + sorted(EXTRA_CONFIGS).index(config_id)
    r = np.random.default_rng([2024, k, n, index, SEED_SALT.get((k, config_id), 0)])
    X = (r.random((M, n)) < ONES_SHARE).astype(np.float64) if c.data == "binary" else r.random((M, n))
    u = r.random((M, n))
    mask = None
    if c.mask == "bool":
        mask = u < OBSERVED_SHARE
        if dead_row is not None:
            mask[dead_row] = False                    # a row observed nowhere: 0 / 0 in its renormalisation
    elif c.mask == "weights":
        mask = 0.05 + 0.95 * (1.0 - u)                # in (0.05, 1]
    H = r.uniform(0.02, 0.98, (k, n))
    W0 = r.uniform(0.1, 0.9, (M, k))
    return _readonly(X, mask, H, W0)


def as_float(mask, dtype=np.float64):
    return None if mask is None else np.asarray(mask).astype(dtype)


def w_step(X, H, mask, W, denominators="reference"):
    """One iteration of the transform loop (src/nbmf_mm/_base.py:180-193) from W (m, k), in the dtype it is given; no final
    clip.  ``denominators="plain"``: the ratios as the sweeps' PLAIN variant forms them, from |Theta - z| -- the
    reference's arithmetic only while 0 <= Theta < 1 (the sensitivity leg: what a dispatch to the wrong variant computes)."""
    Wt = W.T
    th = H.T @ Wt
    yt, zt = (X.T, (1 - X).T) if mask is None else (X.T * mask.T, (1 - X).T * mask.T)
    if denominators == "reference":
        d1, d2 = th + EPS, 1 - th + EPS
    else:
        assert denominators == "plain"
        d1, d2 = np.abs(th) + EPS, np.abs(1 - th) + EPS
    Wt = Wt * (H @ (yt / d1) + (1 - H) @ (zt / d2))
    Wt = Wt / X.shape[1]
    Wt = Wt / Wt.sum(axis=0, keepdims=True)
    return Wt.T


def step_bound(W_next):
    """Per row, for a step whose float64 result is ``W_next``: 1e-11 max(1, max |W_next| of the row)^2 -- a row whose column
    sum nearly cancels amplifies rounding by its magnitude (the bound of test_gpu_parity.py's step-by-step comparison)."""
    return 1e-11 * np.maximum(1.0, np.abs(W_next).max(axis=1, keepdims=True)) ** 2


@functools.lru_cache(maxsize=None)
def a_states(k, config_id):
    """The float64 oracle's states ``[W0, W1, W2, W3]`` of the case (each (M, k)): step j is compared from states[j] against
    states[j + 1].  Computed once, read-only."""
    X, mask, H, W0 = problem(k, config_id)
    maskf = as_float(mask)
    states = [W0]
    with np.errstate(all="ignore"):
        for _ in range(A_STEPS):
            states.append(w_step(X, H, maskf, states[-1]))
    return _readonly(*states)


def theta_max(k, config_id, j):
    _, _, H, _ = problem(k, config_id)
    return float((a_states(k, config_id)[j] @ H).max())


@functools.lru_cache(maxsize=None)
def loop_reference(k, loop_id):
    """``(W_end, positive_from_step_1)`` of the float64 oracle: ``steps`` iterations from W0, and whether every row (but a
    row observed nowhere, which is NaN) kept all entries positive with Theta < 1 from the first step on."""
    lp = LOOPS[loop_id]
    X, mask, H, W0 = problem(k, lp.config, lp.n, lp.dead_row)
    maskf = as_float(mask)
    live = np.ones(M, dtype=bool)
    if lp.dead_row is not None:
        live[lp.dead_row] = False
    W, ok = W0, True
    with np.errstate(all="ignore"):
        for _ in range(lp.steps):
            W = w_step(X, H, maskf, W)
            ok = ok and bool((W[live] > 0).all()) and bool((W[live] @ H).max() < 1.0)
    return _readonly(np.ascontiguousarray(W))[0], ok


def device_loop(hip, k, loop_id):
    """The loop case on the device (``hip``: the ``nbmf_mm_amd._hip`` module): one context, ``w_only_steps(steps)`` from W0.
    Returns ``(W (M, k), H, full_w_launches, ragged_k_launches)``, the launch counts being those of this call."""
    lp = LOOPS[loop_id]
    c = CONFIGS[lp.config]
    X, mask, H, W0 = problem(k, lp.config, lp.n, lp.dead_row)
    with hip.Context(M, lp.n, k) as ctx:
        ctx.set_hyper(1.2, 1.2, EPS)
        ctx.set_storage(c.storage)
        assert ctx.upload(X, mask=mask) == c.binary_path
        ctx.set_factors(np.ascontiguousarray(W0.T), H)
        before = hip.variant_stats()
        ctx.w_only_steps(lp.steps)
        full_w, ragged = (a - b for a, b in zip(hip.variant_stats()[:2], before[:2]))
        Wk, Hk = ctx.get_factors()
    return np.ascontiguousarray(Wk.T), Hk, full_w, ragged


def loop_extended(k, loop_id):
    """The same loop in ``np.longdouble`` (data, factors and start all long double)."""
    L = np.longdouble
    lp = LOOPS[loop_id]
    X, mask, H, W0 = problem(k, lp.config, lp.n, lp.dead_row)
    X, H, W, maskf = X.astype(L), H.astype(L), W0.astype(L), as_float(mask, L)
    with np.errstate(all="ignore"):
        for _ in range(lp.steps):
            W = w_step(X, H, maskf, W)
    assert W.dtype == L
    return W


@functools.lru_cache(maxsize=None)
def estimator_data(k):
    """``(X, mask)`` of the estimator cases: binary (M, N) and an 85 % bool mask."""
    X, mask, _, _ = problem(k, "binary-mask")
    return X, mask


def estimator_reference(X, H, mask, dtype=np.float64):
    """What ``transform(X)``, ``transform(X, mask)`` and ``score(X, mask)`` compute in the reference after
    ``np.random.seed(C_DRAW_SEED)`` (each call draws its own start, so each is seeded again): ``(W_plain, W_masked, score,
    positive_from_step_1)``; the score's inner transform runs WITHOUT the mask (_base.py:235).  In ``dtype``."""
    X, H, maskf = X.astype(dtype), H.astype(dtype), as_float(mask, dtype)
    np.random.seed(C_DRAW_SEED)
    W0 = np.random.uniform(0.1, 0.9, (X.shape[0], H.shape[0]))
    ok, W = True, W0.astype(dtype)
    for _ in range(LOOP_STEPS):
        W = w_step(X, H, None, W)
        ok = ok and bool((W > 0).all()) and bool((W @ H).max() < 1.0)
    W_plain = orc.w_only_transform(X, H, None, W0=W0.astype(dtype))
    W_masked = orc.w_only_transform(X, H, maskf, W0=W0.astype(dtype))
    Wm = W0.astype(dtype)
    for _ in range(LOOP_STEPS):
        Wm = w_step(X, H, maskf, Wm)
        ok = ok and bool((Wm > 0).all()) and bool((Wm @ H).max() < 1.0)
    return W_plain, W_masked, orc.score(X, W_plain, H, maskf), ok


@functools.lru_cache(maxsize=None)
def oracle_components(k, orientation):
    """``components_`` (k, N) of the float64 oracle's fit of the estimator data (C_FIT_ITERS iterations, masked): what the
    CPU gates stand on -- the device's own fit differs from it by rounding, and the GPU test hands the oracle the DEVICE's."""
    X, mask = estimator_data(k)
    _, H, _, _, _ = orc.solve(X, k, max_iter=C_FIT_ITERS, tol=0, mask=mask, random_state=C_FIT_SEED, orientation=orientation)
    return _readonly(np.ascontiguousarray(H))[0]
