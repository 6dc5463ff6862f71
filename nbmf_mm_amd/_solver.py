"""Host side of the solver: same signature and return value as the reference's
``nbmf_mm_solver`` (src/nbmf_mm/_solver.py:61-216), with the hot loop (:143-175) executed by
libnbmf_hip on an MI355X.  Seeding, init draws, the orientation transpose and the final
simplex touch-up stay on the host exactly as the reference orders them.
"""
from __future__ import annotations

import contextlib

import numpy as np

from . import _hip
from ._packed import PackedBits

_PROJECTIONS = {"normalize": _hip.PROJ_NORMALIZE, "duchi": _hip.PROJ_DUCHI}


def _projection_code(projection):
    if projection not in _PROJECTIONS:
        raise ValueError(f"Unknown projection: {projection}. Must be one of {list(_PROJECTIONS)}")
    return _PROJECTIONS[projection]


def _draw_init(m, k, n, W_init, H_init):
    """Init draws in the reference's order: W (m,k) first, then H (k,n); each only if absent
    (src/nbmf_mm/_solver.py:126-129)."""
    if W_init is None:
        W_init = np.random.uniform(0.1, 0.9, (m, k))
    if H_init is None:
        H_init = np.random.uniform(0.1, 0.9, (k, n))
    return W_init, H_init


def _binary_pattern(A):
    """``(indptr, indices)`` of a scipy sparse matrix whose stored values are all 1 (after summing duplicates
    and dropping explicit zeros), else None."""
    A = A.tocsr(copy=True)
    A.sum_duplicates()
    A.eliminate_zeros()
    if A.nnz and not np.all(A.data == 1):
        return None
    if A.shape[1] >= 2 ** 31:
        return None
    return A.indptr.astype(np.int64), A.indices.astype(np.int32)


def _dense(X):
    """Dense data as the library takes it: bool / uint8 arrays as they are (one byte per entry up to the device,
    ``nbmf_upload_v``), float32 as it is (four; the device's conversion is the exact one ``astype(float64)`` does),
    everything else as float64 (the reference converts every input, _base.py:83)."""
    X = np.asarray(X)
    return X if X.dtype in (np.bool_, np.uint8, np.float32) else np.asarray(X, dtype=np.float64)


def upload_any(ctx, X, mask=None, transposed=False):
    """Upload dense or scipy-sparse data: binary sparse patterns (with no mask or a sparse pattern mask) go up as
    CSR (``nbmf_upload_csr``); everything else is densified first, as the reference does (:28-29,106-107).  A
    :class:`PackedBits` X or mask goes up as bits, with a dense operand of any kind beside it; it does not go with a
    sparse one (``nbmf_upload_csr`` takes patterns only)."""
    if isinstance(X, PackedBits) or isinstance(mask, PackedBits):
        if any(hasattr(a, "toarray") and not isinstance(a, PackedBits) for a in (X, mask)):
            raise ValueError("PackedBits input does not go with scipy-sparse input: the CSR upload (nbmf_upload_csr) takes "
                             "patterns only (densify the sparse operand, or pack it)")
        return ctx.upload(X if isinstance(X, PackedBits) else _dense(X), mask=mask, transposed=transposed)
    if hasattr(X, "toarray"):
        csr = _binary_pattern(X)
        csr_mask = None
        if csr is not None and mask is not None:
            csr_mask = _binary_pattern(mask) if hasattr(mask, "toarray") else None
            if csr_mask is None:
                csr = None
        if csr is not None:
            return ctx.upload_csr(csr, csr_mask, transposed=transposed)
        X = X.toarray()
    if mask is not None and hasattr(mask, "toarray"):
        mask = mask.toarray()
    return ctx.upload(_dense(X), mask=mask, transposed=transposed)


def eval_pairs(Y, eval_mask, eval_every=10, patience=0, orientation="beta-dir", n_gpus=1, devices=None):
    """The held-out entries of a fit as ``Context.set_eval`` takes them, after every check of the eval arguments -- none
    needs a device: ``(rows, cols, x)`` in the internal layout (``orientation="dir-beta"`` swaps rows and columns), in
    row-major order of that layout, ``x`` the truth ``Y`` holds at them as uint8; or None without an ``eval_mask``.
    ``eval_mask`` is dense (bool or numeric) or scipy-sparse of Y's shape, its nonzeros the held-out entries.  Raises
    ``ValueError`` for a wrong shape, an empty eval set, a Y value at an eval entry that is not 0 or 1, ``eval_every < 1``,
    ``patience < 0``, ``patience > 0`` without an ``eval_mask``, and an eval set together with ``n_gpus > 1`` or
    ``devices``.  ``Y`` may be a :class:`PackedBits` (its truth is read with ``.at``); a packed ``eval_mask`` is not taken."""
    if isinstance(eval_mask, PackedBits):
        raise ValueError("eval_mask as PackedBits is not supported: pass it dense (bool) or scipy-sparse (X may be packed)")
    if eval_mask is not None:
        y_shape = tuple(Y.shape) if isinstance(Y, PackedBits) else tuple(np.shape(Y))
        E = eval_mask if hasattr(eval_mask, "toarray") else np.asarray(eval_mask)
        if E.dtype != np.bool_ and not np.issubdtype(E.dtype, np.number):
            raise ValueError(f"eval_mask must be a bool or numeric matrix (got dtype {E.dtype})")
        if E.ndim != 2 or tuple(E.shape) != y_shape:
            raise ValueError(f"eval_mask has shape {tuple(E.shape)}, X has {y_shape}")
        if hasattr(E, "toarray"):
            E = (E != 0).tocoo()
            r, c = E.row.astype(np.int64), E.col.astype(np.int64)
        else:
            r, c = np.nonzero(E)
        if r.size == 0:
            raise ValueError("eval_mask marks no entry: the eval set is empty")
        v = Y.at(r, c) if isinstance(Y, PackedBits) else np.asarray(Y[r, c]).ravel()
        if not np.all((v == 0) | (v == 1)):
            raise ValueError("X must be 0 or 1 at the entries eval_mask marks")
    if isinstance(eval_every, (bool, np.bool_)) or not isinstance(eval_every, (int, np.integer)) or eval_every < 1:
        raise ValueError(f"eval_every must be an integer >= 1 (got {eval_every!r})")
    if isinstance(patience, (bool, np.bool_)) or not isinstance(patience, (int, np.integer)) or patience < 0:
        raise ValueError(f"patience must be an integer >= 0 (got {patience!r})")
    if eval_mask is None:
        if patience > 0:
            raise ValueError("patience > 0 needs an eval_mask: early stopping watches the held-out log-likelihood")
        return None
    if int(n_gpus) != 1 or devices is not None:
        raise ValueError("an eval set is evaluated on one GPU: eval_mask does not go with n_gpus > 1 or devices")
    if orientation == "dir-beta":
        r, c = c, r
    order = np.lexsort((c, r))                         # row-major in the internal layout
    return (np.ascontiguousarray(r[order], dtype=np.int64), np.ascontiguousarray(c[order], dtype=np.int64),
            np.ascontiguousarray(v[order] != 0).view(np.uint8))


def holdout_args(holdout, holdout_seed=None, eval_mask=None, eval_every=10, patience=0, n_gpus=1, devices=None):
    """Every check of a fit's hold-out arguments -- none needs a device: ``((lo, hi), seed)`` with ``seed`` None where
    the fit is to choose it, or None without a ``holdout``.  Raises ``ValueError`` for a bad interval
    (``_hip.holdout_interval``), a ``holdout_seed`` that is no integer in ``[0, 2**64)``, a ``holdout_seed`` without a
    ``holdout``, ``holdout`` together with ``eval_mask``, with ``n_gpus > 1`` or with ``devices``, ``eval_every < 1`` and
    ``patience < 0``."""
    if holdout is None:
        if holdout_seed is not None:
            raise ValueError("holdout_seed needs a holdout: it seeds the split")
        return None
    if eval_mask is not None:
        raise ValueError("holdout draws the eval set on the device: it does not go with eval_mask")
    interval = _hip.holdout_interval(holdout)
    if holdout_seed is not None:
        try:
            holdout_seed = _hip.sample_seed(holdout_seed)
        except ValueError:
            raise ValueError(f"holdout_seed must be None or an integer in [0, 2**64) (got {holdout_seed!r})") from None
    if int(n_gpus) != 1 or devices is not None:
        raise ValueError("an eval set is evaluated on one GPU: holdout does not go with n_gpus > 1 or devices")
    if isinstance(eval_every, (bool, np.bool_)) or not isinstance(eval_every, (int, np.integer)) or eval_every < 1:
        raise ValueError(f"eval_every must be an integer >= 1 (got {eval_every!r})")
    if isinstance(patience, (bool, np.bool_)) or not isinstance(patience, (int, np.integer)) or patience < 0:
        raise ValueError(f"patience must be an integer >= 0 (got {patience!r})")
    return interval, holdout_seed


def nbmf_mm_solver(Y, n_components, max_iter=500, tol=1e-5, alpha=1.2, beta=1.2, W_init=None,
                   H_init=None, mask=None, random_state=None, verbose=0, orientation="beta-dir",
                   eps=1e-8, projection="normalize", device=0, n_gpus=1, devices=None, _ctx_hook=None,
                   eval_mask=None, eval_every=10, patience=0, restore_best=True, _eval_out=None, holdout=None,
                   holdout_seed=None):
    """NBMF-MM on the GPU.  Returns ``(W (m,k), H (k,n), losses, 0.0, n_iter)``.

    Mirrors src/nbmf_mm/_solver.py:61-216 argument for argument; ``projection``, ``device`` and ``n_gpus`` / ``devices``
    are extensions.  ``time_elapsed`` is 0.0 as in the reference (:216).  ``n_gpus > 1``: the same fit with the rows of
    Y sharded over that many GPUs from this one process (``_dist.fit_in_process``: one host thread and context per GPU,
    one exchange of the K x N H-step products per iteration); ``devices`` names the GPUs (default 0 .. n_gpus-1).

    ``eval_mask`` (extension; see :func:`eval_pairs`): its nonzeros are held-out entries whose truth ``Y`` holds; they
    stay on the device, their log-likelihood is summed there every ``eval_every`` iterations, and with ``patience > 0``
    the run ends at the ``patience``-th consecutive evaluation that does not improve.  With ``restore_best`` the factors
    returned are those of the best evaluation; ``losses`` and ``n_iter`` are the run's own either way.  The return value
    stays the reference's 5-tuple: the curve is left in the dict ``_eval_out`` (``iters``, ``logliks``, ``count``,
    ``best_iter``, ``stopped_early``), which is how the estimator gets it.

    ``holdout`` (extension; see :func:`holdout_args`): the eval set is drawn on the device instead -- a fraction ``f`` of the
    observed entries (those ``mask`` leaves in), or those whose uniform lies in a pair ``(lo, hi)``, by the counter-based
    rule of ``_hip.holdout_reference`` with ``holdout_seed`` (default: ``random_state`` when that is an int, else a fresh
    draw).  They leave the fit and are evaluated exactly as an ``eval_mask`` of the same entries would be, bit for bit; no
    mask and no index list crosses from the host.  ``_eval_out`` also receives ``seed`` and ``interval``.  Binary data
    only; not with ``eval_mask``, ``n_gpus > 1`` or ``devices``.
    """
    split = holdout_args(holdout, holdout_seed, eval_mask, eval_every, patience, n_gpus, devices)
    pairs = None if split is not None else eval_pairs(
        Y if hasattr(Y, "toarray") or eval_mask is None else np.asarray(Y), eval_mask, eval_every, patience, orientation, n_gpus,
        devices)
    if (int(n_gpus) != 1 or devices is not None) and (isinstance(Y, PackedBits) or isinstance(mask, PackedBits)):
        raise ValueError("PackedBits input is fitted on one GPU: it does not go with n_gpus > 1 or devices")
    if int(n_gpus) != 1 or devices is not None:
        n = int(n_gpus) if devices is None else len(list(devices))
        if devices is not None and int(n_gpus) not in (1, n):
            raise ValueError(f"devices names {n} GPUs, n_gpus is {n_gpus}")
        if n < 1:
            raise ValueError("n_gpus must be >= 1")
        if n > 1:
            from ._dist import fit_in_process
            return fit_in_process(Y, n_components, n, devices=devices, orientation=orientation, max_iter=max_iter, tol=tol,
                                  alpha=alpha, beta=beta, W_init=W_init, H_init=H_init, mask=mask, random_state=random_state,
                                  verbose=verbose, eps=eps, projection=projection)
        if devices is not None:
            device = int(list(devices)[0])
    proj = _projection_code(projection)
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1")      # the reference dies with UnboundLocalError here (:215)
    if random_state is not None:
        np.random.seed(random_state)                   # GLOBAL legacy RNG, as :102-103
    if split is not None and split[1] is None:         # the split's seed: random_state itself, else drawn before the init draws
        is_int = isinstance(random_state, (int, np.integer)) and not isinstance(random_state, (bool, np.bool_))
        split = (split[0], _hip.sample_seed(int(random_state) if is_int else None))
    # (sparse input: the reference densifies, :28-29,106-107; here upload_any keeps binary patterns sparse)
    if not hasattr(Y, "toarray"):
        Y = np.asarray(Y)
    m, n = Y.shape
    k = int(n_components)
    transposed = orientation == "dir-beta"
    if transposed:                                     # transpose trick, :113-123
        m, n = n, m
        if W_init is not None and H_init is not None:
            W_init, H_init = np.asarray(H_init).T, np.asarray(W_init).T
    W_init, H_init = _draw_init(m, k, n, W_init, H_init)
    W = np.asarray(W_init, dtype=np.float64).T         # (k, m), :132
    H = np.asarray(H_init, dtype=np.float64)           # (k, n), :133
    W = W / W.sum(axis=0, keepdims=True)               # :136 (a wrong-shaped init raises here, as in the reference)
    if W.shape != (k, m) or H.shape != (k, n):
        raise ValueError(f"operands could not be broadcast together: W_init/H_init give {W.shape}, {H.shape}; "
                         f"expected ({k},{m}), ({k},{n})")

    with _hip.Context(m, n, k, device=device) as ctx:
        ctx.set_hyper(alpha, beta, eps, proj)
        # the user's array goes up untransposed; the pack kernel applies the orientation
        upload_any(ctx, Y, mask, transposed=transposed)
        if _ctx_hook is not None:
            _ctx_hook(ctx)
        ctx.set_factors(W, H)
        if verbose > 0:
            # the reference prints inside its loop (:165-166): the library reports the losses every ten
            # iterations while it runs (one iteration behind the device, see nbmf_set_progress)
            def _report(first, values):
                for it, loss in enumerate(values, start=first):
                    if it % 10 == 0:
                        print(f"Iter {it:4d}: Loss = {loss:.6f}", flush=True)
            ctx.set_progress(_report, every=10)
        count = 0
        if pairs is not None:
            ctx.set_eval(*pairs, every=int(eval_every), patience=int(patience))
            count = int(pairs[0].size)
        elif split is not None:
            try:
                count = ctx.hold_out(split[1], *split[0], transposed=transposed, every=int(eval_every), patience=int(patience))
            except _hip.NBMFHipError as e:             # (data on a real-valued storage path: the library's own words)
                raise ValueError(str(e)) from None
        evaluated = pairs is not None or split is not None
        losses, n_iter = ctx.run(int(max_iter), float(tol))
        stopped_early = False
        if evaluated:
            iters, logliks, best_iter, stopped_early = ctx.eval_curve()
            if _eval_out is not None:
                _eval_out.update(iters=iters, logliks=logliks, count=count, best_iter=best_iter, stopped_early=stopped_early)
                if split is not None:
                    _eval_out.update(seed=split[1], interval=split[0])
        Wk, Hk = ctx.best_factors() if evaluated and restore_best else ctx.get_factors()

    losses = [float(v) for v in losses]
    if verbose > 0 and stopped_early:
        print(f"Stopped early at iteration {n_iter}: best held-out log-likelihood at iteration {best_iter}")
    elif verbose > 0 and (n_iter < int(max_iter) or (n_iter > 1 and losses[-2] != 0 and
                                                   abs(losses[-2] - losses[-1]) / abs(losses[-2]) < tol)):
        print(f"Converged at iteration {n_iter - 1}")   # :172-173

    W_final, H_final = Wk.T, Hk                        # :178-179
    if transposed:
        W_final, H_final = H_final.T, W_final.T        # :182-184
    W_final, H_final = _touch_up(W_final, H_final, orientation)
    return W_final, H_final, losses, 0.0, n_iter


def nbmf_mm_restarts(Y, n_components, n_init, max_iter=500, tol=1e-5, alpha=1.2, beta=1.2, W_init=None, H_init=None,
                     mask=None, random_state=None, orientation="beta-dir", eps=1e-8, projection="normalize", device=0):
    """``n_init`` restarts of :func:`nbmf_mm_solver` (README.md:144; seeds ``random_state + r``) with ONE upload of the
    data and ONE ``nbmf_run_batch`` call: small problems run several restarts at a time in one launch.  Every restart is
    bit for bit the sequential call with that seed (same draws from the global generator, in the same order).  Returns
    ``(W, H, losses, 0.0, n_iter)`` of the restart with the lowest final loss (the first one on ties) and its index."""
    proj = _projection_code(projection)
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1")
    if not hasattr(Y, "toarray"):
        Y = np.asarray(Y)
    m, n = Y.shape
    k = int(n_components)
    transposed = orientation == "dir-beta"
    if transposed:
        m, n = n, m
        if W_init is not None and H_init is not None:
            W_init, H_init = np.asarray(H_init).T, np.asarray(W_init).T
    W0s, H0s = [], []
    for r in range(int(n_init)):
        if random_state is not None:
            np.random.seed(random_state + r)           # restarts: consecutive seeds, each seeding the GLOBAL generator (:102-103)
        Wi, Hi = _draw_init(m, k, n, W_init, H_init)
        W = np.asarray(Wi, dtype=np.float64).T
        W0s.append(W / W.sum(axis=0, keepdims=True))
        H0s.append(np.asarray(Hi, dtype=np.float64))
        if W0s[-1].shape != (k, m) or H0s[-1].shape != (k, n):
            raise ValueError(f"operands could not be broadcast together: W_init/H_init give {W0s[-1].shape}, {H0s[-1].shape}; "
                             f"expected ({k},{m}), ({k},{n})")
    with _hip.Context(m, n, k, device=device) as ctx:
        ctx.set_hyper(alpha, beta, eps, proj)
        upload_any(ctx, Y, mask, transposed=transposed)
        curves, n_iters, Ws, Hs = ctx.run_batch([alpha] * len(W0s), [beta] * len(W0s), np.stack(W0s), np.stack(H0s),
                                                int(max_iter), float(tol))
    best = min(range(len(curves)), key=lambda r: (curves[r][-1], r))
    W_final, H_final = Ws[best].T, Hs[best]
    if transposed:
        W_final, H_final = H_final.T, W_final.T
    W_final, H_final = _touch_up(W_final, H_final, orientation)
    return (W_final, H_final, [float(v) for v in curves[best]], 0.0, int(n_iters[best])), best


def _touch_up(W_final, H_final, orientation):
    """Final renormalisation only where the simplex sums drifted by more than 1e-9
    (src/nbmf_mm/_solver.py:192-213); normally a no-op."""
    if orientation == "beta-dir":
        sums = W_final.sum(axis=1, keepdims=True)
        dev = np.max(np.abs(sums - 1.0)) if sums.size else 0.0
        if np.isfinite(dev) and dev > 1e-9:
            ok = (sums > 1e-12).ravel()
            if np.any(ok):
                W_final = np.array(W_final)
                W_final[ok, :] = W_final[ok, :] / sums[ok]
    else:
        sums = H_final.sum(axis=0, keepdims=True)
        dev = np.max(np.abs(sums - 1.0)) if sums.size else 0.0
        if np.isfinite(dev) and dev > 1e-9:
            ok = (sums > 1e-12).ravel()
            if np.any(ok):
                H_final = np.array(H_final)
                H_final[:, ok] = H_final[:, ok] / sums[:, ok]
    return W_final, H_final


def w_only_transform(X, H, mask=None, W0=None, n_iter=50, device=0):
    """The loop of ``NBMFMM.transform`` (src/nbmf_mm/_base.py:170-199) on the GPU: ``n_iter``
    simplex-factor updates with ``H`` frozen, then clip to [1e-8, 1] and row-renormalise."""
    if not hasattr(X, "toarray"):
        X = _dense(X)
    m, n = X.shape
    k = H.shape[0]
    if W0 is None:
        W0 = np.random.uniform(0.1, 0.9, (m, k))      # global RNG, :175
    with _hip.Context(m, n, k, device=device) as ctx:
        ctx.set_hyper(1.2, 1.2, 1e-8, _hip.PROJ_NORMALIZE)   # eps is hard-coded 1e-8 at :190
        upload_any(ctx, X, mask)
        ctx.set_factors(np.ascontiguousarray(W0.T), H)
        ctx.w_only_steps(int(n_iter))
        Wk, _ = ctx.get_factors()
    W = Wk.T
    W = np.clip(W, 1e-8, 1.0)                          # :196
    W = W / W.sum(axis=1, keepdims=True)               # :198
    return W


def device_score(X, H, mask=None, n_iter=50, device=0):
    """``NBMFMM.score`` on the GPU (src/nbmf_mm/_base.py:212-247): the inner transform runs WITHOUT
    the mask (:235), then the mean log-likelihood per observed entry of W @ H under ``mask``.
    The reference clips W @ H to [0, 1] first (:210); so does the device sweep (clip_theta)."""
    if not hasattr(X, "toarray"):
        X = _dense(X)
    m, n = X.shape
    k = H.shape[0]
    W0 = np.random.uniform(0.1, 0.9, (m, k))          # global RNG, :175
    with _hip.Context(m, n, k, device=device) as ctx:
        ctx.set_hyper(1.2, 1.2, 1e-8, _hip.PROJ_NORMALIZE)
        upload_any(ctx, X, None)
        ctx.set_factors(np.ascontiguousarray(W0.T), H)
        ctx.w_only_steps(int(n_iter))
        Wk, _ = ctx.get_factors()
        W = np.clip(Wk.T, 1e-8, 1.0)                  # :196
        W = W / W.sum(axis=1, keepdims=True)          # :198
        if mask is not None:
            upload_any(ctx, X, mask)
        ctx.set_factors(np.ascontiguousarray(W.T), H)
        ll = ctx.loglik(clip_theta=True)
        n_obs = ctx.n_obs()
    return float(ll / n_obs)


@contextlib.contextmanager
def _factors_only(W, H, device):
    """``(ctx, m, n)``: a context that holds the factors ``W`` (m, k) and ``H`` (k, n) and no data -- what the functions
    that read Theta back run on."""
    m, k = W.shape
    n = H.shape[1]
    with _hip.Context(m, n, k, device=device) as ctx:
        ctx.set_factors(np.ascontiguousarray(W.T), H)
        yield ctx, m, n


def device_predict(W, H, rows=None, cols=None, threshold=None, device=0):
    """Theta = ``W @ H`` clipped to [0, 1] (``NBMFMM.inverse_transform``, src/nbmf_mm/_base.py:201-210) on the GPU, for
    ``W`` (rows, k) and ``H`` (k, features) as the estimator holds them (user layout in both orientations: the solver
    has un-transposed them).  With ``rows`` / ``cols`` (already validated: ``_hip.index_pairs``) the values at those
    pairs; otherwise the dense matrix, as float64 or, with a ``threshold``, as the bool matrix ``Theta > threshold``
    compared on the device.  The context holds factors only: no data is uploaded."""
    with _factors_only(W, H, device) as (ctx, m, n):
        if rows is not None:
            return ctx.predict_at(rows, cols, clip_theta=True)
        return ctx.predict_rows(0, m, clip_theta=True, threshold=threshold)


def device_theta_bits(W, H, threshold=None, seed=None, device=0):
    """A decision per entry of Theta = clip(``W @ H``, 0, 1), made and bit-packed on the GPU (``Context.theta_bits``): the
    :class:`PackedBits` of ``Theta > threshold``, or with a ``seed`` (already validated: ``_hip.sample_seed``) of one draw
    ``_hip.hash_uniform(rows, features, seed) < Theta`` of Bernoulli(Theta).  ``W``, ``H`` as in :func:`device_predict`.
    One bit per entry comes back.  Factors only: no data is uploaded."""
    with _factors_only(W, H, device) as (ctx, m, n):
        return ctx.theta_bits(0, m, threshold=threshold, seed=seed, clip_theta=True)


#: bytes of densified ``exclude`` that :func:`device_top_n` holds at a time (one row block)
TOP_N_EXCLUDE_BLOCK_BYTES = 64 << 20


def device_top_n(W, H, top, exclude=None, device=0):
    """The ``top`` features with the largest Theta = clip(``W @ H``, 0, 1) for every row of ``W``, ranked on the GPU
    (``Context.top_n``): ``(cols, scores)``, both ``(rows, top)``.  ``W``, ``H`` as in :func:`device_predict`; ``top`` and
    ``exclude`` already validated (``_hip.top_n_count``; shape ``(rows, features)``, dense of a bool / integer / floating
    dtype or scipy-sparse, nonzero = skip).  ``exclude`` is made dense one row block at a time, so the host never holds
    more than ``TOP_N_EXCLUDE_BLOCK_BYTES`` of it beyond what the caller passed.  Factors only: no data is uploaded."""
    if hasattr(exclude, "toarray") and not isinstance(exclude, PackedBits):
        exclude = exclude.tocsr()
    with _factors_only(W, H, device) as (ctx, m, n):
        if exclude is None:
            return ctx.top_n(top, 0, m, clip_theta=True)
        cols = np.empty((m, top), dtype=np.int64)
        scores = np.empty((m, top), dtype=np.float64)
        block = max(1, min(m, TOP_N_EXCLUDE_BLOCK_BYTES // _row_bytes(exclude, n)))
        for r0 in range(0, m, block):
            nr = min(block, m - r0)
            x = _row_block(exclude, r0, nr, True)
            cols[r0:r0 + nr], scores[r0:r0 + nr] = ctx.top_n(top, r0, nr, exclude=x, clip_theta=True)
        return cols, scores


def device_neighbors(W, H, top, axis=1, metric="cosine", query=None, skip_self=True, device=0):
    """The ``top`` items most similar to each ``query`` item within one side of the matrix, ranked on the GPU
    (``Context.neighbors``): ``(idx, scores)``, both ``(len(query), top)``.  ``W`` (rows, k) and ``H`` (k, features) as in
    :func:`device_predict`; ``axis`` 0 compares rows of ``W`` (samples), 1 columns of ``H`` (features); ``metric`` one of
    ``"dot"``, ``"cosine"``, ``"profile"``; ``query`` None for all items.  Factors only: no data is uploaded."""
    with _factors_only(W, H, device) as (ctx, m, n):
        return ctx.neighbors(top, axis=axis, metric=metric, query=query, skip_self=skip_self)


def device_similarity(W, H, axis=1, metric="cosine", query=None, device=0):
    """The float64 ``(len(query), items)`` similarity slab behind :func:`device_neighbors` (``Context.similarity``)."""
    with _factors_only(W, H, device) as (ctx, m, n):
        return ctx.similarity(axis=axis, metric=metric, query=query)


def _one_call_operand(A, is_mask, what="X"):
    """A binary ``(rows, features)`` operand of :func:`device_top_pairs` in a form that goes to the device in ONE call: a
    dense bool / uint8 array with unit stride along a row and a :class:`PackedBits` as they are; anything else --
    scipy-sparse, or dense of another dtype -- as a :class:`PackedBits` filled one row block of at most
    ``TOP_N_EXCLUDE_BLOCK_BYTES`` dense bytes at a time, so the host never holds an m x n byte matrix of it.  Data
    (``is_mask`` false) that is not exactly {0, 1} is a ``ValueError``; a mask or an exclude is ``!= 0``."""
    if A is None or isinstance(A, PackedBits):
        return A
    if hasattr(A, "toarray"):
        A = A.tocsr()
    else:
        A = np.asarray(A)
        if A.dtype in (np.bool_, np.uint8):
            return _row_block(A, 0, A.shape[0], is_mask)
    m, n = A.shape
    bits = np.zeros((m, (n + 7) // 8), dtype=np.uint8)
    block = max(1, min(m, TOP_N_EXCLUDE_BLOCK_BYTES // max(n, 1)))
    for r0 in range(0, m, block):
        a = _row_block(A, r0, min(block, m - r0), is_mask)
        if a.dtype == np.float64:
            raise ValueError(f"{what} must be binary")
        bits[r0:r0 + a.shape[0]] = np.packbits(a != 0, axis=1)
    return PackedBits(bits, (m, n))


def device_top_pairs(W, H, top, kind="theta", x=None, mask=None, device=0):
    """The ``top`` best entries of Theta = clip(``W @ H``, 0, 1) over the whole matrix, selected on the GPU
    (``Context.top_pairs``): ``(rows, cols, scores)``.  ``W``, ``H`` as in :func:`device_predict`; ``top`` already
    validated (``_hip.top_pairs_count``).  ``kind="theta"``: the largest Theta, ``x`` an exclude matrix or None;
    ``kind="likelihood"``: the observed entries of the binary data ``x`` that the model gives the lowest probability,
    ``mask`` nonzero = observed.  ``x`` and ``mask``: shape ``(rows, features)``, dense or scipy-sparse or
    :class:`PackedBits`.  The call keeps its operands on the device through all its passes, so they go up in one piece:
    bool / uint8 arrays and packed bits as they are, anything else packed on the host block by block
    (:func:`_one_call_operand`).  Factors only: no context holds the data."""
    x = _one_call_operand(x, kind == "theta", "X")
    mask = _one_call_operand(mask, True)
    with _factors_only(W, H, device) as (ctx, m, n):
        return ctx.top_pairs(top, kind, x=x, mask=mask, row0=0, nrows=m, clip_theta=True)


def device_rank_of(W, H, targets_csr, exclude=None, device=0):
    """Where the target features of every row of ``W`` stand in the order :func:`device_top_n` ranks the row by, counted on
    the GPU (``Context.rank_of``): ``(rank, above, tied, scores, eligible)``, the first four indexed like the targets'
    ``indices``, ``eligible`` per row.  ``W``, ``H`` as in :func:`device_predict`; ``targets_csr`` the ``(indptr, indices)``
    of a CSR pattern with ``W.shape[0]`` rows, already validated (``_hip.csr_targets``); ``exclude`` as in
    :func:`device_top_n`, made dense one row block of at most ``TOP_N_EXCLUDE_BLOCK_BYTES`` at a time -- a block passes its
    slice of ``indptr`` and the whole ``indices``, and a row's result does not depend on the blocks.  Factors only: no data
    is uploaded."""
    indptr, indices = targets_csr
    if hasattr(exclude, "toarray") and not isinstance(exclude, PackedBits):
        exclude = exclude.tocsr()
    with _factors_only(W, H, device) as (ctx, m, n):
        if exclude is None:
            return ctx.rank_of(indptr, indices, 0, m, clip_theta=True)
        count = int(indptr[-1])
        rank, above, tied = (np.full(count, -1, dtype=np.int64) for _ in range(3))
        scores = np.full(count, np.nan)
        eligible = np.empty(m, dtype=np.int64)
        block = max(1, min(m, TOP_N_EXCLUDE_BLOCK_BYTES // _row_bytes(exclude, n)))
        for r0 in range(0, m, block):
            nr = min(block, m - r0)
            x = _row_block(exclude, r0, nr, True)
            got = ctx.rank_of(indptr[r0:r0 + nr + 1], indices, r0, nr, exclude=x, clip_theta=True)
            t = slice(int(indptr[r0]), int(indptr[r0 + nr]))
            for whole, part in zip((rank, above, tied, scores), got):
                whole[t] = part[t]
            eligible[r0:r0 + nr] = got[4]
        return rank, above, tied, scores, eligible


#: bytes of data (and as many of mask) that :func:`device_score_samples` converts or makes dense at a time (one row block)
SCORE_SAMPLES_BLOCK_BYTES = 64 << 20


def _row_bytes(A, n):
    """Bytes a row of ``n`` entries of a mask-like ``A`` takes on its way to the device: ``ceil(n / 8)`` packed, else n."""
    return max((n + 7) // 8 if isinstance(A, PackedBits) else n, 1)


def _row_block(A, r0, nr, is_mask):
    """Rows ``[r0, r0 + nr)`` of the data of ``Context.score_rows``, or of a mask (its ``mask``, the ``exclude`` of
    ``Context.top_n``), as the context takes them.  A bool / uint8 block is passed as it is; a mask of another dtype as
    ``!= 0``; other data as uint8 when the block is exactly {0, 1}, else as float64.  A sparse block is made dense first
    (a mask as a bool block, whatever the stored dtype); a block that is not laid out row after row is copied.  The rows
    of a :class:`PackedBits` are passed as they are (a view)."""
    a = A[r0:r0 + nr]
    if isinstance(a, PackedBits):
        return a
    if hasattr(a, "toarray"):
        a = (a != 0).toarray() if is_mask else a.toarray()
    a = np.asarray(a)
    if a.dtype != np.bool_ and a.dtype != np.uint8:
        if is_mask:
            a = a != 0
        elif np.all((a == 0) | (a == 1)):
            a = a.astype(np.uint8)
        else:
            a = np.asarray(a, dtype=np.float64)
    if a.size and (a.strides[1] != a.itemsize or a.strides[0] < a.shape[1] * a.itemsize or a.strides[0] % a.itemsize):
        a = np.ascontiguousarray(a)
    return a


def _sliceable(X, mask):
    """``(X, mask, one_call)``: the data and the mask of :func:`device_score_samples` / :func:`device_theta_hist` in a form
    whose row blocks ``_row_block`` can take (sparse as CSR, anything else an ndarray), and whether they can go to the
    device in one call as they are: both dense bool / uint8 or :class:`PackedBits` (or no mask)."""
    packed = lambda a: isinstance(a, PackedBits)   # noqa: E731
    byte = lambda a: a is None or packed(a) or (not hasattr(a, "toarray") and a.dtype in (np.bool_, np.uint8))   # noqa: E731
    if packed(X):
        pass
    elif hasattr(X, "toarray"):
        X = X.tocsr()
    elif not isinstance(X, np.ndarray):
        X = np.asarray(X)
    if mask is not None and not packed(mask):
        mask = mask.tocsr() if hasattr(mask, "toarray") else np.asarray(mask)
    return X, mask, byte(X) and byte(mask)


def device_score_samples(W, H, X, mask=None, axis=0, device=0):
    """The log-likelihood of Theta = clip(``W @ H``, 0, 1) against ``X`` (eps = 1e-8, as ``NBMFMM.score``), summed on the
    GPU (``Context.score_rows``) over the observed entries of every row (``axis=0``) or of every feature (``axis=1``):
    ``(sums float64, counts int64)``.  ``W``, ``H`` as in :func:`device_predict`; ``X`` and ``mask`` (nonzero = observed)
    dense or scipy-sparse of shape ``(rows, features)``, already validated.  Factors only: no context holds the data.
    Dense bool / uint8 input with a bool / uint8 (or no) mask goes to the device in one call as it is.  Anything else goes
    in row blocks of at most ``SCORE_SAMPLES_BLOCK_BYTES`` (a multiple of 16 rows): sparse blocks are made dense, float
    data goes as uint8 where the block is exactly {0, 1} and as float64 otherwise.  A row's result does not depend on the
    blocks.  For ``axis=1`` the blocks' sums and counts are added on the host in ascending order: feature scores of
    block-streamed input equal the one-call result to rounding, not bit for bit."""
    X, mask, one_call = _sliceable(X, mask)
    with _factors_only(W, H, device) as (ctx, m, n):
        block = m if one_call else max(16, SCORE_SAMPLES_BLOCK_BYTES // (8 * max(n, 1)) // 16 * 16)
        sums = np.zeros(n if axis else m, dtype=np.float64)
        counts = np.zeros(n if axis else m, dtype=np.int64)
        for r0 in range(0, m, max(block, 1)):
            nr = min(block, m - r0)
            x = _row_block(X, r0, nr, False)
            mk = None if mask is None else _row_block(mask, r0, nr, True)
            rl, ro, cl, co = ctx.score_rows(x, mk, r0, nr, clip_theta=True, eps=1e-8, rows=not axis, cols=bool(axis))
            if axis:
                sums += cl
                counts += co
            else:
                sums[r0:r0 + nr], counts[r0:r0 + nr] = rl, ro
    return sums, counts


def device_theta_hist(W, H, X, mask=None, bins=256, device=0):
    """The observed entries of the binary ``X``, counted on the GPU (``Context.theta_hist``) by class and by the bin of
    Theta = clip(``W @ H``, 0, 1) they fall in: ``(hist int64 (2, bins), nan_count int64 (2,))``.  ``W``, ``H`` as in
    :func:`device_predict`; ``X`` and ``mask`` (nonzero = observed) dense or scipy-sparse of shape ``(rows, features)``,
    already validated.  Factors only: no context holds the data.  Dense bool / uint8 input with a bool / uint8 (or no)
    mask goes to the device in one call as it is.  Anything else goes in row blocks of at most
    ``SCORE_SAMPLES_BLOCK_BYTES``: sparse blocks are made dense, a block of another dtype goes as uint8 when it is exactly
    {0, 1} and is otherwise not binary: ``ValueError("X must be binary")``.  The blocks' counts are added on the host as
    int64 -- unlike the feature sums of :func:`device_score_samples`, integers: block-streamed input gives exactly the
    arrays of the one-call form."""
    X, mask, one_call = _sliceable(X, mask)
    with _factors_only(W, H, device) as (ctx, m, n):
        block = m if one_call else max(16, SCORE_SAMPLES_BLOCK_BYTES // (8 * max(n, 1)) // 16 * 16)
        hist = np.zeros((2, bins), dtype=np.int64)
        nan_count = np.zeros(2, dtype=np.int64)
        for r0 in range(0, m, max(block, 1)):
            nr = min(block, m - r0)
            x = _row_block(X, r0, nr, False)
            if not isinstance(x, PackedBits) and x.dtype == np.float64:
                raise ValueError("X must be binary")
            mk = None if mask is None else _row_block(mask, r0, nr, True)
            h, c = ctx.theta_hist(x, mk, r0, nr, bins=bins)
            hist += h
            nan_count += c
    return hist, nan_count


def device_moments(W, H, X, mask=None, groups=None, n_groups=None, keep_rows=None, device=0, _pass_groups=_hip.MOMENT_MAX_GROUPS):
    """The observed entries of the binary ``X``, summed on the GPU (``Context.moments``) into the five integers per slot
    that the expected count of ones under Theta = clip(``W @ H``, 0, 1), its variance and the observed count are functions of:
    ``(row_tab int64 (rows, n_groups, 5), col_tab int64 (features, 5), nan_count int64 (2,))``.  ``W``, ``H`` as in
    :func:`device_predict`; ``X`` and ``mask`` as in :func:`device_theta_hist`, already validated; ``groups`` / ``n_groups``
    the feature labels, already validated (``_hip.group_labels``; any number of groups).  Factors only: no context holds
    the data.  Dense bool / uint8 input with a bool / uint8 (or no) mask and every :class:`PackedBits` goes to the device as
    it is, in one call per pass; anything else goes in row blocks of at most ``SCORE_SAMPLES_BLOCK_BYTES`` made dense
    one at a time.  The blocks' column sums are added on the host as int64: integers, so block-streamed input gives
    exactly the arrays of the one-call form.  More than ``MOMENT_MAX_GROUPS`` groups run in passes of that many labels
    each (``_pass_groups``: a test hook), the other labels set to -1, and the row tables are put side by side -- a slot's
    sum does not depend on the passes; the column table and the NaN counts are those of the first pass (they do not look
    at the groups).  ``keep_rows`` (bool per row, None: all): the rows that are False count nowhere -- their mask is
    dropped on the host, one row block at a time (such a request is block-streamed) -- and their ``row_tab`` is zero."""
    X, mask, one_call = _sliceable(X, mask)
    if keep_rows is not None and np.all(keep_rows):
        keep_rows = None
    labels, n_groups = _hip.group_labels(groups, H.shape[1], n_groups)
    with _factors_only(W, H, device) as (ctx, m, n):
        one_call = one_call and keep_rows is None
        block = m if one_call else max(16, SCORE_SAMPLES_BLOCK_BYTES // (8 * max(n, 1)) // 16 * 16)
        row_tab = np.zeros((m, n_groups, len(_hip.MOMENT_FIELDS)), dtype=np.int64)
        col_tab = np.zeros((n, len(_hip.MOMENT_FIELDS)), dtype=np.int64)
        nan_count = np.zeros(2, dtype=np.int64)
        for r0 in range(0, m, max(block, 1)):
            nr = min(block, m - r0)
            x = _row_block(X, r0, nr, False)
            if not isinstance(x, PackedBits) and x.dtype == np.float64:
                raise ValueError("X must be binary")
            mk = None if mask is None else _row_block(mask, r0, nr, True)
            if keep_rows is not None and not np.all(keep_rows[r0:r0 + nr]):
                mk = np.ones((nr, n), dtype=bool) if mk is None else np.array(mk.toarray() if isinstance(mk, PackedBits) else mk) != 0
                mk[~keep_rows[r0:r0 + nr]] = False
            for g0 in range(0, n_groups, _pass_groups):
                ng = min(_pass_groups, n_groups - g0)
                part = labels if ng == n_groups else np.where((labels >= g0) & (labels < g0 + ng), labels - g0, -1)
                rt, ct, nc = ctx.moments(x, mk, groups=None if groups is None else part, n_groups=ng, row0=r0, nrows=nr,
                                         rows=True, cols=g0 == 0)
                row_tab[r0:r0 + nr, g0:g0 + ng] = rt
                if g0 == 0:
                    col_tab += ct
                    nan_count += nc
    return row_tab, col_tab, nan_count
