"""scikit-learn style estimator with the reference's public surface
(src/nbmf_mm/_base.py:7-269): same constructor arguments, methods, attributes, orientation
aliases and error messages; ``fit`` and ``transform`` run on an MI355X through libnbmf_hip.
"""
import inspect

import numpy as np
from sklearn.base import BaseEstimator, TransformerMixin
from sklearn.utils import check_array

from . import _hip, _metrics
from ._packed import PackedBits
from ._solver import (device_moments, device_neighbors, device_predict, device_rank_of, device_score, device_score_samples, device_theta_bits, device_theta_hist,
                      device_top_n, device_top_pairs, eval_pairs, holdout_args, nbmf_mm_restarts, nbmf_mm_solver, w_only_transform)
from ._utils import check_is_fitted

# Accepted spellings of the two orientations: the exact strings of src/nbmf_mm/_base.py:127-137
# (matching is exact, not case-folding; the order is the reference's, it shows in the error message).
_SPELLINGS = (
    ("beta-dir", "beta-dir"), ("dir-beta", "dir-beta"), ("Beta-Dir", "beta-dir"), ("Dir-Beta", "dir-beta"),
    ("Dir Beta", "dir-beta"), ("binary ICA", "beta-dir"), ("Binary ICA", "beta-dir"), ("bICA", "beta-dir"),
    ("Aspect Bernoulli", "dir-beta"),
)
_ORIENTATION_ALIASES = dict(_SPELLINGS)
# (the name of check_array's switch for its NaN / inf pass changed with scikit-learn 1.6)
_FINITE_KW = "ensure_all_finite" if "ensure_all_finite" in inspect.signature(check_array).parameters else "force_all_finite"


class NBMFMM(BaseEstimator, TransformerMixin):
    """Mean-parameterised Bernoulli matrix factorisation by majorisation-minimisation
    (Magron & Fevotte 2022), GPU-resident.

    Parameters follow src/nbmf_mm/_base.py:63-66.  Extensions: ``projection`` (alias
    ``projection_method``) in {"normalize", "duchi"} (README.md:27-35 of the reference), ``n_init``
    (README.md:144: keep the best of several random restarts), ``device``, and ``n_gpus`` / ``devices``: ``fit`` with the
    rows of X sharded over several GPUs of this machine, driven from this one process (SURVEY section 5's config row;
    one exchange of the K x N H-step products per iteration, BASELINE.json's north star) -- same results to 1e-12.

    Attributes after ``fit``: ``W_`` (n_samples, k), ``components_`` (k, n_features),
    ``loss_curve_`` / ``objective_history_``, ``loss_`` / ``reconstruction_err_``, ``n_iter_``
    (_base.py:114-120).
    """

    def __init__(self, n_components=10, alpha=1.2, beta=1.2, max_iter=2000, tol=1e-5, W_init=None,
                 H_init=None, init=None, random_state=None, verbose=0, orientation="beta-dir",
                 projection="normalize", projection_method=None, n_init=1, device=0, n_gpus=1, devices=None):
        self.n_components = n_components
        self.alpha = alpha
        self.beta = beta
        self.max_iter = max_iter
        self.tol = tol
        self.W_init = W_init
        self.H_init = H_init
        self.init = init            # accepted and ignored, as in the reference (_base.py:74)
        self.random_state = random_state
        self.verbose = verbose
        self.orientation = orientation
        self.projection = projection
        self.projection_method = projection_method
        self.n_init = n_init
        self.device = device
        self.n_gpus = n_gpus            # fit() shards the rows of X over this many GPUs from this one process
        self.devices = devices          # ... these ones (default 0 .. n_gpus-1); transform / score use `device`

    # -- helpers -----------------------------------------------------------------------------
    def _normalize_orientation(self, orientation):
        try:
            return _ORIENTATION_ALIASES[orientation]
        except (KeyError, TypeError):
            raise ValueError(f"Unknown orientation: {orientation}. "
                             f"Must be one of {list(_ORIENTATION_ALIASES.keys())}") from None

    def _projection(self):
        return self.projection_method if self.projection_method is not None else self.projection

    @staticmethod
    def _validated(X, keep_sparse=False):
        # A PackedBits is 2-D, binary and finite by construction, and check_array does not know the type: what is left of
        # its checks is that there is at least one row and one feature.
        if isinstance(X, PackedBits):
            if X.shape[0] < 1 or X.shape[1] < 1:
                raise ValueError(f"Found array with shape {X.shape}: at least one sample and one feature are required")
            return X
        # _base.py:83 converts every input to float64.  A dense bool / uint8 matrix stays as it is here -- one byte per
        # entry up to the device, where the pack kernel reads the bytes (nbmf_upload_v): the same fit bit for bit, without
        # the 8-byte-per-entry host copy (BASELINE configs[4]: 6.1 GB instead of 49 GB).  Shape and dimension checks are
        # check_array's either way; a uint8 value above 1 is "X must be binary" (:90-91), raised by the device pack.
        dt = getattr(X, "dtype", None)
        if dt is not None and not hasattr(X, "toarray") and (dt == np.bool_ or dt == np.uint8):
            X = check_array(X, dtype=None)
            return X
        if isinstance(X, np.ndarray) and dt == np.float32 and X.ndim == 2 and X.size > (1 << 24):
            # a big float32 matrix likewise: four bytes per entry up to the device, which converts (exactly) and checks
            return check_array(X, dtype=None, **{_FINITE_KW: False})
        # A big dense float array: check_array's pass over every entry for NaN / inf (0.16 s on the 4.3 GB of BASELINE
        # configs[2], a third of a 50-iteration fit) is left to the device pack, which reads every entry anyway and counts
        # the ones that are not finite or out of range; if it finds any, `_finite_or_binary_error` runs sklearn's own check
        # then, so the error raised -- and its wording -- is the reference's, in the reference's order (:83 before :90-91).
        big_dense = (isinstance(X, np.ndarray) and X.dtype == np.float64 and X.ndim == 2 and X.size > (1 << 24))
        kw = {_FINITE_KW: False} if big_dense else {}
        X = check_array(X, accept_sparse="csr", dtype=np.float64, **kw)     # _base.py:83
        if hasattr(X, "toarray") and not keep_sparse:
            X = X.toarray()                                            # :86-87
        return X

    @staticmethod
    def _finite_or_binary_error(X, err):
        """The device pack refused X ("X must be binary": something outside [0, 1] or not finite).  For an input whose
        finite check was left to the device this is where sklearn's check runs: NaN / inf raise ITS error (_base.py:83),
        anything else the reference's ValueError (:90-91)."""
        if isinstance(X, np.ndarray) and X.dtype in (np.float64, np.float32) and "must be binary" in str(err):
            check_array(X, dtype=None)
        raise err

    # -- estimator API ---------------------------------------------------------------------------
    def fit(self, X, y=None, mask=None, eval_mask=None, eval_every=10, patience=0, restore_best=True, holdout=None,
            holdout_seed=None):
        """Fit the factorisation to X (entries in [0, 1]); ``mask`` marks observed entries.

        ``eval_mask`` (dense bool / 0-1 or scipy-sparse, of X's shape): its nonzeros are HELD-OUT entries whose truth X
        holds (0 or 1) -- normally entries ``mask`` leaves out.  They stay on the device as index pairs; every
        ``eval_every`` iterations their Bernoulli log-likelihood under the current factors is summed there, without the
        factors leaving the device.  With ``patience > 0`` the fit ends at the ``patience``-th consecutive
        evaluation that does not improve on the best so far.  New attributes (only when an eval set was given):
        ``eval_iters_`` (iterations the evaluated factors had had; the last one equals ``n_iter_``), ``eval_loglik_`` (mean
        per held-out entry), ``eval_perplexity_`` (``exp(-eval_loglik_)``), ``best_iter_`` and ``stopped_early_``.  With
        ``restore_best`` (the default) ``W_`` and ``components_`` are the factors at ``best_iter_``; ``loss_curve_``,
        ``loss_`` and ``n_iter_`` stay the run's own -- they describe all ``n_iter_`` iterations that were made, not the
        restored factors.  ``n_init > 1`` with an eval set runs the restarts one after the other and keeps, as without
        one, the restart with the lowest final training loss.  Not available with ``n_gpus > 1`` / ``devices``.

        ``holdout`` draws that eval set on the device instead: a fraction ``f`` in (0, 1), or a pair
        ``(lo, hi)``, of the observed entries -- ``mask``, when given, is the pool the split draws from, so entries it leaves
        out (a test set of the caller's own) are never held out -- chosen by a counter-based hash of ``(holdout_seed, entry)``;
        :func:`holdout_mask` gives the same entries as a bool matrix.  They leave the fit and are evaluated exactly as
        ``fit(X, mask=mask & ~held, eval_mask=held, ...)`` would, attribute for attribute and bit for bit, without a mask or
        an index list crossing from the host.  ``holdout_seed`` defaults to ``random_state`` when that is an int, else to a
        fresh draw; every restart of ``n_init > 1`` uses the same split.  Further attributes, only after a ``holdout`` fit:
        ``holdout_seed_``, ``holdout_interval_`` and ``holdout_count_``.  Binary X with a binary (or no) mask only; not
        together with ``eval_mask``, ``n_gpus > 1`` or ``devices``."""
        X = self._validated(X, keep_sparse=True)       # sparse V stays sparse up to the device (the solver decides)
        packed = isinstance(X, PackedBits)
        if isinstance(mask, PackedBits) and mask.shape != tuple(X.shape):
            raise ValueError(f"mask has shape {mask.shape}, X has {tuple(X.shape)}")
        if (packed or isinstance(mask, PackedBits)) and (int(self.n_gpus) != 1 or self.devices is not None):
            raise ValueError("PackedBits input is fitted on one GPU: it does not go with n_gpus > 1 or devices")
        # every error of the eval arguments is raised here, before any device work (the solver makes the pairs again)
        split = holdout_args(holdout, holdout_seed, eval_mask, eval_every, patience, self.n_gpus, self.devices)
        if split is None:
            eval_pairs(X, eval_mask, eval_every, patience, "beta-dir", self.n_gpus, self.devices)
        ev = None if eval_mask is None else dict(eval_mask=eval_mask, eval_every=eval_every, patience=patience,
                                                 restore_best=bool(restore_best))
        if split is not None:
            seed = split[1]
            if seed is None:                            # one split for every restart: random_state itself, else a fresh draw
                rs = self.random_state
                is_int = isinstance(rs, (int, np.integer)) and not isinstance(rs, (bool, np.bool_))
                seed = _hip.sample_seed(int(rs) if is_int else None)
            ev = dict(holdout=split[0], holdout_seed=seed, eval_every=eval_every, patience=patience,
                      restore_best=bool(restore_best))
        if packed:                                      # (bits are binary: nothing to check; `sparse` skips the dense checks)
            return self._fit_validated(X, mask, sparse=True, ev=ev)
        if hasattr(X, "toarray"):
            if X.nnz and (X.data.min() < 0 or X.data.max() > 1):
                raise ValueError("X must be binary")                  # :90-91 on the stored values (zeros are fine)
            return self._fit_validated(X, mask, sparse=True, ev=ev)
        return self._fit_validated(X, mask, sparse=False, ev=ev)

    def _fit_validated(self, X, mask, sparse, ev=None):
        # "X must be binary" (:90-91).  For big inputs the device pack, which sees every entry anyway, raises
        # it (a host-side pass costs 0.3 s on the 4 GB of BASELINE configs[2], more than the upload itself);
        # small inputs -- and any input whose orientation is bad too, to keep the reference's order of
        # errors -- are checked here as the reference does.
        big = sparse or X.size > (1 << 24)
        try:
            orientation = self._normalize_orientation(self.orientation)
        except ValueError:
            big = False
            raise
        finally:
            if not big and not sparse and X.dtype != np.bool_:
                if X.dtype in (np.float64, np.float32) and X.size > (1 << 24):
                    check_array(X, dtype=None)                  # the NaN / inf pass _validated left to the device (:83 comes first)
                if not np.all((X >= 0) & (X <= 1)):
                    raise ValueError("X must be binary") from None
        self.orientation = orientation                                # written back, :95
        n_init = int(self.n_init)
        if n_init < 1:
            raise ValueError("n_init must be >= 1")
        multi = dict(n_gpus=self.n_gpus, devices=self.devices) if (int(self.n_gpus) != 1 or self.devices is not None) else {}
        try:
            return self._run_fit(X, mask, orientation, n_init, multi, ev)
        except ValueError as e:
            self._finite_or_binary_error(X, e)

    def _run_fit(self, X, mask, orientation, n_init, multi, ev=None):
        curve = None
        if n_init > 1 and not self.verbose and not multi and ev is None:
            # restarts share one upload and one library call; small problems run several at a time in one launch
            best, _ = nbmf_mm_restarts(
                X, self.n_components, n_init, max_iter=self.max_iter, tol=self.tol, alpha=self.alpha, beta=self.beta,
                W_init=self.W_init, H_init=self.H_init, mask=mask, random_state=self.random_state, orientation=orientation,
                projection=self._projection(), device=self.device)
            n_init = 0
        else:
            best = None
        for r in range(n_init):
            seed = self.random_state
            if r > 0 and seed is not None:
                seed = seed + r                                       # restarts: consecutive seeds
            this_curve = {}                                           # the held-out curve comes back beside the 5-tuple
            result = nbmf_mm_solver(
                Y=X, n_components=self.n_components, max_iter=self.max_iter, tol=self.tol,
                alpha=self.alpha, beta=self.beta, W_init=self.W_init, H_init=self.H_init, mask=mask,
                random_state=seed, verbose=self.verbose, orientation=orientation,
                projection=self._projection(), device=self.device, **multi,
                **({} if ev is None else dict(ev, _eval_out=this_curve)))
            if best is None or result[2][-1] < best[2][-1]:
                best = result
                curve = None if ev is None else this_curve
        W, H, losses, _, n_iter = best
        self.W_ = W
        self.components_ = H
        self.loss_curve_ = losses
        self.objective_history_ = losses
        self.loss_ = losses[-1] if losses else np.inf
        self.n_iter_ = n_iter
        self.reconstruction_err_ = losses[-1] if losses else np.inf
        for name in ("eval_iters_", "eval_loglik_", "eval_perplexity_", "best_iter_", "stopped_early_", "holdout_seed_",
                     "holdout_interval_", "holdout_count_"):
            if hasattr(self, name):
                delattr(self, name)                                   # present only when an eval set was given
        if curve is not None:
            self.eval_iters_ = np.asarray(curve["iters"], dtype=np.int64)
            self.eval_loglik_ = np.asarray(curve["logliks"], dtype=np.float64) / curve["count"]
            self.eval_perplexity_ = np.exp(-self.eval_loglik_)
            self.best_iter_ = int(curve["best_iter"])
            self.stopped_early_ = bool(curve["stopped_early"])
            if "seed" in curve:                                       # a holdout fit: what names the split
                self.holdout_seed_ = int(curve["seed"])
                self.holdout_interval_ = tuple(curve["interval"])
                self.holdout_count_ = int(curve["count"])
        return self

    def fit_transform(self, X, y=None):
        """Fit and return ``W_`` (no mask argument, as _base.py:145-160)."""
        self.fit(X)
        return self.W_

    def transform(self, X, mask=None):
        """Find W for new rows X with ``components_`` frozen: 50 simplex-factor updates from a
        draw of the global NumPy RNG (_base.py:162-199)."""
        check_is_fitted(self, ["components_"])
        X = self._validated(X, keep_sparse=True)
        self._packed_features(X, mask)
        try:
            return w_only_transform(X, self.components_, mask=mask, n_iter=50, device=self.device)
        except ValueError as e:
            self._finite_or_binary_error(X, e)

    def _packed_features(self, X, mask):
        """The shape checks of packed input to :meth:`transform` / :meth:`score`, without a device: a packed X has the
        model's features, a packed mask X's shape."""
        if isinstance(X, PackedBits) and X.shape[1] != np.shape(self.components_)[1]:
            raise ValueError(f"X has {X.shape[1]} features, the model has {np.shape(self.components_)[1]}")
        if isinstance(mask, PackedBits) and mask.shape != tuple(X.shape):
            raise ValueError(f"mask has shape {mask.shape}, X has {tuple(X.shape)}")

    def inverse_transform(self, W):
        """clip(W @ components_, 0, 1) (_base.py:201-210), on the host; :meth:`predict_proba` is the same on the device,
        whole or at chosen entries."""
        check_is_fitted(self, ["components_"])
        W = check_array(W, dtype=np.float64)
        return np.clip(W @ self.components_, 0.0, 1.0)

    # -- prediction on the device (no reference counterpart beyond inverse_transform) ----------------------------
    def _prediction_factors(self, W):
        check_is_fitted(self, ["components_"])
        H = np.asarray(self.components_, dtype=np.float64)
        if W is None:
            check_is_fitted(self, ["W_"])
            W = self.W_
        W = check_array(W, dtype=np.float64)
        if W.shape[1] != H.shape[0]:
            raise ValueError(f"W has {W.shape[1]} columns, the model has {H.shape[0]} components")
        return W, H

    def predict_proba(self, W=None, rows=None, cols=None):
        """Theta = clip(W @ components_, 0, 1) computed on the GPU, ``W`` defaulting to ``W_``: the dense
        ``(W.shape[0], n_features)`` float64 matrix (``inverse_transform(W)`` to rounding), or, with the integer arrays
        ``rows`` and ``cols``, the 1-D array of ``Theta[rows[t], cols[t]]`` -- only those entries are formed.
        Measured on an MI355X at 65536 x 8192, K = 64 (profiles/predict_on_device.txt): 2^22 pairs in
        4.7 ms against 0.95 s for ``inverse_transform(W)[rows, cols]``; a dense 8192-row slab in 10.1 ms against 116 ms,
        nearly all of it the copy of the result to the host."""
        W, H = self._prediction_factors(W)
        if (rows is None) != (cols is None):
            raise ValueError("rows and cols go together: give both or neither")
        if rows is not None:
            rows, cols = _hip.index_pairs(rows, cols)
        return device_predict(W, H, rows=rows, cols=cols, device=self.device)

    def predict(self, W=None, threshold=0.5, packed=False):
        """The bool matrix ``predict_proba(W) > threshold``, compared on the device: one byte per entry comes back.  With
        ``packed=True`` one BIT per entry comes back: a :class:`PackedBits` of shape ``(W.shape[0], n_features)`` whose
        ``toarray()`` is that bool matrix, an eighth of its host memory."""
        if not isinstance(packed, (bool, np.bool_)):
            raise ValueError(f"packed must be a bool (got {packed!r})")
        W, H = self._prediction_factors(W)
        threshold = float(threshold)
        if np.isnan(threshold):
            raise ValueError("threshold is NaN")
        if packed:
            return device_theta_bits(W, H, threshold=threshold, device=self.device)
        return device_predict(W, H, threshold=threshold, device=self.device)

    def sample(self, W=None, random_state=None, packed=False):
        """One draw ``X_rep ~ Bernoulli(predict_proba(W))`` of the fitted model, made on the device (``W`` defaulting to
        ``W_``): a bool ``(W.shape[0], n_features)`` array, or with ``packed=True`` the :class:`PackedBits` the device
        produced (the dense form is its ``toarray()``), which ``fit``, ``score_samples``, ``theta_histogram`` and
        ``top_n(exclude=)`` take as it is.

        The draw is counter-based: ``X_rep[i, j] = u[i, j] < predict_proba(W)[i, j]`` with
        ``u[i, j] = (splitmix64(seed * 0x100000001B3 + i * n_features + j) >> 11) * 2**-53`` (arithmetic modulo 2**64;
        ``_hip.hash_uniform(W.shape[0], n_features, seed)`` is that matrix, or any entries of it), so any entry can be
        regenerated on the host.  ``random_state``: the seed, an int in ``[0, 2**64)``, or None for one drawn from NumPy's
        global RNG.  The result is deterministic in ``(W, components_, random_state)``; different seeds give independent
        matrices.  An entry with probability 0 is never drawn, one with probability 1 always is.

        Uses: posterior-predictive checks (replicated row and column sums against the data's:
        examples/posterior_predictive.py), a parametric bootstrap -- ``NBMF(...).fit(model.sample(packed=True))`` --, and
        planted benchmark data from known factors."""
        if not isinstance(packed, (bool, np.bool_)):
            raise ValueError(f"packed must be a bool (got {packed!r})")
        seed = _hip.sample_seed(random_state)
        W, H = self._prediction_factors(W)
        bits = device_theta_bits(W, H, seed=seed, device=self.device)
        return bits if packed else bits.toarray()

    def top_n(self, n=10, W=None, exclude=None):
        """The ``n`` most probable features of every row of ``W`` (default ``W_``), ranked on the GPU: ``(cols, scores)``,
        int64 and float64 of shape ``(W.shape[0], n)``.  Row i lists the features by ``predict_proba(W)[i]`` descending,
        ties by ascending feature, and ``scores`` holds exactly those entries of ``predict_proba(W)``.  ``exclude``: a dense
        (bool, uint8 or 0/1 numeric) or scipy-sparse matrix of shape ``(W.shape[0], n_features)`` whose nonzero entries are
        never returned -- ``exclude=X`` means "do not recommend what the row already has".  A row with fewer than ``n``
        features left ends in feature -1 / score NaN.  ``n`` is at most 256.  Only ``n`` entries per row come back from
        the device instead of ``n_features``: measured figures are in DESIGN.md 4.7 (profiles/top_n_on_device.txt)."""
        W, H = self._prediction_factors(W)
        n = _hip.top_n_count(n, name="n")
        exclude = self._entry_matrix(exclude, "exclude", W, H)
        return device_top_n(W, H, n, exclude=exclude, device=self.device)

    # -- similar items within one side of the matrix: the factors as an embedding ------------------------
    def similar_features(self, n=10, features=None, metric="cosine"):
        """The ``n`` features most similar to each of ``features`` (integer indices, any order, repeats allowed; None: every
        feature), ranked on the GPU: ``(idx, scores)``, int64 and float64 of shape ``(len(features), n)``, as
        :meth:`top_n` returns its columns.  A feature's vector is its column of ``components_``.  ``metric``: ``"dot"``;
        ``"cosine"`` (a zero vector scores 0 with everything); or ``"profile"``, the cosine between the features'
        predicted columns of ``W_ @ components_`` (unclipped), which does not count two correlated components as
        unrelated.  Scores descending, ties by ascending index; the queried feature itself is left out by index, so a
        duplicate of it is still returned.  A row with fewer than ``n`` other features ends in -1 / NaN.  ``n`` is at
        most 256 (measured figures in profiles/neighbors_on_device.txt)."""
        W, H = self._prediction_factors(None)
        n = _hip.top_n_count(n, name="n")
        metric = _hip.sim_metric(metric)
        features, _ = _hip.item_query(features, H.shape[1], name="features")
        return device_neighbors(W, H, n, axis=1, metric=metric, query=features, device=self.device)

    def similar_samples(self, n=10, W=None, rows=None, metric="cosine"):
        """The ``n`` rows of ``W`` (default ``W_``; ``transform(X_new)`` for unseen samples) most similar to each of its
        ``rows`` (None: every row), ranked on the GPU: ``(idx, scores)`` of shape ``(len(rows), n)``.  A sample's vector is
        its row of ``W``; ``metric`` as in :meth:`similar_features`, ``"profile"`` comparing the samples' predicted rows
        ``W @ components_``.  The same order, tie rule and treatment of the queried row itself."""
        W, H = self._prediction_factors(W)
        n = _hip.top_n_count(n, name="n")
        metric = _hip.sim_metric(metric)
        rows, _ = _hip.item_query(rows, W.shape[0], name="rows")
        return device_neighbors(W, H, n, axis=0, metric=metric, query=rows, device=self.device)

    # -- the global questions: the best entries of the whole matrix as (row, feature) pairs ----------------
    def top_pairs(self, n=100, W=None, exclude=None):
        """The ``n`` most probable entries of ``predict_proba(W)`` over the WHOLE matrix (``W`` defaulting to ``W_``) that
        ``exclude`` does not mark, selected on the GPU: ``(rows, cols, scores)``, int64, int64 and float64, each
        ``min(n, eligible entries)`` long, ordered by score descending, then row, then feature; ``scores`` holds exactly
        those entries of ``predict_proba(W)``.  ``exclude`` as in :meth:`top_n` (dense bool / uint8 / 0-1 numeric,
        :class:`PackedBits` or scipy-sparse; nonzero = never returned): ``exclude=X`` is the link-prediction query -- which
        missing links are the most probable?  ``n`` is at most 2**22.  Unlike :meth:`top_n` this is one list, not one per
        row, and it is not bounded by 256 slots a row; only ``n`` pairs leave the device and no Theta panel is ever stored
        (DESIGN.md 4.15).  A sparse ``exclude`` goes up as packed bits, made row block by row block."""
        W, H = self._prediction_factors(W)
        n = _hip.top_pairs_count(n, name="n")
        exclude = self._entry_matrix(exclude, "exclude", W, H)
        return device_top_pairs(W, H, n, "theta", x=exclude, device=self.device)

    def least_likely(self, X, mask=None, n=100, W=None):
        """The ``n`` observed entries of the binary ``X`` to which the model gives the LOWEST probability, worst first,
        selected on the GPU: ``(rows, cols, prob)`` with ``prob = predict_proba(W)`` where ``X`` is 1 and
        ``1 - predict_proba(W)`` where it is 0, ordered by ``prob`` ascending, then row, then feature.  These are the
        suspect cells of a data set: recorded presences the model does not believe and recorded absences it expects to be
        presences.  ``X`` and ``mask`` as in :meth:`theta_histogram` (``X`` exactly 0 / 1: dense bool / uint8 / numeric,
        :class:`PackedBits` or scipy-sparse; ``mask`` nonzero = observed, None: every entry); ``n`` is at most 2**22
        (DESIGN.md 4.15)."""
        W, H = self._prediction_factors(W)
        n = _hip.top_pairs_count(n, name="n")
        X, mask = self._scored_inputs(X, mask, W, H, exact=True)
        return device_top_pairs(W, H, n, "likelihood", x=X, mask=mask, device=self.device)

    @staticmethod
    def _entry_matrix(a, name, W, H):
        """A matrix that marks entries of ``predict_proba(W)`` by its nonzeros (the ``exclude`` of :meth:`top_n`, the
        ``targets`` of :meth:`rank_of`), validated without a device: dense (an ndarray is made of it) or scipy-sparse, of
        a bool or numeric dtype and of shape ``(W.shape[0], n_features)``.  None passes through."""
        if a is None:
            return None
        want = (W.shape[0], H.shape[1])
        if isinstance(a, PackedBits):
            if name == "targets":
                raise ValueError("targets as PackedBits is not supported: pass them dense or scipy-sparse "
                                 "(exclude may be packed)")
            if a.shape != want:
                raise ValueError(f"{name} has shape {a.shape}, the request describes {want}")
            return a
        if not hasattr(a, "toarray"):
            a = np.asarray(a)
        if a.dtype != np.bool_ and not np.issubdtype(a.dtype, np.number):
            raise ValueError(f"{name} must be a bool or numeric matrix (got dtype {a.dtype})")
        want = (W.shape[0], H.shape[1])
        if a.ndim != 2 or tuple(a.shape) != want:
            raise ValueError(f"{name} has shape {tuple(a.shape)}, the request describes {want}")
        return a

    # -- how good the ranking is: where held-out entries stand in top_n's order ----------------------------
    def rank_of(self, targets, W=None, exclude=None):
        """Where the entries marked by ``targets`` stand in the order :meth:`top_n` ranks their row by, counted on the GPU:
        a :class:`~nbmf_mm_amd._metrics.Ranks` ``(rows, cols, rank, score, above, tied, eligible)``.  ``targets``: a dense
        (bool or numeric) or scipy-sparse matrix of shape ``(W.shape[0], n_features)`` whose nonzero entries are the ones
        to rank; ``rows`` / ``cols`` list them row by row, columns ascending.  ``exclude`` as in :meth:`top_n`.  Over the
        ELIGIBLE features of its row (not excluded; ``eligible`` counts them per row), a target has ``above`` features
        with a larger ``predict_proba(W)``, ``tied`` others with an equal one, and ``rank = above +`` the tied features
        left of it: 0-based, exactly the slot :meth:`top_n` would show it in (``top_n(n, exclude=...)[0][i, rank] == col``
        wherever ``rank < n``), but at any depth, not only the first 256.  ``score`` is the target's entry of
        ``predict_proba(W)``.  A target that is itself excluded gets -1 / -1 / -1 and its score.  HELD-OUT USE:
        ``fit(X_train)``, then ``rank_of(X_heldout, exclude=X_train)`` -- where do the ones the fit never saw land among
        what the row does not have yet?  :meth:`ranking_metrics` turns the answer into recall@k, NDCG@k, MRR, mean
        percentile rank and per-row AUC.  The cost of a row is one pass over its features per 8 targets, and a few integers
        per target leave the device instead of the row."""
        W, H = self._prediction_factors(W)
        targets = self._entry_matrix(targets, "targets", W, H)
        if targets is None:
            raise ValueError("targets must be a matrix whose nonzero entries are the ones to rank (got None)")
        exclude = self._entry_matrix(exclude, "exclude", W, H)
        m = W.shape[0]
        if hasattr(targets, "toarray"):                       # canonical CSR: no stored zeros, no repeats, columns ascending
            t = (targets != 0).tocsr()
            t.sum_duplicates()
            t.eliminate_zeros()
            t.sort_indices()
            indptr, cols = t.indptr, t.indices
            rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(indptr))
        else:
            rows, cols = np.nonzero(targets)                  # row by row, columns ascending
            indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=m))))
        indptr, indices = _hip.csr_targets(indptr, cols, m, H.shape[1])
        rank, above, tied, score, eligible = device_rank_of(W, H, (indptr, indices), exclude=exclude, device=self.device)
        return _metrics.Ranks(np.asarray(rows, dtype=np.int64), indices.astype(np.int64), rank, score, above, tied, eligible)

    def ranking_metrics(self, X_heldout, exclude=None, W=None, k=10):
        """The ranking metrics of the held-out entries ``X_heldout`` (its nonzeros, as the ``targets`` of :meth:`rank_of`)
        under ``predict_proba(W)``: the dict of ``_metrics.ranking_from_ranks`` -- ``rows_scored``, ``hit_rate@k``,
        ``recall@k``, ``precision@k``, ``ndcg@k``, ``mrr``, ``mean_percentile_rank`` and ``auc`` (the mean per-row ROC AUC).
        HELD-OUT USE: ``fit(X_train)``, then ``ranking_metrics(X_heldout, exclude=X_train)``: the entries the fit saw are
        left out of every ranking, as ``top_n(exclude=X_train)`` leaves them out of the recommendations.  The ``@k``
        metrics and ``mrr`` judge the list :meth:`top_n` would show (ties go to the lower feature); ``auc`` and
        ``mean_percentile_rank`` count a tie one half.  ``k`` is any positive integer -- it is not bounded by the 256 slots
        of :meth:`top_n`.  Rows without an eligible held-out entry enter no mean."""
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"k must be a positive integer (got {k!r})")
        return _metrics.ranking_from_ranks(self.rank_of(X_heldout, W=W, exclude=exclude), k=int(k))

    def impute(self, X, mask):
        """A float64 copy of ``X`` in which every entry with ``mask == 0`` is replaced by ``predict_proba`` at exactly
        that position (``W_``, so ``X`` is the fitted matrix or one of its shape); observed entries are returned as given."""
        check_is_fitted(self, ["components_", "W_"])
        if mask is None:
            raise ValueError("impute needs the mask that marks the observed entries")
        if isinstance(X, PackedBits) or isinstance(mask, PackedBits):
            raise ValueError("impute does not take PackedBits input: its result is a dense float64 matrix (pass toarray())")
        X = self._validated(X)
        want = (np.shape(self.W_)[0], np.shape(self.components_)[1])
        if X.shape != want:
            raise ValueError(f"X has shape {X.shape}, the fitted model describes {want}")
        if hasattr(mask, "toarray"):
            mask = mask.toarray()
        mask = np.asarray(mask)
        if mask.shape != X.shape:
            mask = np.broadcast_to(mask, X.shape)              # as fit's Y * mask does
        out = np.array(X, dtype=np.float64)
        rows, cols = np.nonzero(mask == 0)
        if rows.size:
            out[rows, cols] = self.predict_proba(rows=rows, cols=cols)
        return out

    def score(self, X, mask=None):
        """Mean log-likelihood per observed entry of the reconstruction (_base.py:212-247).
        As in the reference the inner ``transform`` is called WITHOUT the mask (:235)."""
        check_is_fitted(self, ["components_"])
        X = self._validated(X, keep_sparse=True)
        self._packed_features(X, mask)
        H = np.asarray(self.components_, dtype=np.float64)
        try:
            return device_score(X, H, mask=mask, n_iter=50, device=self.device)
        except ValueError as e:
            self._finite_or_binary_error(X, e)

    def perplexity(self, X, mask=None):
        """exp(-score) (_base.py:249-265)."""
        return np.exp(-self.score(X, mask))

    def _scored_inputs(self, X, mask, W, H, exact=False):
        """``(X, mask)`` of a request that sets Theta = ``predict_proba(W)`` against data (:meth:`score_samples`, the
        histogram methods), validated without a device: X through fit's checks with their errors in fit's order -- shape,
        then sklearn's own NaN / inf error, then "X must be binary" for anything outside [0, 1], with ``exact`` for
        anything but 0 and 1 -- and the mask's dtype and shape."""
        X = self._validated(X, keep_sparse=True)
        want = (W.shape[0], H.shape[1])
        if tuple(X.shape) != want:
            raise ValueError(f"X has shape {tuple(X.shape)}, the request describes {want}")
        inside = (lambda v: (v == 0) | (v == 1)) if exact else (lambda v: (v >= 0) & (v <= 1))
        if isinstance(X, PackedBits):
            pass                                                      # (binary by construction)
        elif hasattr(X, "toarray"):
            if X.nnz and not np.all(inside(X.data)):
                raise ValueError("X must be binary")                  # fit's check of the stored values
        elif X.dtype != np.bool_ and not np.all(inside(X)):
            if X.dtype != np.uint8:
                check_array(X, dtype=None)                            # NaN / inf: sklearn's own error first, as in fit
            raise ValueError("X must be binary")
        if isinstance(mask, PackedBits):
            if mask.shape != want:
                raise ValueError(f"mask has shape {mask.shape}, the request describes {want}")
        elif mask is not None:
            if not hasattr(mask, "toarray"):
                mask = np.asarray(mask)
            if mask.dtype != np.bool_ and not np.issubdtype(mask.dtype, np.number):
                raise ValueError(f"mask must be a bool or numeric matrix (got dtype {mask.dtype})")
            if mask.ndim != 2 or tuple(mask.shape) != want:
                raise ValueError(f"mask has shape {tuple(mask.shape)}, the request describes {want}")
        return X, mask

    def score_samples(self, X, mask=None, W=None, axis=0, return_counts=False):
        """Mean log-likelihood per observed entry of every row of ``X`` (``axis=0``) or of every feature (``axis=1``) under
        ``predict_proba(W)``, summed on the GPU: a float64 1-D array, NaN where nothing is observed; with
        ``return_counts`` also the int64 counts of observed entries, ``(scores, counts)``.  The summand is :meth:`score`'s
        (``x log(theta + 1e-8) + (1 - x) log(1 - theta + 1e-8)``) over observed entries only.  ``W`` defaults to ``W_``
        and ``X`` then has the fitted shape; with ``W`` given (``transform`` the new rows first) ``X`` has ``W.shape[0]``
        rows.  Unlike :meth:`score` nothing here draws from an RNG: the result is a function of the factors and the data.
        ``mask``: dense or scipy-sparse of X's shape, of any numeric dtype: nonzero = observed.  Sparse or float input is
        streamed in row blocks; feature scores of block-streamed input equal the one-call result to rounding, row scores
        bit for bit.  Only rows + features numbers leave the device, and X goes up at one byte per entry when it is
        binary.  Measured on an MI355X at 65536 x 8192, K = 64 (profiles/score_samples_on_device.txt): 8192 rows
        of uint8 data under a 90 % mask, rows and features, in 3.2 ms against 557 ms for ``predict_proba`` plus NumPy; 0.48 ms
        of it is the kernel, the rest mostly the upload of X and mask."""
        W, H = self._prediction_factors(W)
        if axis not in (0, 1) or isinstance(axis, (bool, np.bool_)):
            raise ValueError(f"axis must be 0 (rows) or 1 (features) (got {axis!r})")
        X, mask = self._scored_inputs(X, mask, W, H)
        sums, counts = device_score_samples(W, H, X, mask=mask, axis=int(axis), device=self.device)
        with np.errstate(invalid="ignore", divide="ignore"):
            scores = np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)
        return (scores, counts) if return_counts else scores

    # -- how good the predictions are: class histograms of Theta on the device -----------------------------
    def _theta_hist(self, X, mask, W, bins):
        W, H = self._prediction_factors(W)
        X, mask = self._scored_inputs(X, mask, W, H, exact=True)
        hist, nan_count = device_theta_hist(W, H, X, mask=mask, bins=bins, device=self.device)
        if nan_count.any():
            raise ValueError(f"Theta has NaN entries ({int(nan_count.sum())} of the observed ones): the factors are not finite")
        return hist

    def theta_histogram(self, X, mask=None, W=None, bins=256):
        """The observed entries of the binary ``X``, counted on the GPU by class and by ``predict_proba(W)``:
        ``(hist, edges)``, ``hist`` int64 of shape ``(2, bins)`` -- ``hist[0]`` the observed zeros, ``hist[1]`` the observed
        ones -- and ``edges = np.arange(bins + 1) / bins``.  Bin b holds the Thetas with ``min(int(Theta * bins), bins - 1)
        == b``, that is ``[edges[b], edges[b + 1])``, the last one closed at 1.  ``bins`` is at most 1024.  ``W`` defaults
        to ``W_``; ``X`` and ``mask`` as in :meth:`score_samples` (``mask`` nonzero = counted), except that ``X`` must be
        exactly 0 / 1.  HELD-OUT USE: ``fit(X, mask=train)``, then ``theta_histogram(X, mask=held_out)`` with ``held_out``
        the complement of ``train`` -- the two histograms of the entries the fit never saw, of which :meth:`roc_auc` and
        :meth:`calibration_curve` are functions.  The counts are exact integers: they do not depend on how the input is
        streamed (sparse and float input goes up in row blocks and gives exactly the arrays of dense bool input) or on the
        order the device adds them in.  Raises ``ValueError("Theta has NaN entries ...")`` if any observed Theta is NaN.
        Only ``2 * bins + 2`` integers leave the device, and X goes up at one byte per entry."""
        bins = _hip.hist_bins(bins)
        return self._theta_hist(X, mask, W, bins), np.arange(bins + 1) / bins

    def roc_auc(self, X, mask=None, W=None, bins=1024, return_slack=False):
        """The ROC AUC of ``predict_proba(W)`` as a ranking of the observed ones of ``X`` above its observed zeros, from
        the ``bins``-bin :meth:`theta_histogram`: the AUC of the binned Thetas, ties counted one half
        (``_metrics.auc_from_hist``).  With ``return_slack`` the pair ``(auc, slack)``: the exact AUC of the unbinned
        Thetas lies within ``slack`` of ``auc`` (half the share of (zero, one) pairs that fall into one bin).  NaN where
        a class has no observed entry.  HELD-OUT USE: ``fit(X, mask=train)``, then ``roc_auc(X, mask=held_out)``.  No
        score leaves the device and nothing is sorted: the cost is :meth:`theta_histogram`'s."""
        bins = _hip.hist_bins(bins)
        auc, slack = _metrics.auc_from_hist(self._theta_hist(X, mask, W, bins))
        return (auc, slack) if return_slack else auc

    def calibration_curve(self, X, mask=None, W=None, n_bins=10, resolution=100):
        """``(prob_true, prob_pred, counts)`` over ``n_bins`` equal-width bins of [0, 1]: the share of ones among the
        observed entries whose ``predict_proba(W)`` lies in the bin, their mean predicted probability, and how many they
        are (int64) -- is a predicted 0.3 a one 30 % of the time?  From a :meth:`theta_histogram` of ``n_bins *
        resolution`` fine bins (at most 1024: ``ValueError`` beyond), ``resolution`` fine bins per coarse one
        (``_metrics.calibration_from_hist``): ``counts`` and ``prob_true`` are exact, ``prob_pred`` is within
        ``1 / (2 n_bins resolution)`` of the bin's true mean.  Bin q is ``[q / n_bins, (q + 1) / n_bins)``, the last one
        closed at 1; NaN where a bin is empty.  HELD-OUT USE: ``fit(X, mask=train)``, then
        ``calibration_curve(X, mask=held_out)``."""
        n_bins = _hip.hist_bins(n_bins, name="n_bins")
        resolution = _hip.hist_bins(resolution, name="resolution")
        if n_bins * resolution > _hip.HIST_MAX_BINS:
            raise ValueError(f"n_bins * resolution must be at most {_hip.HIST_MAX_BINS} (got {n_bins} * {resolution})")
        return _metrics.calibration_from_hist(self._theta_hist(X, mask, W, n_bins * resolution), n_bins)

    # -- does the model reproduce the marginals: expected against observed counts on the device -----------
    def expected_counts(self, X, mask=None, W=None, feature_groups=None, sample_groups=None):
        """How many ones ``predict_proba(W)`` expects among the observed entries of the binary ``X`` -- per sample and
        feature group, and per feature -- next to how many there are, summed on the GPU: ``(by_sample, by_feature)``, two
        :class:`~nbmf_mm_amd.Moments`.  ``by_sample`` has shape ``(n_samples, n_feature_groups)``, or with
        ``sample_groups`` ``(n_sample_groups, n_feature_groups)``; ``by_feature`` has shape ``(n_features,)``.  Each holds
        the exact integer sums ``n_obs``, ``n_ones``, ``s1``, ``s2``, ``s1_ones`` of its slots and, as float64 properties,
        ``expected`` (the expected number of ones), ``variance``, ``z = (n_ones - expected) / sqrt(variance)``,
        ``mean_theta``, ``brier`` and ``tjur`` (the mean probability of the ones less that of the zeros).  This is the
        degree / popularity check of a posterior-predictive check without drawing replicates, calibration by segment (is
        a user segment over-predicted on an item category?), and observed-against-expected enrichment of a feature set
        in a sample.  ``feature_groups`` / ``sample_groups``: integer 1-D arrays with one label ``>= -1`` per feature /
        sample, ``n_*_groups = max label + 1``; None: one group of all features / every sample its own slot.  A feature
        labelled -1 is in no column of ``by_sample`` and still has its entry of ``by_feature``; a sample labelled -1
        counts nowhere, ``by_feature`` included (its mask is dropped on the host, one row block at a time, before the
        block goes to the device).  ``X``, ``mask`` and ``W`` as in :meth:`theta_histogram`.  HELD-OUT USE:
        ``fit(X, mask=train)``, then ``expected_counts(X, mask=held_out, ...)`` with ``held_out`` the complement of
        ``train``: the counts over the entries the fit never saw.  The sums are exact integers: they do not depend on how
        the input is streamed or grouped, or on the order the device adds in; more than 16 feature groups take one pass
        over the matrix per 16.  Raises ``ValueError("Theta has NaN entries ...")`` if any observed Theta is NaN.  Only
        ``5 (n_samples * n_feature_groups + n_features)`` integers leave the device."""
        W, H = self._prediction_factors(W)
        X, mask = self._scored_inputs(X, mask, W, H, exact=True)
        flabels, n_fgroups = _hip.group_labels(feature_groups, H.shape[1], name="feature_groups")
        keep = None
        if sample_groups is not None:
            slabels, n_sgroups = _hip.group_labels(sample_groups, W.shape[0], name="sample_groups")
            keep = slabels >= 0
        row_tab, col_tab, nan_count = device_moments(W, H, X, mask=mask, groups=None if feature_groups is None else flabels,
                                                     n_groups=n_fgroups, keep_rows=keep, device=self.device)
        if nan_count.any():
            raise ValueError(f"Theta has NaN entries ({int(nan_count.sum())} of the observed ones): the factors are not finite")
        by_sample = _metrics.Moments.from_table(row_tab)
        if sample_groups is not None:
            by_sample = by_sample.grouped(slabels, n_sgroups)
        return by_sample, _metrics.Moments.from_table(col_tab)


# alias kept for backwards compatibility (_base.py:269)
NBMF = NBMFMM


def holdout_mask(shape, seed, holdout, mask=None, rows=None, cols=None):
    """The entries ``fit(X, mask=mask, holdout=holdout, holdout_seed=seed)`` holds out, as a bool matrix of X's ``shape``
    (the same under both orientations): what to hand to ``roc_auc(X, mask=...)``, ``score_samples`` or ``rank_of``
    afterwards, with ``seed = model.holdout_seed_`` and ``holdout = model.holdout_interval_``.  ``holdout`` is a fraction or
    a pair as in ``fit`` (``_hip.holdout_interval``); ``mask`` the pool the split drew from (``None``: every entry).  Computed
    on the host from the counter-based rule (``_hip.holdout_reference``).  Entries are hashed independently, so with index
    arrays ``rows`` / ``cols`` -- the row slicing of ``hash_uniform`` -- the sub-matrix ``[rows][:, cols]`` costs only its own
    size (``mask`` is then that sub-matrix's): a large shape is affordable one row block at a time."""
    lo, hi = _hip.holdout_interval(holdout)
    return _hip.holdout_reference(shape, seed, lo, hi, mask=mask, rows=rows, cols=cols)
