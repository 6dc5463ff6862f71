#!/usr/bin/env python3
"""Prediction on the device against the host routes it replaces, at the headline shape (65536 x 8192, K = 64): seeded
random factors, no data upload.  One command, one machine, every leg warmed once, median of five, wall time around calls
that end in a synchronise (the library's predict calls do; NumPy's are synchronous).

  (a) Theta at 2^22 seeded random index pairs: Context.predict_at against the cheapest host route (a gathered einsum over
      W[rows] and H[:, cols]) and against the only route the estimator had before (inverse_transform(W)[rows, cols]: the
      whole 69 GFLOP product and its 4.3 GB array);
  (b) Theta for 8192 rows, as float64 and as bytes (> 0.5): Context.predict_rows against np.clip(W[:8192] @ H, 0, 1);
  (c) the top N columns of each of those 8192 rows, N = 10 and 100, with and without a 10 %-dense exclude:
      Context.top_n against the best route there was before it (predict_rows float64, then np.argpartition and a sort of
      the N on the host) and against the pure host route (clip(W @ H), then the same selection);
  (d) the log-likelihood per row and per column of those rows: Context.score_rows against predict_rows plus NumPy;
  (e) the class histograms of Theta over those rows (uint8 data, 90 % mask): Context.theta_hist at 256, 1024 and 1 bins and
      without a mask, against predict_rows float64 plus np.bincount per class, and -- what the histograms are for --
      against sklearn.metrics.roc_auc_score on the slab.  Once with the tool's factors (K = 64 uniform factors: Theta lies
      in [0.37, 0.63], a few bins that every wave hits) and once with factors that spread Theta over [0, 1];
  (f) where held-out entries of those rows stand in top_n's order: Context.rank_of with 10 targets per row under a
      10 %-dense exclude and with 100 targets per row, against predict_rows float64 plus NumPy rank counting (compares of
      the whole slab per target slot, or one sort of every row and binary searches, whichever is faster), with top_n(10)
      under the same exclude beside it for orientation;
  (g) the held-out log-likelihood during a fit (``eval_curve``): real dense data this time -- X at 25 % ones, 90 % of the
      entries observed by the fit, the unobserved 10 % (and the 1 % of them with the largest draw) held out as index
      pairs -- Context.eval_loglik on the training context against the route there was before it (get_factors, then
      set_factors into a second context that holds the data under the dense held-out mask, then loglik_strict), and a
      50-iteration fit with an evaluation every 10 iterations against the same fit without an eval set;
  (h) the calls that upload binary operands, from bit-packed ones (``PackedBits``: one bit per entry over PCIe, unpacked on
      the device) beside the same call from uint8 -- ``score_samples_bits`` (rows and columns, 90 % mask), ``theta_hist_bits``
      (256 bins, the same data and mask) and ``top_n_bits`` (N = 10, a 10 %-dense exclude) -- on one set of data of the legs'
      own stream, the packed result checked for equality with the uint8 one before any time is taken;
  (i) decisions per entry of those rows leaving the device as bits (``Context.theta_bits``): ``predict_bits`` -- Theta > 0.5
      as a ``PackedBits`` beside the thresholded bytes of (b) in the same process, the two differing in the bytes that cross
      PCIe (1/8) -- and ``sample`` -- one draw of Bernoulli(Theta) against the host route there was before it
      (predict_rows float64, ``default_rng().random(...) <``, ``np.packbits``).  The bits are checked for equality with
      np.packbits of the byte slab, and with ``hash_uniform < `` the device's own float64 slab, before any time is taken;
  (j) the held-out split drawn on the device (``hold_out``): the data of (g) under its 90 % mask; ``Context.hold_out`` of 1 %
      and of 10 % of the observed entries and ``Context.hold_out_undo``, median of five each, against the host route they
      replace, timed once, stage by stage: ``rng.random(shape)``, the two comparisons, ``eval_pairs`` (np.nonzero and
      np.lexsort), ``set_eval`` and the upload under the train mask.  The device's list is compared for equality with the
      host's pairs of the same entries (``holdout_reference``) before any time is taken;
  (k) the best entries of the WHOLE matrix as (row, column) pairs (``top_pairs``; runs alone, all m rows): Context.top_pairs at
      N = 100, 10^3, 10^5 and 2^22, plain and under a 10 %-dense exclude given as bytes and as bits, and the 10^4 least likely
      observed entries of uint8 data under a 90 % mask -- against the host route there was before it, timed once: predict_rows
      slab by slab, np.argpartition of every slab, a merge and a sort; for N <= 256 also top_n(N) on every row plus a host
      merge.  The device result is compared for equality with the host selection over the device's own slabs before any
      time is taken; the digit passes and the device memory of every request are the library's own report (NBMF_PAIRS_TRACE).
  (l) the items most similar to given items within one side of the matrix (``neighbors``; runs alone): Context.neighbors for
      all 8192 features against the 8192 features, and for 8192 query samples (a seeded list) against all 65536 samples, at
      N = 10 and N = 100 under each of the three metrics, median of five after a warm-up -- against the host route, timed once
      in the same process: NumPy normalisation of the factor (for "profile" the Gram matrix and the two scaled operands),
      ``A[:, query].T @ B``, the query's own column removed, np.argpartition and a sort of the N.  Before any time is taken
      the device result is compared for EQUALITY with ``host_neighbors`` over the device's own slab (Context.similarity).
  (m) expected counts by (row, feature group) and by feature over those rows (``moments``): the rows, data and 90 % mask of
      (e); Context.moments, both tables, with one group, with 16 groups in contiguous runs and with 16 groups drawn at
      random (the unfavourable layout: every wave flushes all 16 slots of each of its rows), from uint8 and from packed
      bits, with and without the mask -- against the host route there was before it (predict_rows float64, then the five
      sums per slot in float64 NumPy: masked copies and matrix products with the one-hot group matrix), and beside
      Context.theta_hist at 1024 bins on the same operands in the same process.  The tables are compared for EQUALITY with
      the integer contract in NumPy over the device's own slab before any time is taken.

The host legs are the comparison; the device path is never its own yardstick.  Before any time is taken the device and host
results are compared at these sizes within tests/test_gpu_predict.py's bound, 2.1 K 2^-53 (|W| @ |H|) per entry; the
ranking is compared exactly with the host selection over the device's own slab (the shape has no ties); the score sums are
compared with the host's over the device's own slab within tests/test_gpu_score_samples.py's bound plus NumPy's own
summation error; the class histograms and the ranks are compared for EQUALITY with NumPy's over the device's own slab.
``--legs`` picks the legs to time (default: the first four; ``theta_hist``, ``moments``, ``rank_of``, ``eval_curve`` and the ``*_bits`` legs are
asked for by name, as are ``predict_bits`` and ``sample``; ``eval_curve`` alone, or ``hold_out`` alone, skips the factors-only
context and its agreement checks).
Prints progress lines and, last, ONE JSON line.  Needs an MI355X: there is no CPU fallback."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from nbmf_mm_amd import _hip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--m", type=int, default=65536)
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--pairs", type=int, default=1 << 22)
ap.add_argument("--rows", type=int, default=8192)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--legs", default="pairs,slabs,top_n,score_samples",
                help="comma-separated: pairs, slabs, top_n, score_samples, theta_hist, rank_of, eval_curve, score_samples_bits, "
                     "theta_hist_bits, top_n_bits, predict_bits, sample, hold_out, top_pairs, neighbors, moments")
ap.add_argument("--device-only", action="store_true",
                help="theta_hist, moments, rank_of, predict_bits, sample: skip the timed host legs (for a kernel trace of the device legs)")
args = ap.parse_args()
legs = set(args.legs.split(","))
BITS_LEGS = {"score_samples_bits", "theta_hist_bits", "top_n_bits"}
DECISION_LEGS = {"predict_bits", "sample"}
assert legs <= {"pairs", "slabs", "top_n", "score_samples", "theta_hist", "rank_of", "eval_curve", "hold_out", "top_pairs", "neighbors", "moments"} | BITS_LEGS | DECISION_LEGS, f"unknown leg in {args.legs}"
m, n, k, P, R = args.m, args.n, args.k, args.pairs, min(args.rows, args.m)


def median_s(fn):
    fn()                                                    # warm-up: code objects, pools, page faults of the outputs
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), [round(t, 6) for t in ts]


def say(*a):
    print(*a, flush=True)


def eval_curve_leg():
    """(g): see the module docstring.  Its own data and contexts; the agreement of the two routes is printed and held to
    1e-9 relative (the second context's sweep uses the table logarithm and another order of the products)."""
    ge = np.random.default_rng(2027)
    X = ge.random((m, n), dtype=np.float32) < 0.25
    u = ge.random((m, n), dtype=np.float32)
    train_mask = u < 0.90
    W0 = ge.uniform(0.1, 0.9, (k, m))
    W0 /= W0.sum(0, keepdims=True)
    H0 = ge.uniform(0.1, 0.9, (k, n))
    h = {"observed_by_the_fit": float(train_mask.mean()), "fit_iterations": 50, "every": 10}
    with _hip.Context(m, n, k) as train:
        train.set_hyper(1.2, 1.2, 1e-8)
        train.upload(X, mask=train_mask)
        del train_mask

        def fit():
            train.set_factors(W0, H0)
            return train.run(50, 0.0)

        h["fit_plain_s"], h["fit_plain_all_s"] = median_s(fit)
        say("50-iteration fit, no eval set", h["fit_plain_s"])
        plain_losses = fit()[0]
        for name, lo in (("1pct", 0.99), ("10pct", 0.90)):
            ev = u >= lo
            r, c = np.nonzero(ev)
            x = X[r, c]
            t = {"pairs": int(r.size), "share": float(r.size) / (m * n), "resident_bytes": 9 * int(r.size),
                 "gathered_factor_bytes": 2 * k * 8 * int(r.size)}
            with _hip.Context(m, n, k) as second:
                second.set_hyper(1.2, 1.2, 1e-8)
                second.upload(X, mask=ev)
                del ev
                assert second.n_obs() == r.size

                def second_context_route():
                    Wf, Hf = train.get_factors()
                    second.set_factors(Wf, Hf)
                    return second.loglik_strict()

                t0 = time.perf_counter()
                train.set_eval(r, c, x, every=10, patience=0)
                t["set_eval_s"] = time.perf_counter() - t0
                a, b = train.eval_loglik(), second_context_route()
                t["eval_loglik"], t["second_context_loglik_strict"] = a, b
                t["relative_difference"] = abs(a - b) / abs(b)
                assert t["relative_difference"] <= 1e-9, f"eval_loglik {a!r} against the second context's {b!r}"
                t["eval_loglik_s"], t["eval_loglik_all_s"] = median_s(train.eval_loglik)
                say(f"{name}: eval_loglik {t['eval_loglik_s']:.6f} s ({t['pairs']} pairs)")
                t["second_context_route_s"], t["second_context_route_all_s"] = median_s(second_context_route)
                say(f"{name}: get_factors -> set_factors -> loglik_strict {t['second_context_route_s']:.6f} s")
                t["eval_gathered_GBps"] = t["gathered_factor_bytes"] / t["eval_loglik_s"] / 1e9
                t["speedup_vs_second_context"] = t["second_context_route_s"] / t["eval_loglik_s"]
                t["device_wins"] = bool(t["eval_loglik_s"] < t["second_context_route_s"])
            t["fit_with_eval_s"], t["fit_with_eval_all_s"] = median_s(fit)
            losses = fit()[0]
            assert np.array_equal(losses, plain_losses), "the eval set changed the losses of the fit"
            t["evaluations_per_fit"] = int(train.eval_curve()[0].size)
            t["fit_overhead"] = t["fit_with_eval_s"] / h["fit_plain_s"] - 1.0
            say(f"{name}: 50-iteration fit with every = 10: {t['fit_with_eval_s']:.6f} s ({100 * t['fit_overhead']:+.2f} %)")
            train.set_eval(r[:0], c[:0], x[:0])
            h[name] = t
    return h


def hold_out_leg():
    """(j): see the module docstring.  Its own data and context; ``--device-only`` skips the host route (for a kernel trace)."""
    from nbmf_mm_amd._solver import eval_pairs
    gh = np.random.default_rng(2029)
    X = gh.random((m, n), dtype=np.float32) < 0.25
    mask = gh.random((m, n), dtype=np.float32) < 0.90
    image = ((m + 127) // 128 * 128) * ((n + 127) // 128 * 128)            # bytes of one code image
    h = {"observed": int(mask.sum()), "image_bytes": image}
    with _hip.Context(m, n, k) as ctx:
        ctx.set_hyper(1.2, 1.2, 1e-8)
        t0 = time.perf_counter()
        ctx.upload(X, mask=mask)
        h["upload_s"] = time.perf_counter() - t0
        for name, f in (("1pct", 0.01), ("10pct", 0.10)):
            t = {"fraction": f}
            # equality first: the device's list against the host's pairs of the entries the rule names (row blocks: 8 bytes per entry)
            count = ctx.hold_out(11, 0.0, f)
            rows, cols, x = ctx.eval_pairs()
            at = 0
            for r0 in range(0, m, 4096):
                r1 = min(m, r0 + 4096)
                held = _hip.holdout_reference((m, n), 11, 0.0, f, mask=mask[r0:r1], rows=np.arange(r0, r1))
                r, c = np.nonzero(held)
                assert np.array_equal(rows[at:at + r.size], r + r0) and np.array_equal(cols[at:at + r.size], c), "list differs"
                assert np.array_equal(x[at:at + r.size], X[r0:r1][r, c]), "truth differs"
                at += r.size
            assert at == count == rows.size and ctx.n_obs() == h["observed"] - count
            ctx.hold_out_undo()
            assert ctx.n_obs() == h["observed"]
            del rows, cols, x
            t["pairs"] = int(count)
            outs, undos = [], []
            for _ in range(args.reps + 1):                      # (the first round is the warm-up)
                t0 = time.perf_counter()
                ctx.hold_out(11, 0.0, f)
                t1 = time.perf_counter()
                ctx.hold_out_undo()
                t2 = time.perf_counter()
                outs.append(t1 - t0)
                undos.append(t2 - t1)
            t["hold_out_s"], t["hold_out_all_s"] = float(np.median(outs[1:])), [round(v, 6) for v in outs[1:]]
            t["undo_s"], t["undo_all_s"] = float(np.median(undos[1:])), [round(v, 6) for v in undos[1:]]
            # what the call moves: image B read by the count, the scatter and the row counts, both images read and a quarter
            # of each written by the lane masks; 9 bytes listed and 2 bytes cleared per pair
            t["hold_out_bytes"] = int(5.5 * image + 11 * count)
            t["hold_out_GBps"] = t["hold_out_bytes"] / t["hold_out_s"] / 1e9
            t["undo_bytes"] = int(3.5 * image + 11 * count)
            t["undo_GBps"] = t["undo_bytes"] / t["undo_s"] / 1e9
            say(f"{name}: hold_out {t['hold_out_s']:.6f} s ({t['hold_out_GBps']:.0f} GB/s), undo {t['undo_s']:.6f} s "
                f"({t['undo_GBps']:.0f} GB/s), {count} pairs")
            if not args.device_only:
                host = {}
                t0 = time.perf_counter()
                u = np.random.default_rng(11).random((m, n))
                host["rng_random_s"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                held = mask & (u < f)
                train = mask & ~held
                host["comparisons_s"] = time.perf_counter() - t0
                del u
                t0 = time.perf_counter()
                pairs = eval_pairs(X, held, 10, 0)
                host["eval_pairs_s"] = time.perf_counter() - t0
                del held
                t0 = time.perf_counter()
                ctx.upload(X, mask=train)
                host["upload_train_mask_s"] = time.perf_counter() - t0
                t0 = time.perf_counter()
                ctx.set_eval(*pairs, every=10, patience=0)
                host["set_eval_s"] = time.perf_counter() - t0
                host["pairs"] = int(pairs[0].size)
                host["total_s"] = sum(v for key, v in host.items() if key.endswith("_s"))
                say(f"{name}: host route {host}")
                ctx.set_eval(pairs[0][:0], pairs[1][:0], pairs[2][:0])
                del pairs, train
                ctx.upload(X, mask=mask)                        # the next split starts from the full pool again
                t["host_route"] = host
                t["speedup_vs_host_route"] = host["total_s"] / t["hold_out_s"]
            h[name] = t
    return h


def top_pairs_leg():
    """(k): see the module docstring.  Its own factors-only context; ``--device-only`` skips the host routes (for a kernel trace)."""
    import tempfile
    from nbmf_mm_amd import PackedBits
    gp = np.random.default_rng(2030)
    W = gp.uniform(0.1, 0.9, (m, k))
    W /= W.sum(1, keepdims=True)
    H = gp.uniform(0.05, 0.95, (k, n))
    excl = gp.random((m, n), dtype=np.float32) < 0.10
    X = gp.random((m, n), dtype=np.float32) < 0.25
    mask = gp.random((m, n), dtype=np.float32) < 0.90
    pexcl = PackedBits.from_dense(excl)
    slab = np.empty((R, n))

    def traced(call):
        """The call's result and the library's own report of it: digit passes, tie pass, candidates, device bytes."""
        with tempfile.TemporaryFile() as f:
            sys.stderr.flush()
            keep = os.dup(2)
            os.dup2(f.fileno(), 2)
            os.environ["NBMF_PAIRS_TRACE"] = "1"
            try:
                out = call()
            finally:
                del os.environ["NBMF_PAIRS_TRACE"]
                os.dup2(keep, 2)
                os.close(keep)
            f.seek(0)
            words = f.read().decode().split()
        rep = {key: int(words[words.index(key) + 1]) for key in ("digit_passes", "tie_pass", "collected", "device_bytes")}
        return out, rep

    def host_route(ctx, N, score_of, eligible, largest):
        """predict_rows slab by slab, the N best of every slab by np.argpartition, a merge, and the sort by (score, row, col)."""
        vals, rws, cls = [], [], []
        for r0 in range(0, m, R):
            nr = min(R, m - r0)
            s = score_of(ctx.predict_rows(r0, nr, out=slab[:nr]), r0, nr)
            if eligible is not None:
                s = np.where(eligible[r0:r0 + nr], s, -np.inf if largest else np.inf)
            flat = s.ravel()
            keep = min(N, flat.size)
            part = np.argpartition(flat, flat.size - keep)[flat.size - keep:] if largest else np.argpartition(flat, keep - 1)[:keep]
            vals.append(flat[part])
            rws.append(part // n + r0)
            cls.append(part % n)
        vals, rws, cls = np.concatenate(vals), np.concatenate(rws), np.concatenate(cls)
        live = np.isfinite(vals)
        vals, rws, cls = vals[live], rws[live], cls[live]
        order = np.lexsort((cls, rws, -vals if largest else vals))[:N]
        return rws[order], cls[order], vals[order]

    def top_n_route(ctx, N):
        """top_n(N) of every row on the device, then the merge on the host (N <= 256 only)."""
        c, s = ctx.top_n(N, 0, m)
        rws = np.repeat(np.arange(m), N)
        c, s = c.ravel(), s.ravel()
        part = np.argpartition(s, s.size - N)[s.size - N:]
        order = part[np.lexsort((c[part], rws[part], -s[part]))]
        return rws[order], c[order], s[order]

    h = {"exclude_density": float(excl.mean()), "observed": float(mask.mean())}
    with _hip.Context(m, n, k) as ctx:
        ctx.set_factors(np.ascontiguousarray(W.T), H)
        requests = []
        for N in (100, 1000, 100000, 1 << 22):
            requests.append((f"N{N}_plain", N, lambda N=N: ctx.top_pairs(N), None, None))
            requests.append((f"N{N}_exclude_u8", N, lambda N=N: ctx.top_pairs(N, x=excl), ~excl, None))
            requests.append((f"N{N}_exclude_bits", N, lambda N=N: ctx.top_pairs(N, x=pexcl), ~excl, f"N{N}_exclude_u8"))
        requests.append(("least_likely_N10000", 10000, lambda: ctx.top_pairs(10000, kind="likelihood", x=X, mask=mask), mask, None))
        for name, N, call, eligible, same_as in requests:
            t = {"N": N}
            likelihood = name.startswith("least_likely")
            got, t["report"] = traced(call)
            if same_as is not None:                             # the packed form: the host route is that of the byte form
                t["host_route_s"] = h[same_as].get("host_route_s")
                want = h[same_as].pop("_result")
            elif not args.device_only:
                score_of = (lambda th, r0, nr: np.where(X[r0:r0 + nr], th, 1.0 - th)) if likelihood else (lambda th, r0, nr: th)
                t0 = time.perf_counter()
                want = host_route(ctx, N, score_of, eligible, not likelihood)
                t["host_route_s"] = time.perf_counter() - t0
            else:
                want = got
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), f"top_pairs {name} disagrees with the host selection"
            if name.endswith("_exclude_u8"):
                t["_result"] = want
            t["device_s"], t["device_all_s"] = median_s(call)
            say(f"top_pairs {name}: device {t['device_s']:.6f} s {t['report']}, host route {t.get('host_route_s')}")
            if N <= _hip.TOP_N_MAX and name.endswith("_plain") and not args.device_only:
                assert all(np.array_equal(a, b) for a, b in zip(got, top_n_route(ctx, N))), "top_n + merge disagrees"
                t["top_n_then_merge_s"], t["top_n_then_merge_all_s"] = median_s(lambda: top_n_route(ctx, N))
                say(f"top_pairs {name}: top_n({N}) of every row + host merge {t['top_n_then_merge_s']:.6f} s")
            if t.get("host_route_s") is not None:
                best = min(v for key, v in t.items() if key in ("host_route_s", "top_n_then_merge_s"))
                t["speedup_vs_best_host_route"] = best / t["device_s"]
                t["device_wins"] = bool(t["device_s"] < best)
            h[name] = t
        for t in h.values():
            if isinstance(t, dict):
                t.pop("_result", None)
        wins = [t["device_wins"] for t in h.values() if isinstance(t, dict) and "device_wins" in t]
        if wins:
            h["no_device_leg_loses"] = all(wins)
    return h


def host_neighbors(S, top, self_idx):
    """``host_neighbors`` of tests/test_neighbors_cpu.py -- score descending, ties by ascending index, ``self_idx[t]`` left
    out of row t by index -- for a slab without NaN, a row block at a time: np.argpartition picks the candidates, and a row
    whose ``top``-th score is tied with an entry outside them (the partition is then not the answer) is redone by np.lexsort
    over the whole row."""
    nq, L = S.shape
    top = min(top, L - 1)
    idx = np.empty((nq, top), dtype=np.int64)
    sc = np.empty((nq, top))
    for r0 in range(0, nq, 512):
        blk = np.array(S[r0:r0 + 512])
        ar = np.arange(blk.shape[0])
        blk[ar, self_idx[r0:r0 + 512]] = -np.inf
        cand = np.argpartition(-blk, top - 1, axis=1)[:, :top]
        cs = blk[ar[:, None], cand]
        order = np.lexsort((cand, -cs), axis=1)
        cand, cs = np.take_along_axis(cand, order, 1), np.take_along_axis(cs, order, 1)
        for t in np.nonzero((blk >= cs[:, -1:]).sum(1) != top)[0]:         # a tie across the cut
            full = np.lexsort((np.arange(L), -blk[t]))[:top]
            cand[t], cs[t] = full, blk[t, full]
        idx[r0:r0 + 512], sc[r0:r0 + 512] = cand, cs
    return idx, sc


def neighbors_leg():
    """(l): see the module docstring.  Its own factors-only context; ``--device-only`` skips the host route (for a kernel trace)."""
    gn = np.random.default_rng(2030)
    W = gn.uniform(0.1, 0.9, (k, m))
    W /= W.sum(0, keepdims=True)
    H = gn.uniform(0.05, 0.95, (k, n))
    h = {}

    def host_operands(F, C, metric):
        if metric == "dot":
            return F, F
        if metric == "cosine":
            Un = F / np.sqrt((F * F).sum(0))
            return Un, Un
        B = (C @ C.T) @ F
        root = np.sqrt((F * B).sum(0))
        return F / root, B / root

    def host_route(F, C, metric, query, top):
        A, B = host_operands(F, C, metric)
        S = A[:, query].T @ B
        S[np.arange(query.size), query] = -np.inf                          # the diagonal removed
        cand = np.argpartition(-S, top - 1, axis=1)[:, :top]
        cs = S[np.arange(query.size)[:, None], cand]
        order = np.argsort(-cs, axis=1, kind="stable")
        return np.take_along_axis(cand, order, 1), np.take_along_axis(cs, order, 1)

    with _hip.Context(m, n, k) as ctx:
        ctx.set_factors(W, H)
        for name, axis, F, C in (("features", 1, H, W), ("samples", 0, W, H)):
            L = F.shape[1]
            query = np.arange(L) if L <= R else np.sort(gn.choice(L, R, replace=False))
            e = {"items": int(L), "queries": int(query.size)}
            for metric in ("dot", "cosine", "profile"):
                t = {}
                slab = ctx.similarity(axis=axis, metric=metric, query=query)
                want = host_neighbors(slab, 100, query)
                del slab
                for N in (100, 10):
                    got = ctx.neighbors(N, axis=axis, metric=metric, query=query)
                    assert np.array_equal(got[0], want[0][:, :N]), f"{name} {metric} N = {N}: the ranking differs from the slab's"
                    assert np.array_equal(got[1], want[1][:, :N]), f"{name} {metric} N = {N}: a score differs from the slab's"
                    key = f"n{N}"
                    t[key + "_device_s"], t[key + "_device_all_s"] = median_s(
                        lambda: ctx.neighbors(N, axis=axis, metric=metric, query=query))
                    say(f"neighbors {name} {metric} N = {N}: device {t[key + '_device_s']:.6f} s")
                    if not args.device_only:
                        t0 = time.perf_counter()
                        host = host_route(F, C, metric, query, N)
                        t[key + "_host_s"] = time.perf_counter() - t0
                        t[key + "_host_agrees"] = float(np.mean(host[0] == got[0]))   # (another rounding: near-ties may swap)
                        t[key + "_speedup"] = t[key + "_host_s"] / t[key + "_device_s"]
                        t[key + "_device_wins"] = bool(t[key + "_device_s"] < t[key + "_host_s"])
                        say(f"neighbors {name} {metric} N = {N}: host {t[key + '_host_s']:.6f} s, the same index in "
                            f"{100 * t[key + '_host_agrees']:.4f} % of the slots")
                t["similarity_s"], t["similarity_all_s"] = median_s(lambda: ctx.similarity(axis=axis, metric=metric, query=query))
                say(f"similarity {name} {metric}: device slab to the host {t['similarity_s']:.6f} s")
                e[metric] = t
            h[name] = e
    wins = [v for e in h.values() for t in e.values() if isinstance(t, dict) for key, v in t.items() if key.endswith("_device_wins")]
    if wins:
        h["no_device_leg_loses"] = all(wins)
    return h


if legs == {"neighbors"}:
    res = {"tool": "bench_predict", "library": _hip.source_hash(), "shape": [m, n, k], "reps": args.reps, "slab_rows": R,
           "neighbors_leg": neighbors_leg()}
    print(json.dumps(res))
    sys.exit(0)
assert "neighbors" not in legs, "the neighbors leg runs alone: --legs neighbors"

if legs == {"top_pairs"}:
    res = {"tool": "bench_predict", "library": _hip.source_hash(), "shape": [m, n, k], "reps": args.reps, "slab_rows": R,
           "top_pairs_leg": top_pairs_leg()}
    print(json.dumps(res))
    sys.exit(0)
assert "top_pairs" not in legs, "the top_pairs leg runs alone: --legs top_pairs"

if legs == {"hold_out"}:
    res = {"tool": "bench_predict", "library": _hip.source_hash(), "shape": [m, n, k], "reps": args.reps,
           "hold_out_leg": hold_out_leg()}
    print(json.dumps(res))
    sys.exit(0)
assert "hold_out" not in legs, "the hold_out leg runs alone: --legs hold_out"

if legs == {"eval_curve"}:
    res = {"tool": "bench_predict", "library": _hip.source_hash(), "shape": [m, n, k], "reps": args.reps,
           "eval_curve_leg": eval_curve_leg()}
    print(json.dumps(res))
    sys.exit(0)

g = np.random.default_rng(2024)
W = g.uniform(0.1, 0.9, (m, k))
W /= W.sum(1, keepdims=True)                                # user layout: W (m, k) rows on the simplex, H (k, n) in (0, 1)
H = g.uniform(0.05, 0.95, (k, n))
rows, cols = g.integers(0, m, P), g.integers(0, n, P)
unit = 2.1 * k * 2.0 ** -53                                 # the bound is unit * (|W| @ |H|); the factors are positive

res = {"tool": "bench_predict", "library": _hip.source_hash(), "shape": [m, n, k], "pairs": P, "slab_rows": R, "reps": args.reps}
with _hip.Context(m, n, k) as ctx:
    ctx.set_factors(np.ascontiguousarray(W.T), H)

    # ---- agreement first ----------------------------------------------------------------------------------------------
    def host_einsum():
        return np.clip(np.einsum("pk,kp->p", W[rows], H[:, cols]), 0.0, 1.0)

    def host_parent():
        return np.clip(W @ H, 0.0, 1.0)[rows, cols]         # inverse_transform(W)[rows, cols]

    def host_slab():
        return np.clip(W[:R] @ H, 0.0, 1.0)

    ref_at = host_einsum()
    dev_at = ctx.predict_at(rows, cols)
    worst_at = float(np.max(np.abs(dev_at - ref_at) / (unit * ref_at)))
    assert worst_at <= 1.0, f"predict_at is {worst_at} bounds away from the host product"
    ref_slab = host_slab()
    out64 = np.empty((R, n))
    out8 = np.empty((R, n), dtype=np.bool_)
    ctx.predict_rows(0, R, out=out64)
    worst_rows = float(np.max(np.abs(out64 - ref_slab) / (unit * ref_slab)))
    assert worst_rows <= 1.0, f"predict_rows is {worst_rows} bounds away from the host product"
    ctx.predict_rows(0, R, threshold=0.5, out=out8)
    decided = np.abs(ref_slab - 0.5) > unit * ref_slab      # entries the bound lets either side call
    assert np.array_equal(out8[decided], ref_slab[decided] > 0.5), "the byte slab disagrees with the host product"
    res["agreement"] = {"predict_at_worst_over_bound": worst_at, "predict_rows_worst_over_bound": worst_rows,
                        "byte_entries_within_bound_of_threshold": int(decided.size - decided.sum())}
    say("agreement:", res["agreement"])
    del ref_at, dev_at, decided

    # ---- (a) pairs -------------------------------------------------------------------------------------------------------
    if "pairs" in legs:
        a = {}
        a["device_s"], a["device_all_s"] = median_s(lambda: ctx.predict_at(rows, cols))
        say("predict_at", a["device_s"])
        a["host_einsum_s"], a["host_einsum_all_s"] = median_s(host_einsum)
        say("host einsum", a["host_einsum_s"])
        a["host_inverse_transform_s"], a["host_inverse_transform_all_s"] = median_s(host_parent)
        say("host inverse_transform", a["host_inverse_transform_s"])
        a["gathered_factor_bytes"] = 2 * k * 8 * P
        a["device_gathered_GBps"] = a["gathered_factor_bytes"] / a["device_s"] / 1e9
        a["speedup_vs_einsum"] = a["host_einsum_s"] / a["device_s"]
        a["speedup_vs_inverse_transform"] = a["host_inverse_transform_s"] / a["device_s"]
        res["pairs_leg"] = a

    # ---- (b) slabs -------------------------------------------------------------------------------------------------------
    if "slabs" in legs:
        b = {}
        b["device_f64_s"], b["device_f64_all_s"] = median_s(lambda: ctx.predict_rows(0, R, out=out64))
        say("predict_rows f64", b["device_f64_s"])
        b["device_u8_s"], b["device_u8_all_s"] = median_s(lambda: ctx.predict_rows(0, R, threshold=0.5, out=out8))
        say("predict_rows u8", b["device_u8_s"])
        b["host_f64_s"], b["host_f64_all_s"] = median_s(host_slab)
        say("host slab", b["host_f64_s"])
        b["host_u8_s"], b["host_u8_all_s"] = median_s(lambda: host_slab() > 0.5)
        say("host slab > 0.5", b["host_u8_s"])
        b["f64_output_bytes"], b["u8_output_bytes"] = R * n * 8, R * n
        b["device_f64_output_GBps"] = b["f64_output_bytes"] / b["device_f64_s"] / 1e9
        b["device_u8_output_GBps"] = b["u8_output_bytes"] / b["device_u8_s"] / 1e9
        # The two device legs run the same product and differ in the bytes that cross PCIe (8 against 1 per entry): their
        # difference is the time of 7/8 of the float64 copy.  An estimate derived from two end-to-end times, not a trace.
        copy_s = max(0.0, b["device_f64_s"] - b["device_u8_s"]) * 8.0 / 7.0
        b["f64_pcie_share_estimated"] = min(1.0, copy_s / b["device_f64_s"])
        b["speedup_f64_vs_host"] = b["host_f64_s"] / b["device_f64_s"]
        b["speedup_u8_vs_host"] = b["host_u8_s"] / b["device_u8_s"]
        res["slab_leg"] = b

    # ---- (c) top-N ---------------------------------------------------------------------------------------------------------
    if "top_n" in legs:
        def host_select(theta, N, ex):
            """The N largest of every row, ordered: argpartition, then a sort of the N (theta descending, column ascending)."""
            if ex is not None:
                theta = np.where(ex, -np.inf, theta)
            part = np.argpartition(theta, n - N, axis=1)[:, n - N:]
            vals = np.take_along_axis(theta, part, axis=1)
            order = np.lexsort((part, -vals))
            return np.take_along_axis(part, order, axis=1), np.take_along_axis(vals, order, axis=1)

        excl = g.random((R, n)) < 0.10
        c = {"exclude_density": float(excl.mean())}
        for N in (10, 100):
            for name, ex in (("plain", None), ("exclude", excl)):
                dev_cols, dev_scores = ctx.top_n(N, 0, R, exclude=ex)
                ctx.predict_rows(0, R, out=out64)
                want_cols, want_scores = host_select(out64, N, ex)
                assert np.array_equal(dev_cols, want_cols) and np.array_equal(dev_scores, want_scores), \
                    f"top_n (N = {N}, {name}) disagrees with the host selection over predict_rows"
                t = {}
                t["device_s"], t["device_all_s"] = median_s(lambda: ctx.top_n(N, 0, R, exclude=ex))
                t["predict_rows_then_host_s"], t["predict_rows_then_host_all_s"] = median_s(
                    lambda: host_select(ctx.predict_rows(0, R, out=out64), N, ex))
                t["host_only_s"], t["host_only_all_s"] = median_s(lambda: host_select(host_slab(), N, ex))
                t["speedup_vs_predict_rows_then_host"] = t["predict_rows_then_host_s"] / t["device_s"]
                t["speedup_vs_host_only"] = t["host_only_s"] / t["device_s"]
                t["device_wins"] = bool(t["device_s"] < min(t["predict_rows_then_host_s"], t["host_only_s"]))
                say(f"top_n N={N} {name}: device {t['device_s']:.6f} s, predict_rows + host {t['predict_rows_then_host_s']:.6f} s, "
                    f"host only {t['host_only_s']:.6f} s")
                c[f"N{N}_{name}"] = t
        c["no_device_leg_loses"] = all(v["device_wins"] for v in c.values() if isinstance(v, dict))
        res["top_n_leg"] = c

    # ---- (d) score_samples ---------------------------------------------------------------------------------------------------
    if "score_samples" in legs:
        eps = 1e-8
        X = g.random((R, n)) < 0.25
        mask = g.random((R, n)) < 0.90

        def host_scores():
            """predict_rows, then the same sums on the host: one logarithm per entry, as the device forms it."""
            theta = ctx.predict_rows(0, R, out=out64)
            t = np.where(mask, np.log(np.where(X, theta + eps, (1.0 - theta) + eps)), 0.0)
            return t.sum(1), mask.sum(1), t.sum(0), mask.sum(0), t

        d = {"data": "uint8", "observed": float(mask.mean()), "input_bytes": 2 * R * n, "output_bytes": 16 * (R + n)}
        got = ctx.score_rows(X, mask, 0, R, rows=True, cols=True)
        want = host_scores()
        absum = np.abs(want[4])
        for name, ll, obs, w_ll, w_obs, w_abs in (("rows", got[0], got[1], want[0], want[1], absum.sum(1)),
                                                  ("cols", got[2], got[3], want[2], want[3], absum.sum(0))):
            assert np.array_equal(obs, w_obs), f"score_rows: the {name} counts disagree with the host"
            # the tests' bound against an exactly rounded sum, plus NumPy's pairwise summation (at most c 2^-53 sum|t|)
            worst = float(np.max(np.abs(ll - w_ll) / ((1.5 * w_obs + 8) * 2.0 ** -52 * w_abs)))
            assert worst <= 1.0, f"score_rows: the {name} sums are {worst} bounds away from the host's"
            d[f"{name}_worst_over_bound"] = worst
        del want, absum
        d["device_s"], d["device_all_s"] = median_s(lambda: ctx.score_rows(X, mask, 0, R, rows=True, cols=True))
        say("score_rows rows + cols", d["device_s"])
        d["device_rows_only_s"], d["device_rows_only_all_s"] = median_s(lambda: ctx.score_rows(X, mask, 0, R))
        say("score_rows rows", d["device_rows_only_s"])
        d["device_no_mask_s"], d["device_no_mask_all_s"] = median_s(lambda: ctx.score_rows(X, None, 0, R, rows=True, cols=True))
        say("score_rows without a mask", d["device_no_mask_s"])
        d["predict_rows_then_host_s"], d["predict_rows_then_host_all_s"] = median_s(host_scores)
        say("predict_rows + host sums", d["predict_rows_then_host_s"])
        d["device_input_GBps"] = d["input_bytes"] / d["device_s"] / 1e9
        # the call with and without the mask differs by one of the two byte panels that cross PCIe: twice the difference
        # estimates the upload's share of the call.  Derived from two end-to-end times, not a trace.
        d["upload_share_estimated"] = min(1.0, 2.0 * max(0.0, d["device_s"] - d["device_no_mask_s"]) / d["device_s"])
        d["speedup_vs_predict_rows_then_host"] = d["predict_rows_then_host_s"] / d["device_s"]
        res["score_samples_leg"] = d

    # ---- (h) the uploading calls from bit-packed operands, beside the same call from uint8 ----------------------------------------
    if legs & BITS_LEGS:
        from nbmf_mm_amd import PackedBits
        gb = np.random.default_rng(2028)                    # (its own stream: the same data whichever legs ran before)
        X = gb.random((R, n)) < 0.25
        mask = gb.random((R, n)) < 0.90
        excl = gb.random((R, n)) < 0.10
        PX, PM, PE = (PackedBits.from_dense(a) for a in (X, mask, excl))
        h = {"observed": float(mask.mean()), "exclude_density": float(excl.mean()), "uint8_bytes_per_operand": R * n,
             "packed_bytes_per_operand": PX.nbytes}

        def both(name, from_uint8, from_bits):
            want, got = from_uint8(), from_bits()
            assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(want, got)), f"{name}: packed and uint8 input disagree"
            t = {}
            t["uint8_s"], t["uint8_all_s"] = median_s(from_uint8)
            t["bits_s"], t["bits_all_s"] = median_s(from_bits)
            t["bits_over_uint8"] = t["bits_s"] / t["uint8_s"]
            say(f"{name}: uint8 {t['uint8_s']:.6f} s, bits {t['bits_s']:.6f} s")
            return t

        if "score_samples_bits" in legs:
            h["score_samples"] = both("score_rows rows + cols", lambda: ctx.score_rows(X, mask, 0, R, rows=True, cols=True),
                                      lambda: ctx.score_rows(PX, PM, 0, R, rows=True, cols=True))
        if "theta_hist_bits" in legs:
            h["theta_hist_256"] = both("theta_hist 256 bins", lambda: ctx.theta_hist(X, mask, 0, R, bins=256),
                                       lambda: ctx.theta_hist(PX, PM, 0, R, bins=256))
        if "top_n_bits" in legs:
            h["top_n_10_exclude"] = both("top_n N=10 exclude", lambda: ctx.top_n(10, 0, R, exclude=excl),
                                         lambda: ctx.top_n(10, 0, R, exclude=PE))
        res["packed_bits_leg"] = h
        del X, mask, excl, PX, PM, PE

    # ---- (i) decisions per entry as bits: Theta > 0.5, and one draw of Bernoulli(Theta) ---------------------------------------------
    if legs & DECISION_LEGS:
        nb = (n + 7) // 8
        outb = np.empty((R, nb), dtype=np.uint8)
        i = {"packed_output_bytes": R * nb, "u8_output_bytes": R * n}
        if "predict_bits" in legs:
            ctx.predict_rows(0, R, threshold=0.5, out=out8)
            ctx.theta_bits(0, R, threshold=0.5, out=outb)
            assert np.array_equal(outb, np.packbits(out8, axis=1)), "theta_bits(threshold) is not the packed byte slab"
            t = {}
            t["device_u8_s"], t["device_u8_all_s"] = median_s(lambda: ctx.predict_rows(0, R, threshold=0.5, out=out8))
            t["device_bits_s"], t["device_bits_all_s"] = median_s(lambda: ctx.theta_bits(0, R, threshold=0.5, out=outb))
            say(f"predict: bytes {t['device_u8_s']:.6f} s, bits {t['device_bits_s']:.6f} s")
            t["bits_over_u8"] = t["device_bits_s"] / t["device_u8_s"]
            t["bits_faster_end_to_end"] = bool(t["device_bits_s"] < t["device_u8_s"])
            if not args.device_only:
                t["u8_then_packbits_s"], t["u8_then_packbits_all_s"] = median_s(
                    lambda: np.packbits(ctx.predict_rows(0, R, threshold=0.5, out=out8), axis=1))
                say(f"predict: bytes + np.packbits {t['u8_then_packbits_s']:.6f} s")
            i["predict_bits"] = t
        if "sample" in legs:
            seed = 2029
            ctx.predict_rows(0, R, out=out64)
            ctx.theta_bits(0, R, seed=seed, out=outb)
            want = _hip.hash_uniform(m, n, seed, rows=np.arange(R)) < out64
            assert np.array_equal(outb, np.packbits(want, axis=1)), "theta_bits(seed) is not hash_uniform < predict_rows"
            t = {"ones": float(want.mean())}
            del want
            t["device_s"], t["device_all_s"] = median_s(lambda: ctx.theta_bits(0, R, seed=seed, out=outb))
            say(f"sample: device {t['device_s']:.6f} s")
            if not args.device_only:
                gs = np.random.default_rng(2029)            # (its own stream)
                t["predict_rows_then_host_s"], t["predict_rows_then_host_all_s"] = median_s(
                    lambda: np.packbits(gs.random((R, n)) < ctx.predict_rows(0, R, out=out64), axis=1))
                say(f"sample: predict_rows + default_rng().random < + np.packbits {t['predict_rows_then_host_s']:.6f} s")
                t["speedup_vs_predict_rows_then_host"] = t["predict_rows_then_host_s"] / t["device_s"]
            i["sample"] = t
        res["decision_bits_leg"] = i
        del outb

    # ---- (f) ranks of held-out entries (before (e), which changes the factors) ---------------------------------------------------
    if "rank_of" in legs:
        gr = np.random.default_rng(2026)                    # (its own stream: the same data whichever legs ran before)
        excl = gr.random((R, n)) < 0.10

        def host_by_compares(theta, tcols, ex):
            """Per target slot three compares of the whole slab: rows x targets x n of them."""
            ok = ~np.isnan(theta) if ex is None else ~np.isnan(theta) & ~ex
            col = np.arange(n)[None, :]
            out = np.empty((3,) + tcols.shape, dtype=np.int64)
            for q in range(tcols.shape[1]):
                j = tcols[:, q:q + 1]
                v = np.take_along_axis(theta, j, axis=1)
                same = ok & (theta == v)
                out[1, :, q] = (ok & (theta > v)).sum(1)
                out[2, :, q] = same.sum(1) - 1
                out[0, :, q] = out[1, :, q] + (same & (col < j)).sum(1)
            out[:, ~np.take_along_axis(ok, tcols, axis=1)] = -1
            return out[0], out[1], out[2], ok.sum(1)

        def host_by_sort(theta, tcols, ex):
            """One sort of every row's eligible entries, then two binary searches per target; ties are settled by a scan
            of the row, only where there are any."""
            ok = ~np.isnan(theta) if ex is None else ~np.isnan(theta) & ~ex
            E = ok.sum(1)
            srt = np.sort(np.where(ok, theta, np.nan), axis=1)          # NaN last: the first E of a row are the eligible
            out = np.empty((3,) + tcols.shape, dtype=np.int64)
            for i in range(theta.shape[0]):
                v = theta[i, tcols[i]]
                lo, hi = np.searchsorted(srt[i, :E[i]], v, "left"), np.searchsorted(srt[i, :E[i]], v, "right")
                out[1, i], out[2, i] = E[i] - hi, hi - lo - 1
                out[0, i] = out[1, i]
                for q in np.flatnonzero(out[2, i] > 0):
                    j = tcols[i, q]
                    out[0, i, q] += np.count_nonzero(ok[i, :j] & (theta[i, :j] == v[q]))
            out[:, ~np.take_along_axis(ok, tcols, axis=1)] = -1
            return out[0], out[1], out[2], E

        f = {"exclude_density": float(excl.mean())}
        for T, ex in ((10, excl), (100, None)):
            # T distinct columns per row, one from each of T stripes, in shuffled order
            tcols = gr.permuted(gr.integers(0, n // T, (R, T)) + np.arange(T) * (n // T), axis=1).astype(np.int32)
            indptr, indices = np.arange(R + 1, dtype=np.int64) * T, np.ascontiguousarray(tcols.ravel())
            call = lambda: ctx.rank_of(indptr, indices, 0, R, exclude=ex)   # noqa: E731
            rank, above, tied, scores, eligible = call()
            ctx.predict_rows(0, R, out=out64)
            t = {"targets_per_row": T, "exclude": ex is not None, "output_bytes": 8 * (4 * R * T + R)}
            for route in (host_by_compares, host_by_sort) if T <= 10 else (host_by_sort,):
                want = route(out64, tcols, ex)
                assert all(np.array_equal(a.reshape(R, T) if a.size == R * T else a, w)
                           for a, w in zip((rank, above, tied, eligible), want)), \
                    f"rank_of ({T} targets per row) disagrees with {route.__name__} over predict_rows"
            assert np.array_equal(scores.reshape(R, T), np.take_along_axis(out64, tcols, axis=1)), "rank_of: scores"
            t["ineligible_targets"] = int((rank < 0).sum())
            t["device_s"], t["device_all_s"] = median_s(call)
            say(f"rank_of T={T}: device {t['device_s']:.6f} s")
            kept = []                                           # the same call with every result kept alive: median_s drops a
            t["device_results_kept_s"], t["device_results_kept_all_s"] = median_s(lambda: kept.append(call()))   # result inside the timed region
            say(f"rank_of T={T}: device, results kept alive {t['device_results_kept_s']:.6f} s")
            del kept
            t["top_n_10_same_exclude_s"], t["top_n_10_same_exclude_all_s"] = median_s(lambda: ctx.top_n(10, 0, R, exclude=ex))
            say(f"top_n(10), the same exclude: {t['top_n_10_same_exclude_s']:.6f} s")
            if not args.device_only:
                for route in (host_by_compares, host_by_sort) if T <= 10 else (host_by_sort,):
                    name = "predict_rows_then_" + route.__name__
                    t[name + "_s"], t[name + "_all_s"] = median_s(lambda: route(ctx.predict_rows(0, R, out=out64), tcols, ex))
                    say(f"rank_of T={T}: {name} {t[name + '_s']:.6f} s")
                best = min(v for key, v in t.items() if key.startswith("predict_rows_then_") and key.endswith("_s")
                           and not key.endswith("_all_s"))
                t["speedup_vs_best_host_route"] = best / t["device_s"]
            f[f"T{T}"] = t
        res["rank_of_leg"] = f

    # ---- (m) expected counts by (row, feature group) and by feature (before (e), which replaces the factors) ------------------
    if "moments" in legs:
        from nbmf_mm_amd import PackedBits
        gh = np.random.default_rng(2025)                    # the stream of (e): the same data and mask
        X = gh.random((R, n)) < 0.25
        mask = gh.random((R, n)) < 0.90
        PX, PM = PackedBits.from_dense(X), PackedBits.from_dense(mask)
        gm = np.random.default_rng(2029)
        layouts = {"G1": (None, 1), "G16_runs": (np.arange(n) * 16 // n, 16), "G16_random": (gm.integers(0, 16, n), 16)}

        def exact_terms(mk):
            """The five integer terms of every entry under the contract, in NumPy over the device's own slab."""
            theta = ctx.predict_rows(0, R, out=out64)
            obs = np.ones((R, n), dtype=bool) if mk is None else mk
            q1 = np.rint(theta * 2.0 ** 32).astype(np.int64)
            q2 = np.rint((theta * theta) * 2.0 ** 32).astype(np.int64)
            return (obs.astype(np.int64), (obs & X).astype(np.int64), np.where(obs, q1, 0), np.where(obs, q2, 0), np.where(obs & X, q1, 0))

        def exact_tables(terms, groups, G):
            lab = np.zeros(n, dtype=np.int64) if groups is None else groups
            rows_ = np.stack([np.stack([t[:, lab == g].sum(1) for g in range(G)], axis=1) for t in terms], axis=-1)
            return rows_, np.stack([t.sum(0) for t in terms], axis=-1)

        def host_float(groups, G, mk):
            """predict_rows, then the five sums per slot in float64: what a user had before the device call."""
            theta = ctx.predict_rows(0, R, out=out64)
            obs = np.ones((R, n), dtype=bool) if mk is None else mk
            onehot = np.zeros((n, G))
            onehot[np.arange(n), 0 if groups is None else groups] = 1.0
            t = np.where(obs, theta, 0.0)
            terms = (obs.astype(np.float64), (obs & X).astype(np.float64), t, t * t, np.where(X, t, 0.0))
            return [a @ onehot for a in terms], [a.sum(0) for a in terms]

        mo = {"data": "uint8 and bits", "observed": float(mask.mean()), "input_bytes_uint8": 2 * R * n,
              "output_bytes": {name: 8 * 5 * (R * G + n) + 16 for name, (_, G) in layouts.items()}}
        for mk in () if args.device_only else (mask, None):  # (a trace run skips the host's half minute of integer NumPy)
            terms = exact_terms(mk)
            for name, (groups, G) in layouts.items():
                row_tab, col_tab, nan_count = ctx.moments(X, mk, groups=groups, n_groups=G, row0=0, nrows=R, cols=True)
                want_rows, want_cols = exact_tables(terms, groups, G)
                assert np.array_equal(row_tab, want_rows) and np.array_equal(col_tab, want_cols) and not nan_count.any(), \
                    f"moments ({name}) disagrees with NumPy over predict_rows"
            del terms, want_rows, want_cols
        for name, (groups, G) in layouts.items():
            got = ctx.moments(PX, PM, groups=groups, n_groups=G, row0=0, nrows=R, cols=True)
            want = ctx.moments(X, mask, groups=groups, n_groups=G, row0=0, nrows=R, cols=True)
            assert all(np.array_equal(a, b) for a, b in zip(got, want)), f"moments ({name}) from bits differs from uint8"
        for name, (groups, G) in layouts.items():
            for tag, x, mk, kw in (("uint8", X, mask, {}), ("bits", PX, PM, {}), ("uint8_no_mask", X, None, {}),
                                   ("uint8_rows_only", X, mask, {"cols": False}), ("uint8_cols_only", X, mask, {"rows": False})):
                key = f"{name}_{tag}"
                call = lambda: ctx.moments(x, mk, groups=groups, n_groups=G, row0=0, nrows=R, **{"cols": True, **kw})   # noqa: E731
                mo[key + "_s"], mo[key + "_all_s"] = median_s(call)
                say(f"moments {key}", mo[key + "_s"])
            # the two byte panels differ by one with and without the mask: twice the difference estimates the upload's share
            mo[name + "_upload_share_estimated"] = min(1.0, 2.0 * max(0.0, mo[name + "_uint8_s"] - mo[name + "_uint8_no_mask_s"]) / mo[name + "_uint8_s"])
        for copies in ("1", "4", "32", "256"):
            os.environ["NBMF_MOMENT_COPIES"] = copies
            groups, G = layouts["G16_random"]
            mo[f"G16_random_uint8_copies_{copies}_s"], _ = median_s(lambda: ctx.moments(X, mask, groups=groups, n_groups=G, row0=0, nrows=R, cols=True))
            say(f"moments G16_random uint8 copies {copies}", mo[f"G16_random_uint8_copies_{copies}_s"])
        del os.environ["NBMF_MOMENT_COPIES"]
        mo["theta_hist_1024_uint8_s"], mo["theta_hist_1024_uint8_all_s"] = median_s(lambda: ctx.theta_hist(X, mask, 0, R, bins=1024))
        say("theta_hist 1024 bins uint8 (the same operands)", mo["theta_hist_1024_uint8_s"])
        mo["theta_hist_1024_bits_s"], _ = median_s(lambda: ctx.theta_hist(PX, PM, 0, R, bins=1024))
        say("theta_hist 1024 bins bits", mo["theta_hist_1024_bits_s"])
        mo["predict_rows_f64_s"], _ = median_s(lambda: ctx.predict_rows(0, R, out=out64))
        say("predict_rows float64 (the slab the host route starts from)", mo["predict_rows_f64_s"])
        if not args.device_only:
            for name, (groups, G) in layouts.items():
                mo[name + "_predict_rows_then_numpy_s"], mo[name + "_predict_rows_then_numpy_all_s"] = median_s(lambda: host_float(groups, G, mask))
                say(f"{name} predict_rows + NumPy float sums", mo[name + "_predict_rows_then_numpy_s"])
                mo[name + "_speedup_vs_predict_rows_then_numpy"] = mo[name + "_predict_rows_then_numpy_s"] / mo[name + "_uint8_s"]
        res["moments_leg"] = mo
        del X, mask, PX, PM

    # ---- (e) class histograms of Theta ------------------------------------------------------------------------------------------
    if "theta_hist" in legs:
        gh = np.random.default_rng(2025)                    # (its own stream: the same data whichever legs ran before)
        X = gh.random((R, n)) < 0.25
        mask = gh.random((R, n)) < 0.90

        def host_hist(bins, mk):
            """predict_rows, then the contract on the host: one multiplication per entry, np.bincount per class."""
            theta = ctx.predict_rows(0, R, out=out64)
            obs = np.ones((R, n), dtype=bool) if mk is None else mk
            b = np.minimum((theta * bins).astype(np.int64), bins - 1)
            return np.stack([np.bincount(b[obs & ~X], minlength=bins), np.bincount(b[obs & X], minlength=bins)])

        def host_auc():
            from sklearn.metrics import roc_auc_score
            theta = ctx.predict_rows(0, R, out=out64)
            return roc_auc_score(X[mask], theta[mask])

        def timed_legs(tag):
            """Equality first, then the device legs (and, unless --device-only, the host legs) for the factors in ctx."""
            from nbmf_mm_amd import _metrics
            t = {}
            for bins, mk in ((256, mask), (1024, mask), (1, mask), (1024, None)):
                hist, nan_count = ctx.theta_hist(X, mk, 0, R, bins=bins)
                assert np.array_equal(hist, host_hist(bins, mk)) and not nan_count.any(), \
                    f"theta_hist ({tag}, bins = {bins}) disagrees with NumPy over predict_rows"
            hist, _ = ctx.theta_hist(X, mask, 0, R, bins=1024)
            t["bins_hit_1024"] = int(np.count_nonzero(hist.sum(0)))
            t["auc_1024"], t["auc_slack_1024"] = _metrics.auc_from_hist(hist)
            for name, bins, mk in (("device_256", 256, mask), ("device_1024", 1024, mask), ("device_1", 1, mask),
                                   ("device_1024_no_mask", 1024, None)):
                t[name + "_s"], t[name + "_all_s"] = median_s(lambda: ctx.theta_hist(X, mk, 0, R, bins=bins))
                say(f"theta_hist {tag} {name}", t[name + "_s"])
            if not args.device_only:
                t["predict_rows_then_bincount_s"], t["predict_rows_then_bincount_all_s"] = median_s(lambda: host_hist(1024, mask))
                say(f"{tag} predict_rows + np.bincount", t["predict_rows_then_bincount_s"])
                exact = host_auc()
                assert abs(exact - t["auc_1024"]) <= t["auc_slack_1024"] + 1e-15, "the binned AUC is outside its slack"
                t["exact_auc"] = exact
                t["predict_rows_then_sklearn_auc_s"], t["predict_rows_then_sklearn_auc_all_s"] = median_s(host_auc)
                say(f"{tag} predict_rows + roc_auc_score", t["predict_rows_then_sklearn_auc_s"])
                t["speedup_vs_predict_rows_then_bincount"] = t["predict_rows_then_bincount_s"] / t["device_1024_s"]
                t["speedup_vs_predict_rows_then_sklearn_auc"] = t["predict_rows_then_sklearn_auc_s"] / t["device_1024_s"]
            # with and without the mask differ by one of the two byte panels that cross PCIe: twice the difference estimates
            # the upload's share of the call.  Derived from two end-to-end times, not a trace.
            t["upload_share_estimated"] = min(1.0, 2.0 * max(0.0, t["device_1024_s"] - t["device_1024_no_mask_s"]) / t["device_1024_s"])
            return t

        e = {"data": "uint8", "observed": float(mask.mean()), "input_bytes": 2 * R * n, "output_bytes": 8 * (2 * 1024 + 2)}
        e["concentrated"] = timed_legs("concentrated")
        # factors that spread Theta over [0, 1]: each row of W leans on a few components, H is bimodal
        W2 = gh.random((m, k)) ** 12
        W2 /= W2.sum(1, keepdims=True)
        H2 = np.where(gh.random((k, n)) < 0.5, gh.uniform(0.0, 0.2, (k, n)), gh.uniform(0.8, 1.0, (k, n)))
        ctx.set_factors(np.ascontiguousarray(W2.T), H2)
        e["spread"] = timed_legs("spread")
        res["theta_hist_leg"] = e

if "eval_curve" in legs:
    res["eval_curve_leg"] = eval_curve_leg()

print(json.dumps(res))
