#!/usr/bin/env python3
"""Host -> device upload + pack of the c3 workload (65536 x 8192, a 90 % mask) handed over as uint8 V + bool mask (1.07 GB)
and as bit-packed V + bit-packed mask (PackedBits: 0.13 GB, unpacked on the device), in one process, repeated; then a
50-iteration fit from each form.  The two forms give the same data image (n_obs and the loss curves are compared).
NBMF_UPLOAD_TRACE=1 prints where each upload's time goes.  Prints progress lines and, last, ONE JSON line."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from nbmf_mm_amd import PackedBits, _hip  # noqa: E402

M, N, K = 65536, 8192, 64
g = np.random.default_rng(0)
X8 = (g.random((M, N)) < 0.25).astype(np.uint8)
Mk = g.random((M, N)) < 0.9
PX, PM = PackedBits.from_dense(X8), PackedBits.from_dense(Mk)
W0 = g.uniform(0.1, 0.9, (K, M))
W0 /= W0.sum(0, keepdims=True)
H0 = g.uniform(0.1, 0.9, (K, N))
res = {"tool": "bench_upload_bits", "library": _hip.source_hash(), "shape": [M, N, K], "uint8_bytes": int(X8.nbytes + Mk.nbytes),
       "packed_bytes": int(PX.nbytes + PM.nbytes)}
with _hip.Context(M, N, K) as ctx:
    ctx.set_hyper(1.2, 1.2, 1e-8)
    for name, x, mk in (("uint8", X8, Mk), ("bits", PX, PM)):
        ts = []
        for rep in range(6):                                # the first one warms the pools and the code objects
            t0 = time.perf_counter()
            ctx.upload(x, mask=mk)
            ts.append(time.perf_counter() - t0)
            print("%s upload %.4f s" % (name, ts[-1]), flush=True)
        res[name + "_upload_s"], res[name + "_upload_all_s"] = float(np.median(ts[1:])), [round(t, 5) for t in ts]
        res[name + "_n_obs"] = ctx.n_obs()
        fits = []
        for rep in range(3):
            t0 = time.perf_counter()
            ctx.upload(x, mask=mk)
            ctx.set_factors(W0, H0)
            losses, _ = ctx.run(50, 0.0)
            fits.append(time.perf_counter() - t0)
            print("%s upload + 50 iterations %.4f s" % (name, fits[-1]), flush=True)
        res[name + "_upload_and_50_iterations_s"] = float(np.median(fits))
        res[name + "_final_loss"] = float(losses[-1])
assert res["uint8_n_obs"] == res["bits_n_obs"] == float(Mk.sum()) and res["uint8_final_loss"] == res["bits_final_loss"]
print(json.dumps(res))
