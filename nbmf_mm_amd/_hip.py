"""ctypes binding of libnbmf_hip.so (see include/nbmf_hip.h for the C ABI).

The library is the product path: if it is missing, or there is no MI355X, every entry point
raises — there is no CPU fallback (the CPU oracle under oracle/ is test infrastructure only).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_int64, c_uint64, c_void_p

import numpy as np

from ._packed import PackedBits

_HERE = os.path.dirname(os.path.abspath(__file__))

NBMF_OK = 0
NBMF_ERR_ARG = -1
NBMF_ERR_HIP = -2
NBMF_ERR_RANGE = -3
NBMF_ERR_STATE = -4
NBMF_ERR_COMM = -5

MASK_NONE, MASK_F64, MASK_U8, MASK_BITS = 0, 1, 2, 3
PROJ_NORMALIZE, PROJ_DUCHI = 0, 1
FLAG_BINARY_PATH = 1
STORAGE = {"auto": 0, "f64": 1, "f64w": 2}
MAX_K = 512
PEER_HANDLE_BYTES = 192

#: every symbol include/nbmf_hip.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "nbmf_abi_version", "nbmf_last_error", "nbmf_device_count", "nbmf_create", "nbmf_destroy",
    "nbmf_set_hyper", "nbmf_upload", "nbmf_upload_csr", "nbmf_generate", "nbmf_get_n_obs", "nbmf_set_factors", "nbmf_get_factors",
    "nbmf_run", "nbmf_w_only_steps", "nbmf_loss", "nbmf_loglik", "nbmf_loglik_strict", "nbmf_comm_unique_id", "nbmf_comm_init",
    "nbmf_comm_init_host", "nbmf_peer_export", "nbmf_comm_init_peer", "nbmf_comm_detach",
    "nbmf_timing_enable", "nbmf_timing_get", "nbmf_synchronize", "nbmf_selftest_unary",
    "nbmf_set_progress", "nbmf_device_synchronize", "nbmf_small_stats", "nbmf_generate_slice", "nbmf_set_storage",
    "nbmf_set_exchange_panels", "nbmf_set_peer_timeout_ms", "nbmf_run_batch", "nbmf_batch_stats", "nbmf_sweep_info",
    "nbmf_upload_v", "nbmf_selftest_mfma_peak", "nbmf_engine_stats", "nbmf_source_hash", "nbmf_comm_info", "nbmf_cancel", "nbmf_variant_stats", "nbmf_device_bus_id",
    "nbmf_predict_at", "nbmf_predict_rows", "nbmf_top_n", "nbmf_score_rows", "nbmf_theta_hist",
    "nbmf_rank_rows", "nbmf_set_eval", "nbmf_eval_loglik", "nbmf_get_eval", "nbmf_get_best_factors",
    "nbmf_top_n_v", "nbmf_score_rows_v", "nbmf_theta_hist_v", "nbmf_rank_rows_v", "nbmf_selftest_unpack_bits",
    "nbmf_theta_bits", "nbmf_hold_out", "nbmf_hold_out_undo", "nbmf_get_eval_pairs",
    "nbmf_top_pairs", "nbmf_similarity", "nbmf_neighbors", "nbmf_moment_rows_v",
]
DATA_F64, DATA_U8, DATA_F32, DATA_BITS = 0, 1, 2, 3
PREDICT_F64, PREDICT_U8 = 0, 1
BITS_THRESHOLD, BITS_SAMPLE = 0, 1
TOP_N_MAX = 256
TOP_PAIRS_MAX = 1 << 22
PAIRS_THETA, PAIRS_LIKELIHOOD = 0, 1
HIST_MAX_BINS = 1024
MOMENT_MAX_GROUPS = 16
MOMENT_FRAC_BITS = 32
#: the five sums of a slot of ``Context.moments``, in the order of the tables' last axis
MOMENT_FIELDS = ("n_obs", "n_ones", "s1", "s2", "s1_ones")
SIM_DOT, SIM_COSINE, SIM_PROFILE = 0, 1, 2
#: the metric names of ``similarity`` / ``neighbors`` (``nbmf_similarity``)
SIM_METRICS = {"dot": SIM_DOT, "cosine": SIM_COSINE, "profile": SIM_PROFILE}


#: int fn(void* user, double* buf, int64 count) -- in-place sum over ranks on a host buffer
HOST_ALLREDUCE_FN = ctypes.CFUNCTYPE(c_int, c_void_p, POINTER(c_double), c_int64)
#: void fn(void* user, int first, int count, const double* losses) -- nbmf_set_progress
PROGRESS_FN = ctypes.CFUNCTYPE(None, c_void_p, c_int, c_int, POINTER(c_double))


class NBMFHipError(RuntimeError):
    """A libnbmf_hip call failed (HIP error, missing GPU, bad state)."""


def library_path() -> str:
    return os.environ.get("NBMF_HIP_LIBRARY", os.path.join(_HERE, "libnbmf_hip.so"))


_lib = None


def _autobuild(path):
    """Build the library once if the toolchain is here.  Several ranks may arrive together from a fresh
    checkout: the build is serialised by a file lock, written under a temporary name and renamed into place,
    so nobody ever maps a half-written file; a failed build reports the compiler's own message."""
    import fcntl
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if not (shutil.which("make") and hipcc):
        return
    with open(path + ".build.lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if os.path.exists(path):            # another rank built it while this one waited
            return
        tmp = f"{path}.tmp.{os.getpid()}"
        r = subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), f"OUT={tmp}", f"HIPCC={hipcc}"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode == 0 and os.path.exists(tmp):
            os.replace(tmp, path)
        else:
            if os.path.exists(tmp):
                os.remove(tmp)
            raise NBMFHipError(f"building {path} failed:\n{r.stdout[-2000:]}")


# GPU_MAX_HW_QUEUES is read by the HIP runtime at ITS first call, whoever makes it -- another HIP user of the process
# (PyTorch, say) may do so before this library is ever loaded.  The earliest moment this package can observe the variable
# is its own import: that value is recorded, and it is an UPPER bound on what the runtime has only if nothing in the
# process started HIP before with a smaller one (set it before ANY HIP user of the process starts).
_HW_QUEUES_AT_LOAD = os.environ.get("GPU_MAX_HW_QUEUES")


def hw_queues_at_load():
    """GPU_MAX_HW_QUEUES as it stood when this package was imported (no later than the library's load and hence, unless
    another HIP user of the process was there first, than the runtime's start); the runtime's default (4) if unset."""
    try:
        return int(_HW_QUEUES_AT_LOAD) if _HW_QUEUES_AT_LOAD is not None else 4
    except ValueError:
        return 4


def load():
    """Load libnbmf_hip.so (built by nbmf_mm_amd/csrc/Makefile or __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path) and "NBMF_HIP_LIBRARY" not in os.environ and not os.environ.get("NBMF_NO_AUTOBUILD"):
        _autobuild(path)                    # a source checkout without the built artefact
    if not os.path.exists(path):
        raise NBMFHipError(
            f"{path} not found: build it with `make -C nbmf_mm_amd/csrc` (needs hipcc); "
            "nbmf_mm_amd has no CPU fallback")
    lib = ctypes.CDLL(path)
    if "NBMF_HIP_LIBRARY" in os.environ:
        # an explicitly named build (A/B measurements against an older library): entry points it lacks raise when called
        class _Missing:
            def __init__(self, name):
                self.name, self.argtypes, self.restype = name, None, None

            def __call__(self, *a):
                raise NBMFHipError(f"{path} does not export {self.name}")
        for name in SYMBOLS:
            if not hasattr(lib, name):
                setattr(lib, name, _Missing(name))
    dp = POINTER(c_double)
    lib.nbmf_abi_version.restype = c_int
    lib.nbmf_source_hash.restype = c_char_p
    lib.nbmf_cancel.argtypes = [c_void_p]
    lib.nbmf_device_bus_id.argtypes = [c_int, c_char_p, c_int]
    lib.nbmf_variant_stats.argtypes = [POINTER(ctypes.c_longlong), POINTER(ctypes.c_longlong), POINTER(ctypes.c_longlong)]
    lib.nbmf_comm_info.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)]
    lib.nbmf_last_error.restype = c_char_p
    lib.nbmf_device_count.argtypes = [POINTER(c_int)]
    lib.nbmf_create.argtypes = [c_int64, c_int64, c_int, c_int, POINTER(c_void_p)]
    lib.nbmf_destroy.argtypes = [c_void_p]
    lib.nbmf_set_hyper.argtypes = [c_void_p, c_double, c_double, c_double, c_int]
    lib.nbmf_upload.argtypes = [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int, c_int64, POINTER(c_int)]
    lib.nbmf_upload_v.argtypes = [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_int, c_int64, POINTER(c_int)]
    lib.nbmf_selftest_mfma_peak.argtypes = [c_int, c_double, dp, dp, dp]
    lib.nbmf_engine_stats.argtypes = [POINTER(ctypes.c_longlong), POINTER(ctypes.c_longlong), POINTER(ctypes.c_longlong)]
    lib.nbmf_generate.argtypes = [c_void_p, ctypes.c_uint64, c_double, c_double]
    lib.nbmf_generate_slice.argtypes = [c_void_p, ctypes.c_uint64, c_double, c_double, c_int64, c_int64, c_int64]
    lib.nbmf_set_storage.argtypes = [c_void_p, c_int]
    lib.nbmf_get_n_obs.argtypes = [c_void_p, dp]
    lib.nbmf_set_factors.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.nbmf_get_factors.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.nbmf_run.argtypes = [c_void_p, c_int, c_double, c_void_p, POINTER(c_int)]
    lib.nbmf_run_batch.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_double, c_void_p, c_void_p,
                                   c_void_p, c_void_p]
    lib.nbmf_batch_stats.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int)]
    lib.nbmf_sweep_info.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)]
    lib.nbmf_w_only_steps.argtypes = [c_void_p, c_int]
    lib.nbmf_loss.argtypes = [c_void_p, dp]
    lib.nbmf_loglik.argtypes = [c_void_p, c_int, dp]
    lib.nbmf_loglik_strict.argtypes = [c_void_p, dp]
    lib.nbmf_comm_unique_id.argtypes = [c_void_p]
    lib.nbmf_comm_init.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int]
    lib.nbmf_comm_init_host.argtypes = [c_void_p, HOST_ALLREDUCE_FN, c_void_p, c_int, c_int, c_int]
    lib.nbmf_upload_csr.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int64, POINTER(c_int)]
    lib.nbmf_peer_export.argtypes = [c_void_p, c_int, c_void_p]
    lib.nbmf_comm_init_peer.argtypes = [c_void_p, c_void_p, c_int, c_int, c_int]
    lib.nbmf_comm_detach.argtypes = [c_void_p]
    lib.nbmf_set_exchange_panels.argtypes = [c_void_p, c_int]
    lib.nbmf_set_peer_timeout_ms.argtypes = [c_void_p, c_double]
    lib.nbmf_timing_enable.argtypes = [c_void_p, c_int]
    lib.nbmf_timing_get.argtypes = [c_void_p, dp, POINTER(c_int), dp, POINTER(c_int)]
    lib.nbmf_synchronize.argtypes = [c_void_p]
    lib.nbmf_set_progress.argtypes = [c_void_p, PROGRESS_FN, c_void_p, c_int]
    lib.nbmf_device_synchronize.argtypes = [c_int]
    lib.nbmf_small_stats.argtypes = [c_void_p, POINTER(c_int), POINTER(c_int)]
    lib.nbmf_selftest_unary.argtypes = [c_int, c_int, c_int, c_void_p, c_void_p]
    lib.nbmf_predict_at.argtypes = [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]
    lib.nbmf_predict_rows.argtypes = [c_void_p, c_int64, c_int64, c_int, c_int, c_double, c_void_p, c_int64]
    lib.nbmf_top_n.argtypes = [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64]
    lib.nbmf_score_rows.argtypes = [c_void_p, c_int64, c_int64, c_int, c_double, c_void_p, c_int, c_int64, c_void_p, c_int64,
                                    c_void_p, c_void_p, c_void_p, c_void_p]
    lib.nbmf_theta_hist.argtypes = [c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]
    lib.nbmf_rank_rows.argtypes = [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p]
    lib.nbmf_top_n_v.argtypes = [c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int64]
    lib.nbmf_score_rows_v.argtypes = [c_void_p, c_int64, c_int64, c_int, c_double, c_void_p, c_int, c_int64, c_void_p, c_int,
                                      c_int64, c_void_p, c_void_p, c_void_p, c_void_p]
    lib.nbmf_top_pairs.argtypes = [c_void_p, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_int, c_int64, c_void_p, c_int, c_int64,
                                   c_void_p, c_void_p, c_void_p, c_void_p]
    lib.nbmf_theta_hist_v.argtypes = [c_void_p, c_int64, c_int64, c_int, c_void_p, c_int, c_int64, c_void_p, c_int, c_int64,
                                      c_void_p, c_void_p]
    lib.nbmf_rank_rows_v.argtypes = [c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int64, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_void_p]
    lib.nbmf_selftest_unpack_bits.argtypes = [c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64]
    lib.nbmf_theta_bits.argtypes = [c_void_p, c_int64, c_int64, c_int, c_int, c_double, c_uint64, c_void_p, c_int64]
    lib.nbmf_set_eval.argtypes = [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int]
    lib.nbmf_eval_loglik.argtypes = [c_void_p, dp]
    lib.nbmf_get_eval.argtypes = [c_void_p, c_int, POINTER(c_int), c_void_p, c_void_p, POINTER(c_int), POINTER(c_int)]
    lib.nbmf_get_best_factors.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.nbmf_hold_out.argtypes = [c_void_p, c_uint64, c_int, c_double, c_double, c_int, c_int, POINTER(c_int64)]
    lib.nbmf_hold_out_undo.argtypes = [c_void_p]
    lib.nbmf_get_eval_pairs.argtypes = [c_void_p, c_int64, POINTER(c_int64), c_void_p, c_void_p, c_void_p]
    lib.nbmf_similarity.argtypes = [c_void_p, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64]
    lib.nbmf_neighbors.argtypes = [c_void_p, c_int, c_int, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int64]
    lib.nbmf_moment_rows_v.argtypes = [c_void_p, c_int64, c_int64, c_void_p, c_int, c_int64, c_void_p, c_int, c_int64, c_void_p, c_int,
                                       c_void_p, c_void_p, c_void_p]
    for name in SYMBOLS:
        if name not in ("nbmf_last_error", "nbmf_source_hash"):
            getattr(lib, name).restype = c_int
    _lib = lib
    return lib


def _check(rc):
    if rc == NBMF_OK:
        return
    msg = load().nbmf_last_error().decode("utf-8", "replace")
    if rc == NBMF_ERR_RANGE:
        raise ValueError("X must be binary")          # _base.py:91 wording
    if rc == NBMF_ERR_ARG:
        raise ValueError(msg)
    raise NBMFHipError(msg)


def source_hash() -> str:
    """The content hash of the sources the loaded library was compiled from (``nbmf_source_hash``)."""
    try:
        return load().nbmf_source_hash().decode()
    except NBMFHipError:                    # an older build named by NBMF_HIP_LIBRARY
        return "unknown"


def tree_source_hash():
    """The same hash computed from the sources next to this file (csrc/Makefile's recipe; tools/src_hash.sh), or None
    where the package was installed without them."""
    import glob
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    files = ([os.path.join(csrc, "nbmf_hip.hip")] + sorted(glob.glob(os.path.join(csrc, "*.inc"))) +
             [os.path.join(_HERE, "..", "include", "nbmf_hip.h")])
    if not all(os.path.exists(f) for f in files):
        return None
    h = hashlib.sha256()
    for f in files:
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:12]


def device_count() -> int:
    n = c_int(0)
    rc = load().nbmf_device_count(byref(n))
    return n.value if rc == NBMF_OK else 0


def device_bus_id(device=0) -> str:
    """PCI bus id of HIP device ``device`` in this process: the physical card behind the index (``nbmf_device_bus_id``)."""
    buf = ctypes.create_string_buffer(64)
    _check(load().nbmf_device_bus_id(int(device), buf, 64))
    return buf.value.decode()


def _f64c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def index_pairs(rows, cols):
    """The two index arrays of ``predict_at`` as the library takes them (C-contiguous int64), after the checks that need
    no device: integer-typed, 1-D, equally long.  Raises ``ValueError`` otherwise."""
    rows, cols = np.asarray(rows), np.asarray(cols)
    for name, a in (("rows", rows), ("cols", cols)):
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must be an integer array (got dtype {a.dtype})")
        if a.ndim != 1:
            raise ValueError(f"{name} must be 1-D (got shape {a.shape})")
    if rows.shape != cols.shape:
        raise ValueError(f"rows and cols must be equally long (got {rows.size} and {cols.size})")
    return np.ascontiguousarray(rows, dtype=np.int64), np.ascontiguousarray(cols, dtype=np.int64)


def top_n_count(top, name="top"):
    """``top`` of ``top_n`` as an int, after the checks that need no device: an integer (not a bool) in
    ``[1, TOP_N_MAX]``.  Raises ``ValueError`` otherwise."""
    if isinstance(top, (bool, np.bool_)) or not isinstance(top, (int, np.integer)):
        raise ValueError(f"{name} must be an integer (got {top!r})")
    if not 1 <= int(top) <= TOP_N_MAX:
        raise ValueError(f"{name} must be in [1, {TOP_N_MAX}] (got {int(top)})")
    return int(top)


def sim_axis(axis):
    """``axis`` of ``similarity`` / ``neighbors`` as an int: 0 (samples) or 1 (features), not a bool.  ``ValueError``
    otherwise."""
    if isinstance(axis, (bool, np.bool_)) or not isinstance(axis, (int, np.integer)) or int(axis) not in (0, 1):
        raise ValueError(f"axis must be 0 (samples) or 1 (features) (got {axis!r})")
    return int(axis)


def sim_metric(metric):
    """``metric`` of ``similarity`` / ``neighbors`` as the library's code: one of the names in ``SIM_METRICS`` or its
    code.  ``ValueError`` otherwise."""
    if isinstance(metric, str) and metric in SIM_METRICS:
        return SIM_METRICS[metric]
    if not isinstance(metric, (bool, np.bool_)) and isinstance(metric, (int, np.integer)) and int(metric) in SIM_METRICS.values():
        return int(metric)
    raise ValueError(f"metric must be one of {sorted(SIM_METRICS)} (got {metric!r})")


def item_query(query, L, name="query"):
    """The ``query`` of ``similarity`` / ``neighbors`` as the library takes it (C-contiguous int64) and its length, after
    the checks that need no device: integer-typed, 1-D, every index in ``[0, L)`` -- any order, repeats allowed.  None means
    all ``L`` items: ``(None, L)``.  Raises ``ValueError`` otherwise, naming the lowest offending position."""
    if query is None:
        return None, int(L)
    q = np.asarray(query)
    if q.dtype == np.bool_ or not np.issubdtype(q.dtype, np.integer):
        raise ValueError(f"{name} must be an integer array (got dtype {q.dtype})")
    if q.ndim != 1:
        raise ValueError(f"{name} must be 1-D (got shape {q.shape})")
    bad = np.nonzero((q < 0) | (q >= L))[0]
    if bad.size:
        raise ValueError(f"{name} index at position {int(bad[0])} is outside [0, {int(L)})")
    return np.ascontiguousarray(q, dtype=np.int64), int(q.size)


def top_pairs_count(top, name="top"):
    """``top`` of ``top_pairs`` as an int, after the checks that need no device: an integer (not a bool) in
    ``[1, TOP_PAIRS_MAX]``.  Raises ``ValueError`` otherwise."""
    if isinstance(top, (bool, np.bool_)) or not isinstance(top, (int, np.integer)):
        raise ValueError(f"{name} must be an integer (got {top!r})")
    if not 1 <= int(top) <= TOP_PAIRS_MAX:
        raise ValueError(f"{name} must be in [1, {TOP_PAIRS_MAX}] (got {int(top)})")
    return int(top)


def hist_bins(bins, name="bins"):
    """``bins`` of ``theta_hist`` as an int, after the checks that need no device: an integer (not a bool) in
    ``[1, HIST_MAX_BINS]``.  Raises ``ValueError`` otherwise."""
    if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)):
        raise ValueError(f"{name} must be an integer (got {bins!r})")
    if not 1 <= int(bins) <= HIST_MAX_BINS:
        raise ValueError(f"{name} must be in [1, {HIST_MAX_BINS}] (got {int(bins)})")
    return int(bins)


def group_labels(groups, n, n_groups=None, name="groups", most=None):
    """The labels of ``Context.moments`` (and of ``NBMF.expected_counts`` / ``Moments.grouped``) after the checks that need
    no device: ``(labels, n_groups)``, ``labels`` C-contiguous int32.  ``groups`` is an integer (not bool) 1-D array of
    length ``n`` with values ``>= -1``, -1 meaning "in no group"; None: everything in group 0.  ``n_groups`` defaults to
    ``max label + 1`` (at least 1) and must be an integer above every label, and at most ``most`` where that is given.
    Raises ``ValueError`` otherwise, naming the lowest offending position."""
    if n_groups is not None:
        if isinstance(n_groups, (bool, np.bool_)) or not isinstance(n_groups, (int, np.integer)) or n_groups < 1:
            raise ValueError(f"n_{name} must be a positive integer (got {n_groups!r})")
        n_groups = int(n_groups)
    if groups is None:
        labels = np.zeros(n, dtype=np.int32)
    else:
        g = np.asarray(groups)
        if g.dtype == np.bool_ or not np.issubdtype(g.dtype, np.integer):
            raise ValueError(f"{name} must be an integer array (got dtype {g.dtype})")
        if g.shape != (n,):
            raise ValueError(f"{name} must have shape ({n},) (got {g.shape})")
        bad = np.flatnonzero(g < -1)
        if bad.size:
            raise ValueError(f"{name} label {int(g[bad[0]])} at position {int(bad[0])} is below -1")
        top = int(g.max()) + 1 if g.size else 0
        if n_groups is not None and top > n_groups:
            at = int(np.flatnonzero(g >= n_groups)[0])
            raise ValueError(f"{name} label {int(g[at])} at position {at} is outside [-1, {n_groups})")
        if top > 2 ** 31 - 1:
            raise ValueError(f"{name} labels must be below 2**31 - 1")
        labels = np.ascontiguousarray(g, dtype=np.int32)
    if n_groups is None:
        n_groups = max(int(labels.max()) + 1 if labels.size else 0, 1)
    if most is not None and n_groups > most:
        raise ValueError(f"n_{name} must be at most {most} (got {n_groups})")
    return labels, n_groups


def csr_targets(indptr, indices, nrows, n):
    """The targets of ``rank_of`` as the library takes them -- ``(indptr, indices)``, C-contiguous int64 and int32 -- after
    the checks that need no device: both integer-typed and 1-D, ``indptr`` of length ``nrows + 1``, non-negative and
    non-decreasing (``indptr[0]`` may be above 0: a slice of a larger CSR's ``indptr`` goes with its whole ``indices``),
    ``indices`` at least ``indptr[-1]`` long and every column at a position in ``[indptr[0], indptr[-1])`` inside
    ``[0, n)``.  Raises ``ValueError`` otherwise, naming the lowest offending position."""
    indptr, indices = np.asarray(indptr), np.asarray(indices)
    for name, a in (("indptr", indptr), ("indices", indices)):
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must be an integer array (got dtype {a.dtype})")
        if a.ndim != 1:
            raise ValueError(f"{name} must be 1-D (got shape {a.shape})")
    if indptr.size != nrows + 1:
        raise ValueError(f"indptr must have nrows + 1 = {nrows + 1} entries (got {indptr.size})")
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    if indptr[0] < 0:
        raise ValueError(f"indptr[0] = {int(indptr[0])} is negative")
    down = np.flatnonzero(indptr[1:] < indptr[:-1])
    if down.size:
        r = int(down[0])
        raise ValueError(f"indptr decreases at row {r} ({int(indptr[r + 1])} after {int(indptr[r])})")
    first, last = int(indptr[0]), int(indptr[-1])
    if indices.size < last:
        raise ValueError(f"indices has {indices.size} entries, indptr describes {last}")
    live = indices[first:last]
    bad = np.flatnonzero((live < 0) | (live >= min(int(n), 2 ** 31)))
    if bad.size:
        p = first + int(bad[0])
        raise ValueError(f"target column {int(indices[p])} at position {p} is outside [0, {int(n)})")
    if indices.dtype != np.int32:               # (the positions outside [first, last) are never read: they go as zeros)
        narrow = np.zeros(indices.size, dtype=np.int32)
        narrow[first:last] = live
        indices = narrow
    return indptr, np.ascontiguousarray(indices)


#: the dtypes a row array may have: one byte per entry (passed to the library as uint8), or float64
BYTE_KINDS = (np.bool_, np.uint8)
ANY_KINDS = BYTE_KINDS + (np.float64,)


def row_array(a, nrows, n, name, kinds, packed=False):
    """A caller's ``(nrows, n)`` array as the row-slab calls of the library take it -- the ``out`` of ``predict_rows``,
    the ``exclude`` of ``top_n``, the data and the mask of ``score_rows`` and of ``theta_hist``: ``(array, kind, ld)``,
    ``kind`` DATA_U8 (a bool or uint8 array, returned as its uint8 view) or DATA_F64, ``ld`` the leading dimension in elements.  The dtype must be
    one of ``kinds`` (BYTE_KINDS, ANY_KINDS or ``(np.float64,)``), the shape ``(nrows, n)``, the stride along a row one
    element, the row stride at least n elements and whole elements -- a slice of a wider array is passed through as it is,
    nothing is copied.  The row stride of a single row or of an empty array is ignored: ``ld = n``.  Raises ``ValueError``
    otherwise.  With ``packed`` a :class:`PackedBits` of shape ``(nrows, n)`` is taken as well: ``(its bytes, DATA_BITS, the
    row stride in bytes)``."""
    if isinstance(a, PackedBits):
        if not packed:
            raise ValueError(f"{name} must be a NumPy array (got a PackedBits)")
        if a.shape != (nrows, n):
            raise ValueError(f"{name} must have shape ({nrows}, {n}) (got {a.shape})")
        return a.bits, DATA_BITS, a.ld
    a = np.asarray(a)
    if a.dtype not in kinds:
        *first, last = [np.dtype(t).name for t in kinds]          # "bool, uint8 or float64"
        raise ValueError(f"{name} must be a {', '.join(first) + ' or ' if first else ''}{last} array (got dtype {a.dtype})")
    if a.shape != (nrows, n):
        raise ValueError(f"{name} must have shape ({nrows}, {n}) (got {a.shape})")
    size = a.itemsize
    if a.size and ((n > 1 and a.strides[1] != size) or (nrows > 1 and (a.strides[0] < n * size or a.strides[0] % size))):
        raise ValueError(f"{name} must have unit stride along a row and a row stride of at least n elements")
    ld = a.strides[0] // size if a.size and nrows > 1 else n
    return (a.view(np.uint8), DATA_U8, int(ld)) if a.dtype != np.float64 else (a, DATA_F64, int(ld))


class Context:
    """One m x n x k internal problem on one GPU (internal layout: Y m x n, W k x m, H k x n)."""

    def __init__(self, m, n, k, device=0):
        self._lib = load()
        self._h = c_void_p()
        _check(self._lib.nbmf_create(int(m), int(n), int(k), int(device), byref(self._h)))
        self.m, self.n, self.k = int(m), int(n), int(k)
        self.binary_path = None

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.nbmf_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_hyper(self, alpha, beta, eps=1e-8, projection=PROJ_NORMALIZE):
        _check(self._lib.nbmf_set_hyper(self._h, float(alpha), float(beta), float(eps), int(projection)))

    def upload(self, x, mask=None, transposed=False):
        """x: the m x n internal matrix, or (transposed=True) the n x m user matrix whose transpose it is.
        A bool / uint8 array goes up as it is, one byte per entry, a float32 array as it is, four (``nbmf_upload_v``: the
        device converts, exactly); anything else as float64.  A :class:`PackedBits` x and / or mask goes up as bits, one
        per entry, and is unpacked on the device (``NBMF_DATA_BITS`` / ``NBMF_MASK_BITS``): the image is that of the bool
        arrays, bit for bit; a packed mask has x's shape (no broadcasting)."""
        want = (self.n, self.m) if transposed else (self.m, self.n)
        if isinstance(x, PackedBits):                      # bits up, unpacked on the device (leading dimension in bytes)
            shape, x, x_kind, ldx = x.shape, x.bits, DATA_BITS, x.ld
        else:
            x = np.asarray(x)
            if x.dtype == np.bool_ or x.dtype == np.uint8:
                x, x_kind = np.ascontiguousarray(x).view(np.uint8), DATA_U8
            elif x.dtype == np.float32:
                x, x_kind = np.ascontiguousarray(x), DATA_F32
            else:
                x, x_kind = _f64c(x), DATA_F64
            shape, ldx = x.shape, (x.shape[1] if x.ndim == 2 else 0)
        if shape != want:
            raise ValueError(f"data has shape {shape}, context expects {want}")
        kind, mptr, ldm = MASK_NONE, None, 0
        if isinstance(mask, PackedBits):
            if mask.shape != shape:
                raise ValueError(f"a packed mask has the shape of the data: got {mask.shape}, data is {shape}")
            kind, mptr, ldm = MASK_BITS, mask.bits.ctypes.data_as(c_void_p), mask.ld
        elif mask is not None:
            mask = np.asarray(mask)
            if mask.shape != shape:
                mask = np.broadcast_to(mask, shape)        # Y * mask broadcasting, _solver.py:30
            if mask.dtype == np.bool_ or mask.dtype == np.uint8:
                mask = np.ascontiguousarray(mask).view(np.uint8)
                kind = MASK_U8
            else:
                mask = _f64c(mask)
                kind = MASK_F64
            mptr, ldm = mask.ctypes.data_as(c_void_p), mask.shape[1]
        flags = c_int(0)
        _check(self._lib.nbmf_upload_v(self._h, x.ctypes.data_as(c_void_p), x_kind, ldx, int(bool(transposed)),
                                       mptr, kind, ldm, byref(flags)))
        self.binary_path = bool(flags.value & FLAG_BINARY_PATH)
        return self.binary_path

    def upload_csr(self, x_pattern, mask_pattern=None, transposed=False):
        """Binary data from CSR patterns: ``x_pattern`` / ``mask_pattern`` are ``(indptr, indices)`` pairs of the
        user's matrix (rows = its rows) whose stored entries mean 1 / observed; no dense copy is made anywhere."""
        def prep(p):
            ip = np.ascontiguousarray(p[0], dtype=np.int64)
            ix = np.ascontiguousarray(p[1], dtype=np.int32)
            rows = self.n if transposed else self.m
            if ip.shape != (rows + 1,) or ix.shape != (int(ip[-1]),):
                raise ValueError(f"CSR pattern does not describe {rows} rows")
            return ip, ix
        ip, ix = prep(x_pattern)
        mp, mx = prep(mask_pattern) if mask_pattern is not None else (None, None)
        flags = c_int(0)
        _check(self._lib.nbmf_upload_csr(
            self._h, ip.ctypes.data_as(c_void_p), ix.ctypes.data_as(c_void_p), int(ix.size), int(bool(transposed)),
            None if mp is None else mp.ctypes.data_as(c_void_p), None if mx is None else mx.ctypes.data_as(c_void_p),
            0 if mx is None else int(mx.size), byref(flags)))
        self.binary_path = True
        return True

    def generate(self, seed, density=0.25, observed=1.0, row0=0, col0=0, n_global=None):
        """Fill the context with synthetic binary data generated on the device (see synthetic_reference); with
        ``row0`` / ``col0`` / ``n_global`` the context holds that slice of a larger matrix ``n_global`` columns wide
        (every rank of a sharded run generates its own rows of the same global matrix)."""
        _check(self._lib.nbmf_generate_slice(self._h, int(seed), float(density), float(observed), int(row0), int(col0),
                                             int(self.n if n_global is None else n_global)))
        self.binary_path = True

    def set_storage(self, storage="auto"):
        """Hold the next :meth:`upload` to a storage path: "auto" (byte codes when the data allow), "f64" (doubles even
        for binary values: the reference's arithmetic for real-valued V), "f64w" (doubles plus float64 weight tiles)."""
        if storage not in STORAGE:
            raise ValueError(f"storage must be one of {list(STORAGE)}")
        _check(self._lib.nbmf_set_storage(self._h, STORAGE[storage]))

    def n_obs(self):
        v = c_double(0)
        _check(self._lib.nbmf_get_n_obs(self._h, byref(v)))
        return v.value

    def set_factors(self, W_kxm, H_kxn):
        W, H = _f64c(W_kxm), _f64c(H_kxn)
        if W.shape != (self.k, self.m) or H.shape != (self.k, self.n):
            raise ValueError(f"factor shapes {W.shape}, {H.shape} do not match (k,m)=({self.k},{self.m}), "
                             f"(k,n)=({self.k},{self.n})")
        _check(self._lib.nbmf_set_factors(self._h, W.ctypes.data_as(c_void_p), H.ctypes.data_as(c_void_p)))

    def get_factors(self):
        W = np.empty((self.k, self.m), dtype=np.float64)
        H = np.empty((self.k, self.n), dtype=np.float64)
        _check(self._lib.nbmf_get_factors(self._h, W.ctypes.data_as(c_void_p), H.ctypes.data_as(c_void_p)))
        return W, H

    def run(self, max_iter, tol):
        losses = np.empty(int(max_iter), dtype=np.float64)
        n_iter = c_int(0)
        _check(self._lib.nbmf_run(self._h, int(max_iter), float(tol), losses.ctypes.data_as(c_void_p), byref(n_iter)))
        return losses[: n_iter.value].copy(), n_iter.value

    def run_batch(self, alphas, betas, W0, H0, max_iter, tol):
        """Independent fits of this context's data, one per (alpha, beta, W0, H0) -- a prior grid, restarts -- as many at
        a time as the chip holds, in one launch per group (``nbmf_run_batch``).  ``W0`` is (P, k, m) or (k, m) (the same
        start for every problem), ``H0`` likewise.  Returns ``(losses, n_iter, W, H)``: a list of P loss curves, an int
        array, and the final factors (P, k, m) / (P, k, n).  Problem p's results are bitwise those of ``set_hyper`` +
        ``set_factors`` + ``run`` + ``get_factors``."""
        alphas = np.ascontiguousarray(np.atleast_1d(alphas), dtype=np.float64)
        P = alphas.size
        betas = np.ascontiguousarray(np.broadcast_to(np.atleast_1d(np.asarray(betas, dtype=np.float64)), (P,)))
        W0 = np.ascontiguousarray(np.broadcast_to(_f64c(W0), (P, self.k, self.m)))
        H0 = np.ascontiguousarray(np.broadcast_to(_f64c(H0), (P, self.k, self.n)))
        losses = np.zeros((P, int(max_iter)), dtype=np.float64)
        n_iter = np.zeros(P, dtype=np.int32)
        W = np.empty_like(W0)
        H = np.empty_like(H0)
        ptr = lambda a: a.ctypes.data_as(c_void_p)   # noqa: E731
        _check(self._lib.nbmf_run_batch(self._h, int(P), ptr(alphas), ptr(betas), ptr(W0), ptr(H0), int(max_iter), float(tol),
                                        ptr(losses), ptr(n_iter), ptr(W), ptr(H)))
        return [losses[p, :n_iter[p]].copy() for p in range(P)], n_iter, W, H

    def batch_stats(self):
        """(persistent launches made by run_batch on this context, problems they served)."""
        a, b = c_int(0), c_int(0)
        _check(self._lib.nbmf_batch_stats(self._h, byref(a), byref(b)))
        return a.value, b.value

    def sweep_info(self):
        """{"h_chunks", "h_blocks", "w_chunks", "w_blocks"}: how the two sweeps are cut (after an upload / generate)."""
        v = [c_int(0) for _ in range(4)]
        _check(self._lib.nbmf_sweep_info(self._h, *[byref(x) for x in v]))
        return dict(zip(("h_chunks", "h_blocks", "w_chunks", "w_blocks"), (x.value for x in v)))

    def w_only_steps(self, n_steps):
        _check(self._lib.nbmf_w_only_steps(self._h, int(n_steps)))

    def loss(self):
        v = c_double(0)
        _check(self._lib.nbmf_loss(self._h, byref(v)))
        return v.value

    def loglik(self, clip_theta=False):
        """Data log-likelihood sum of the current factors (no prior, not divided by n_obs);
        clip_theta clips W^T H to [0, 1] first (the reference's inverse_transform)."""
        v = c_double(0)
        _check(self._lib.nbmf_loglik(self._h, int(bool(clip_theta)), byref(v)))
        return v.value

    def loglik_strict(self):
        """Log-likelihood summed over observed entries only (held-out perplexity numerator)."""
        v = c_double(0)
        _check(self._lib.nbmf_loglik_strict(self._h, byref(v)))
        return v.value

    def predict_at(self, rows, cols, clip_theta=True):
        """Theta = W^T H of the current factors at the index pairs ``(rows[t], cols[t])`` of the internal m x n matrix
        (``nbmf_predict_at``): a float64 1-D array.  Needs factors, not data.  An index outside the matrix raises
        ``ValueError`` naming the lowest offending position; the context stays usable."""
        rows, cols = index_pairs(rows, cols)
        out = np.empty(rows.size, dtype=np.float64)
        _check(self._lib.nbmf_predict_at(self._h, rows.ctypes.data_as(c_void_p), cols.ctypes.data_as(c_void_p), int(rows.size),
                                         int(bool(clip_theta)), out.ctypes.data_as(c_void_p)))
        return out

    def set_eval(self, rows, cols, x, every=10, patience=0):
        """Keep the held-out entries ``(rows[t], cols[t])`` of the internal m x n matrix and their truth ``x[t]`` (nonzero
        means 1) on the device (``nbmf_set_eval``): :meth:`eval_loglik` sums their log-likelihood there, and :meth:`run`
        evaluates them every ``every`` iterations, keeps the best factors and, with ``patience > 0``, ends at the
        ``patience``-th consecutive evaluation that does not improve (:meth:`eval_curve`, :meth:`best_factors`).  An empty
        set switches evaluation off.  A pair outside the matrix raises ``ValueError`` naming the lowest offending
        position, and the eval set in place stays."""
        rows, cols = index_pairs(rows, cols)
        x = np.asarray(x)
        if x.shape != rows.shape:
            raise ValueError(f"x must be as long as rows and cols (got {x.size} and {rows.size})")
        x = np.ascontiguousarray(x != 0).view(np.uint8)
        ptr = lambda a: a.ctypes.data_as(c_void_p)   # noqa: E731
        _check(self._lib.nbmf_set_eval(self._h, ptr(rows), ptr(cols), ptr(x), int(rows.size), int(every), int(patience)))

    def eval_loglik(self):
        """The Bernoulli log-likelihood sum of the eval set under the factors the context holds now
        (``nbmf_eval_loglik``): Theta at each pair is bit for bit :meth:`predict_at` with ``clip_theta=False``."""
        v = c_double(0)
        _check(self._lib.nbmf_eval_loglik(self._h, byref(v)))
        return v.value

    def eval_curve(self):
        """What the last :meth:`run` recorded (``nbmf_get_eval``): ``(iters, logliks, best_iter, stopped_early)`` -- the
        labels (iterations the evaluated factors had had; the last one equals ``n_iter``) as an int array, the sums as a
        float64 array, the label of the best evaluation and whether the patience rule ended the run."""
        n, best, early = c_int(0), c_int(0), c_int(0)
        _check(self._lib.nbmf_get_eval(self._h, 0, byref(n), None, None, None, None))
        iters = np.zeros(n.value, dtype=np.intc)
        logliks = np.zeros(n.value, dtype=np.float64)
        _check(self._lib.nbmf_get_eval(self._h, n.value, byref(n), iters.ctypes.data_as(c_void_p),
                                       logliks.ctypes.data_as(c_void_p), byref(best), byref(early)))
        return iters.astype(np.int64), logliks, best.value, bool(early.value)

    def best_factors(self):
        """The factors at the best evaluation of the last :meth:`run`, laid out as :meth:`get_factors` does
        (``nbmf_get_best_factors``)."""
        W = np.empty((self.k, self.m), dtype=np.float64)
        H = np.empty((self.k, self.n), dtype=np.float64)
        _check(self._lib.nbmf_get_best_factors(self._h, W.ctypes.data_as(c_void_p), H.ctypes.data_as(c_void_p)))
        return W, H

    def hold_out(self, seed, lo, hi, transposed=False, every=10, patience=0):
        """Draw the held-out split on the device (``nbmf_hold_out``): every observed entry of the data the context holds
        whose salted counter-based uniform lies in ``[lo, hi)`` -- :func:`holdout_reference` is the rule in NumPy, in the
        USER's shape; ``transposed`` says that the user's matrix is the transpose of the internal one -- becomes
        unobserved, and the list of them becomes the eval set, as :meth:`set_eval` with the pairs ``np.nonzero`` gives
        for the internal matrix would have installed it.  Returns how many entries are held out.  Needs binary data on
        the byte-code path; a split that holds out nothing, or everything observed, raises ``ValueError`` and changes
        nothing.  :meth:`hold_out_undo` puts the entries back."""
        count = c_int64(0)
        _check(self._lib.nbmf_hold_out(self._h, sample_seed(seed), int(bool(transposed)), float(lo), float(hi), int(every),
                                       int(patience), byref(count)))
        return count.value

    def hold_out_undo(self):
        """Make the held-out entries observed again and release the eval set (``nbmf_hold_out_undo``): the context is as
        it was before :meth:`hold_out`, with no new upload."""
        _check(self._lib.nbmf_hold_out_undo(self._h))

    def eval_pairs(self):
        """The eval set the context holds (``nbmf_get_eval_pairs``), from :meth:`hold_out` or :meth:`set_eval`:
        ``(rows, cols, x)`` as int64 / int64 / uint8 arrays in internal coordinates, empty without one."""
        n = c_int64(0)
        _check(self._lib.nbmf_get_eval_pairs(self._h, 0, byref(n), None, None, None))
        rows, cols, x = np.zeros(n.value, np.int64), np.zeros(n.value, np.int64), np.zeros(n.value, np.uint8)
        ptr = lambda a: a.ctypes.data_as(c_void_p)   # noqa: E731
        _check(self._lib.nbmf_get_eval_pairs(self._h, n.value, byref(n), ptr(rows), ptr(cols), ptr(x)))
        return rows, cols, x

    def _rows(self, row0, nrows):
        """``(row0, nrows)`` of a row-slab call as ints, ``nrows`` defaulting to the rest of the matrix: inside ``[0, m)``,
        or the library's own ``ValueError``."""
        row0 = int(row0)
        nrows = self.m - row0 if nrows is None else int(nrows)
        if row0 < 0 or nrows < 0 or row0 + nrows > self.m:
            raise ValueError(f"rows [{row0}, {row0} + {nrows}) are not inside [0, {self.m})")
        return row0, nrows

    def _mask_rows(self, mask, nrows):
        """The ``mask`` of a row-slab call as the library takes it: ``(pointer, mask kind, leading dimension)``; the array
        behind the pointer is the caller's own, which outlives the call."""
        if mask is None:
            return None, MASK_NONE, 0
        m, kind, ld = row_array(mask, nrows, self.n, "mask", BYTE_KINDS, packed=True)
        return m.ctypes.data_as(c_void_p), MASK_BITS if kind == DATA_BITS else MASK_U8, ld

    def predict_rows(self, row0=0, nrows=None, clip_theta=True, threshold=None, out=None):
        """Theta for rows ``[row0, row0 + nrows)`` and all n columns (``nbmf_predict_rows``): a float64 ``(nrows, n)``
        array, or with a ``threshold`` the bool array ``Theta > threshold``, compared on the device (one byte per entry
        comes back).  ``out``, if given, is written and returned: shape ``(nrows, n)``, float64 (bool or uint8 with a
        threshold), unit stride along a row and any row stride of at least n elements -- a slice of a wider array is fine,
        and nothing outside the slice is touched."""
        row0, nrows = self._rows(row0, nrows)
        byte_kind = threshold is not None
        if out is None:
            out = np.empty((nrows, self.n), dtype=np.bool_ if byte_kind else np.float64)
        elif not isinstance(out, np.ndarray):
            raise ValueError(f"out must be a NumPy array: it is written in place (got {type(out).__name__})")
        ld = row_array(out, nrows, self.n, "out", BYTE_KINDS if byte_kind else (np.float64,))[2]
        _check(self._lib.nbmf_predict_rows(self._h, row0, nrows, int(bool(clip_theta)), PREDICT_U8 if byte_kind else PREDICT_F64,
                                           float(threshold) if byte_kind else 0.0, out.ctypes.data_as(c_void_p), ld))
        return out

    def theta_bits(self, row0=0, nrows=None, *, threshold=None, seed=None, clip_theta=True, out=None):
        """A yes / no decision per entry of Theta for rows ``[row0, row0 + nrows)`` and all n columns, decided and packed
        on the device (``nbmf_theta_bits``): a :class:`PackedBits` of shape ``(nrows, n)`` -- one bit per entry comes back.
        Exactly one of ``threshold`` (the bits of ``predict_rows(threshold=...)``: ``Theta > threshold``, strictly) and
        ``seed`` (an int in ``[0, 2**64)``: one draw of Bernoulli(Theta), ``hash_uniform(m, n, seed) < Theta``) is given.
        ``out``, if given, receives the bytes and backs the result: a uint8 array of shape ``(nrows, ceil(n / 8))``, unit
        stride along a row and any row stride of at least ``ceil(n / 8)`` bytes -- a slice of a wider array is fine, and
        nothing outside the slice is touched.  The pad bits of a row's last byte are zeros: ``.bits`` equals
        ``np.packbits(dense, axis=1)``."""
        row0, nrows = self._rows(row0, nrows)
        if (threshold is None) == (seed is None):
            raise ValueError("give exactly one of threshold and seed")
        if seed is not None:
            seed = sample_seed(seed)
        nb = (self.n + 7) // 8
        if out is None:
            out = np.empty((nrows, nb), dtype=np.uint8)
        elif not isinstance(out, np.ndarray):
            raise ValueError(f"out must be a NumPy array: it is written in place (got {type(out).__name__})")
        ld = row_array(out, nrows, nb, "out", (np.uint8,))[2]
        _check(self._lib.nbmf_theta_bits(self._h, row0, nrows, int(bool(clip_theta)), BITS_THRESHOLD if seed is None else BITS_SAMPLE,
                                         0.0 if threshold is None else float(threshold), seed or 0,
                                         out.ctypes.data_as(c_void_p), ld))
        return PackedBits(out, (nrows, self.n))

    def top_n(self, top, row0=0, nrows=None, exclude=None, clip_theta=True, return_scores=True):
        """The ``top`` columns with the largest Theta in each of the rows ``[row0, row0 + nrows)``, ranked on the device
        (``nbmf_top_n``): ``(cols, scores)``, ``cols`` int64 ``(nrows, top)`` and ``scores`` float64 of the same shape (None
        without ``return_scores``).  Slot s of a row holds the s-th column in the order "Theta descending, ties by
        ascending column" and its Theta, bit for bit the entry :meth:`predict_rows` returns.  ``exclude``: a bool or uint8
        array of shape ``(nrows, n)``, nonzero = never return this column (unit stride along a row, any row stride of at
        least n: a slice of a wider array is fine), or a :class:`PackedBits` of that shape (unpacked on the device: the same
        result).  A NaN Theta is never returned.  A row with fewer than ``top`` columns
        left ends in column -1 / score NaN.  Only ``top`` entries per row come back from the device, not n."""
        top = top_n_count(top)
        row0, nrows = self._rows(row0, nrows)
        xptr, xkind, ldx = None, DATA_U8, 0
        if exclude is not None:
            exclude, xkind, ldx = row_array(exclude, nrows, self.n, "exclude", BYTE_KINDS, packed=True)
            xptr = exclude.ctypes.data_as(c_void_p)
        cols = np.empty((nrows, top), dtype=np.int64)
        scores = np.empty((nrows, top), dtype=np.float64) if return_scores else None
        _check(self._lib.nbmf_top_n_v(self._h, row0, nrows, top, int(bool(clip_theta)), xptr, xkind, ldx,
                                      cols.ctypes.data_as(c_void_p), None if scores is None else scores.ctypes.data_as(c_void_p),
                                      top))
        return cols, scores

    def similarity(self, axis=1, metric="cosine", query=None, out=None):
        """The similarity of the ``query`` items to ALL items of one side of the matrix (``nbmf_similarity``): a float64
        ``(len(query), L)`` slab.  ``axis`` 0: the items are the m samples (the columns of the internal W), 1: the n features
        (the columns of H); L is m or n.  ``metric``: ``"dot"``, ``"cosine"`` (a zero vector scores 0 with everything, not
        NaN) or ``"profile"`` -- the cosine between the items' predicted profiles, their unclipped rows (samples) or
        columns (features) of Theta, which does not treat two correlated components as unrelated.  ``query``: integer
        indices in ``[0, L)``, any order, repeats allowed; None: all items in order.  ``out``, if given, is written and
        returned: float64 of shape ``(len(query), L)``, unit stride along a row, any row stride of at least L."""
        axis, metric = sim_axis(axis), sim_metric(metric)
        L = self.m if axis == 0 else self.n
        query, nq = item_query(query, L)
        if out is None:
            out = np.empty((nq, L), dtype=np.float64)
        elif not isinstance(out, np.ndarray):
            raise ValueError(f"out must be a NumPy array: it is written in place (got {type(out).__name__})")
        ld = row_array(out, nq, L, "out", (np.float64,))[2]
        _check(self._lib.nbmf_similarity(self._h, axis, metric, None if query is None else query.ctypes.data_as(c_void_p), nq,
                                         out.ctypes.data_as(c_void_p), ld))
        return out

    def neighbors(self, top, axis=1, metric="cosine", query=None, skip_self=True, return_scores=True):
        """The ``top`` items most similar to each ``query`` item, ranked on the device (``nbmf_neighbors``):
        ``(idx, scores)``, int64 and float64 of shape ``(len(query), top)`` (scores None without ``return_scores``).
        ``axis``, ``metric`` and ``query`` as in :meth:`similarity`; slot s of a row holds the s-th item in the order "score
        descending, ties by ascending index" and its score, bit for bit the entry :meth:`similarity` returns.  With
        ``skip_self`` the query item itself is never returned -- by index: another item with the same vector is, and
        ties by index.  A NaN score is never returned; a row with fewer than ``top`` items left ends in -1 / NaN."""
        top = top_n_count(top)
        axis, metric = sim_axis(axis), sim_metric(metric)
        if not isinstance(skip_self, (bool, np.bool_)):
            raise ValueError(f"skip_self must be a bool (got {skip_self!r})")
        query, nq = item_query(query, self.m if axis == 0 else self.n)
        idx = np.empty((nq, top), dtype=np.int64)
        scores = np.empty((nq, top), dtype=np.float64) if return_scores else None
        _check(self._lib.nbmf_neighbors(self._h, axis, metric, None if query is None else query.ctypes.data_as(c_void_p), nq, top,
                                        int(bool(skip_self)), idx.ctypes.data_as(c_void_p),
                                        None if scores is None else scores.ctypes.data_as(c_void_p), top))
        return idx, scores

    def score_rows(self, x, mask=None, row0=0, nrows=None, clip_theta=True, eps=1e-8, rows=True, cols=False):
        """The Bernoulli log-likelihood of Theta against the data ``x`` of the rows ``[row0, row0 + nrows)``, summed per
        row and / or per column on the device (``nbmf_score_rows``): ``(row_ll, row_obs, col_ll, col_obs)``, float64 sums and
        int64 counts of the observed entries, ``nrows`` long for the rows and ``n`` long for the columns; None for the pair
        not asked for (``rows`` / ``cols``).  ``x``: shape ``(nrows, n)``, bool / uint8 (nonzero means 1; the term is
        ``log(x ? theta + eps : (1 - theta) + eps)``) or float64 in [0, 1] (``x log(theta + eps) + (1 - x) log((1 - theta)
        + eps)``).  ``mask``: bool / uint8 of the same shape, nonzero = observed; None: every entry.  Both may be slices of
        wider arrays (unit stride along a row); nothing is copied on the host.  Either may be a :class:`PackedBits` of that
        shape instead (one bit per entry up, unpacked on the device: the same sums and counts).  Theta is bit for bit what
        :meth:`predict_rows` returns.  Only ``nrows + n`` sums and counts come back from the device."""
        row0, nrows = self._rows(row0, nrows)
        if not rows and not cols:
            raise ValueError("nothing requested: rows and cols are both false")
        eps = float(eps)
        if not eps >= 0.0:
            raise ValueError(f"eps must be >= 0 (got {eps})")
        x, x_kind, ldx = row_array(x, nrows, self.n, "x", ANY_KINDS, packed=True)
        mptr, mkind, ldm = self._mask_rows(mask, nrows)
        row_ll = np.empty(nrows, dtype=np.float64) if rows else None
        row_obs = np.empty(nrows, dtype=np.int64) if rows else None
        col_ll = np.empty(self.n, dtype=np.float64) if cols else None
        col_obs = np.empty(self.n, dtype=np.int64) if cols else None
        ptr = lambda a: None if a is None else a.ctypes.data_as(c_void_p)   # noqa: E731
        _check(self._lib.nbmf_score_rows_v(self._h, row0, nrows, int(bool(clip_theta)), eps, ptr(x), x_kind, ldx, mptr, mkind, ldm,
                                           ptr(row_ll), ptr(row_obs), ptr(col_ll), ptr(col_obs)))
        return row_ll, row_obs, col_ll, col_obs

    def theta_hist(self, x, mask=None, row0=0, nrows=None, bins=256):
        """The observed entries of the rows ``[row0, row0 + nrows)`` of the binary data ``x``, counted on the device by
        class and by the Theta they got (``nbmf_theta_hist``): ``(hist, nan_count)``, int64 of shape ``(2, bins)`` and
        ``(2,)``.  ``hist[c, b]`` counts the observed entries of class ``c = (x != 0)`` whose Theta, clipped to [0, 1], has
        ``min(int(theta * bins), bins - 1) == b``: bin b is ``[b / bins, (b + 1) / bins)``, the last one holds 1 as well.
        A NaN Theta is counted in ``nan_count[c]`` instead.  ``x``: bool / uint8 of shape ``(nrows, n)``; ``mask``: the
        same, nonzero = observed, None: every entry.  Both may be slices of wider arrays (unit stride along a row); nothing
        is copied on the host; either may be a :class:`PackedBits` of that shape instead (the same counts).  Theta is bit for bit what :meth:`predict_rows` returns.  The counts are exact: the same
        whatever the panels and the order of the device's additions, and those of disjoint row ranges add up.  Only
        ``2 * bins + 2`` integers come back from the device."""
        row0, nrows = self._rows(row0, nrows)
        bins = hist_bins(bins)
        x, x_kind, ldx = row_array(x, nrows, self.n, "x", BYTE_KINDS, packed=True)
        mptr, mkind, ldm = self._mask_rows(mask, nrows)
        hist = np.empty((2, bins), dtype=np.int64)
        nan_count = np.empty(2, dtype=np.int64)
        _check(self._lib.nbmf_theta_hist_v(self._h, row0, nrows, bins, x.ctypes.data_as(c_void_p), x_kind, ldx, mptr, mkind, ldm,
                                           hist.ctypes.data_as(c_void_p), nan_count.ctypes.data_as(c_void_p)))
        return hist, nan_count

    def moments(self, x, mask=None, groups=None, n_groups=None, row0=0, nrows=None, rows=True, cols=False):
        """The observed entries of the rows ``[row0, row0 + nrows)`` of the binary data ``x``, summed on the device by
        (row, column group) and / or by column (``nbmf_moment_rows_v``): ``(row_tab, col_tab, nan_count)``, int64 of shape
        ``(nrows, n_groups, 5)``, ``(n, 5)`` and ``(2,)``; None for a table not asked for (``rows`` / ``cols``).  The last
        axis is ``MOMENT_FIELDS``: the observed entries of the slot, the ones among them, ``S1 = sum rint(theta * 2**32)``,
        ``S2 = sum rint((theta * theta) * 2**32)`` and S1 over the ones alone -- ``S1 / 2**32`` is the number of ones the
        model expects in the slot and ``(S1 - S2) / 2**32`` its variance (:class:`~nbmf_mm_amd._metrics.Moments`).  An entry
        whose Theta is NaN is counted in ``nan_count[x != 0]`` instead.  ``groups``: an integer array of ``n`` labels in
        ``[-1, n_groups)``, -1 = in no group (such a column still counts in ``col_tab``); None: one group of all columns.
        ``n_groups`` (default ``max label + 1``) is at most 16.  ``x`` and ``mask`` as in :meth:`theta_hist`: bool / uint8
        of shape ``(nrows, n)``, slices of wider arrays are fine, or :class:`PackedBits` (the same arrays).  Theta is bit
        for bit what :meth:`predict_rows` returns, clipped.  The sums are exact integers: the same whatever the panels and
        the order of the device's additions, and ``col_tab`` of disjoint row ranges adds up."""
        row0, nrows = self._rows(row0, nrows)
        if not rows and not cols:
            raise ValueError("nothing requested: rows and cols are both false")
        labels, n_groups = group_labels(groups, self.n, n_groups, most=MOMENT_MAX_GROUPS)
        x, x_kind, ldx = row_array(x, nrows, self.n, "x", BYTE_KINDS, packed=True)
        mptr, mkind, ldm = self._mask_rows(mask, nrows)
        row_tab = np.empty((nrows, n_groups, len(MOMENT_FIELDS)), dtype=np.int64) if rows else None
        col_tab = np.empty((self.n, len(MOMENT_FIELDS)), dtype=np.int64) if cols else None
        nan_count = np.empty(2, dtype=np.int64)
        ptr = lambda a: None if a is None else a.ctypes.data_as(c_void_p)   # noqa: E731
        _check(self._lib.nbmf_moment_rows_v(self._h, row0, nrows, ptr(x), x_kind, ldx, mptr, mkind, ldm,
                                            None if groups is None else ptr(labels), n_groups, ptr(row_tab), ptr(col_tab),
                                            ptr(nan_count)))
        return row_tab, col_tab, nan_count

    def top_pairs(self, top, kind="theta", x=None, mask=None, row0=0, nrows=None, clip_theta=True, return_scores=True):
        """The ``top`` best entries of Theta over ALL of the rows ``[row0, row0 + nrows)``, selected on the device
        (``nbmf_top_pairs``): ``(rows, cols, scores)``, int64, int64 and float64 (None without ``return_scores``), each
        ``count = min(top, eligible entries)`` long; ``rows`` are absolute row numbers.  ``kind="theta"``: the largest
        Theta first; ``x`` is an exclude matrix (nonzero = never return this entry) or None, and there is no mask.
        ``kind="likelihood"``: ``x`` is the binary data, the score is ``Theta`` where ``x != 0`` and ``1 - Theta`` elsewhere
        -- the probability the model gave to what was observed -- the smallest first, over the entries ``mask`` marks
        (None: all).  The order is score, then row, then column (-0.0 ties +0.0); a NaN score is never returned; Theta is
        bit for bit what :meth:`predict_rows` returns.  ``x`` and ``mask``: bool / uint8 of shape ``(nrows, n)`` (slices of
        wider arrays are fine) or a :class:`PackedBits` of that shape (the same result).  Only ``count`` entries come back
        from the device; no Theta panel is stored."""
        top = top_pairs_count(top)
        if kind not in ("theta", "likelihood"):
            raise ValueError(f'kind must be "theta" or "likelihood" (got {kind!r})')
        row0, nrows = self._rows(row0, nrows)
        if kind == "theta" and mask is not None:
            raise ValueError('kind="theta" takes an exclude matrix as x, not a mask')
        if kind == "likelihood" and x is None:
            raise ValueError('kind="likelihood" needs the data x')
        xptr, xkind, ldx = None, DATA_U8, 0
        if x is not None:
            x, xkind, ldx = row_array(x, nrows, self.n, "x", BYTE_KINDS, packed=True)
            xptr = x.ctypes.data_as(c_void_p)
        mptr, mkind, ldm = self._mask_rows(mask, nrows)
        rows = np.empty(top, dtype=np.int64)
        cols = np.empty(top, dtype=np.int64)
        scores = np.empty(top, dtype=np.float64) if return_scores else None
        count = c_int64(0)
        _check(self._lib.nbmf_top_pairs(self._h, row0, nrows, top, int(bool(clip_theta)),
                                        PAIRS_THETA if kind == "theta" else PAIRS_LIKELIHOOD, xptr, xkind, ldx, mptr, mkind, ldm,
                                        rows.ctypes.data_as(c_void_p), cols.ctypes.data_as(c_void_p),
                                        None if scores is None else scores.ctypes.data_as(c_void_p), byref(count)))
        cnt = int(count.value)
        return rows[:cnt].copy(), cols[:cnt].copy(), None if scores is None else scores[:cnt].copy()

    def rank_of(self, indptr, indices, row0=0, nrows=None, exclude=None, clip_theta=True):
        """Where given columns stand in the order :meth:`top_n` ranks their row by, counted on the device
        (``nbmf_rank_rows``): ``(rank, above, tied, scores, eligible)``.  The TARGETS of row ``row0 + r`` are the columns
        ``indices[indptr[r]:indptr[r + 1]]`` (a CSR slice; ``indptr[0]`` may be above 0), in any order, repeats allowed.
        The first four arrays are indexed like ``indices`` and ``indptr[-1]`` long (int64, ``scores`` float64); positions
        below ``indptr[0]`` hold -1 / NaN.  ``eligible`` (int64, ``nrows``) counts the columns of the row that are neither
        NaN nor excluded.  Over those columns, for a target j that is one of them: ``above`` columns have a larger Theta,
        ``tied`` other columns an equal one, and ``rank = above +`` the tied columns left of j -- 0-based, the slot
        :meth:`top_n` would put j in, at any depth.  ``scores`` is Theta at the target, bit for bit the entry
        :meth:`predict_rows` returns.  A target that is itself excluded or NaN gets -1 / -1 / -1 and its Theta.
        ``exclude`` as in :meth:`top_n` (a :class:`PackedBits` included).  The cost of a row is ``ceil(targets / 8)`` passes over its n columns; only a few
        integers per target come back from the device."""
        row0, nrows = self._rows(row0, nrows)
        indptr, indices = csr_targets(indptr, indices, nrows, self.n)
        xptr, xkind, ldx = None, DATA_U8, 0
        if exclude is not None:
            exclude, xkind, ldx = row_array(exclude, nrows, self.n, "exclude", BYTE_KINDS, packed=True)
            xptr = exclude.ctypes.data_as(c_void_p)
        count = int(indptr[-1])
        rank, above, tied = (np.full(count, -1, dtype=np.int64) for _ in range(3))
        scores = np.full(count, np.nan)
        eligible = np.empty(nrows, dtype=np.int64)
        ptr = lambda a: a.ctypes.data_as(c_void_p)   # noqa: E731
        _check(self._lib.nbmf_rank_rows_v(self._h, row0, nrows, int(bool(clip_theta)), ptr(indptr), ptr(indices), xptr, xkind, ldx,
                                          ptr(rank), ptr(above), ptr(tied), ptr(scores), ptr(eligible)))
        return rank, above, tied, scores, eligible

    def comm_init(self, uid: bytes, nranks: int, rank: int, shard_axis: int = 0):
        """Attach an RCCL communicator; shard_axis 0 = rows of the internal Y are split, 1 = columns."""
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        _check(self._lib.nbmf_comm_init(self._h, buf, int(nranks), int(rank), int(shard_axis)))

    def comm_init_host(self, allreduce, nranks: int, rank: int, shard_axis: int = 0):
        """Attach a host-mediated all-reduce: ``allreduce(arr)`` must sum the float64 NumPy array
        ``arr`` over all ranks IN PLACE (e.g. gloo).  Same device work as the RCCL path."""
        def _cb(_user, ptr, count):
            try:
                arr = np.ctypeslib.as_array(ptr, shape=(int(count),))
                allreduce(arr)
                return 0
            except Exception:      # never unwind through the C frame
                import traceback
                traceback.print_exc()
                return 1
        self._host_cb = HOST_ALLREDUCE_FN(_cb)          # keep alive as long as the context
        _check(self._lib.nbmf_comm_init_host(self._h, self._host_cb, None, int(nranks), int(rank), int(shard_axis)))

    def peer_export(self, shard_axis: int = 0) -> bytes:
        """Allocate this rank's exchange arena for the peer (xGMI) transport and return its opaque
        PEER_HANDLE_BYTES handle block; all-gather the blocks in rank order and pass them to
        :meth:`comm_init_peer`."""
        buf = ctypes.create_string_buffer(PEER_HANDLE_BYTES)
        _check(self._lib.nbmf_peer_export(self._h, int(shard_axis), buf))
        return buf.raw

    def comm_init_peer(self, handles: bytes, nranks: int, rank: int, shard_axis: int = 0):
        """Attach the peer transport (one process per rank); on failure the context stays unattached."""
        handles = bytes(handles)
        if len(handles) != PEER_HANDLE_BYTES * int(nranks):
            raise ValueError(f"expected {PEER_HANDLE_BYTES} handle bytes per rank")
        buf = ctypes.create_string_buffer(handles, len(handles))
        _check(self._lib.nbmf_comm_init_peer(self._h, buf, int(nranks), int(rank), int(shard_axis)))

    def set_exchange_panels(self, panels=0):
        """Row split: exchange in 1 or 2 column panels at the next attach (0 = default); same on every rank."""
        _check(self._lib.nbmf_set_exchange_panels(self._h, int(panels)))

    def set_peer_timeout_ms(self, ms=0.0):
        """Bound on every wait of the peer transport attached next (0 = default: NBMF_PEER_TIMEOUT_MS or 30 s)."""
        _check(self._lib.nbmf_set_peer_timeout_ms(self._h, float(ms)))

    def comm_detach(self):
        """Drop the attached communicator; every rank must do the same."""
        _check(self._lib.nbmf_comm_detach(self._h))
        self._host_cb = None

    def cancel(self):
        """From ANOTHER thread: make the owner's ``run`` return (NBMFHipError "cancelled") at its next iteration boundary and
        cut short what it has enqueued (``nbmf_cancel``).  Sticky: the context can only be closed afterwards."""
        if self._h:
            _check(self._lib.nbmf_cancel(self._h))

    COMM_KINDS = {0: "none", 1: "rccl", 2: "peer", 3: "host"}

    def comm_info(self):
        """What the attached transport itself reports (``nbmf_comm_info``): ``{"kind", "nranks_seen", "remote"}`` --
        RCCL: ncclCommCount / ncclCommCuDevice of the communicator (-1 where librccl lacks the symbol); peer: arenas
        mapped (own included) / how many of them belong to other ranks; host: as given."""
        k, n, r = c_int(0), c_int(0), c_int(0)
        _check(self._lib.nbmf_comm_info(self._h, byref(k), byref(n), byref(r)))
        return {"kind": self.COMM_KINDS.get(k.value, str(k.value)), "nranks_seen": n.value, "remote": r.value}

    def timing_enable(self, on=True):
        """on: False / True, or an int n > 1 for the sweeps of every n-th iteration only."""
        _check(self._lib.nbmf_timing_enable(self._h, int(on) if not isinstance(on, bool) else int(on)))

    def timing(self):
        hm, wm, hn, wn = c_double(0), c_double(0), c_int(0), c_int(0)
        _check(self._lib.nbmf_timing_get(self._h, byref(hm), byref(hn), byref(wm), byref(wn)))
        return {"hpass_ms": hm.value, "hpass_launches": hn.value, "wpass_ms": wm.value, "wpass_launches": wn.value}

    def synchronize(self):
        _check(self._lib.nbmf_synchronize(self._h))

    def small_stats(self):
        """(runs served by the single-launch path for small problems, how many of those fell back)."""
        r, a = c_int(0), c_int(0)
        _check(self._lib.nbmf_small_stats(self._h, byref(r), byref(a)))
        return r.value, a.value

    def set_progress(self, callback=None, every=10):
        """``callback(first, losses)`` is called from inside :meth:`run` with the losses of iterations
        ``first, first+1, ...`` as they become final (every ``every`` iterations); None switches it off."""
        if callback is None:
            self._progress_cb = None
            _check(self._lib.nbmf_set_progress(self._h, PROGRESS_FN(), None, 0))
            return

        def _cb(_user, first, count, ptr):
            try:
                callback(int(first), [ptr[i] for i in range(int(count))])
            except Exception:      # never unwind through the C frame
                import traceback
                traceback.print_exc()
        self._progress_cb = PROGRESS_FN(_cb)             # keep alive as long as the context
        _check(self._lib.nbmf_set_progress(self._h, self._progress_cb, None, int(every)))


def device_synchronize(device=0):
    _check(load().nbmf_device_synchronize(int(device)))


def comm_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(load().nbmf_comm_unique_id(buf))
    return buf.raw


def engine_stats():
    """Process-wide: (fits the single-launch engine served, persistent launches that gave up, nbmf_run calls the
    launch-per-kernel engine served)."""
    a, b, c = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
    _check(load().nbmf_engine_stats(byref(a), byref(b), byref(c)))
    return a.value, b.value, c.value


def variant_stats():
    """Process-wide: (sweeps launched in the two-state W variant, sweeps launched in the ragged-K variant, runs that resumed
    after a sweep could not assemble a loss within its bound)."""
    a, b, c = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
    _check(load().nbmf_variant_stats(byref(a), byref(b), byref(c)))
    return a.value, b.value, c.value


def mfma_peak(device=0, target_ms=100.0):
    """The f64 MFMA rate of ``device`` as measured now: ``{"tflops", "cycles_per_mfma_at_2p4GHz", "launch_ms"}``
    (``nbmf_selftest_mfma_peak``: a loop of bare v_mfma_f64_16x16x4_f64, VGPR accumulators, all SIMDs)."""
    t, cy, ms = c_double(0), c_double(0), c_double(0)
    _check(load().nbmf_selftest_mfma_peak(int(device), float(target_ms), byref(t), byref(cy), byref(ms)))
    return {"tflops": t.value, "cycles_per_mfma_at_2p4GHz": cy.value, "launch_ms": ms.value}


def selftest_unary(op, x, device=0):
    """Apply a device scalar routine of the pass kernel (0: Newton reciprocal, 1: log) to `x` (GPU tests)."""
    d = _f64c(x).ravel()
    out = np.empty_like(d)
    _check(load().nbmf_selftest_unary(int(device), int(op), int(d.size), d.ctypes.data_as(c_void_p),
                                      out.ctypes.data_as(c_void_p)))
    return out


def selftest_unpack_bits(bits, n, out, device=0):
    """Run the kernel that unpacks bit-packed operands on ``bits`` (2-D uint8, C-contiguous: ``shape[1]`` is its leading
    dimension, at least ``ceil(n / 8)``) into ``out`` (2-D uint8, C-contiguous, as many rows, ``shape[1] >= n`` its leading
    dimension), in place: ``out`` goes to the device whole and comes back whole (GPU tests)."""
    for name, a in (("bits", bits), ("out", out)):
        if not (isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.ndim == 2 and a.flags.c_contiguous):
            raise ValueError(f"{name} must be a C-contiguous 2-D uint8 array")
    if bits.shape[0] != out.shape[0]:
        raise ValueError(f"bits has {bits.shape[0]} rows, out has {out.shape[0]}")
    _check(load().nbmf_selftest_unpack_bits(int(device), bits.ctypes.data_as(c_void_p), bits.shape[1], bits.shape[0], int(n),
                                            out.ctypes.data_as(c_void_p), out.shape[1]))
    return out


def _hash_u01(m, n, seed, rows, cols, salt=0):
    """A uniform of the device's counter-based generator (``synth_code`` in nbmf_pack_kernels.inc) for the m x n matrix or
    its sub-matrix ``[rows][:, cols]``: the top 53 bits of splitmix64 of ``(seed * 0x100000001B3 + i * n + j) ^ salt``
    (arithmetic modulo 2^64) times 2^-53."""
    def mix(x):
        x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))
    ri = np.arange(m, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)
    ci = np.arange(n, dtype=np.uint64) if cols is None else np.asarray(cols, dtype=np.uint64)
    with np.errstate(over="ignore"):
        idx = ri[:, None] * np.uint64(n) + ci[None, :]
        base = np.uint64(seed) * np.uint64(0x100000001B3) + idx
        return (mix(base ^ np.uint64(salt)) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def hash_uniform(m, n, seed, rows=None, cols=None):
    """The uniforms in [0, 1) that ``Context.generate`` and ``Context.theta_bits(seed=...)`` compare against, regenerated in
    NumPy: ``u[i, j] = (splitmix64(seed * 0x100000001B3 + i * n + j) >> 11) * 2**-53``, the arithmetic modulo 2**64, as a
    float64 ``(m, n)`` matrix, or its sub-matrix ``[rows][:, cols]`` when index arrays are given (entries are hashed
    independently, so a slice costs only its own size).  ``seed``: an int in ``[0, 2**64)``."""
    return _hash_u01(m, n, seed, rows, cols)


def synthetic_reference(m, n, seed, density=0.25, observed=1.0, rows=None, cols=None):
    """NumPy regeneration of ``Context.generate`` (same splitmix64 hash of (seed, i*n + j): :func:`hash_uniform`): returns
    (Y float64, mask bool) of the m x n matrix, or of its sub-matrix ``[rows][:, cols]`` when index
    arrays are given (entries are hashed independently, so a slice costs only its own size).
    For the tests; O(rows * cols) host memory."""
    u = hash_uniform(m, n, seed, rows, cols)
    v = _hash_u01(m, n, seed, rows, cols, salt=0xD6E8FEB86659FD93)      # the observed-or-not uniform of the same entry
    return (u < density).astype(np.float64), v < observed


def sample_seed(random_state):
    """The 64-bit seed of ``theta_bits(seed=...)`` / ``NBMF.sample`` from a ``random_state``, without a device: an int
    (not a bool) in ``[0, 2**64)`` is used as it is; ``None`` draws one from NumPy's global RNG, as ``transform`` draws its
    start.  Raises ``ValueError`` for anything else."""
    if random_state is None:
        return int.from_bytes(np.random.bytes(8), "little")
    if isinstance(random_state, (bool, np.bool_)) or not isinstance(random_state, (int, np.integer)):
        raise ValueError(f"random_state must be None or an integer in [0, 2**64) (got {random_state!r})")
    if not 0 <= int(random_state) < 2 ** 64:
        raise ValueError(f"random_state must be in [0, 2**64) (got {int(random_state)})")
    return int(random_state)


#: the salt of the hold-out uniform (``HO_SALT`` in nbmf_holdout_kernels.inc): a split is not the draw ``sample`` or ``generate`` made
HOLDOUT_SALT = 0xA0761D6478BD642F


def holdout_interval(holdout):
    """The interval ``(lo, hi)`` of a ``holdout`` argument, checked without a device: a float ``f`` in (0, 1) means
    ``(0.0, f)``, a pair ``(lo, hi)`` with ``0 <= lo < hi <= 1`` means itself.  Bools, NaN, ``lo >= hi`` and anything outside
    [0, 1] raise ``ValueError``."""
    def num(v):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"holdout must be a fraction in (0, 1) or a pair (lo, hi) of numbers (got {holdout!r})")
        v = float(v)
        if not 0.0 <= v <= 1.0:   # (NaN fails both comparisons)
            raise ValueError(f"holdout must lie in [0, 1] (got {holdout!r})")
        return v
    if isinstance(holdout, (tuple, list)):
        if len(holdout) != 2:
            raise ValueError(f"holdout must be a fraction in (0, 1) or a pair (lo, hi) (got {holdout!r})")
        lo, hi = num(holdout[0]), num(holdout[1])
    else:
        lo, hi = 0.0, num(holdout)
        if hi == 1.0:
            raise ValueError(f"a holdout fraction must lie in (0, 1): {holdout!r} leaves nothing to fit")
    if not lo < hi:
        raise ValueError(f"holdout must be a fraction in (0, 1) or a pair 0 <= lo < hi <= 1 (got {holdout!r})")
    return lo, hi


def holdout_reference(shape, seed, lo, hi, mask=None, rows=None, cols=None):
    """The entries ``Context.hold_out(seed, lo, hi)`` holds out, regenerated in NumPy: a bool matrix in the USER's shape
    ``(U, V)`` -- under ``orientation="dir-beta"`` too: the counter of the entry at row u, column v is ``u * V + v`` whatever
    the orientation -- true where the entry is observed (``mask`` nonzero; ``None``: everywhere) and
    ``lo <= (splitmix64((seed * 0x100000001B3 + u * V + v) ^ 0xA0761D6478BD642F) >> 11) * 2**-53 < hi``.  With index arrays
    ``rows`` / ``cols`` the sub-matrix ``[rows][:, cols]`` (``mask`` is then that sub-matrix's): entries are hashed
    independently, so a slice costs only its own size."""
    U, V = (int(d) for d in shape)
    u = _hash_u01(U, V, sample_seed(seed), rows, cols, salt=HOLDOUT_SALT)
    held = (u >= float(lo)) & (u < float(hi))
    if mask is not None:
        mask = np.asarray(mask)
        held &= np.broadcast_to(mask, held.shape) != 0
    return held
