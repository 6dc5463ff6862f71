// libnbmf_hip — NBMF-MM multiplicative-update inner loop for MI355X (gfx950 / CDNA4).
//
// What runs here (reference: siddC/nbmf_mm, src/nbmf_mm/_solver.py:5-59 and :143-175):
//   H-pass   one fused sweep over Y:  Theta = W^T H (f64 MFMA) -> ratios -> P1 = W R1, P2 = W R2
//            (f64 MFMA, Theta's accumulator registers are the B operands) + log-likelihood of the
//            CURRENT factors (= the loss of the previous iteration, _solver.py:148-155).
//   H-update k x n Beta-MAP update (_solver.py:42-47) + Beta log-prior sums (:158-159).
//   W-pass   one fused sweep over Y^T: Theta' = H'^T W -> ratios -> Q = H'(S1-S2)^T + 1 (x) sum S2
//            (algebraically _solver.py:53; one back-product instead of two).
//   W-update k x m multiplicative step, /n, column renormalise (_solver.py:53-57) or the Duchi
//            extension (README.md:27-35).
//   finalize loss assembly and the relative-change stop rule on device (_solver.py:162-174).
//
// Layout in HBM: Y is packed once into MFMA accumulator order, 16x16 tiles, one
// byte per entry on the binary path ({ym, zero-observed, valid} bits) or one double per entry,
// in two sweep orders (strip-major for each pass) so every wave streams contiguous memory.
// Factors are kept in natural [k][len] order plus two operand-ordered copies ("T": Theta operand,
// "G": gradient/back-product operand) so LDS staging is a linear copy and ds_reads are lane-linear.
//
// No BLAS, no PyTorch: plain HIP + (optionally, loaded at run time) RCCL.

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <dlfcn.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/nbmf_hip.h"

// Build switches.  Three, all for measurement or self-test builds; every experiment that was measured and rejected
// (two strips per wave, rotating priorities, even placement, the replicated logarithm table, register staging, IEEE /
// residual division, inline-assembly selects, 32 KiB stages, ...) lives in docs/HISTORY.md with the commit that last
// contained it, not here.
#ifndef NBMF_NO_MFMA
#define NBMF_NO_MFMA 0   // 1 = measurement build: the sweeps without their MFMAs (see NBMF_MFMA in nbmf_pass_kernel.inc)
#endif
#ifndef NBMF_HAZARD_SEED
#define NBMF_HAZARD_SEED 0   // 1 = compile a kernel with a deliberate MFMA-after-inline-assembly hazard (build self-test only)
#endif

namespace {

// ------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------
thread_local std::string g_err;
// which engine served the fits of this process (nbmf_engine_stats): fits the single-launch engine ran to the end,
// persistent launches that gave up, qualifying fits it declined because the context's kernel had given up before, and
// nbmf_run calls served by the launches
std::atomic<long long> g_engine_persistent_served{0}, g_engine_persistent_aborted{0}, g_engine_persistent_declined{0},
    g_engine_launches_served{0};

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  // A failed runtime call also leaves its code in the thread's "last error", which stays until somebody reads it: the
  // next launch check (HIPCHK(hipGetLastError())) of this thread -- in this context or any other -- would report it as its
  // own (an upload that ran out of memory made the NEXT, small, fit fail with "out of memory": tests/test_gpu_lifecycle.py).
  // Reading it here resets it.
  if (code == NBMF_ERR_HIP) (void)hipGetLastError();
  return code;
}

#define HIPCHK(call)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (call);                                                                       \
    if (e_ != hipSuccess)                                                                         \
      return fail(NBMF_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,  \
                  __LINE__);                                                                      \
  } while (0)

inline int64_t round_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// Environment switches: set at all, or its number (atoll / atof, as the C library parses it) with a default when unset.
// Each is read where the call that uses it runs (tests switch them between calls), or once per process where a
// `static const` holds it.
inline bool env_set(const char* name) { return getenv(name) != nullptr; }
template <typename T>
T env_int(const char* name, T dflt) {
  const char* e = getenv(name);
  return e ? (T)atoll(e) : dflt;
}
inline double env_double(const char* name, double dflt) {
  const char* e = getenv(name);
  return e ? atof(e) : dflt;
}

typedef double d4 __attribute__((ext_vector_type(4)));

enum { DATA_BIN = 0, DATA_F64 = 1, DATA_F64M = 2 };
enum { MODE_H = 0, MODE_W = 1, MODE_L = 2, MODE_T = 3 };

// code bits of the binary path
enum : unsigned { CB_YM = 1u, CB_ZOBS = 2u, CB_VALID = 4u };

constexpr int SLICE_K = 128;      // n_components beyond this run as slices of SLICE_K components
constexpr int PAD = 128;          // m and n are padded to multiples of 128 (8 row blocks, 8 strips)
constexpr int WG_WAVES = 4;   // waves (= column strips) per workgroup of the pass kernel; measured: 2-wave workgroups run 30 % slower (125 vs 179 it/s at c3)
constexpr size_t PASS_SLACK = 65536;   // bytes allocated behind every image the sweeps stream: their prefetch runs one stage (<= 32 KiB) past the last block
constexpr int STAGE_BYTES = 32768; // one LDS stage: NB row blocks x (T + G operand images); two stages per workgroup

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
// Reciprocal of d in [eps, 1+eps]: hardware seed + two Newton steps (<= 1 ulp; no scaling needed in
// this range).  Stands in for the IEEE divides of _solver.py:42-43,53 on the binary path, where the
// numerator is exactly 0 or 1.
__device__ __forceinline__ double rcp_nr(double d) {
  // seed, then one cubically convergent step: r1 = r0 (1 + e + e^2), e = 1 - d r0  (3 FMAs;
  // |e| <= 2^-20 for v_rcp_f64, so the truncation term e^3 is far below 1 ulp)
  double r = __builtin_amdgcn_rcp(d);
  const double e = __builtin_fma(-d, r, 1.0);
  const double p = __builtin_fma(e, e, e);
  return __builtin_fma(r, p, r);
}

// double from its two 32-bit halves / back (bit-level selects cost one VALU op per half)
__device__ __forceinline__ double mk_double(uint32_t lo, uint32_t hi) {
  return __hiloint2double((int)hi, (int)lo);
}

// Natural logarithm for the general (real-valued / weighted) path, where two logarithms per entry feed the
// loss and every VALU instruction adds to the f64 MFMA time: a 256-entry table in LDS plus a short series,
// 13 VALU instructions and one ds_read_b128 (the library routine: ~75; the fdlibm-style routine this replaces: ~35).
//   x = 2^e * m, m in [0.5, 1);  bin j = top 8 fraction bits of m;  table[j] = {c_j, -log(c_j)}, c_j = 1/(bin centre)
//   r = m c_j - 1 (one FMA, |r| <= 2^-9);  log x = e ln2 - log c_j + log1p(r),  log1p to r^5/5 (next term 2^-56.6)
// Absolute error <= 2.5e-16 + 1 ulp of the result (the table value and e ln2 are each rounded once): sums of
// millions of such terms of size ~0.5 keep the loss well inside its 1e-10 tolerance.  GUARD: arguments that are
// not positive normal numbers (1 - Theta + eps <= 0 needs factors off the simplex; eps is at least the smallest
// normal number) take the library routine: same NaN / -inf as NumPy.
// max(x, 0) with a NaN x giving 0 (v_max_f64 returns the operand that is a number): one instruction, where the
// compiler's fmax adds a canonicalising one in front for a value it has loaded from memory.
__device__ __forceinline__ double max0(double x) {
  double r;
  __asm__("v_max_f64 %0, %1, 0" : "=v"(r) : "v"(x));
  return r;
}
constexpr int LOG_TABLE_BYTES = 256 * 16;
// (TB index bits: 8 -> 256 entries and the series to r^5/5; 10 -> 1024 entries, |r| <= 2^-11, and the series to r^4/4 --
//  the next term is below 2^-57 -- one FMA fewer per logarithm where the table is there for the taking)
template <int TB>
__device__ __forceinline__ double2 log_table_entry(int j) {
  const double c = 1.0 / (0.5 + ((double)j + 0.5) * (1.0 / (double)(2 << TB)));
  return double2{c, -log(c)};
}
__device__ __forceinline__ void log_table_fill(double2* tab /* LDS, 256 entries; threads 0..255 */) {
  if (threadIdx.x < 256) tab[threadIdx.x] = log_table_entry<8>(threadIdx.x);
}
// (LDS_ABS: `tab` is not a pointer but the table's byte address in LDS, known at compile time -- the caller's kernel has
//  no static LDS, so its dynamic region starts at 0 -- and becomes the gather's immediate offset; through a pointer
//  derived from the dynamic region's symbol hipcc spends a vector add per gather on a base it cannot fold)
template <bool GUARD, int TB = 8, bool LDS_ABS = false, typename TAB = const double2*>
__device__ __forceinline__ double log_tab(double x, TAB tab, double c3 = 0.33333333333333331483, double c4 = -0.25) {
  static_assert(TB == 8 || TB == 10, "256 or 1024 entries");
  if (GUARD && __builtin_expect(!__builtin_amdgcn_class(x, 0x100), 0)) return log(x);   // not a positive normal number
  const uint32_t hi = (uint32_t)__double2hiint(x);
  const double m = __builtin_amdgcn_frexp_mant(x);   // in [0.5, 1); a NaN stays a NaN and so reaches the result
  const uint32_t off = (hi >> (16 - TB)) & (((1u << TB) - 1u) << 4);   // byte offset of the entry: two instructions
  double2 e;
  if constexpr (LDS_ABS) {
    typedef double d2raw __attribute__((ext_vector_type(2)));
    const d2raw v = *(const __attribute__((address_space(3))) d2raw*)(uintptr_t)(off + (uint32_t)tab);
    e = double2{v[0], v[1]};
  } else {
    e = *(const double2*)((const char*)tab + off);
  }
  const double r = __builtin_fma(m, e.x, -1.0);
  double p;
  if (TB == 8) {
    p = __builtin_fma(r, 0.2, -0.25);
    p = __builtin_fma(r, p, c3);
  } else {
    p = __builtin_fma(r, c4, c3);   // (callers in a hot loop hand both constants over in registers: two literals do not fit one instruction)
  }
  p = __builtin_fma(r, p, -0.5);
  p = __builtin_fma(r, p, 1.0);
  const double k = (double)__builtin_amdgcn_frexp_exp(x);
  return __builtin_fma(r, p, __builtin_fma(k, 0.69314718055994530942, e.y));
}
// The 1024-entry table, once per device and process in memory (a workgroup of the general path's sweeps copies it
// into LDS: 16 KiB from L2 instead of 1024 library logarithms).
__global__ __launch_bounds__(256) void log_table_kernel(double2* tab) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  tab[j] = log_table_entry<10>(j);
}

// log(prod) + pexp ln 2 for the running product of a sweep's likelihood (one call per lane and sweep), without a trip to
// memory (the library's logarithm reads tables from constant memory; in a workgroup's epilogue that is a chain of cold
// misses).  Mantissa m in [1/sqrt 2, sqrt 2), s = (m - 1) / (m + 1), log m = 2 s (1 + s^2/3 + ... + s^18/19): |s| <= 0.172,
// the next term is below 2^-55.  Absolute error <= 2.5e-16 + 1 ulp of the result (op 7 of nbmf_selftest_unary).  Zero,
// NaN, infinities and negative products take the library routine: NumPy's -inf / NaN.  (Built in round 4 on the suspicion
// that the H sweep's long epilogue -- 9 us against the W sweep's 2.7 at configs[1] -- was the library call; the finer trace
// says 5 us of it are the workgroup's waves waiting for each other at the loss block's barrier, and the sweep's time did
// not change.  Kept: it is deterministic, self-contained and no slower.)
__device__ __forceinline__ double log_of_product(double prod, int pexp) {
  const double m = __builtin_amdgcn_frexp_mant(prod);
  if (__builtin_expect(!(m >= 0.5 && m < 1.0), 0))   // (zero: m = 0; negative: m < 0; NaN and infinity: the comparisons fail)
    return log(prod) + (double)pexp * 0.6931471805599453094;
  int e = __builtin_amdgcn_frexp_exp(prod) + pexp;
  const bool low = m < 0.70710678118654752440;
  const double m2 = low ? m + m : m;
  e -= low ? 1 : 0;
  const double s = (m2 - 1.0) * rcp_nr(m2 + 1.0);
  const double w = s * s;
  double p = __builtin_fma(w, 1.0 / 19.0, 1.0 / 17.0);
  p = __builtin_fma(w, p, 1.0 / 15.0);
  p = __builtin_fma(w, p, 1.0 / 13.0);
  p = __builtin_fma(w, p, 1.0 / 11.0);
  p = __builtin_fma(w, p, 1.0 / 9.0);
  p = __builtin_fma(w, p, 1.0 / 7.0);
  p = __builtin_fma(w, p, 0.2);
  p = __builtin_fma(w, p, 0.33333333333333331483);
  p = __builtin_fma(w, p, 1.0);
  return __builtin_fma(s + s, p, (double)e * 0.69314718055994530942);
}

// Per-lane selects on a 64-bit wave mask, written out because the pass kernels are VALU-issue bound next to
// their MFMAs: a byte test is ONE SDWA compare (hipcc otherwise emits v_and + v_cmp), a double select is two
// v_cndmask_b32 (with the zero / negated alternative folded into the operand).
// CAUTION for callers: hipcc does not know that these statements are vector instructions, so it does not insert the
// two wait states gfx950 needs between a vector write of a register and an MFMA that reads it.  A select's result
// must therefore not be the operand of the very next MFMA: the pass kernel has the operand loads of the product
// loop and a scheduling barrier in between, the single-launch kernel an explicit s_nop (see small_tile).
typedef unsigned long long lanemask_t;
// The four byte tests of a code word in ONE statement: LLVM's hazard table for this chip asks for two wait states
// between a vector instruction writing an SGPR pair and a vector instruction reading it; hipcc cannot see into the
// assembly, and it does move a lone compare right in front of its select.  Kept together, the compares are followed
// by the selects' own preparation (1 - Theta, ...), and tools/check_asm_mfma_hazard.py --sgpr verifies the distance
// in every build (tests/test_isa_hazards.py).  (With an s_nop 1 inside the statement instead: -0.8 % on the bench.)
__device__ __forceinline__ void byte_set4(uint32_t x, lanemask_t (&m)[4]) {
  const uint32_t zero = 0u;
  __asm__("v_cmp_ne_u32_sdwa %0, %4, %5 src0_sel:BYTE_0 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %1, %4, %5 src0_sel:BYTE_1 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %2, %4, %5 src0_sel:BYTE_2 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %3, %4, %5 src0_sel:BYTE_3 src1_sel:DWORD"
          : "=&s"(m[0]), "=&s"(m[1]), "=&s"(m[2]), "=&s"(m[3])
          : "v"(x), "v"(zero));
}
// The eight byte tests of a W-sweep tile (observed ones, then observed zeros) in ONE statement.  Distance by
// construction: an observed-one mask is followed by at least the four observed-zero compares; an observed-zero mask
// is first read by a select whose other operand is the reciprocal, which depends (through d = select(ym, ...) + eps) on
// selects that come after this whole statement.
__device__ __forceinline__ void byte_set8(uint32_t x, uint32_t y, lanemask_t (&m)[4], lanemask_t (&n)[4]) {
  const uint32_t zero = 0u;
  __asm__("v_cmp_ne_u32_sdwa %0, %8, %10 src0_sel:BYTE_0 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %1, %8, %10 src0_sel:BYTE_1 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %2, %8, %10 src0_sel:BYTE_2 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %3, %8, %10 src0_sel:BYTE_3 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %4, %9, %10 src0_sel:BYTE_0 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %5, %9, %10 src0_sel:BYTE_1 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %6, %9, %10 src0_sel:BYTE_2 src1_sel:DWORD\n\t"
          "v_cmp_ne_u32_sdwa %7, %9, %10 src0_sel:BYTE_3 src1_sel:DWORD"
          : "=&s"(m[0]), "=&s"(m[1]), "=&s"(m[2]), "=&s"(m[3]), "=&s"(n[0]), "=&s"(n[1]), "=&s"(n[2]), "=&s"(n[3])
          : "v"(x), "v"(y), "v"(zero));
}
__device__ __forceinline__ lanemask_t byte_set(uint32_t x, int byte) {   // one of them (callers: keep it two instructions away from its select)
  lanemask_t m;
  const uint32_t zero = 0u;
  switch (byte) {
    case 0: __asm__("v_cmp_ne_u32_sdwa %0, %1, %2 src0_sel:BYTE_0 src1_sel:DWORD" : "=s"(m) : "v"(x), "v"(zero)); break;
    case 1: __asm__("v_cmp_ne_u32_sdwa %0, %1, %2 src0_sel:BYTE_1 src1_sel:DWORD" : "=s"(m) : "v"(x), "v"(zero)); break;
    case 2: __asm__("v_cmp_ne_u32_sdwa %0, %1, %2 src0_sel:BYTE_2 src1_sel:DWORD" : "=s"(m) : "v"(x), "v"(zero)); break;
    default: __asm__("v_cmp_ne_u32_sdwa %0, %1, %2 src0_sel:BYTE_3 src1_sel:DWORD" : "=s"(m) : "v"(x), "v"(zero)); break;
  }
  return m;
}
// Selects on such a mask: __builtin_amdgcn_inverse_ballot_w64 hands the SGPR pair to the compiler as a per-lane
// condition, so the select is the compiler's own pair of v_cndmask_b32 (zero / negated alternatives folded in) --
// and being instructions hipcc knows, it inserts the wait states an MFMA reading the result needs itself.  (Round 2
// wrote them as inline assembly: a select two instructions in front of an MFMA then went unprotected, found as
// run-to-run differences in the single-launch kernel.)
__device__ __forceinline__ double sel64(lanemask_t m, double a, double b) { return __builtin_amdgcn_inverse_ballot_w64(m) ? a : b; }
__device__ __forceinline__ double sel64_or0(lanemask_t m, double a) { return __builtin_amdgcn_inverse_ballot_w64(m) ? a : 0.0; }
__device__ __forceinline__ double sel64_0or(lanemask_t m, double b) { return __builtin_amdgcn_inverse_ballot_w64(m) ? 0.0 : b; }
// m ? a : -b is the one select that stays inline assembly: the sign flip rides on the second
// v_cndmask_b32 as a source modifier, where hipcc spends a v_xor_b32 of its own (it splits the f64 select into 32-bit
// halves only after the negation has become an instruction; written on the halves by hand, with a float negation for
// the modifier to absorb, the select comes back as divergent BRANCHES) -- one vector instruction per entry of every W
// sweep.  Its result is an MFMA operand, so the two wait states are the caller's business again: the pass kernel has
// the product loop's LDS reads in between, the single-launch kernel an s_nop tied to the operand, and `make` checks
// every build (tools/check_asm_mfma_hazard.py) and removes a library that gets it wrong.
__device__ __forceinline__ double sel64_neg(lanemask_t m, double a, double b) {
  const uint32_t alo = (uint32_t)__double2loint(a), ahi = (uint32_t)__double2hiint(a);
  const uint32_t blo = (uint32_t)__double2loint(b), bhi = (uint32_t)__double2hiint(b);
  uint32_t lo, hi;
  __asm__("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(lo) : "v"(blo), "v"(alo), "s"(m));
  __asm__("v_cndmask_b32_e64 %0, -%1, %2, %3" : "=v"(hi) : "v"(bhi), "v"(ahi), "s"(m));   // the float negate modifier flips bit 31
  return mk_double(lo, hi);
}

__device__ __forceinline__ double wave_sum(double v) {
  // fixed butterfly order -> bitwise reproducible
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

#include "nbmf_pass_kernel.inc"
#include "nbmf_update_kernels.inc"
#include "nbmf_pack_kernels.inc"
#include "nbmf_peer_kernels.inc"
#include "nbmf_small_kernel.inc"
#include "nbmf_predict_kernels.inc"
#include "nbmf_score_kernels.inc"
#include "nbmf_hist_kernels.inc"
#include "nbmf_moment_kernels.inc"
#include "nbmf_pairs_kernels.inc"
#include "nbmf_rank_kernels.inc"
#include "nbmf_eval_kernels.inc"
#include "nbmf_bits_kernels.inc"
#include "nbmf_theta_bits_kernels.inc"
#include "nbmf_holdout_kernels.inc"
#include "nbmf_neighbors_kernels.inc"

}  // namespace

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
struct nbmf_ctx {
  int device = 0;
  int cus = 256;            // compute units of the device (read once at creation)
  hipStream_t stream = nullptr;
  int64_t m = 0, n = 0, mA = 0, nA = 0;
  int k = 0, KP = 0, KB = 0;
  int KS = 1;               // slices of SLICE_K components (n_components > 128); KP = SLICE_K * KS then
  double* theta = nullptr;  // KS > 1: Theta in tile order, shared by the slices' sweeps
  int data_kind = -1;   // -1 = nothing uploaded
  int storage = NBMF_STORAGE_AUTO;   // storage path the next nbmf_upload is held to (nbmf_set_storage)
  void *dataA = nullptr, *dataB = nullptr, *maskA = nullptr, *maskB = nullptr;
  unsigned long long *bitsA = nullptr, *bitsB = nullptr;   // binary path: the lane-mask images the sweeps read (built from the codes)
  double n_obs = 0, n_obs_global = 0;
  double* rowcnt = nullptr;
  double *Wn = nullptr, *WT = nullptr, *WG = nullptr, *Hn = nullptr, *HT = nullptr, *HG = nullptr;
  bool have_factors = false;
  bool padB_ones = false;          // binary data observed everywhere: image B's pad rows are "ones" in its lane masks (mark_pad_rows_b)
  bool w_free = false;             // inside nbmf_w_only_steps (the W sweeps' variant, w_pass_args)
  bool factors_in_range = false;   // W >= 0 with column sums <= 1 + 1e-12, 0 <= H <= 1 - 1e-9 when they were set: Theta stays in [0, 1) for good
  int chunksH = 0, CH_H = 0, chunksW = 0, CH_W = 0;
  int *cstartH = nullptr, *cstartW = nullptr;   // device: chunk boundaries of the two sweeps
  double *slabH = nullptr, *slabW = nullptr, *Pbuf = nullptr, *lossbuf = nullptr, *prior = nullptr, *scal = nullptr;
  double* lossfin = nullptr;   // the slots of the fused loss assembly (PassFin): LL_EMPTY in every slot between sweeps
  int n_prior_blocks = 0;
  int* flags = nullptr;
  double* losses_d = nullptr;
  int losses_cap = 0;
  double* stage = nullptr;   // host->device staging for factors
  size_t stage_bytes = 0;
  unsigned long long* stats = nullptr;
  double alpha = 1.2, beta = 1.2, eps = 1e-8;
  int projection = NBMF_PROJ_NORMALIZE;
  // comm: RCCL communicator, or a host-mediated all-reduce callback (tests / fallback transport)
  void* comm = nullptr;
  nbmf_host_allreduce_fn host_reduce = nullptr;
  void* host_reduce_user = nullptr;
  double* host_buf = nullptr;   // pinned
  size_t host_buf_count = 0;
  int nranks = 1, rank = 0;
  // which internal axis is split over the ranks: 0 = rows of Y (W local, H replicated, exchange in the
  // H-step); 1 = columns of Y (H local, W replicated, exchange in the W-step)
  int shard_axis = 0;
  double n_div_global = 0;      // axis 1: global number of internal columns (the "/ n" of _solver.py:54)
  double* Qbuf = nullptr;       // axis 1: reduced W-step bracket [KP][mA], the all-reduce payload
  double* sbuf = nullptr;       // scalar exchange slot: [loglik, prior A, prior B]
  const double* ll_ptr = nullptr;   // where the most recent sweep left the (global) log-likelihood
  // axis 0: the K x N exchange is cut into column panels so that the second panel's all-reduce runs (on
  // stream2) while the first panel's H-update and its share of the W-pass compute
  int npanel = 1;
  int panels_wanted = 0;            // nbmf_set_exchange_panels: 0 = default / environment
  double peer_timeout_ms = 0;       // nbmf_set_peer_timeout_ms: 0 = default / environment
  long long pc0[3] = {0, 0, 0};     // panel column boundaries
  size_t pbase[2] = {0, 0};         // panel-major offsets into Pbuf: [P1_p (KP x wp) | P2_p (KP x wp)]
  size_t ll_index = 0;              // loglik slot, right behind panel 0 (travels with it)
  int wsplit = 0;                   // W-pass chunks [0, wsplit) read only panel 0's columns of H
  std::vector<int> bW_host;         // host copy of the W-pass chunk boundaries
  hipStream_t stream2 = nullptr;
  hipEvent_t evH = nullptr, evF = nullptr, ev1 = nullptr;
  // Beta log-prior partial sums the next loss assembly reads (the local array, or the arena's copy of the
  // most recent peer H-step)
  const double* prior_src = nullptr;
  int n_prior_src = 0;
  // peer transport (nbmf_peer_kernels.inc): own arena + flag block, every rank's mapping of them
  double* arena = nullptr;
  unsigned long long* pflags = nullptr;
  size_t arena_doubles = 0;
  int arena_axis = -1;
  struct ArenaSlotRef { void* p = nullptr; } arena_slot;   // pool entry behind arena / pflags (ArenaSlot*)
  bool peer = false;
  PeerView pv{};
  std::vector<void*> peer_mapped;   // hipIpcOpenMemHandle results to close
  unsigned long long epoch = 0, hseq = 0;
  long long offHX = 0, offPR = 0, offSC = 0, x_doubles = 0;
  long long sl_c0 = 0, sl_wp = 0;   // axis 0: the column slice of H this rank updates
  long long psl_c0[2] = {0, 0}, psl_wp[2] = {0, 0};   // ... per column panel when the exchange runs in two panels
  double *Pbuf_own = nullptr, *sbuf_own = nullptr, *Qbuf_own = nullptr;   // the private buffers while the arena stands in
  // the whole-fit-in-one-launch path for small problems (nbmf_small_kernel.inc): second parity of the factor
  // images, hand-off words, a snapshot of the factors for the fall-back
  struct SmallWs {
    double *Wn = nullptr, *WT = nullptr, *WG = nullptr, *Hn = nullptr, *HT = nullptr, *HG = nullptr;
    double *snapW = nullptr, *snapH = nullptr, *ll_part = nullptr, *prior_part = nullptr;
    unsigned long long* sync = nullptr;
    int* result = nullptr;
    double *part_buf = nullptr, *part_ll = nullptr;   // hand-off of split strips
    unsigned long long* part_flag = nullptr;
    char* slab = nullptr;        // the one allocation behind all of the above
    bool ready = false, disabled = false;
    int runs = 0, aborted = 0;   // statistics (nbmf_small_stats)
  } small;
  // batched runs (nbmf_run_batch): per-problem factor images / hand-off words for as many problems as fit the chip at once
  struct SmallBatchWs {
    char* slab = nullptr;          // [cap] per-problem blocks, `stride` bytes apart (small_batch_layout)
    double* table = nullptr;       // [2][cap] alpha - 1 | beta - 1 of the problems of a launch
    double* io = nullptr;          // staging for the factors of a whole batch (up and down)
    int cap = 0, losses_cap = 0;
    size_t io_doubles = 0;
    int launches = 0, problems = 0;   // statistics
  } small_batch;
  // progress reports out of nbmf_run (nbmf_set_progress)
  nbmf_progress_fn progress = nullptr;
  void* progress_user = nullptr;
  int progress_every = 0;
  // held-out evaluation (nbmf_set_eval; nbmf_eval_kernels.inc): the resident pairs, the scratch of one
  // evaluation, the snapshot of the best factors, and what the last nbmf_run recorded
  struct EvalWs {
    int64_t count = 0;   // 0 = no eval set
    int every = 0, patience = 0;
    int *rows = nullptr, *cols = nullptr;
    unsigned char* x = nullptr;
    double *Wk = nullptr, *Hk = nullptr;   // k-major copies of the factors (k_major_kernel), remade per evaluation
    double* partials = nullptr;            // one per workgroup of eval_pairs_kernel
    double* eval_ll_d = nullptr;           // the sums: slot 0 for nbmf_eval_loglik, slot 1 + e for a run's e-th evaluation
    int ll_cap = 0;
    double *bestW = nullptr, *bestH = nullptr;   // the factor images Wn / Hn at the best evaluation of the last run
    bool have_best = false;
    std::vector<int> iters;
    std::vector<double> logliks;
    int best_iter = 0, stopped_early = 0;
    bool held_out = false;   // the set is a hold-out in place (nbmf_hold_out): its entries are unobserved in the images until the undo
  } eval;
  std::atomic<int> cancelled{0};   // nbmf_cancel (any thread): sticky; runs return NBMF_ERR_STATE at the next iteration boundary
  // timing
  bool timing = false;
  int timing_stride = 1;   // events on the sweeps of every timing_stride-th iteration of a run (nbmf_timing_enable)
  int timing_it = 0;       // the iteration being enqueued
  std::vector<hipEvent_t> ev;   // pairs
  std::vector<int> ev_kind;     // 0 = H-pass, 1 = W-pass
  size_t ev_used = 0;
  double t_ms[2] = {0, 0};
  int t_n[2] = {0, 0};
};

namespace {

// ---- device memory: a small caching allocator ---------------------------------------------------
// A fit of one of the reference's datasets is over in 2-3 ms; creating and destroying its context cost more than
// that in hipMalloc / hipFree calls (measured: 1.9 + 1.4 ms at 100 x 500, K = 6).  Blocks of up to 64 MiB are
// therefore kept on release -- per device, by exact size, up to NBMF_POOL_MB (default 1024) in total -- and handed to
// the next context that asks for that size.  A context synchronises its stream before it releases anything, so a
// reused block is never still in use; nothing relies on fresh memory being zero (every buffer is written or cleared
// before it is read).
struct DevPool {
  std::mutex mu;
  struct Key {
    int device;
    size_t bytes;
    bool operator<(const Key& o) const { return device != o.device ? device < o.device : bytes < o.bytes; }
  };
  std::multimap<Key, void*> free_blocks;
  std::map<void*, Key> live;     // every block handed out (pooled or not), for dfree to find its size
  size_t held = 0;
} g_pool;

template <typename T>
hipError_t dmalloc(T** out, size_t bytes) {
  *out = nullptr;
  if (bytes == 0) bytes = 256;
  int dev = 0;
  hipGetDevice(&dev);
  const DevPool::Key key{dev, (bytes + 255) / 256 * 256};
  {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    auto it = g_pool.free_blocks.find(key);
    if (it != g_pool.free_blocks.end()) {
      *out = (T*)it->second;
      g_pool.held -= key.bytes;
      g_pool.free_blocks.erase(it);
      g_pool.live[(void*)*out] = key;
      return hipSuccess;
    }
  }
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, key.bytes);
  if (e != hipSuccess) {   // out of memory: give back what is held and try once more
    (void)hipGetLastError();   // (the failed attempt's code must not outlive a retry that succeeds: see fail())
    std::vector<void*> drop;
    {
      std::lock_guard<std::mutex> lk(g_pool.mu);
      for (auto& kv : g_pool.free_blocks) drop.push_back(kv.second);
      g_pool.free_blocks.clear();
      g_pool.held = 0;
    }
    for (void* q : drop) hipFree(q);
    e = hipMalloc(&p, key.bytes);
    if (e != hipSuccess) return e;
  }
  std::lock_guard<std::mutex> lk(g_pool.mu);
  g_pool.live[p] = key;
  *out = (T*)p;
  return hipSuccess;
}

hipError_t dfree(void* p) {
  if (!p) return hipSuccess;
  static const size_t cap = (size_t)std::max(0, env_int("NBMF_POOL_MB", 1024)) << 20;
  {
    std::lock_guard<std::mutex> lk(g_pool.mu);
    auto it = g_pool.live.find(p);
    if (it != g_pool.live.end()) {
      const DevPool::Key key = it->second;
      g_pool.live.erase(it);
      if (key.bytes <= (64u << 20) && g_pool.held + key.bytes <= cap) {
        g_pool.free_blocks.emplace(key, p);
        g_pool.held += key.bytes;
        return hipSuccess;
      }
    }
  }
  return hipFree(p);
}

// ... and the same for what else a context needs from the runtime: device properties are read once per device and
// process (hipGetDeviceProperties takes ~1 ms), streams are kept on release and reused (create + destroy ~1 ms).
struct DevInfo {
  bool known = false, gfx950 = false;
  int cus = 256;
  char arch[64] = {0};
};
DevInfo g_devinfo[64];
std::mutex g_devinfo_mu;

hipError_t device_info(int device, DevInfo* out) {
  std::lock_guard<std::mutex> lk(g_devinfo_mu);
  DevInfo& d = g_devinfo[device & 63];
  if (!d.known) {
    hipDeviceProp_t prop;
    hipError_t e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) return e;
    d.known = true;
    d.gfx950 = strncmp(prop.gcnArchName, "gfx950", 6) == 0;
    d.cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    strncpy(d.arch, prop.gcnArchName, sizeof d.arch - 1);
  }
  *out = d;
  return hipSuccess;
}

std::vector<hipStream_t> g_streams[64];
std::mutex g_streams_mu;

hipError_t stream_acquire(int device, hipStream_t* out) {
  {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    auto& v = g_streams[device & 63];
    if (!v.empty()) {
      *out = v.back();
      v.pop_back();
      return hipSuccess;
    }
  }
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

void stream_release(int device, hipStream_t st) {   // the caller has synchronised it
  std::lock_guard<std::mutex> lk(g_streams_mu);
  auto& v = g_streams[device & 63];
  if (v.size() < 64)
    v.push_back(st);
  else
    hipStreamDestroy(st);
}

// Wait for a stream whose work lasts milliseconds.  hipStreamSynchronize spins briefly and then sleeps on the
// completion interrupt; about one wake-up in 70 arrives ~8.6 ms late (tools/bimodal_probe.py: the kernel's own clock
// shows the same 35.0 ms on the device for a 3000-iteration fit whether the host saw 35.2 or 43.7 ms -- what round 2
// took for a second, slower "speed" of the single-launch path).  For a fit that lasts 3 ms that is the run three times
// over, so the small-problem paths poll the stream for up to `spin_ms` before they fall back to the blocking call.
hipError_t stream_wait_spin(hipStream_t st, double spin_ms = -1.0) {
  // (the budget: 200 ms unless NBMF_SPIN_MS says otherwise -- a host whose cores are shared by many rank threads may
  //  prefer to sleep at once: NBMF_SPIN_MS=0)
  static const double spin_default = std::max(0.0, env_double("NBMF_SPIN_MS", 200.0));
  if (spin_ms < 0.0) spin_ms = spin_default;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t e = hipStreamQuery(st);
    if (e != hipErrorNotReady) return e;
    if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > spin_ms) break;
  }
  return hipStreamSynchronize(st);
}

// ---- RCCL, loaded lazily so that single-GPU use has no dependency on it ---------------------
struct Uid {
  char internal[128];
};
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, /*ncclUniqueId by value*/ Uid, int) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*CommCount)(void*, int*) = nullptr;      // optional: how many ranks the communicator itself says it joins (nbmf_comm_info)
  int (*CommCuDevice)(void*, int*) = nullptr;   // optional: the device it is bound to
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;

int load_rccl() {
  if (g_rccl.lib) return NBMF_OK;
  // Which librccl: the one that belongs to the HIP runtime THIS library is linked against (the file next to
  // that libamdhip64), not whatever a plain soname lookup finds first -- a PyTorch wheel in the same process
  // brings its own, older copy bound to its own runtime.  NBMF_RCCL_LIBRARY overrides; the soname is the last
  // resort.
  std::vector<std::string> names;
  if (const char* e = getenv("NBMF_RCCL_LIBRARY")) names.push_back(e);
  Dl_info info;
  if (dladdr((const void*)&hipGetDeviceCount, &info) && info.dli_fname) {
    std::string dir(info.dli_fname);
    const size_t slash = dir.rfind('/');
    if (slash != std::string::npos) {
      dir.resize(slash + 1);
      names.push_back(dir + "librccl.so.1");
      names.push_back(dir + "librccl.so");
    }
  }
  for (const char* nm : {"/opt/rocm/lib/librccl.so.1", "librccl.so.1", "librccl.so"}) names.push_back(nm);
  void* lib = nullptr;
  std::string tried;
  for (const std::string& nm : names) {
    lib = dlopen(nm.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (lib) {
      if (env_set("NBMF_DEBUG")) fprintf(stderr, "[nbmf] RCCL: %s\n", nm.c_str());
      break;
    }
    tried += nm + " ";
  }
  if (!lib) return fail(NBMF_ERR_COMM, "cannot load librccl (tried %s): %s", tried.c_str(), dlerror());
  g_rccl.GetUniqueId = (int (*)(void*))dlsym(lib, "ncclGetUniqueId");
  g_rccl.CommInitRank = (int (*)(void**, int, Uid, int))dlsym(lib, "ncclCommInitRank");
  g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(lib, "ncclAllReduce");
  g_rccl.CommDestroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
  g_rccl.GetErrorString = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
  g_rccl.CommCount = (int (*)(void*, int*))dlsym(lib, "ncclCommCount");
  g_rccl.CommCuDevice = (int (*)(void*, int*))dlsym(lib, "ncclCommCuDevice");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy)
    return fail(NBMF_ERR_COMM, "librccl is missing expected symbols");
  g_rccl.lib = lib;
  return NBMF_OK;
}
constexpr int kNcclFloat64 = 8;   // ncclDouble (rccl.h ncclDataType_t)
constexpr int kNcclSum = 0;       // ncclSum

#define NCCLCHK(call)                                                                                     \
  do {                                                                                                    \
    int r_ = (call);                                                                                      \
    if (r_ != 0)                                                                                          \
      return fail(NBMF_ERR_COMM, "%s failed: %s", #call, g_rccl.GetErrorString ? g_rccl.GetErrorString(r_) : "?"); \
  } while (0)

// ---- peer-transport arenas: a process-wide pool ---------------------------------------------------
// Memory that has been exported through HIP IPC is never given back to the allocator while the process lives:
// a context returns its arena (payload block + flag block + their IPC handles) to this pool and the next
// context of a fitting size takes it over.  Freeing an exported arena and exporting a fresh allocation that
// lands on the same address handed the peers a mapping of the OLD memory (seen as a wrong factor in the second
// of two sharded fits in one process); a handle that stays valid for good cannot go stale.
struct PeerOrigin {   // tail of a handle block
  unsigned long long pid, arena, flags;   // pid: not the process id (two containers of a node may both run a pid 1) but a
  int device, reserved;                   // 64-bit number drawn once per process: process_nonce()
};
// Who exported a handle block: a rank of THIS process is addressed through the exporter's own pointers, so "this
// process" must not be decided by something two processes can share.  Process ids are unique per PID namespace only;
// a random 64-bit number drawn once at first use (mixed with the pid and the clock in case the random device is a
// constant) is unique for practical purposes.
unsigned long long process_nonce() {
  static const unsigned long long nonce = [] {
    unsigned long long v = 0;
    if (FILE* f = fopen("/dev/urandom", "rb")) {
      if (fread(&v, sizeof v, 1, f) != 1) v = 0;
      fclose(f);
    }
    v ^= (unsigned long long)getpid() * 0x9E3779B97F4A7C15ull;
    v ^= (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count() * 0xBF58476D1CE4E5B9ull;
    return v ? v : 1ull;
  }();
  return nonce;
}
struct ArenaSlot {
  int device;
  size_t doubles;
  double* arena;
  unsigned long long* flags;
  char handles[NBMF_PEER_HANDLE_BYTES];
  bool in_use;
};
std::vector<ArenaSlot*> g_arenas;
std::mutex g_arena_mu;

int arena_acquire(int device, size_t doubles, ArenaSlot** out) {
  std::lock_guard<std::mutex> lk(g_arena_mu);
  ArenaSlot* best = nullptr;
  for (ArenaSlot* a : g_arenas)
    if (!a->in_use && a->device == device && a->doubles >= doubles && a->doubles <= 4 * doubles + (1u << 20) &&
        (!best || a->doubles < best->doubles))
      best = a;
  if (!best) {
    ArenaSlot* a = new ArenaSlot();
    a->device = device;
    a->doubles = doubles;
    a->arena = nullptr;
    a->flags = nullptr;
    a->in_use = false;
    hipError_t e = hipExtMallocWithFlags((void**)&a->arena, doubles * sizeof(double), hipDeviceMallocUncached);
    if (e == hipSuccess) e = hipExtMallocWithFlags((void**)&a->flags, PF_WORDS * sizeof(unsigned long long), hipDeviceMallocUncached);
    hipIpcMemHandle_t h[2];
    if (e == hipSuccess) e = hipIpcGetMemHandle(&h[0], a->arena);
    if (e == hipSuccess) e = hipIpcGetMemHandle(&h[1], a->flags);
    if (e != hipSuccess) {
      if (a->arena) hipFree(a->arena);   // never exported: safe to free
      if (a->flags) hipFree(a->flags);
      delete a;
      return fail(NBMF_ERR_HIP, "peer arena: %s (allocation or hipIpcGetMemHandle)", hipGetErrorString(e));
    }
    // handle block: two IPC handles, then who exported them and where the memory sits in that process (a rank of
    // the same process cannot open its own process's handles and uses the addresses instead)
    static_assert(2 * sizeof(hipIpcMemHandle_t) + sizeof(PeerOrigin) <= NBMF_PEER_HANDLE_BYTES, "handle block too small");
    memset(a->handles, 0, sizeof a->handles);
    memcpy(a->handles, h, sizeof h);
    const PeerOrigin origin{process_nonce(), (unsigned long long)a->arena, (unsigned long long)a->flags, device, 0};
    memcpy(a->handles + sizeof h, &origin, sizeof origin);
    g_arenas.push_back(a);
    best = a;
  }
  best->in_use = true;
  *out = best;
  return NBMF_OK;
}

void arena_release(ArenaSlot* a) {
  if (!a) return;
  std::lock_guard<std::mutex> lk(g_arena_mu);
  a->in_use = false;
  if (env_int("NBMF_ARENA_POOL", 1) == 0) {   // diagnostic: the old behaviour (free on release), to reproduce the stale-mapping failure
    hipFree(a->arena);
    hipFree(a->flags);
    g_arenas.erase(std::find(g_arenas.begin(), g_arenas.end(), a));
    delete a;
  }
}

// ---- the general path's logarithm table: one copy per device and process ------------------------
// Built when the first context of a device is created (nbmf_create, on that context's stream, which it then waits for --
// creation synchronises anyway), never in the launch path: a first-time build there would allocate and wait for the whole
// device under a process-wide lock -- illegal inside a stream capture, and a stall when another rank's kernel on the same
// device is itself waiting, in-kernel, for this rank (peer transport).  Launches only read the pointer.
std::atomic<const double2*> g_logtab[64];
std::mutex g_logtab_mu;
hipError_t log_table_build(int dev, hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_logtab_mu);
  if (g_logtab[dev & 63].load(std::memory_order_acquire)) return hipSuccess;
  double2* t = nullptr;
  hipError_t e = hipMalloc((void**)&t, 1024 * sizeof(double2));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(log_table_kernel, dim3(4), dim3(256), 0, st, t);
  if ((e = hipGetLastError()) != hipSuccess || (e = hipStreamSynchronize(st)) != hipSuccess) {
    hipFree(t);
    return e;
  }
  g_logtab[dev & 63].store(t, std::memory_order_release);
  return hipSuccess;
}
// (the launch path: a read; hipErrorNotInitialized if no context of this device was ever created)
hipError_t log_table_device(const double2** out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  *out = g_logtab[dev & 63].load(std::memory_order_acquire);
  return *out ? hipSuccess : hipErrorNotInitialized;
}

// ---- pass launch ----------------------------------------------------------------------------
// Timing (nbmf_timing_enable): a sweep that is ONE launch carries its two events in its own dispatch packet
// (hipExtLaunchKernelGGL: start and end of that kernel, no barrier packets in front of and behind it, which at
// configs[1] cost ~4.5 us each, 5 % of the iteration); EvScope puts them here, the next pass launch of this thread
// takes them.  Sweeps of several launches are bracketed by recorded events as before.
thread_local hipEvent_t tl_attach_start = nullptr, tl_attach_stop = nullptr;
std::atomic<long long> g_full_w_launches{0}, g_ragged_launches{0}, g_loss_assembly_recoveries{0};   // nbmf_variant_stats

// NBMF_PASS_TRACE=<n>: every n-th launch of each sweep kernel is traced -- with n > 1 the launches in between run back to
// back, so the traced one meets the chip in the state a real run leaves it in: clocks under sustained load.  `count` is the
// kernel's own launch counter.
bool pass_trace_due(std::atomic<long>& count) {
  static const int every = env_set("NBMF_PASS_TRACE") ? std::max(1, env_int("NBMF_PASS_TRACE", 1)) : 0;
  return every && (count.fetch_add(1) % every) == every - 1;
}
// The traced launch of pass kernel f (K = 16 KB components): where the workgroups of THIS launch spend their time outside
// the loop.  Every workgroup notes the wall clock (100 MHz) at entry, at the top of its loop, at the loop's end and at exit;
// printed: the launch's span, the spread of the entries and exits, mean prologue / loop / epilogue.  Serialises the stream
// (one launch at a time).
hipError_t launch_pass_traced(const void* f, dim3 grid, int lds_bytes, hipStream_t st, PassArgs a, int K, int data, int mode) {
  const size_t n_wg = (size_t)grid.x * grid.y;
  unsigned long long* tr = nullptr;
  hipError_t e = dmalloc(&tr, sizeof(unsigned long long) * 8 * n_wg);
  if (e != hipSuccess) return e;
  a.trace = tr;
  void* params[] = {&a};
  (void)hipLaunchKernel(f, grid, dim3(64 * WG_WAVES), params, lds_bytes, st);
  std::vector<unsigned long long> h(8 * n_wg);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipMemcpy(h.data(), tr, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost);
  dfree(tr);
  if (e != hipSuccess) return e;
  unsigned long long t_first = ~0ull, t_last = 0, last_entry = 0, first_exit = ~0ull;
  double pro = 0, loop = 0, epi = 0, epi_loss = 0, epi_slab = 0, loop_clk = 0;
  std::vector<double> exits;
  size_t live = 0;
  for (size_t i = 0; i < n_wg; ++i) {
    const unsigned long long* t = h.data() + 8 * i;
    if (!t[3]) continue;
    ++live;
    t_first = std::min(t_first, t[0]);
    t_last = std::max(t_last, t[3]);
    last_entry = std::max(last_entry, t[0]);
    first_exit = std::min(first_exit, t[3]);
    pro += (double)(t[1] - t[0]);
    loop += (double)(t[2] - t[1]);
    loop_clk += (double)t[7];
    epi += (double)(t[3] - t[2]);
    epi_loss += (double)(t[5] - t[2]);
    epi_slab += (double)(t[6] - t[5]);
    exits.push_back((double)t[3]);
  }
  if (live) {
    // mean time from entry to exit by the wave slot (HW_ID bits 3:0) the workgroup's first wave was given: does the
    // SIMD's arbiter favour some slots (oldest first)?
    double dur[16] = {0};
    int cnt[16] = {0};
    for (size_t i = 0; i < n_wg; ++i) {
      const unsigned long long* t = h.data() + 8 * i;
      if (!t[3]) continue;
      dur[t[4] & 15] += (double)(t[3] - t[0]);
      ++cnt[t[4] & 15];
    }
    fprintf(stderr, "[nbmf]   mean entry-to-exit by wave slot:");
    for (int w = 0; w < 16; ++w)
      if (cnt[w]) fprintf(stderr, " slot %d: %.1f us (%d)", w, dur[w] / cnt[w] * 0.01, cnt[w]);
    fprintf(stderr, "\n");
    std::sort(exits.begin(), exits.end());
    const double us = 0.01;   // 100 MHz ticks
    fprintf(stderr, "[nbmf] pass<K=%d,data=%d,mode=%d> %zu workgroups: span %.1f us | entries spread over %.1f us | exits: first %.1f, median %.1f, "
                    "last %.1f us before the end | per workgroup: prologue %.2f, loop %.2f, epilogue %.2f us (loss block %.2f, slab stores %.2f) | shader clock in the loops %.3f GHz\n", K, data, mode, live,
            (double)(t_last - t_first) * us, (double)(last_entry - t_first) * us, (double)(t_last - first_exit) * us,
            ((double)t_last - exits[exits.size() / 2]) * us, 0.0, pro / live * us, loop / live * us, epi / live * us, epi_loss / live * us,
            epi_slab / live * us, loop > 0 ? loop_clk / loop * 0.1 : 0.0);
  }
  return hipSuccess;
}

template <int KB, int DATA, int MODE, int TH, bool TINY, bool RAG = false, bool FULL = false>
hipError_t launch_pass_tt(const PassArgs& a_, int chunks, hipStream_t st) {
  if (FULL) g_full_w_launches.fetch_add(1, std::memory_order_relaxed);
  if (RAG) g_ragged_launches.fetch_add(1, std::memory_order_relaxed);
  dim3 grid(a_.Cb / WG_WAVES, chunks);
  constexpr int lds_bytes = pass_lds_bytes(KB, DATA, MODE);
  if (lds_bytes > 65536) {
    hipError_t e = hipFuncSetAttribute((const void*)pass_kernel<KB, DATA, MODE, TH, TINY, RAG, FULL>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
  }
  PassArgs a = a_;
  if (DATA != DATA_BIN && MODE != MODE_W && MODE != MODE_T && pass_log_bits(KB) == 10) {
    hipError_t e = log_table_device(&a.ltab_g);
    if (e != hipSuccess) return e;
  }
  static std::atomic<long> trace_count{0};   // (per instantiation)
  if (MODE != MODE_T && pass_trace_due(trace_count))
    return launch_pass_traced((const void*)pass_kernel<KB, DATA, MODE, TH, TINY, RAG, FULL>, grid, lds_bytes, st, a, 16 * KB, DATA, MODE);
  if (tl_attach_start) {
    hipEvent_t e0 = tl_attach_start, e1 = tl_attach_stop;
    tl_attach_start = tl_attach_stop = nullptr;
    hipExtLaunchKernelGGL((pass_kernel<KB, DATA, MODE, TH, TINY, RAG, FULL>), grid, dim3(64 * WG_WAVES), lds_bytes, st, e0, e1, 0, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL((pass_kernel<KB, DATA, MODE, TH, TINY, RAG, FULL>), grid, dim3(64 * WG_WAVES), lds_bytes, st, a);
  return hipGetLastError();
}
// (eps below 1e-70 on the binary path: the variant with per-entry reciprocals and renormalisation, see pass_kernel)
template <int KB, int DATA, int MODE, int TH = 0>
hipError_t launch_pass_t(const PassArgs& a, int chunks, hipStream_t st) {
  if (MODE != MODE_T && a.tiny_eps) return launch_pass_tt<KB, DATA, MODE, TH, MODE != MODE_T>(a, chunks, st);
  // Fewer components than the layout holds -- 10 in the K = 16 layout, 40 in the K = 64 one: the variant that skips the
  // k-steps and 16-blocks of components that are padding (RAG, nbmf_pass_kernel.inc).  Where it pays (measured, 32768 x 8192,
  // byte codes: k = 4 +19 %, 8 +11-16 %, 10-12 +2-6 %, 20 +9 %, 24 +5 %, 40 +20 %, 48 +15 %): up to the K = 64 layout -- at
  // K = 128 the branches cost the register-tuned schedule more than the skipped MFMAs give back (k = 100: -4.6 %) --, when
  // at least a twelfth of the tile's MFMAs goes (k = 50: three of 48, -1.7 %), and not on the general path at K <= 16 (four
  // tiles per stage with branches between their MFMAs: 250 registers and scratch, -4 % at k = 10).
  constexpr bool HAS_RAG = TH == 0 && MODE != MODE_T && KB <= 4 && (DATA == DATA_BIN || KB >= 2);
  // W sweeps over a matrix that is observed everywhere and has no pad rows in the swept dimension: the two-state variant
  // (FULL, nbmf_pass_kernel.inc; NBMF_NO_FULL_W=1: the three-state kernels on such data -- tests)
  constexpr bool HAS_FULL = TH == 0 && MODE == MODE_W && DATA == DATA_BIN;
  static const bool no_full = env_set("NBMF_NO_FULL_W");
  const bool full = HAS_FULL && a.full && !no_full;
  static const bool no_rag = env_set("NBMF_NO_RAGGED_K");   // (tests: the full-K kernels on a ragged K -- the same bits)
  if (HAS_RAG && !no_rag && a.ksteps > 0 && a.ksteps < 4 * KB) {
    const int per_block = MODE == MODE_H ? 8 : (MODE == MODE_W ? 4 : 0);   // back-product MFMAs of one 16-block of components
    const int skipped = (4 * KB - a.ksteps) + (KB >= 4 ? (KB - a.kblocks) * per_block : 0);
    const int total = 4 * KB + KB * per_block;
    if (12 * skipped >= total)
      return full ? launch_pass_tt<KB, DATA, MODE, TH, false, HAS_RAG, HAS_RAG && HAS_FULL>(a, chunks, st)
                  : launch_pass_tt<KB, DATA, MODE, TH, false, HAS_RAG>(a, chunks, st);
  }
  return full ? launch_pass_tt<KB, DATA, MODE, TH, false, false, HAS_FULL>(a, chunks, st)
              : launch_pass_tt<KB, DATA, MODE, TH, false>(a, chunks, st);
}

// n_components > 128: the sweep of one slice with Theta read from memory (TH = 1: whole; TH = 2: the earlier
// slices' part, completed and stored here), and the Theta sweep itself
template <int MODE, int TH>
hipError_t launch_pass_slice(int data_kind, const PassArgs& a, int chunks, hipStream_t st) {
  switch (data_kind) {
    case DATA_BIN: return launch_pass_t<8, DATA_BIN, MODE, TH>(a, chunks, st);
    case DATA_F64: return launch_pass_t<8, DATA_F64, MODE, TH>(a, chunks, st);
    case DATA_F64M: return launch_pass_t<8, DATA_F64M, MODE, TH>(a, chunks, st);
  }
  return hipErrorInvalidValue;
}
inline hipError_t launch_theta(const PassArgs& a, int chunks, hipStream_t st) {
  return launch_pass_t<8, DATA_BIN, MODE_T, 0>(a, chunks, st);
}

// The (KB, data kind) pairs the sweep kernels are built for: f(integral_constant KB, integral_constant DATA), or `none`
// for a pair that is not one of them
template <typename R, typename F>
R pass_dispatch(int KB, int data_kind, R none, F f) {
  auto by_kb = [&](auto data) -> R {
    switch (KB) {
      case 1: return f(std::integral_constant<int, 1>{}, data);
      case 2: return f(std::integral_constant<int, 2>{}, data);
      case 4: return f(std::integral_constant<int, 4>{}, data);
      case 8: return f(std::integral_constant<int, 8>{}, data);
    }
    return none;
  };
  switch (data_kind) {
    case DATA_BIN: return by_kb(std::integral_constant<int, DATA_BIN>{});
    case DATA_F64: return by_kb(std::integral_constant<int, DATA_F64>{});
    case DATA_F64M: return by_kb(std::integral_constant<int, DATA_F64M>{});
  }
  return none;
}

template <int MODE>
hipError_t launch_pass(int KB, int data_kind, const PassArgs& a, int chunks, hipStream_t st) {
  return pass_dispatch(KB, data_kind, hipErrorInvalidValue, [&](auto kb, auto data) -> hipError_t {
    return launch_pass_t<decltype(kb)::value, decltype(data)::value, MODE>(a, chunks, st);
  });
}

// workgroups of this pass kernel that one CU holds at once (registers and LDS decide)
template <int MODE>
int resident_per_cu(int KB, int data_kind) {
  int n = 0;
  const void* f = pass_dispatch(KB, data_kind, (const void*)nullptr, [](auto kb, auto data) -> const void* {
    return (const void*)pass_kernel<decltype(kb)::value, decltype(data)::value, MODE>;
  });
  const int lds_bytes = pass_lds_bytes(KB, data_kind, MODE);
  if (!f || hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, f, 64 * WG_WAVES, lds_bytes) != hipSuccess || n < 1) n = 2;
  return std::min(n, 8);
}

// Split a sweep of Rb row blocks into chunks: aim for ~2048 workgroups (several rounds over the 512-768
// resident ones, so the dispatcher can even out slow workgroups) without making the sweeps shorter than
// 64 blocks (each workgroup pays a fixed prologue/epilogue and writes its own partial slab).
// Measured at c3 / K=64: 768 workgroups = exactly one round of the 768 resident slots is SLOWER (3.23 ms)
// than 2048 (3.15 ms); anything from 1536 to 4608 is within 1 %.  `slots` is kept for diagnostics.
// NBMF_TARGET_WGS=<n> overrides the target (tuning experiments only).
void pick_chunks(int strips_groups, int Rb, int NB, int slots, int ns, int cus, bool one_round_ok, int* chunks, int* CH) {
  (void)slots;
  const char* target_var = one_round_ok ? "NBMF_TARGET_WGS_H" : "NBMF_TARGET_WGS_W";   // (tuning experiments: one sweep only)
  if (!env_set(target_var)) target_var = "NBMF_TARGET_WGS";
  const bool target_set = env_set(target_var);
  const int target = std::max(1, env_int(target_var, 2048));
  int want = (target + strips_groups - 1) / strips_groups;
  const int max_chunks = std::max(1, Rb / NB);
  want = std::min(std::max(want, 1), max_chunks);
  int ch = (Rb + want - 1) / want;
  // (small problems -- fewer than 512 workgroups even at 64-block chunks -- are bound by the length of the
  //  sweep a single workgroup walks, not by per-workgroup overhead: 8-block chunks there.  BASELINE configs[0],
  //  100 x 500 with K = 6: 37.4 -> 26.2 us per iteration (26 700 -> 38 100 iterations/s); the 36-fit
  //  perplexity grid on the lastfm-sized matrix 0.63 -> 0.33 s.)
  // (ns = strips per wave: a workgroup of the two-strip kernels does a 64-block sweep's work in 32 blocks)
  int min_blocks = (long long)strips_groups * ns * ((Rb + 63) / 64) >= 512 ? 64 / ns : 8;
  if (env_set("NBMF_MIN_BLOCKS")) min_blocks = std::max(NB, env_int("NBMF_MIN_BLOCKS", 0));   // (tuning experiments only)
  const bool clipped = ch < std::min(Rb, min_blocks);   // the sweep is too short for the target at min_blocks per chunk
  ch = std::max(ch, std::min(Rb, min_blocks));
  ch = (int)round_up(ch, NB);
  // The last round.  Workgroups of a sweep are equally long, so they finish in rounds; a CU is as fast with two
  // resident workgroups as with three (the MFMA pipe is full either way), but a last round that leaves CUs EMPTY is
  // lost time: 266 strip groups x 8 chunks = 2128 workgroups on 512 such places (configs[4]'s W-pass, K = 128) are
  // 4.16 rounds -- a fifth round for 80 workgroups, MFMA-busy 84 %.  More chunks are tried (up to four times as many,
  // whole multiples of 8 first: the XCD renumbering of pass_kernel wants those) until the rounds are >= 95 % full.
  // The sweeps of configs[1..3] and of their shards already are (2048 or 1024 workgroups: 4 or 2 full rounds).
  if (cus > 0 && !target_set && !env_set("NBMF_MIN_BLOCKS") && !env_set("NBMF_NO_ROUND_FILL")) {
    const long long places = (long long)cus * std::min(std::max(slots / cus, 1), 2);
    auto fill = [&](int blocks_per_chunk) {   // how full the rounds are with chunks of that many row blocks
      const long long wgs = (long long)strips_groups * ((Rb + blocks_per_chunk - 1) / blocks_per_chunk);
      return (double)wgs / (double)(((wgs + places - 1) / places) * places);
    };
    int base = (Rb + ch - 1) / ch;   // chunks so far
    // (short sweeps at K >= 64, where two workgroups per CU fill the MFMA pipe: ONE round of exactly that many beats two
    //  rounds of half-length workgroups -- the 8192-row shard of configs[2], 128 strip groups x 512 row blocks: 4 chunks
    //  1 443 it/s, 8 chunks 1 422; at K = 32, which wants four waves per SIMD, and for the long sweeps of configs[2]
    //  itself it is the other way round, by 1 %.  The H sweep only: a row-sharded run may launch its W sweep in two parts,
    //  one per exchange panel, and half of four chunks would leave one workgroup per CU)
    if (one_round_ok && clipped && NB <= 2 && places % strips_groups == 0 && places / strips_groups < base &&
        (Rb + (int)(places / strips_groups) - 1) / (int)(places / strips_groups) >= min_blocks) {
      const int n1 = (int)(places / strips_groups);
      ch = (int)round_up((Rb + n1 - 1) / n1, NB);
      base = (Rb + ch - 1) / ch;
    }
    if ((long long)strips_groups * base > places && fill(ch) < 0.95) {
      int best = ch;
      double best_fill = fill(ch);
      for (int pass = 0; pass < 2 && best_fill < 0.95; ++pass) {   // pass 0: whole multiples of 8 chunks only
        for (int n = base + 1; n <= 4 * base; ++n) {
          if (pass == 0 && (n & 7)) continue;
          const int cand = (int)round_up((Rb + n - 1) / n, NB);
          if (cand < std::min(Rb, min_blocks)) break;
          const double f = fill(cand);
          if (f > best_fill + 1e-9) {
            best_fill = f;
            best = cand;
            if (f >= 0.95) break;
          }
        }
      }
      ch = best;
    }
  }
  *CH = ch;
  *chunks = (Rb + ch - 1) / ch;
}

// Chunk boundaries (row blocks) of a sweep.  Equal chunks: cutting the tail of the sweep four times finer
// (so that the last, lonely workgroups on a CU are short) was measured and bought nothing (c3 H-pass 3.15
// vs 3.17 ms) while adding slabs for the update kernels to sum.
std::vector<int> chunk_boundaries(int Rb, int ch) {
  std::vector<int> b;
  b.push_back(0);
  for (int pos = 0; pos < Rb;) {
    pos = std::min(pos + ch, Rb);
    b.push_back(pos);
  }
  return b;
}

struct EvScope {
  nbmf_ctx* c;
  int kind;
  size_t slot = (size_t)-1;
  bool attach;
  // count = false: add the time to `kind` but do not count a launch (second part of a split sweep)
  // attach = true: the scope holds exactly one pass launch, on c->stream, which carries the events itself (launch_pass_tt)
  EvScope(nbmf_ctx* c_, int kind_, bool count = true, bool attach_ = false)
      : c(c_), kind(kind_ | (count ? 0 : 0x100)), attach(attach_ && !env_set("NBMF_TIMING_BRACKET")) {
    if (!c->timing || (c->timing_stride > 1 && c->timing_it % c->timing_stride != 0)) return;
    if (c->ev_used + 2 > c->ev.size()) {
      for (int i = 0; i < 2; ++i) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        c->ev.push_back(e);
      }
      c->ev_kind.push_back(kind);
    } else {
      c->ev_kind[c->ev_used / 2] = kind;
    }
    slot = c->ev_used;
    c->ev_used += 2;
    if (attach) {
      tl_attach_start = c->ev[slot];
      tl_attach_stop = c->ev[slot + 1];
    } else {
      hipEventRecord(c->ev[slot], c->stream);
    }
  }
  ~EvScope() {
    if (slot == (size_t)-1) return;
    if (attach) {
      if (tl_attach_start) {   // (no launch took them: an error path)
        tl_attach_start = tl_attach_stop = nullptr;
        c->ev_used = slot;
      }
    } else {
      hipEventRecord(c->ev[slot + 1], c->stream);
    }
  }
};

void timing_collect(nbmf_ctx* c) {
  // caller has synchronised the stream
  for (size_t s = 0; s + 1 < c->ev_used; s += 2) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[s], c->ev[s + 1]) == hipSuccess) {
      c->t_ms[c->ev_kind[s / 2] & 0xFF] += ms;
      if (!(c->ev_kind[s / 2] & 0x100)) c->t_n[c->ev_kind[s / 2] & 0xFF] += 1;
    }
  }
  c->ev_used = 0;
}

// In-place sum over ranks of `count` doubles at device pointer `p`, on the context's stream.
int all_reduce_inplace(nbmf_ctx* c, double* p, size_t count, hipStream_t st = nullptr) {
  if (c->comm) {
    NCCLCHK(g_rccl.AllReduce(p, p, count, kNcclFloat64, kNcclSum, c->comm, st ? st : c->stream));
  } else if (c->peer) {
    const long long off = p - c->arena;
    if (off < 0 || (size_t)off + count > c->arena_doubles) return fail(NBMF_ERR_STATE, "internal: peer exchange outside the arena");
    hipStream_t s = st ? st : c->stream;
    const unsigned long long e = ++c->epoch;
    const long long slice = ((long long)count + c->pv.nranks - 1) / c->pv.nranks;
    const unsigned grid = (unsigned)std::min<long long>(128, std::max<long long>(1, (slice + 1023) / 1024));
    // (fault injection for the tests of the failure path: NBMF_PEER_FAULT=1 makes the LAST rank skip its part of
    //  every generic exchange, as a rank whose links do not work would -- the others must time out, not hang)
    static const bool fault = env_int("NBMF_PEER_FAULT", 0) != 0;
    if (!(fault && c->pv.nranks > 1 && c->pv.rank == c->pv.nranks - 1))
      hipLaunchKernelGGL(peer_reduce_kernel, dim3(grid), dim3(256), 0, s, c->pv, e, off, (long long)count, c->flags);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(peer_wait_kernel, dim3(1), dim3(64), 0, s, c->pv, e, c->flags);
    HIPCHK(hipGetLastError());
  } else if (c->host_reduce) {
    if (count > c->host_buf_count) return fail(NBMF_ERR_STATE, "internal: host exchange buffer too small");
    HIPCHK(hipMemcpyAsync(c->host_buf, p, count * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->host_reduce(c->host_reduce_user, c->host_buf, (int64_t)count) != 0)
      return fail(NBMF_ERR_COMM, "host all-reduce callback failed");
    HIPCHK(hipMemcpyAsync(p, c->host_buf, count * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  return NBMF_OK;
}

inline bool is_sharded(const nbmf_ctx* c) { return c->comm || c->host_reduce || c->peer; }

// what a sweep reads of the data: the lane-mask image on the binary path, the double tiles otherwise
inline const void* sweep_image(const nbmf_ctx* c, int image) {
  if (c->data_kind == DATA_BIN) return image == 0 ? (const void*)c->bitsA : (const void*)c->bitsB;
  return image == 0 ? c->dataA : c->dataB;
}

// column strips one workgroup of the pass kernels covers (one per wave)
inline int wg_strips(const nbmf_ctx*) { return WG_WAVES; }

// Every sweep over image A takes in all entries of the padded mA x nA grid.  A pad entry has Theta == 0 and
// counts as "not an observed one" (binary path: code 0; general path: y = 0, weight 0), so it contributes
// exactly log(fl(fl(1-0)+eps)) = log(1+eps) to the likelihood; their total is removed before the loss is
// assembled (and before any all-reduce).  A strictly masked sweep skips unobserved entries, pads included --
// except on the general path without a mask, where everything counts as observed.
// Which variant the sweeps over image A (H-pass, evaluation sweep) take on the binary path: the plain one forms the
// ratio block of an H sweep from |Theta - z| (pass_kernel), which IS the reference's arithmetic while
// 0 <= Theta < 1 -- true throughout a fit that starts from factors in range (W on the simplex, H <= 1 - eps stay so) and
// eps >= 1e-12 (so that 1 - eps is below 1).  Anything else -- H_init above 1, negative entries, a tiny eps -- takes the
// TINY variant, whose selects follow `_solver.py:42-43` for any Theta.
// Which variant of the sweeps a run takes.  The plain variant (TINY = false) forms |Theta - z| for the denominators,
// shares one reciprocal among a lane's entries and renormalises the likelihood's product once per trip; all of that is
// the reference's arithmetic to rounding (one-step goldens <= 1e-13, curves <= 1e-10: tests/test_gpu_parity.py) -- since
// round 4 no longer bit for bit on the binary path either: with eps riding in Theta's accumulator the H-update forms
// P1 = P1' - P2' / (1 + 2 eps) from all-entry sums, so a column with no observed one gets a rounding residue (which the
// clip to [eps, 1 - eps] absorbs) where the reference has an exact 0 -- and ONLY under these invariants:
//   eps >= 1e-12            (1 - eps < 1 in double; sixteen factors >= eps stay above 1e-192; products of four or eight
//                            denominators cannot underflow),
//   W >= 0 with column sums <= 1 + 1e-12  and  0 <= H <= 1 - 1e-9   when the factors were set (factors_in_range, checked
//                            on the device by nbmf_set_factors): then 0 <= Theta < 1 for the whole fit -- the W-update
//                            renormalises or projects onto the simplex, the H-update clips to [eps, 1 - eps].
// Anything else -- H_init above 1 (the reference uses it as given, _solver.py:133), negative entries, transform's
// un-normalised start (_base.py:175: w_free), a tiny eps -- takes the TINY variant, which keeps the reference's own
// selects, one reciprocal per entry and a renormalisation per entry
// (tests: test_factors_out_of_the_fits_range_follow_the_reference).
//   eps < 2^-22            (binary path only: the high word of 1 + 2 eps is that of 1.0, so that z = 1 + 2 eps shares it;
//                            the general path forms (1 + 2 eps) - t1 by plain arithmetic and has no such limit).
int tiny_a(const nbmf_ctx* c) {
  return c->eps < 1e-70 || !(c->eps >= 1e-12 && c->factors_in_range) || (c->data_kind == DATA_BIN && !(c->eps < 0x1p-22));
}
// In what form the H sweep of the binary path's plain variant leaves its products: P1' = L r (ALL entries'
// reciprocals) and P2' = (1 + 2 eps) L R2.  The H-update kernels take 1 / (1 + 2 eps) and undo both maps on the summed
// K x N products -- P2 = P2' / (1 + 2 eps), P1 = P1' - P2 (linear: after the sum over chunks and over ranks) --; 0 says
// the products are P1, P2 themselves (general path, the TINY variant, sliced runs).
double pform_inv12(const nbmf_ctx* c) {
  if (c->data_kind != DATA_BIN || c->KS != 1 || tiny_a(c)) return 0.0;
  return 1.0 / ((1.0 + c->eps) + c->eps);
}

double ll_pad_of(const nbmf_ctx* c, int strict = 0) {
  // (strictly masked sweeps count observed entries only, and a pad is never one: nothing to remove.  Until round 4 the
  //  8-byte path with a folded mask was exempted here although its pads -- NaN then, -0.0 now -- contribute nothing either:
  //  held-out perplexities of real-valued data with a binary mask came out 2e-8 off, found by
  //  test_real_valued_data_with_a_binary_mask_every_sweep_variant)
  if (strict) return 0.0;
  const double n_pad = (double)c->mA * (double)c->nA - (double)c->m * (double)c->n;
  return n_pad * log(1.0 + c->eps);
}

// What travels after a sweep over image A (H-pass or Theta-only sweep), and where the global
// log-likelihood ends up (c->ll_ptr):
//   single GPU        nothing; finalize sums the per-wave partials itself
//   axis 0 (rows)     Theta-only sweep: the loglik scalar (the H-pass exchange is enqueue_iteration_rows)
//   axis 1 (columns)  [loglik, prior A, prior B]: the products stay local, the scalars do not
int enqueue_exchange_after_sweep(nbmf_ctx* c, const PassArgs& a, bool with_products, int strict) {
  const int n_loss = c->chunksH * (a.Cb / wg_strips(c));   // one log-likelihood partial per workgroup
  const double pad = ll_pad_of(c, strict);
  if (!is_sharded(c)) {
    c->ll_ptr = nullptr;
    return NBMF_OK;
  }
  if (c->shard_axis == 0 && with_products)
    return fail(NBMF_ERR_STATE, "internal: the row-split H-step exchange is driven by enqueue_iteration_rows");
  hipLaunchKernelGGL(ll_reduce_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)c->lossbuf, n_loss, pad, c->sbuf,
                     c->flags);
  HIPCHK(hipGetLastError());
  size_t cnt = 1;
  if (c->shard_axis == 1) {
    hipLaunchKernelGGL(prior_reduce_kernel, dim3(1), dim3(256), 0, c->stream, (const double*)c->prior, c->n_prior_blocks,
                       c->sbuf + 1, c->flags);
    HIPCHK(hipGetLastError());
    cnt = 3;
  }
  if (int rc = all_reduce_inplace(c, c->sbuf, cnt)) return rc;
  c->ll_ptr = c->sbuf;
  return NBMF_OK;
}

// The two sweeps' arguments over all K_pad components: the sweep over image A (H-pass; the likelihood sweeps take it
// with their own mode bits) and the one over image B (W-pass)
PassArgs h_pass_args(nbmf_ctx* c) {
  PassArgs a{};
  a.data = sweep_image(c, 0);
  a.mask = c->maskA;
  a.LT = c->WT;
  a.LG = c->WG;
  a.RfT = c->HT;
  a.out1 = c->slabH;
  a.out2 = c->slabH + (size_t)c->chunksH * c->KP * c->nA;
  a.lossbuf = c->lossbuf;
  a.done = c->flags;
  a.Rb = (int)(c->mA / 16);
  a.Cb = (int)(c->nA / 16);
  a.chunk_start = c->cstartH;
  a.C_alloc = c->nA;
  a.eps = c->eps;
  a.tiny_eps = tiny_a(c);
  a.ksteps = (c->k + 3) / 4;
  a.kblocks = (c->k + 15) / 16;
  return a;
}
PassArgs w_pass_args(nbmf_ctx* c) {
  PassArgs a{};
  a.data = sweep_image(c, 1);
  a.mask = c->maskB;
  a.LT = c->HT;
  a.LG = c->HG;
  a.RfT = c->WT;
  a.out1 = c->slabW;
  a.out2 = nullptr;
  a.lossbuf = nullptr;
  a.done = c->flags;
  a.Rb = (int)(c->nA / 16);
  a.Cb = (int)(c->mA / 16);
  a.chunk_start = c->cstartW;
  a.C_alloc = c->mA;
  a.eps = c->eps;
  a.tiny_eps = tiny_a(c) || c->w_free;   // (transform's W steps start from a W that is not on the simplex: the select variant)
  // every entry observed (no mask, or a mask of ones); pad rows of the dimension the W sweep walks (the columns of Y) would
  // count as observed zeros in the two-state variant's column sums: there are none, or they are "ones" in image B's lane
  // masks (mark_pad_rows_b)
  a.full = c->data_kind == DATA_BIN && c->n_obs == (double)c->m * (double)c->n && (c->nA == c->n || c->padB_ones);
  a.ksteps = (c->k + 3) / 4;
  a.kblocks = (c->k + 15) / 16;
  return a;
}

// Point a sweep over image `image` (0: A, 1: B) at slice sl of the components: its factor operands and, where it writes
// them, its slabs (slice-major: the chunks of slice 0, then those of slice 1, ...; out2 of image A behind all KS slices'
// out1).
void at_slice(const nbmf_ctx* c, PassArgs& a, int image, int sl) {
  const size_t offW = (size_t)sl * SLICE_K * c->mA, offH = (size_t)sl * SLICE_K * c->nA;
  a.LT = image == 0 ? c->WT + offW : c->HT + offH;
  a.LG = image == 0 ? c->WG + offW : c->HG + offH;
  a.RfT = image == 0 ? c->HT + offH : c->WT + offW;
  const size_t slab_off = image == 0 ? (size_t)c->chunksH * offH : (size_t)c->chunksW * offW;
  if (a.out1) a.out1 += slab_off;
  if (a.out2) a.out2 += slab_off;
}

// ---- n_components > 128: slices of SLICE_K components --------------------------------
// Theta of the current factors WITHOUT the last slice's part into c->theta, in the tile order of image A (image
// 0: H-pass and loglik sweeps) or image B (image 1: W-pass): one Theta-only sweep per slice, each adding onto the
// previous ones.
int enqueue_theta(nbmf_ctx* c, int image) {
  for (int sl = 0; sl < c->KS - 1; ++sl) {   // (the last slice's part is added by that slice's own fused sweep)
    PassArgs a{};
    at_slice(c, a, image, sl);   // (LG is not read by this mode; no slabs)
    a.theta = c->theta;
    a.accum = sl > 0;
    a.done = c->flags;
    a.Rb = (int)((image == 0 ? c->mA : c->nA) / 16);
    a.Cb = (int)((image == 0 ? c->nA : c->mA) / 16);
    a.chunk_start = image == 0 ? c->cstartH : c->cstartW;
    a.C_alloc = image == 0 ? c->nA : c->mA;
    a.eps = c->eps;
    a.tiny_eps = c->eps < 1e-70;
    HIPCHK(launch_theta(a, image == 0 ? c->chunksH : c->chunksW, c->stream));
  }
  return NBMF_OK;
}

// The sweeps over image A of a sliced run: back-products (with_products) of every slice, or the log-likelihood
// only.  Order: Theta-only sweeps of slices 0 .. KS-2; the LAST slice's sweep completes Theta from what they
// stored, stores the total, reports the likelihood and forms its own products; then the other slices' sweeps
// read the total.  (Theta crosses HBM 24 KS - 16 bytes per entry instead of 24 KS - 8, in one sweep fewer.)
int enqueue_a_sweeps_sliced(nbmf_ctx* c, bool with_products, int strict, int clip) {
  if (int rc = enqueue_theta(c, 0)) return rc;
  const int last = c->KS - 1;
  for (int step = 0; step < (with_products ? c->KS : 1); ++step) {
    const int sl = step == 0 ? last : step - 1;
    PassArgs a = h_pass_args(c);
    at_slice(c, a, 0, sl);
    if (step != 0) a.lossbuf = nullptr;   // the likelihood is the same in every slice's sweep
    a.strict = strict;
    a.clip = clip;
    a.theta = c->theta;
    hipError_t e;
    if (with_products)
      e = step == 0 ? launch_pass_slice<MODE_H, 2>(c->data_kind, a, c->chunksH, c->stream)
                    : launch_pass_slice<MODE_H, 1>(c->data_kind, a, c->chunksH, c->stream);
    else
      e = launch_pass_slice<MODE_L, 2>(c->data_kind, a, c->chunksH, c->stream);
    HIPCHK(e);
  }
  return NBMF_OK;
}

// Single GPU, one slice: the sweep that scores iteration t assembles its loss itself (PassFin: no finalize launch).
// every slot of the fused loss assembly empty (PassFin): at set-up, and whenever a sweep may have left some filled
// (a run that was interrupted by an error)
__global__ void fill_u64_kernel(unsigned long long* p, size_t n, unsigned long long v) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}
int fill_ll_empty(nbmf_ctx* c) {
  const size_t n = (size_t)c->chunksH * (c->nA / 16 / WG_WAVES);
  if (!c->lossfin || !n) return NBMF_OK;
  hipLaunchKernelGGL(fill_u64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, (unsigned long long*)c->lossfin, n, LL_EMPTY);
  HIPCHK(hipGetLastError());
  return NBMF_OK;
}
bool fin_fusable(const nbmf_ctx* c) { return !is_sharded(c) && c->KS == 1 && !env_set("NBMF_NO_FUSED_FINALIZE"); }
void fin_fill(nbmf_ctx* c, PassArgs& a, int t, double tol, int strict) {
  a.fin.on = 1;
  a.fin.wait_ticks = LL_WAIT_TICKS;
  const int fault = env_int("NBMF_PASSFIN_FAULT", 0);   // tests: one workgroup withholds its partial, the wait is short
  if (fault == 2) {
    a.fin.wait_ticks = 0;             // (2: nobody withholds anything, but the assembling workgroup does not wait at all -- it
  } else if (fault != 0) {            //  gives up while other workgroups of its sweep are still running, as under a tenant)
    a.fin.on = 2;
    a.fin.wait_ticks = 20000000ull;   // 0.2 s
  }
  a.lossbuf = c->lossfin;   // (the sweep's workgroups hand their partials in here; see PassFin)
  a.fin.t = t;
  a.fin.n_ll = c->chunksH * (int)(c->nA / 16 / wg_strips(c));
  a.fin.n_prior = c->n_prior_src;
  a.fin.ll_pad = ll_pad_of(c, strict);
  a.fin.am1 = c->alpha - 1.0;
  a.fin.bm1 = c->beta - 1.0;
  a.fin.n_obs = c->n_obs_global;
  a.fin.tol = tol;
  a.fin.prior = c->prior_src;
  a.fin.losses = c->losses_d;
  a.fin.scal = c->scal;
  a.fin.flags = c->flags;
}

// The sweep over image A: with_products, the H-pass; without, the Theta-only sweep -- the log-likelihood of the current
// factors at a third of the H-pass's MFMA work, its per-wave partials in lossbuf exactly as an H-pass leaves them.
// fin_t >= 0 (and fin_fusable): also the loss and stop test of iteration fin_t, in the sweep's last workgroup.
int enqueue_a_sweep(nbmf_ctx* c, bool with_products, int strict = 0, int clip = 0, int fin_t = -1, double tol = 0.0) {
  PassArgs a = h_pass_args(c);
  if (c->KS > 1) {
    if (with_products) {
      EvScope ev(c, 0);
      if (int rc = enqueue_a_sweeps_sliced(c, true, 0, 0)) return rc;
    } else {
      if (int rc = enqueue_a_sweeps_sliced(c, false, strict, clip)) return rc;
    }
    return enqueue_exchange_after_sweep(c, a, with_products, strict);
  }
  a.strict = strict;
  a.clip = clip;
  if (!with_products) a.out2 = nullptr;   // (out1 unused)
  if (fin_t >= 0) fin_fill(c, a, fin_t, tol, strict);
  if (with_products) {
    EvScope ev(c, 0, true, /*attach=*/true);
    HIPCHK(launch_pass<MODE_H>(c->KB, c->data_kind, a, c->chunksH, c->stream));
  } else {
    HIPCHK(launch_pass<MODE_L>(c->KB, c->data_kind, a, c->chunksH, c->stream));
  }
  return enqueue_exchange_after_sweep(c, a, with_products, strict);
}

int enqueue_finalize(nbmf_ctx* c, int t, double tol, bool loglik_only = false, int strict = 0) {
  // single GPU: per-wave partials + pad correction here; sharded: the exchanged scalar (pad already removed)
  const bool sh = is_sharded(c) && c->ll_ptr;
  const double* ll_src = sh ? c->ll_ptr : c->lossbuf;
  const int n_ll = sh ? 1 : c->chunksH * (int)(c->nA / 16 / wg_strips(c));
  const double pad = sh ? 0.0 : ll_pad_of(c, strict);
  // axis 1: the prior sums were exchanged with the log-likelihood
  const bool prior_x = sh && c->shard_axis == 1;
  hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(256), 0, c->stream, ll_src, n_ll, pad,
                     prior_x ? (const double*)(c->sbuf + 1) : c->prior_src,
                     loglik_only ? 0 : (prior_x ? 1 : c->n_prior_src),   // no prior term (and no 0 x NaN) in a pure log-likelihood
                     loglik_only ? 0.0 : c->alpha - 1.0, loglik_only ? 0.0 : c->beta - 1.0,
                     loglik_only ? -1.0 : c->n_obs_global, c->losses_d, t, tol, c->scal, c->flags);
  HIPCHK(hipGetLastError());
  return NBMF_OK;
}

// The products of the H-pass as every H-step source holds them: [P1 | P2], each half `chunks` partial sums
// [chunks][KP][wp] of the columns [c0, c0 + wp) (the slabs: chunksH sums, all nA columns; the exchanged sums: one, of a
// panel or of all columns), a slice's rows of a half at chunks x (its first row) x wp.
//
// H-update (h_update_kernel) of slice sl's rows of H, columns [c0, c0 + wp), from the sources at src (its slice, P1 half)
// whose partial sums lie chunk_stride doubles apart.  Grid and prior-sum pairs: one per 256 entries of the slice's KSK
// rows, from entry KSK (sl nA + c0) on.  The blocks are whole: KSK is 16 KB or SLICE_K, nA a multiple of 128, a panel's c0
// and wp multiples of 16.  For all columns of an unsliced run the grid is therefore KP nA / 256 = n_prior_blocks.
void launch_h_update(nbmf_ctx* c, const double* src, int chunks, size_t chunk_stride, long long c0, long long wp, int sl,
                     double pform, hipStream_t st) {
  const int KSK = std::min(c->KP, SLICE_K);
  const size_t per = (size_t)KSK * c->nA;
  const long long blk0 = (long long)KSK * (sl * c->nA + c0) / 256;
  hipLaunchKernelGGL(h_update_kernel, dim3((unsigned)((long long)KSK * wp / 256)), dim3(256), 0, st, src,
                     src + (size_t)chunks * c->KP * wp, chunks, chunk_stride, wp, c0, c0, wp, c->Hn + sl * per, c->HT + sl * per,
                     c->HG + sl * per, c->prior + 2 * (size_t)blk0, std::min(KSK, c->k - sl * KSK), KSK, (long long)c->n,
                     (long long)c->nA, c->alpha - 1.0, c->beta - 1.0, c->eps, c->flags, pform);
}

// Ordered sum (reduce_h_kernel) of slice sl's H-pass slabs, columns [c0, c0 + wp), into [P1 | P2] at dst (rows dst_ld
// apart, P2 KP rows behind P1) in the form P1, P2 themselves; ll_dst not null: the log-likelihood partials, summed, there.
void launch_reduce_h(nbmf_ctx* c, int sl, long long c0, long long wp, double* dst, long long dst_ld, double* ll_dst, hipStream_t st) {
  const int KSK = std::min(c->KP, SLICE_K);
  const size_t per = (size_t)KSK * c->nA;
  const int n_loss = c->chunksH * (int)(c->nA / 16 / wg_strips(c));
  hipLaunchKernelGGL(reduce_h_kernel, dim3((unsigned)(((long long)KSK * wp + 255) / 256)), dim3(256), 0, st,
                     (const double*)(c->slabH + (size_t)sl * c->chunksH * per),
                     (const double*)(c->slabH + (size_t)(c->KS + sl) * c->chunksH * per), c->chunksH, (long long)per,
                     (long long)c->nA, c0, wp, dst_ld, KSK, dst, dst + (size_t)c->KP * dst_ld, (const double*)c->lossbuf, n_loss,
                     ll_pad_of(c), ll_dst, c->flags, pform_inv12(c));
}

// H-update of all columns, one launch per slice, from [P1 | P2] at `src`: the H-pass slabs (slabs: in the form
// pform_inv12), or the products summed over chunks and ranks (P1, P2 themselves: reduce_h_kernel)
int enqueue_h_update_from(nbmf_ctx* c, const double* src, bool slabs, hipStream_t st) {
  const size_t per = (size_t)std::min(c->KP, SLICE_K) * c->nA;
  const int chunks = slabs ? c->chunksH : 1;
  for (int sl = 0; sl < c->KS; ++sl) {
    launch_h_update(c, src + (size_t)sl * chunks * per, chunks, slabs ? per : 0, 0, c->nA, sl, slabs ? pform_inv12(c) : 0.0, st);
    HIPCHK(hipGetLastError());
  }
  c->prior_src = c->prior;
  c->n_prior_src = c->n_prior_blocks;
  return NBMF_OK;
}
// (single GPU or column split: the update is elementwise in k -- one launch per slice on that slice's rows and slabs)
int enqueue_h_update(nbmf_ctx* c) { return enqueue_h_update_from(c, c->slabH, /*slabs=*/true, c->stream); }

template <int GROUPS>
int launch_w_update(nbmf_ctx* c, const double* q, int chunks, double n_div, int projection) {
  const size_t lds_bytes = sizeof(double) * ((size_t)c->KP + 2) * WU_COLS;
  if (lds_bytes > 65536)
    HIPCHK(hipFuncSetAttribute((const void*)w_update_kernel<GROUPS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(w_update_kernel<GROUPS>, dim3((unsigned)(c->mA / WU_COLS)), dim3(WU_COLS * GROUPS), lds_bytes, c->stream, q,
                     chunks, c->Wn, c->WT, c->WG, c->k, c->KP, std::min(c->KP, SLICE_K), (long long)c->m, (long long)c->mA, n_div,
                     c->rowcnt, projection, c->flags);
  HIPCHK(hipGetLastError());
  return NBMF_OK;
}
int enqueue_w_update(nbmf_ctx* c, const double* q, int chunks, double n_div, int projection) {
  // 1024-thread blocks up to two rounds of them (two are resident per CU), 256-thread blocks beyond (w_update_kernel;
  // measured at K = 64: 32768 rows 28 against 30 us, 65536 rows 50 against 38 us)
  return c->mA / WU_COLS <= 4LL * c->cus ? launch_w_update<32>(c, q, chunks, n_div, projection)
                                        : launch_w_update<8>(c, q, chunks, n_div, projection);
}

// Rows of Y split: ordered sum of the H-pass slabs into [P1 | P2 | loglik] at `dst` (natural [KP][nA] twice);
// with slices, one launch per slice on its rows.
int enqueue_reduce_h_all(nbmf_ctx* c, double* dst, hipStream_t st) {
  const size_t per = (size_t)std::min(c->KP, SLICE_K) * c->nA, tot = (size_t)c->KP * c->nA;
  for (int sl = 0; sl < c->KS; ++sl) {
    launch_reduce_h(c, sl, 0, c->nA, dst + sl * per, c->nA, sl == 0 ? dst + 2 * tot : (double*)nullptr, st);
    HIPCHK(hipGetLastError());
  }
  return NBMF_OK;
}

int enqueue_w_step(nbmf_ctx* c, int projection);

// Rows of Y split, peer transport: the H-step exchange is this library's own reduce-scatter over xGMI with
// the H-update fused in (each rank updates 1/R of the columns and broadcasts H', so the update is not
// repeated R times and only K*N instead of 2*K*N doubles come back).  Order on the stream:
//   H-pass -> slab reduction into the arena -> peer_h_kernel (H' staged in every arena, loglik total)
//   -> loss + stop test of iteration it-1 -> peer_h_apply_kernel (skipped once the stop flag is up, so the
//   factors stay those of iteration it-1, as in the single-GPU run) -> W-pass -> W-update.
int enqueue_iteration_rows_peer(nbmf_ctx* c, int it, double tol) {
  const size_t per = (size_t)c->KP * c->nA;
  {
    EvScope ev(c, 0, true, /*attach=*/c->KS == 1);
    if (c->KS > 1) {
      if (int rc = enqueue_a_sweeps_sliced(c, true, 0, 0)) return rc;
    } else {
      HIPCHK(launch_pass<MODE_H>(c->KB, c->data_kind, h_pass_args(c), c->chunksH, c->stream));
    }
  }
  double* X = c->arena;   // [P1 (KP x nA) | P2 (KP x nA) | loglik], natural order
  const unsigned long long hs = ++c->hseq;
  const int slots_per_panel = PEER_H_WGS * c->pv.nranks;
  const long long offPR_now = c->offPR + (long long)(hs & 1) * 2 * 2 * PEER_H_WGS * PEER_MAX_RANKS;
  double* ll_slot = c->scal + 4;
  // the loss and stop test of iteration it-1 ride in the exchange kernel (its first workgroup): they read the
  // prior sums the PREVIOUS exchange left in the arena
  const long long offPR_prev = c->prior_src ? (long long)(c->prior_src - c->arena) : 0;
  const bool prev_in_arena = c->prior_src >= c->arena && c->prior_src < c->arena + c->arena_doubles;
  const int fin_t = (it > 0 && prev_in_arena) ? it - 1 : -1;
  // One column panel [pc0[p], pc0[p+1]) of the H-step on stream `st`: ordered slab sum into the arena, then the
  // fused reduce-scatter + Beta-MAP update + broadcast of this rank's slice of the panel (flag slot p).
  auto exchange_panel = [&](int p, hipStream_t st, unsigned long long e) -> int {
    const long long c0 = c->pc0[p], wp = c->pc0[p + 1] - c0;
    if (c->KS > 1) {
      if (int rc = enqueue_reduce_h_all(c, X, st)) return rc;   // (slices: one panel, see comm_finish_init)
    } else {
      launch_reduce_h(c, 0, c0, wp, X + c0, c->nA, p == 0 ? X + 2 * per : (double*)nullptr, st);
      HIPCHK(hipGetLastError());
    }
    PeerView pv = c->pv;
    pv.fbase = p * PF_SLOT;
    hipLaunchKernelGGL(peer_h_kernel, dim3(PEER_H_WGS), dim3(256), 0, st, pv, e, (long long)per, p == 0 ? (long long)(2 * per) : -1LL,
                       c->offHX, offPR_now, p * slots_per_panel + PEER_H_WGS * c->pv.rank, c->psl_c0[p], c->psl_wp[p],
                       (const double*)c->Hn, c->k, c->KP, (long long)c->n, (long long)c->nA, c->alpha - 1.0, c->beta - 1.0, c->eps,
                       ll_slot, c->flags, p == 0 ? fin_t : -1, offPR_prev, c->n_prior_src, c->n_obs_global, c->losses_d, tol,
                       c->scal, /*pform=*/0.0);   // (every rank's arena holds P1, P2 themselves: reduce_h_kernel)
    HIPCHK(hipGetLastError());
    return NBMF_OK;
  };
  auto apply_panel = [&](int p, hipStream_t st, unsigned long long e) -> int {
    PeerView pv = c->pv;
    pv.fbase = p * PF_SLOT;
    hipLaunchKernelGGL(peer_h_apply_kernel, dim3(PEER_H_WGS), dim3(256), 0, st, pv, e, c->offHX, c->Hn, c->HT, c->HG, c->KP,
                       std::min(c->KP, SLICE_K), (long long)c->nA, c->pc0[p], c->pc0[p + 1] - c->pc0[p], c->flags);
    HIPCHK(hipGetLastError());
    return NBMF_OK;
  };
  const bool two = c->npanel == 2 && c->stream2;
  hipStream_t s0 = c->stream, s1 = two ? c->stream2 : c->stream;
  const unsigned long long e0 = ++c->epoch, e1 = two ? ++c->epoch : 0;
  // ---- panel 0 (with the log-likelihood, the loss and the stop test of iteration it-1) on the main stream
  if (int rc = exchange_panel(0, s0, e0)) return rc;
  c->ll_ptr = ll_slot;
  if (it > 0 && fin_t < 0)
    if (int rc = enqueue_finalize(c, it - 1, tol)) return rc;   // (first iteration after nbmf_set_factors: local prior sums)
  c->prior_src = c->arena + offPR_now;
  c->n_prior_src = c->npanel * slots_per_panel;
  if (!two) {
    if (int rc = apply_panel(0, s0, e0)) return rc;
    return enqueue_w_step(c, c->projection);   // the rows of W are local: no exchange in the W-step
  }
  // ---- two panels: panel 1's exchange travels on the side stream while panel 0 is applied and the W-pass sweeps
  //      the chunks that read only panel 0's columns of H' (it is chunked over exactly that index); panel 1's H'
  //      is applied behind the stop test and feeds the remaining chunks there.
  // (panel 1's exchange kernel starts behind panel 0's, which settles the stop flag of iteration it-1: every rank
  //  must see the same flag when its kernel decides whether to take part, or the others wait for it in vain)
  HIPCHK(hipEventRecord(c->evF, s0));
  HIPCHK(hipStreamWaitEvent(s1, c->evF, 0));
  if (int rc = exchange_panel(1, s1, e1)) return rc;
  if (int rc = apply_panel(1, s1, e1)) return rc;
  PassArgs w = w_pass_args(c);
  {
    PassArgs w1 = w;
    w1.chunk0 = c->wsplit;
    HIPCHK(launch_pass<MODE_W>(c->KB, c->data_kind, w1, c->chunksW - c->wsplit, s1));
    HIPCHK(hipEventRecord(c->ev1, s1));
  }
  if (int rc = apply_panel(0, s0, e0)) return rc;
  {
    EvScope ev(c, 1);   // until both halves are done (includes any wait for panel 1's exchange)
    HIPCHK(launch_pass<MODE_W>(c->KB, c->data_kind, w, c->wsplit, s0));
    HIPCHK(hipStreamWaitEvent(s0, c->ev1, 0));
  }
  return enqueue_w_update(c, c->slabW, c->chunksW, (double)c->n, c->projection);
}

// One whole iteration when the ROWS of Y are split over the ranks.  The exchange [P1 | P2 | loglik] is
// cut into (at most) two column panels; panel 1's reduction + all-reduce + H-update run on stream2 while
// stream 1 already updates panel 0 and sweeps the W-pass chunks that only read panel 0's columns of H'
// (the W-pass is chunked over exactly that index).  With the host transport everything stays on one
// stream (it synchronises anyway); the arithmetic is the same.
int enqueue_iteration_rows(nbmf_ctx* c, int it, double tol) {
  if (c->peer) return enqueue_iteration_rows_peer(c, it, tol);
  if (c->KS > 1) {
    // slices: one exchange of the whole [P1 | P2 | loglik], no panels
    const size_t tot = (size_t)c->KP * c->nA;
    {
      EvScope ev(c, 0);
      if (int rc = enqueue_a_sweeps_sliced(c, true, 0, 0)) return rc;
    }
    if (int rc = enqueue_reduce_h_all(c, c->Pbuf, c->stream)) return rc;
    if (int rc = all_reduce_inplace(c, c->Pbuf, 2 * tot + 1)) return rc;
    c->ll_ptr = c->Pbuf + 2 * tot;
    if (it > 0)
      if (int rc = enqueue_finalize(c, it - 1, tol)) return rc;
    if (int rc = enqueue_h_update_from(c, c->Pbuf, /*slabs=*/false, c->stream)) return rc;
    return enqueue_w_step(c, c->projection);
  }
  hipStream_t s0 = c->stream;
  const bool two_streams = c->npanel == 2 && c->comm && c->stream2;
  hipStream_t s1 = two_streams ? c->stream2 : s0;
  // ---- H-pass (all columns)
  {
    EvScope ev(c, 0, true, /*attach=*/true);
    HIPCHK(launch_pass<MODE_H>(c->KB, c->data_kind, h_pass_args(c), c->chunksH, s0));
  }
  if (two_streams) HIPCHK(hipEventRecord(c->evH, s0));
  auto reduce_panel = [&](int p, hipStream_t st) -> int {
    const long long c0 = c->pc0[p], wp = c->pc0[p + 1] - c0;
    double* d1 = c->Pbuf + c->pbase[p];
    launch_reduce_h(c, 0, c0, wp, d1, wp, p == 0 ? c->Pbuf + c->ll_index : (double*)nullptr, st);
    HIPCHK(hipGetLastError());
    return all_reduce_inplace(c, d1, 2 * (size_t)c->KP * wp + (p == 0 ? 1 : 0), st);
  };
  auto update_panel = [&](int p, hipStream_t st) -> int {
    const long long c0 = c->pc0[p], wp = c->pc0[p + 1] - c0;
    launch_h_update(c, c->Pbuf + c->pbase[p], 1, 0, c0, wp, 0, /*pform=*/0.0, st);   // (the exchanged sums: P1, P2 themselves)
    HIPCHK(hipGetLastError());
    c->prior_src = c->prior;
    c->n_prior_src = c->n_prior_blocks;
    return NBMF_OK;
  };
  // ---- panel 0 (+ loglik) on the main stream; the loss of iteration it-1 and its stop test
  if (int rc = reduce_panel(0, s0)) return rc;
  c->ll_ptr = c->Pbuf + c->ll_index;
  if (it > 0)
    if (int rc = enqueue_finalize(c, it - 1, tol)) return rc;
  if (two_streams) HIPCHK(hipEventRecord(c->evF, s0));
  // ---- panel 1 on the side stream: behind the H-pass, its update behind the stop test, then straight
  //      into the W-pass chunks that read panel 1's columns (they run beside the other half on the GPU)
  PassArgs w = w_pass_args(c);
  const int first = c->npanel == 2 ? c->wsplit : c->chunksW;
  if (c->npanel == 2) {
    if (two_streams) HIPCHK(hipStreamWaitEvent(s1, c->evH, 0));
    if (int rc = reduce_panel(1, s1)) return rc;
    if (two_streams) HIPCHK(hipStreamWaitEvent(s1, c->evF, 0));
    if (int rc = update_panel(1, s1)) return rc;
    if (two_streams) {
      PassArgs w1 = w;
      w1.chunk0 = first;
      HIPCHK(launch_pass<MODE_W>(c->KB, c->data_kind, w1, c->chunksW - first, s1));
      HIPCHK(hipEventRecord(c->ev1, s1));
    }
  }
  if (int rc = update_panel(0, s0)) return rc;
  // ---- W-pass: the chunks over panel 0's columns on the main stream
  {
    EvScope ev(c, 1);   // with two streams: until both halves are done (includes any wait for panel 1's exchange)
    HIPCHK(launch_pass<MODE_W>(c->KB, c->data_kind, w, first, s0));
    if (c->npanel == 2) {
      if (two_streams) {
        HIPCHK(hipStreamWaitEvent(s0, c->ev1, 0));
      } else {
        w.chunk0 = first;
        HIPCHK(launch_pass<MODE_W>(c->KB, c->data_kind, w, c->chunksW - first, s0));
      }
    }
  }
  return enqueue_w_update(c, c->slabW, c->chunksW, (double)c->n, c->projection);
}

int enqueue_w_step(nbmf_ctx* c, int projection) {
  if (c->KS > 1) {
    {
      EvScope ev(c, 1);
      if (int rc = enqueue_theta(c, 1)) return rc;
      for (int step = 0; step < c->KS; ++step) {   // the last slice first: it completes and stores Theta'
        const int sl = step == 0 ? c->KS - 1 : step - 1;
        PassArgs w = w_pass_args(c);
        at_slice(c, w, 1, sl);
        w.theta = c->theta;
        if (step == 0)
          HIPCHK((launch_pass_slice<MODE_W, 2>(c->data_kind, w, c->chunksW, c->stream)));
        else
          HIPCHK((launch_pass_slice<MODE_W, 1>(c->data_kind, w, c->chunksW, c->stream)));
      }
    }
    if (is_sharded(c) && c->shard_axis == 1) {
      // columns of Y split: sum every slice's slabs into its rows of Qbuf, one exchange of K_pad x m
      const long long per = (long long)SLICE_K * c->mA;
      for (int sl = 0; sl < c->KS; ++sl) {
        hipLaunchKernelGGL(reduce_w_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, c->stream,
                           (const double*)(c->slabW + (size_t)sl * c->chunksW * per), c->Qbuf + sl * per, c->chunksW, per, c->flags);
        HIPCHK(hipGetLastError());
      }
      if (int rc = all_reduce_inplace(c, c->Qbuf, (size_t)c->KP * c->mA)) return rc;
      return enqueue_w_update(c, c->Qbuf, 1, c->n_div_global, projection);
    }
    return enqueue_w_update(c, c->slabW, c->chunksW, (double)c->n, projection);
  }
  PassArgs a = w_pass_args(c);
  {
    EvScope ev(c, 1, true, /*attach=*/true);
    HIPCHK(launch_pass<MODE_W>(c->KB, c->data_kind, a, c->chunksW, c->stream));
  }
  const double* q = c->slabW;
  int chunks = c->chunksW;
  double n_div = (double)c->n;
  if (is_sharded(c) && c->shard_axis == 1) {
    // columns of Y are split: the bracket of _solver.py:53 is a sum over ranks -> one all-reduce of K x m
    const long long per = (long long)c->KP * c->mA;
    hipLaunchKernelGGL(reduce_w_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, c->stream,
                       (const double*)c->slabW, c->Qbuf, c->chunksW, per, c->flags);
    HIPCHK(hipGetLastError());
    if (int rc = all_reduce_inplace(c, c->Qbuf, (size_t)per)) return rc;
    q = c->Qbuf;
    chunks = 1;
    n_div = c->n_div_global;
  }
  return enqueue_w_update(c, q, chunks, n_div, projection);
}

// ---- small problems: the fit in one persistent launch (nbmf_small_kernel.inc) ------------------------------
// natural padded [KP][lenA] -> T and G images (restoring the factors after an abandoned persistent run)
__global__ void expand_factor_kernel(const double* __restrict__ Fn, double* __restrict__ FT, double* __restrict__ FG, int KP,
                                     int KS, long long lenA) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)KP * lenA) return;
  const long long k = idx / lenA, x = idx % lenA;
  FT[t_index(k, x, KS, lenA)] = Fn[idx];
  FG[g_index(k, x, KS, lenA)] = Fn[idx];
}

// The factor launches on the context's stream, for W (h = false: lengths m, mA) or H (h = true: n, nA).  set: natural
// [k][len] at src -> padded natural [KP][lenA] and its T and G images (slice width min(KP, SLICE_K): KP in every unsliced
// run, the single-launch engine's included); get: the other way; expand: the context's own natural factor -> its images.
void launch_set_factor(const nbmf_ctx* c, bool h, const double* src, double* Fn, double* FT, double* FG) {
  const long long len = h ? c->n : c->m, lenA = h ? c->nA : c->mA, tot = (long long)c->KP * lenA;
  hipLaunchKernelGGL(set_factor_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, src, Fn, FT, FG, c->k, c->KP,
                     std::min(c->KP, SLICE_K), len, lenA);
}
void launch_get_factor(const nbmf_ctx* c, bool h, const double* Fn, double* dst) {
  const long long len = h ? c->n : c->m, lenA = h ? c->nA : c->mA, tot = (long long)c->k * len;
  hipLaunchKernelGGL(get_factor_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, Fn, dst, c->k, len, lenA);
}
void launch_expand_factor(const nbmf_ctx* c, bool h) {
  const long long lenA = h ? c->nA : c->mA, tot = (long long)c->KP * lenA;
  hipLaunchKernelGGL(expand_factor_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, (const double*)(h ? c->Hn : c->Wn),
                     h ? c->HT : c->WT, h ? c->HG : c->WG, c->KP, c->KP, lenA);
}

// How many workgroups a strip of the H-step (sweep of Rbe blocks, Cbe strips) or of the W-step is split over: aim at
// two tiles per wave, stay within the CUs, at most 8 parts (one partner hand-off costs ~2 us: not worth it for
// shorter sweeps).
constexpr int SMALL_MAX_WGS = 256;   // workgroups a persistent run may have: the hand-off words, flags and partial buffers are sized for it
int small_parts(const nbmf_ctx* c, long long sweep_blocks, long long strips) {
  const int NW = sm_waves(c->KB);
  long long pp = (sweep_blocks + 2 * NW - 1) / (2 * NW);
  pp = std::min<long long>(pp, std::min<long long>(8, std::min(c->cus, SMALL_MAX_WGS) / std::max<long long>(1, strips)));
  return (int)std::max<long long>(1, pp);
}

// Is this run one for the persistent kernel?  One GPU, at most 32 components (the 16-wave workgroups leave 128
// registers per lane), no per-launch instrumentation asked for, every workgroup on a CU of its own, at most SM_TPW
// tiles per wave and phase, at most 128 H-strips (the loss is summed by one wave, two strips per lane) -- and not
// more than NBMF_SMALL_TILES tiles (default 32768, which the other bounds imply anyway: at 4080 x 2040, K = 16 the
// single launch still runs 1.4x the five-kernel path; larger problems belong to the LDS-staged pass kernels).
bool small_eligible(const nbmf_ctx* c, int cus) {
  // (a progress callback does not change the engine: the run takes milliseconds, its losses are reported right after
  //  it, in the same batches -- so a verbose fit and a silent one give the same bits)
  if (is_sharded(c) || c->KS != 1 || c->KB > 2 || c->timing) return false;
  cus = std::min(cus, SMALL_MAX_WGS);   // a device reporting more CUs than the buffers were sized for uses that many of them
  if (env_int("NBMF_PERSISTENT", 1) == 0) return false;
  const long long Rbe = (c->m + 15) / 16, Cbe = (c->n + 15) / 16;
  const long long max_tiles = env_int("NBMF_SMALL_TILES", 32768LL);
  const int NW = sm_waves(c->KB), PH = small_parts(c, Rbe, Cbe), PW = small_parts(c, Cbe, Rbe);
  const bool fits = (Rbe + (long long)PH * NW - 1) / ((long long)PH * NW) <= SM_TPW && (Cbe + (long long)PW * NW - 1) / ((long long)PW * NW) <= SM_TPW;
  if (!(fits && Cbe <= 128 && Cbe * PH <= cus && Rbe * PW <= cus && Rbe * Cbe <= max_tiles)) return false;
  // the problem qualifies.  A context whose persistent kernel once gave up keeps to the launches -- counted, so that a
  // test which names the single-launch engine can tell that it did not run (nbmf_engine_stats)
  if (c->small.disabled) {
    g_engine_persistent_declined.fetch_add(1, std::memory_order_relaxed);
    return false;
  }
  return true;
}

// Admission of persistent kernels, per device and process-wide: a persistent kernel needs ALL its workgroups
// resident (one per CU) or its first barrier never completes.  Several host threads may run small fits on one GPU
// at once (experiments.perplexity_grid(concurrency=...)); launched together, their kernels would each get a share
// of the CUs and wait for the rest forever.  So a run reserves its CUs first and waits (milliseconds: these runs
// are short) while the ones in flight hold too many.
struct SmallAdmission {
  std::mutex mu;
  std::condition_variable cv;
  int busy[64] = {0};
} g_small_admission;

struct SmallReservation {
  int device, n;
  SmallReservation(int device_, int n_, int capacity) : device(device_ & 63), n(n_) {
    std::unique_lock<std::mutex> lk(g_small_admission.mu);
    g_small_admission.cv.wait(lk, [&] { return g_small_admission.busy[device] + n <= capacity || g_small_admission.busy[device] == 0; });
    g_small_admission.busy[device] += n;
  }
  ~SmallReservation() {
    {
      std::lock_guard<std::mutex> lk(g_small_admission.mu);
      g_small_admission.busy[device] -= n;
    }
    g_small_admission.cv.notify_all();
  }
};

int small_prepare(nbmf_ctx* c) {
  if (c->small.ready) return NBMF_OK;
  // one allocation carved up (a fit of a small problem is over in milliseconds: a dozen hipMallocs would show)
  const size_t fw = (size_t)c->KP * c->mA * sizeof(double), fh = (size_t)c->KP * c->nA * sizeof(double);
  const size_t g_max = 16 * SM_TPW;
  const size_t sync_b = round_up(sizeof(unsigned long long) * (SMALL_MAX_WGS + 8), 256), ll_b = round_up(sizeof(double) * 2 * g_max, 256),
               pr_b = sizeof(double) * 3 * g_max * 8 * 2, res_b = 256;
  const size_t g_all = SMALL_MAX_WGS;   // most workgroups a run can have (one per CU; small_eligible holds runs to it)
  const size_t pb_b = sizeof(double) * g_all * 2 * 16 * (size_t)c->KP, pl_b = sizeof(double) * g_all, pf_b = sizeof(unsigned long long) * g_all;
  const size_t total = 4 * fw + 4 * fh + sync_b + ll_b + pr_b + res_b + pb_b + pl_b + pf_b;
  char* base = nullptr;
  HIPCHK(dmalloc(&base, total));
  HIPCHK(hipMemsetAsync(base, 0, total, c->stream));   // (pad strips of the second set of images are never written: they must read as zero)
  c->small.slab = base;
  char* p = base;
  for (double** q : {&c->small.Wn, &c->small.WT, &c->small.WG, &c->small.snapW}) {
    *q = (double*)p;
    p += fw;
  }
  for (double** q : {&c->small.Hn, &c->small.HT, &c->small.HG, &c->small.snapH}) {
    *q = (double*)p;
    p += fh;
  }
  c->small.sync = (unsigned long long*)p;   // [strip] epoch words + abort word
  p += sync_b;
  c->small.ll_part = (double*)p;            // [parity][strip]
  p += ll_b;
  c->small.prior_part = (double*)p;         // [iteration mod 3][strip][updating wave] (sized for pairs: the second half is unused)
  p += pr_b;
  c->small.result = (int*)p;
  p += res_b;
  c->small.part_buf = (double*)p;           // [workgroup][2][16 KP]
  p += pb_b;
  c->small.part_ll = (double*)p;
  p += pl_b;
  c->small.part_flag = (unsigned long long*)p;
  c->small.ready = true;
  return NBMF_OK;
}

// The single-launch kernel of a run (split: strips over several workgroups; batch: nbmf_run_batch), its waves per
// workgroup and dynamic LDS, with the attribute that allows that much; k->f stays null if no kernel is built for the context.
struct SmallKernel {
  const void* f = nullptr;
  int NW = 0;
  size_t lds_bytes = 0;
};
template <int KB, bool SPLIT, bool BATCH>
const void* small_ptr(int data_kind) {
  switch (data_kind) {
    case DATA_BIN: return (const void*)small_fit_kernel<KB, DATA_BIN, SPLIT, BATCH>;
    case DATA_F64: return (const void*)small_fit_kernel<KB, DATA_F64, SPLIT, BATCH>;
    case DATA_F64M: return (const void*)small_fit_kernel<KB, DATA_F64M, SPLIT, BATCH>;
  }
  return nullptr;
}
template <int KB>
const void* small_ptr(int data_kind, bool split, bool batch) {
  if (batch) return split ? small_ptr<KB, true, true>(data_kind) : small_ptr<KB, false, true>(data_kind);
  return split ? small_ptr<KB, true, false>(data_kind) : small_ptr<KB, false, false>(data_kind);
}
int small_kernel(const nbmf_ctx* c, bool split, bool batch, SmallKernel* k) {
  k->f = c->KB == 1 ? small_ptr<1>(c->data_kind, split, batch) : small_ptr<2>(c->data_kind, split, batch);
  if (!k->f) return NBMF_OK;
  k->NW = sm_waves(c->KB);
  k->lds_bytes = sizeof(double) * ((size_t)k->NW * 2 * c->KB * 4 * 64 + k->NW * 16 + 64 + 2 * c->KP * 16) + LOG_TABLE_BYTES;
  HIPCHK(hipFuncSetAttribute(k->f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k->lds_bytes));
  return NBMF_OK;
}

// Everything in SmallArgs that a run shares with every other run on this context's data: the packed images, the
// geometry, how strips are split over workgroups, the hyper-parameters that are not per problem.
void small_common_args(const nbmf_ctx* c, int max_iter, double tol, SmallArgs* out) {
  SmallArgs& a = *out;
  a.dataA = c->dataA;
  a.maskA = c->maskA;
  a.dataB = c->dataB;
  a.maskB = c->maskB;
  a.rowcnt = c->rowcnt;
  a.m = c->m; a.n = c->n; a.mA = c->mA; a.nA = c->nA;
  a.K = c->k;
  a.RbA = (int)(c->mA / 16);
  a.CbA = (int)(c->nA / 16);
  a.Rbe = (int)((c->m + 15) / 16);
  a.Cbe = (int)((c->n + 15) / 16);
  // strips whose sweep is long are split over several workgroups, a CU each (small_parts)
  a.PH = small_parts(c, a.Rbe, a.Cbe);
  a.PW = small_parts(c, a.Cbe, a.Rbe);
  if (const char* e = getenv("NBMF_SMALL_PARTS")) {   // "ph,pw" (experiments; must still satisfy small_eligible's bounds)
    int x = 0, y = 0;
    const int cap = std::min(c->cus, SMALL_MAX_WGS);
    if (sscanf(e, "%d,%d", &x, &y) == 2 && x >= a.PH && y >= a.PW && x <= 8 && y <= 8 && a.Cbe * x <= cap && a.Rbe * y <= cap) {
      a.PH = x;
      a.PW = y;
    }
  }
  a.G = std::max(a.Cbe * a.PH, a.Rbe * a.PW);
  a.max_iter = max_iter;
  a.projection = c->projection;
  a.tiny_eps = c->eps < 1e-70;
  a.tol = tol;
  a.eps = c->eps;
  a.am1 = c->alpha - 1.0;
  a.bm1 = c->beta - 1.0;
  a.n_obs = c->n_obs_global;
  a.n_div = (double)c->n;
  a.ll_pad = (256.0 * a.Rbe * a.Cbe - (double)c->m * (double)c->n) * log(1.0 + c->eps);
  a.timeout = (unsigned long long)(std::max(1.0, env_double("NBMF_SMALL_TIMEOUT_MS", 2000.0)) * 1e5);
  a.fenced = env_int("NBMF_SMALL_FENCED", 0) != 0;   // release / acquire around every hand-off (nbmf_small_kernel.inc: small_arrive)
}

// END-OF-RUN GUARD of the single-launch engine (round 6).  Its hand-offs are the guide's measured sc1 form, not the memory
// model's release / acquire (which costs more than a phase: DESIGN.md 4.4): a stale read would be a silent wrong answer.
// What CAN be checked from outside at the price of two small launches: the last loss the persistent kernel reported was
// formed from the factors as its workgroups SAW them across the final hand-offs; the launch-per-kernel engine recomputes
// the loss of the factors as they ARE in memory (a kernel boundary: no hand-off involved).  The two engines agree to
// 1e-12 relative when nothing went wrong (different summation orders; tests/test_gpu_parity.py holds them to that), a stale
// factor entry in the last sweep moves the loss by far more unless the fit has converged to that very precision.
// The scale of the comparison is max(|loss|, 1), not |loss| alone: the loss is a MEAN of per-entry terms whose logarithms
// take arguments of size 1 (Theta + eps, 1 - Theta + eps), so two summation orders differ by ~1e-16 ABSOLUTE whatever the
// mean comes to -- and on cleanly separable data under a flat prior it comes to that rounding noise itself (3.6e-18 reported
// against 1.5e-16 recomputed, either sign: tests/test_gpu_converged_regime.py), on which no relative bound can hold.  A
// mismatch is treated like an abandoned barrier: the run is redone by the launches from the snapshot and counted
// (nbmf_engine_stats: gave_up).  NBMF_SMALL_GUARD=0 switches the check off; NBMF_SMALL_GUARD_FAULT=1 (tests) makes it trip.
int loss_by_launches(nbmf_ctx* c, double* out);
bool small_guard_on() {
  static const bool on = env_int("NBMF_SMALL_GUARD", 1) != 0;
  return on;
}
int small_guard(nbmf_ctx* c, double reported, bool* ok) {
  double chk = 0.0;
  if (int rc = loss_by_launches(c, &chk)) return rc;
  if (env_set("NBMF_SMALL_GUARD_FAULT")) chk += 1e-6 * std::max(std::fabs(chk), 1.0);
  *ok = (std::isnan(chk) && std::isnan(reported)) || chk == reported ||
        std::fabs(chk - reported) <= 1e-12 * std::max({std::fabs(chk), std::fabs(reported), 1.0});
  if (!*ok && env_set("NBMF_DEBUG"))
    fprintf(stderr, "[nbmf] single-launch guard: reported loss %.17g, recomputed %.17g: redone by the launches\n", reported, chk);
  return NBMF_OK;
}

// A single-launch run that gave up, counted (nbmf_small_stats, nbmf_engine_stats); disable: a barrier was abandoned,
// and the context keeps to the launches from now on.  fmt: what NBMF_DEBUG prints.
void small_give_up(nbmf_ctx* c, bool disable, const char* fmt = nullptr, ...) {
  ++c->small.aborted;
  g_engine_persistent_aborted.fetch_add(1, std::memory_order_relaxed);
  if (disable) c->small.disabled = true;
  if (fmt && env_set("NBMF_DEBUG")) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
  }
}

// Synchronises a stream when it goes out of scope, whichever way the function returns
struct DrainGuard {
  hipStream_t st;
  ~DrainGuard() { hipStreamSynchronize(st); }
};

// Returns NBMF_OK with *handled = true when the run is complete (losses, n_iter filled, factors in the context's
// buffers); *handled = false means "use the five-kernel path" (factors restored to their state at entry).
int run_small(nbmf_ctx* c, int max_iter, double tol, double* losses, int* n_iter, bool* handled) {
  *handled = false;
  if (!small_eligible(c, c->cus)) return NBMF_OK;
  if (int rc = small_prepare(c)) return rc;
  auto& w = c->small;
  const size_t fw = (size_t)c->KP * c->mA * sizeof(double), fh = (size_t)c->KP * c->nA * sizeof(double);
  SmallArgs a{};
  small_common_args(c, max_iter, tol, &a);
  a.Wn[0] = w.Wn; a.WT[0] = w.WT; a.WG[0] = w.WG; a.Hn[0] = w.Hn; a.HT[0] = w.HT; a.HG[0] = w.HG;
  a.Wn[1] = c->Wn; a.WT[1] = c->WT; a.WG[1] = c->WG; a.Hn[1] = c->Hn; a.HT[1] = c->HT; a.HG[1] = c->HG;
  a.sync = w.sync;
  a.ll_part = w.ll_part;
  a.prior_part = w.prior_part;
  a.losses = c->losses_d;
  a.result = w.result;
  a.part_buf = w.part_buf;
  a.part_ll = w.part_ll;
  a.part_flag = w.part_flag;
  SmallKernel k;
  if (int rc = small_kernel(c, a.PH > 1 || a.PW > 1, /*batch=*/false, &k)) return rc;
  if (!k.f) return NBMF_OK;
  // snapshot for the fall-back, hand-off words cleared
  HIPCHK(hipMemcpyAsync(w.snapW, c->Wn, fw, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(w.snapH, c->Hn, fh, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipMemsetAsync(w.sync, 0, sizeof(unsigned long long) * (a.G + 1), c->stream));
  HIPCHK(hipMemsetAsync(w.part_flag, 0, sizeof(unsigned long long) * SMALL_MAX_WGS, c->stream));
  HIPCHK(hipMemsetAsync(w.result, 0, sizeof(int) * 4, c->stream));
  if (env_set("NBMF_SMALL_FORCE_ABORT")) {   // tests: raise the abort word up front, so that the fall-back runs
    const unsigned long long one = 1;
    HIPCHK(hipMemcpyAsync(w.sync + a.G, &one, sizeof one, hipMemcpyHostToDevice, c->stream));
  }
  // Whichever way this function returns from here on -- every HIPCHK below is an early return -- the stream is
  // drained BEFORE the diagnostic buffers go back to the pool and BEFORE the CU reservation is released: a persistent
  // kernel that is still resident must not see its buffers reused, nor another thread's kernel admitted beside it.
  // (Declaration order: destructors run in reverse, the synchronisation first.)
  unsigned long long *dbg = nullptr, *place = nullptr;
  struct DiagGuard {
    unsigned long long *&a, *&b;
    ~DiagGuard() {
      if (a) dfree(a);
      if (b) dfree(b);
    }
  } diag_guard{dbg, place};
  if (env_set("NBMF_SMALL_DEBUG")) {
    HIPCHK(dmalloc(&dbg, sizeof(unsigned long long) * 64 * 16));
    HIPCHK(hipMemsetAsync(dbg, 0, sizeof(unsigned long long) * 64 * 16, c->stream));
    a.dbg = dbg;
  }
  if (env_set("NBMF_SMALL_PLACEMENT")) {
    HIPCHK(dmalloc(&place, sizeof(unsigned long long) * a.G));
    a.place = place;
  }
  void* params[] = {&a};
  SmallReservation cus_held(c->device, a.G, std::min(c->cus, SMALL_MAX_WGS));
  DrainGuard drain_guard{c->stream};
  HIPCHK(hipLaunchKernel(k.f, dim3(a.G), dim3(64 * k.NW), params, k.lds_bytes, c->stream));
  if (place) {   // where the dispatcher put the workgroups: XCD . shader engine . CU
    std::vector<unsigned long long> h(a.G);
    HIPCHK(hipMemcpyAsync(h.data(), place, sizeof(unsigned long long) * a.G, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    fprintf(stderr, "[nbmf] placement (xcd.se.cu):");
    for (int i = 0; i < a.G; ++i)
      fprintf(stderr, " %u.%u.%u", (unsigned)(h[i] >> 32) & 15u, (unsigned)(h[i] >> 13) & 7u, (unsigned)(h[i] >> 8) & 15u);
    fprintf(stderr, "\n");
  }
  if (dbg) {   // per-phase wall clock of workgroup 0 (10 ns ticks): tiles | update | barrier | tiles | update+loss | barrier
    unsigned long long h[64 * 16];
    HIPCHK(hipMemcpyAsync(h, dbg, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double acc[8] = {0}, fine[7] = {0};
    int cnt = 0;
    for (int t = 8; t < 63 && t + 1 < max_iter; ++t) {
      if (!h[t * 16 + 7] || !h[(t + 1) * 16]) continue;
      for (int p = 0; p < 7; ++p) acc[p] += (double)(h[t * 16 + p + 1] - h[t * 16 + p]) * 0.01;
      acc[7] += (double)(h[(t + 1) * 16] - h[t * 16 + 7]) * 0.01;
      fine[0] += (double)(h[t * 16 + 8] - h[t * 16 + 3]) * 0.01;    // barrier exit -> operand loads issued
      fine[1] += (double)(h[t * 16 + 9] - h[t * 16 + 8]) * 0.01;    // -> operands landed
      fine[2] += (double)(h[t * 16 + 10] - h[t * 16 + 9]) * 0.01;   // -> first tile's arithmetic done
      fine[3] += (double)(h[t * 16 + 11] - h[t * 16 + 10]) * 0.01;  // -> second tile's
      fine[4] += (double)(h[t * 16 + 12] - h[t * 16 + 1]) * 0.01;   // H: tiles done -> all waves' partials in LDS
      fine[5] += (double)(h[t * 16 + 13] - h[t * 16 + 12]) * 0.01;  // -> update computed, stores issued
      fine[6] += (double)(h[t * 16 + 2] - h[t * 16 + 13]) * 0.01;   // -> prior sums published
      ++cnt;
    }
    if (cnt)
      fprintf(stderr, "[nbmf]   W tiles of wave 0 in detail: issue %.2f | operands land %.2f | tile A %.2f | tile B %.2f;  H reduce+update: "
                      "wait for all waves %.2f | update %.2f | prior sums %.2f\n", fine[0] / cnt, fine[1] / cnt, fine[2] / cnt, fine[3] / cnt,
              fine[4] / cnt, fine[5] / cnt, fine[6] / cnt);
    if (h[15] && h[63 * 16 + 15] > h[15])
      fprintf(stderr, "[nbmf]   on the device from the first instruction to the last: %.3f ms\n", (double)(h[63 * 16 + 15] - h[15]) * 1e-5);
    if (h[8 * 16 + 14] && h[62 * 16 + 14] && h[62 * 16] > h[8 * 16])
      fprintf(stderr, "[nbmf]   shader clock over iterations 8..62: %.0f MHz (%llu cycles in %.2f us)\n",
              (double)(h[62 * 16 + 14] - h[8 * 16 + 14]) / ((double)(h[62 * 16] - h[8 * 16]) * 0.01),
              (unsigned long long)(h[62 * 16 + 14] - h[8 * 16 + 14]), (double)(h[62 * 16] - h[8 * 16]) * 0.01);
    if (cnt)
      fprintf(stderr, "[nbmf] persistent fit, workgroup 0, us per iteration part (mean of %d): H tiles %.2f | H reduce+update %.2f | barrier %.2f | "
                      "W tiles %.2f | W reduce+update %.2f | loss %.2f | barrier %.2f | loop %.2f\n", cnt, acc[0] / cnt, acc[1] / cnt,
              acc[2] / cnt, acc[3] / cnt, acc[4] / cnt, acc[5] / cnt, acc[6] / cnt, acc[7] / cnt);
  }
  int res[4] = {0, 0, 0, 0};
  unsigned long long abort_word = 0;
  HIPCHK(hipMemcpyAsync(res, w.result, sizeof res, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&abort_word, w.sync + a.G, sizeof abort_word, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(stream_wait_spin(c->stream));
  ++w.runs;
  auto back_to_entry = [&]() -> int {   // (after small_give_up)
    HIPCHK(hipMemcpyAsync(c->Wn, w.snapW, fw, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->Hn, w.snapH, fh, hipMemcpyDeviceToDevice, c->stream));
    launch_expand_factor(c, /*h=*/false);
    HIPCHK(hipGetLastError());
    launch_expand_factor(c, /*h=*/true);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return NBMF_OK;
  };
  if (res[2] != 0 || abort_word != 0 || res[0] < 1 || res[0] > max_iter) {
    // a barrier was abandoned (workgroups not co-resident for too long): back to the state at entry, and this
    // context keeps to the five-kernel path from now on
    small_give_up(c, /*disable=*/true, "[nbmf] persistent fit abandoned (status %d, abort word %llu): five-kernel path\n", res[2], abort_word);
    return back_to_entry();
  }
  if (res[1] == 0) {   // the final factors sit in the second set of images
    HIPCHK(hipMemcpyAsync(c->Wn, w.Wn, fw, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->WT, w.WT, fw, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->WG, w.WG, fw, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->Hn, w.Hn, fh, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->HT, w.HT, fh, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->HG, w.HG, fh, hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(hipMemcpyAsync(losses, c->losses_d, sizeof(double) * (size_t)res[0], hipMemcpyDeviceToHost, c->stream));
  HIPCHK(stream_wait_spin(c->stream));
  if (small_guard_on()) {   // (see small_guard: the last loss as reported against the loss of the factors as they are in memory)
    bool ok = true;
    if (int rc = small_guard(c, losses[res[0] - 1], &ok)) return rc;
    if (!ok) {   // *handled stays false: the launches redo the run from the state at entry
      small_give_up(c, /*disable=*/false);
      return back_to_entry();
    }
  }
  *n_iter = res[0];
  *handled = true;
  g_engine_persistent_served.fetch_add(1, std::memory_order_relaxed);
  if (c->progress && c->progress_every > 0)   // the reports a launch-by-launch run would have made, in the same batches
    for (int first = 0; first < res[0]; first += c->progress_every)
      c->progress(c->progress_user, first, std::min(c->progress_every, res[0] - first), losses + first);
  return NBMF_OK;
}

// ---- several independent fits of the context's data in ONE persistent launch (nbmf_run_batch) -----------------------
// Problem p gets its own two parities of factor images, hand-off words, partial buffers, loss curve and result;
// the grid is (G workgroups) x (B problems), every workgroup on a CU of its own, and the workgroups of one problem
// synchronise among themselves only.  B = as many problems as the chip holds at once; more run as further launches.
// The arithmetic of a problem is exactly that of the single-problem launch (same kernel code, same G, PH, PW): a
// batched fit is bitwise the fit nbmf_run would have produced.
struct SmallBatchLayout {
  size_t fw, fh, factors, ll_b, pr_b, pb_b, pl_b, sync_b, res_b, pf_b, control, off_partials, off_control, off_losses, stride;
};
SmallBatchLayout small_batch_layout(const nbmf_ctx* c, int losses_cap) {
  SmallBatchLayout L{};
  const size_t g_max = 16 * SM_TPW;
  L.fw = (size_t)c->KP * c->mA * sizeof(double);
  L.fh = (size_t)c->KP * c->nA * sizeof(double);
  L.factors = 2 * (3 * L.fw + 3 * L.fh);                          // two parities of [Wn WT WG Hn HT HG]
  L.ll_b = round_up(sizeof(double) * 2 * g_max, 256);
  L.pr_b = sizeof(double) * 3 * g_max * 8 * 2;
  L.pb_b = sizeof(double) * SMALL_MAX_WGS * 2 * 16 * (size_t)c->KP;
  L.pl_b = round_up(sizeof(double) * SMALL_MAX_WGS, 256);
  L.sync_b = round_up(sizeof(unsigned long long) * (SMALL_MAX_WGS + 8), 256);
  L.res_b = 256;
  L.pf_b = round_up(sizeof(unsigned long long) * SMALL_MAX_WGS, 256);
  L.control = L.sync_b + L.res_b + L.pf_b;                        // cleared before every launch
  L.off_partials = L.factors;
  L.off_control = L.off_partials + L.ll_b + L.pr_b + L.pb_b + L.pl_b;
  L.off_losses = L.off_control + L.control;
  L.stride = round_up(L.off_losses + sizeof(double) * (size_t)losses_cap, 256);
  return L;
}

int small_batch_prepare(nbmf_ctx* c, int cap, int max_iter) {
  auto& b = c->small_batch;
  if (cap > b.cap || max_iter > b.losses_cap) {
    cap = std::max(cap, b.cap);
    const int lcap = std::max(max_iter, b.losses_cap);
    for (void* p : {(void*)b.slab, (void*)b.table, (void*)b.io})
      if (p) HIPCHK(dfree(p));
    b.slab = nullptr;
    b.table = nullptr;
    b.io = nullptr;
    b.cap = b.losses_cap = 0;
    const SmallBatchLayout L = small_batch_layout(c, lcap);
    const size_t total = (size_t)cap * L.stride;
    HIPCHK(dmalloc(&b.slab, total));
    HIPCHK(hipMemsetAsync(b.slab, 0, total, c->stream));   // pad strips of the images are never written with anything but zero
    HIPCHK(dmalloc(&b.table, sizeof(double) * 2 * (size_t)cap));   // [alpha - 1 | beta - 1] of the problems of a launch
    b.io_doubles = (size_t)cap * ((size_t)c->k * c->m + (size_t)c->k * c->n);
    HIPCHK(dmalloc(&b.io, sizeof(double) * b.io_doubles));
    b.cap = cap;
    b.losses_cap = lcap;
  }
  return NBMF_OK;
}

// *handled = false: the problems do not qualify for the persistent kernel (or a launch gave up): the caller runs them
// one by one.  Nothing of the context's own factor state is touched here.
int run_small_batch(nbmf_ctx* c, int nprob, const double* alpha, const double* beta, const double* W0, const double* H0,
                    int max_iter, double tol, double* losses, int* n_iter, double* W_out, double* H_out, bool* handled) {
  *handled = false;
  if (!small_eligible(c, c->cus)) return NBMF_OK;
  SmallArgs a{};
  small_common_args(c, max_iter, tol, &a);
  const int cap_cus = std::min(c->cus, SMALL_MAX_WGS);
  int B = std::max(1, cap_cus / a.G);
  B = std::max(1, std::min(B, env_int("NBMF_BATCH_MAX", B)));   // (B >= 1 already: unset changes nothing)
  B = std::min(B, nprob);
  if (int rc = small_batch_prepare(c, B, max_iter)) return rc;
  auto& b = c->small_batch;
  const SmallBatchLayout L = small_batch_layout(c, b.losses_cap);
  SmallKernel k;
  if (int rc = small_kernel(c, a.PH > 1 || a.PW > 1, /*batch=*/true, &k)) return rc;
  if (!k.f) return NBMF_OK;
  const size_t wsz = (size_t)c->k * c->m, hsz = (size_t)c->k * c->n;
  // problem 0's pointers; problem p's are these plus p * stride (PP() in the kernel, prob() here)
  {
    char* q = b.slab;
    for (int par = 0; par < 2; ++par) {
      a.Wn[par] = (double*)q; q += L.fw;
      a.WT[par] = (double*)q; q += L.fw;
      a.WG[par] = (double*)q; q += L.fw;
      a.Hn[par] = (double*)q; q += L.fh;
      a.HT[par] = (double*)q; q += L.fh;
      a.HG[par] = (double*)q; q += L.fh;
    }
    a.ll_part = (double*)q; q += L.ll_b;
    a.prior_part = (double*)q; q += L.pr_b;
    a.part_buf = (double*)q; q += L.pb_b;
    a.part_ll = (double*)q;
    char* ctl = b.slab + L.off_control;
    a.sync = (unsigned long long*)ctl;
    a.result = (int*)(ctl + L.sync_b);
    a.part_flag = (unsigned long long*)(ctl + L.sync_b + L.res_b);
    a.losses = (double*)(b.slab + L.off_losses);
    a.prob_stride = L.stride;
    a.am1s = (const double*)b.table;
    a.bm1s = (const double*)b.table + b.cap;
  }
  auto prob = [&](auto* p0, int p) { return (decltype(p0))((char*)p0 + (size_t)p * L.stride); };
  std::vector<int> res((size_t)B * 4);
  std::vector<unsigned long long> abort_words((size_t)B);
  std::vector<double> priors((size_t)2 * b.cap);
  for (int p0 = 0; p0 < nprob; p0 += B) {
    const int Bc = std::min(B, nprob - p0);
    for (int p = 0; p < Bc; ++p) {
      priors[(size_t)p] = alpha[p0 + p] - 1.0;
      priors[(size_t)b.cap + p] = beta[p0 + p] - 1.0;
    }
    HIPCHK(hipMemcpyAsync(b.table, priors.data(), sizeof(double) * priors.size(), hipMemcpyHostToDevice, c->stream));
    // initial factors of the whole chunk in one copy each, expanded into every problem's parity-1 images
    HIPCHK(hipMemcpyAsync(b.io, W0 + (size_t)p0 * wsz, sizeof(double) * wsz * Bc, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(b.io + wsz * Bc, H0 + (size_t)p0 * hsz, sizeof(double) * hsz * Bc, hipMemcpyHostToDevice, c->stream));
    for (int p = 0; p < Bc; ++p) {
      launch_set_factor(c, /*h=*/false, b.io + wsz * p, prob(a.Wn[1], p), prob(a.WT[1], p), prob(a.WG[1], p));
      launch_set_factor(c, /*h=*/true, b.io + wsz * Bc + hsz * p, prob(a.Hn[1], p), prob(a.HT[1], p), prob(a.HG[1], p));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemset2DAsync(b.slab + L.off_control, L.stride, 0, L.control, (size_t)Bc, c->stream));   // every problem's control words
    if (env_set("NBMF_SMALL_FORCE_ABORT")) {   // tests: the abort word of the first problem up front
      const unsigned long long one = 1;
      HIPCHK(hipMemcpyAsync(a.sync + a.G, &one, sizeof one, hipMemcpyHostToDevice, c->stream));
    }
    void* params[] = {&a};
    {
      SmallReservation cus_held(c->device, a.G * Bc, cap_cus);
      DrainGuard drain_guard{c->stream};
      HIPCHK(hipLaunchKernel(k.f, dim3(a.G, Bc), dim3(64 * k.NW), params, k.lds_bytes, c->stream));
      // results and abort words of all problems: strided copies
      HIPCHK(hipMemcpy2DAsync(res.data(), sizeof(int) * 4, a.result, L.stride, sizeof(int) * 4, (size_t)Bc, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpy2DAsync(abort_words.data(), sizeof(unsigned long long), a.sync + a.G, L.stride, sizeof(unsigned long long), (size_t)Bc,
                              hipMemcpyDeviceToHost, c->stream));
      HIPCHK(stream_wait_spin(c->stream));
    }
    ++b.launches;
    b.problems += Bc;
    for (int p = 0; p < Bc; ++p)
      if (res[(size_t)p * 4 + 2] != 0 || abort_words[(size_t)p] != 0 || res[(size_t)p * 4] < 1 || res[(size_t)p * 4] > max_iter) {
        small_give_up(c, /*disable=*/true, "[nbmf] batched persistent fit abandoned (problem %d): one by one\n", p0 + p);
        return NBMF_OK;             // *handled stays false: the caller redoes ALL problems one by one
      }
    // the end-of-run guard (small_guard), on ONE problem of every launch, taken in turn: its last reported loss against the
    // loss of its final factors recomputed by the launches -- on the problem's own images (the context's pointers are lent
    // to them for the three launches: no copy, and the context's own factors are untouched)
    if (small_guard_on()) {
      const int ps = (int)(b.launches % Bc), par = res[(size_t)ps * 4 + 1], nit = res[(size_t)ps * 4];
      double reported = 0.0;
      HIPCHK(hipMemcpyAsync(&reported, (const char*)a.losses + (size_t)ps * L.stride + sizeof(double) * (size_t)(nit - 1), sizeof(double),
                            hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      struct Lend {   // (restored on every path out of this block)
        nbmf_ctx* c;
        double *Wn, *WT, *WG, *Hn, *HT, *HG, alpha, beta;
        ~Lend() {
          c->Wn = Wn; c->WT = WT; c->WG = WG; c->Hn = Hn; c->HT = HT; c->HG = HG;
          c->alpha = alpha; c->beta = beta;
        }
      } lend{c, c->Wn, c->WT, c->WG, c->Hn, c->HT, c->HG, c->alpha, c->beta};
      c->Wn = prob(a.Wn[par], ps); c->WT = prob(a.WT[par], ps); c->WG = prob(a.WG[par], ps);
      c->Hn = prob(a.Hn[par], ps); c->HT = prob(a.HT[par], ps); c->HG = prob(a.HG[par], ps);
      c->alpha = alpha[p0 + ps];
      c->beta = beta[p0 + ps];
      bool ok = true;
      if (int rc = small_guard(c, reported, &ok)) return rc;
      if (!ok) {
        small_give_up(c, /*disable=*/false);
        return NBMF_OK;             // *handled stays false: the caller redoes ALL problems one by one, by the launches
      }
    }
    // results: final factors (the parity each problem ended on) through one staging copy, the loss curves in one strided copy
    for (int p = 0; p < Bc; ++p) {
      const int par = res[(size_t)p * 4 + 1];
      launch_get_factor(c, /*h=*/false, prob(a.Wn[par], p), b.io + wsz * p);
      launch_get_factor(c, /*h=*/true, prob(a.Hn[par], p), b.io + wsz * Bc + hsz * p);
      n_iter[p0 + p] = res[(size_t)p * 4];
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy2DAsync(losses + (size_t)p0 * max_iter, sizeof(double) * (size_t)max_iter, a.losses, L.stride, sizeof(double) * (size_t)max_iter,
                            (size_t)Bc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(W_out + (size_t)p0 * wsz, b.io, sizeof(double) * wsz * Bc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(H_out + (size_t)p0 * hsz, b.io + wsz * Bc, sizeof(double) * hsz * Bc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(stream_wait_spin(c->stream));
  }
  c->small.runs += nprob;
  g_engine_persistent_served.fetch_add(nprob, std::memory_order_relaxed);
  *handled = true;
  return NBMF_OK;
}

int ensure_losses(nbmf_ctx* c, int cap) {
  if (cap <= c->losses_cap) return NBMF_OK;
  if (c->losses_d) HIPCHK(dfree(c->losses_d));
  c->losses_d = nullptr;
  HIPCHK(dmalloc(&c->losses_d, sizeof(double) * (size_t)cap));
  c->losses_cap = cap;
  return NBMF_OK;
}

// ---- held-out evaluation (nbmf_eval_kernels.inc) --------------------------------------------------------
// Room for `cap` sums at eval_ll_d (values of earlier evaluations are not kept across a growth: each is read back by the
// host right behind its launch).
int ensure_eval_slots(nbmf_ctx* c, int cap) {
  auto& ev = c->eval;
  if (cap <= ev.ll_cap) return NBMF_OK;
  if (ev.eval_ll_d) HIPCHK(dfree(ev.eval_ll_d));
  ev.eval_ll_d = nullptr;
  ev.ll_cap = 0;
  HIPCHK(dmalloc(&ev.eval_ll_d, sizeof(double) * (size_t)cap));
  ev.ll_cap = cap;
  return NBMF_OK;
}

// One evaluation of the context's eval set for the factors the stream holds at this point, its sum left at
// eval_ll_d[slot]: the k-major copies of both factors, one partial per 32 pairs, the fold.  Nothing is read back here.
int enqueue_eval(nbmf_ctx* c, int slot) {
  auto& ev = c->eval;
  for (const bool h : {false, true}) {
    const long long len = h ? c->n : c->m, lenA = h ? c->nA : c->mA;
    hipLaunchKernelGGL(k_major_kernel, dim3((unsigned)((len + PT_TILE - 1) / PT_TILE), (unsigned)((c->k + PT_TILE - 1) / PT_TILE)),
                       dim3(PT_TILE * 8), 0, c->stream, (const double*)(h ? c->Hn : c->Wn), h ? ev.Hk : ev.Wk, c->k, len, lenA);
    HIPCHK(hipGetLastError());
  }
  const long long nparts = (ev.count + EV_PAIRS - 1) / EV_PAIRS;
  hipLaunchKernelGGL(eval_pairs_kernel, dim3((unsigned)nparts), dim3(EV_THREADS), 0, c->stream, (const double*)ev.Wk,
                     (const double*)ev.Hk, c->k, (const int*)ev.rows, (const int*)ev.cols, (const unsigned char*)ev.x,
                     (long long)ev.count, c->eps, ev.partials);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(EV_FOLD), 0, c->stream, (const double*)ev.partials, nparts,
                     ev.eval_ll_d + slot);
  HIPCHK(hipGetLastError());
  return NBMF_OK;
}

void eval_release(nbmf_ctx* c) {   // the caller has drained the stream
  auto& ev = c->eval;
  void* ptrs[] = {ev.rows, ev.cols, ev.x, ev.Wk, ev.Hk, ev.partials};
  for (void* p : ptrs)
    if (p) dfree(p);
  ev.rows = ev.cols = nullptr;
  ev.x = nullptr;
  ev.Wk = ev.Hk = ev.partials = nullptr;
  ev.count = 0;
}

// After an upload of binary data that is observed everywhere: see mask_pad_rows_kernel (the two-state W sweep then
// applies whatever the shape).  Called once n_obs is known; setup_workspaces has just rebuilt the lane masks.
int mark_pad_rows_b(nbmf_ctx* c) {
  c->padB_ones = false;
  if (c->data_kind != DATA_BIN || !c->bitsB || c->n_obs != (double)c->m * (double)c->n || c->nA == c->n) return NBMF_OK;
  const long long RbB = c->nA / 16, CbB = c->mA / 16, nblk = RbB - (c->n >> 4);
  const long long threads = CbB * nblk * 4;
  hipLaunchKernelGGL(mask_pad_rows_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c->stream, c->bitsB, RbB, CbB,
                     (long long)c->n);
  HIPCHK(hipGetLastError());
  c->padB_ones = true;
  return NBMF_OK;
}

// Chunking of the two sweeps and the slabs that go with it; needs the storage path (it decides the
// kernels' residency), so it runs at the end of nbmf_upload.
int setup_workspaces(nbmf_ctx* c) {
  const int cus = c->cus;
  const int NB = 8 / c->KB;
  const int slotsH = cus * resident_per_cu<MODE_H>(c->KB, c->data_kind);
  const int slotsW = cus * resident_per_cu<MODE_W>(c->KB, c->data_kind);
  const int ns = wg_strips(c) / WG_WAVES;
  pick_chunks((int)(c->nA / 16 / wg_strips(c)), (int)(c->mA / 16), NB, slotsH, ns, cus, /*one_round_ok=*/true, &c->chunksH, &c->CH_H);
  pick_chunks((int)(c->mA / 16 / wg_strips(c)), (int)(c->nA / 16), NB, slotsW, ns, cus, /*one_round_ok=*/false, &c->chunksW, &c->CH_W);
  const std::vector<int> bH = chunk_boundaries((int)(c->mA / 16), c->CH_H);
  const std::vector<int> bW = chunk_boundaries((int)(c->nA / 16), c->CH_W);
  c->chunksH = (int)bH.size() - 1;
  c->chunksW = (int)bW.size() - 1;
  c->bW_host = bW;
  for (int** p : {&c->cstartH, &c->cstartW}) {
    if (*p) HIPCHK(dfree(*p));
    *p = nullptr;
  }
  HIPCHK(dmalloc(&c->cstartH, sizeof(int) * bH.size()));
  HIPCHK(dmalloc(&c->cstartW, sizeof(int) * bW.size()));
  HIPCHK(hipMemcpy(c->cstartH, bH.data(), sizeof(int) * bH.size(), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->cstartW, bW.data(), sizeof(int) * bW.size(), hipMemcpyHostToDevice));
  if (env_set("NBMF_DEBUG"))
    fprintf(stderr, "[nbmf] K_pad=%d path=%d: H-pass %d x %d workgroups (chunk %d blocks, %d slots), W-pass %d x %d (chunk %d, %d slots)\n",
            c->KP, c->data_kind, (int)(c->nA / 64), c->chunksH, c->CH_H, slotsH, (int)(c->mA / 64), c->chunksW, c->CH_W, slotsW);
  for (double** p : {&c->slabH, &c->slabW, &c->lossbuf, &c->lossfin}) {
    if (*p) HIPCHK(dfree(*p));
    *p = nullptr;
  }
  // binary path: the lane-mask images of the two code images (what the sweeps read)
  for (unsigned long long** p : {&c->bitsA, &c->bitsB}) {
    if (*p) HIPCHK(dfree(*p));
    *p = nullptr;
  }
  if (c->data_kind == DATA_BIN) {
    const long long n_tiles = (long long)(c->mA / 16) * (c->nA / 16);
    HIPCHK(dmalloc(&c->bitsA, sizeof(unsigned long long) * 8 * (size_t)n_tiles + PASS_SLACK));   // (slack: record requests and
    HIPCHK(dmalloc(&c->bitsB, sizeof(unsigned long long) * 8 * (size_t)n_tiles + PASS_SLACK));   //  prefetches run past the end)
    for (int image = 0; image < 2; ++image) {
      hipLaunchKernelGGL(mask_build_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, c->stream,
                         (const uint32_t*)(image == 0 ? c->dataA : c->dataB), image == 0 ? c->bitsA : c->bitsB, n_tiles);
      HIPCHK(hipGetLastError());
    }
  }
  const size_t fw = (size_t)c->KP * c->mA * sizeof(double), fh = (size_t)c->KP * c->nA * sizeof(double);
  HIPCHK(dmalloc(&c->slabH, 2 * (size_t)c->chunksH * fh));
  HIPCHK(dmalloc(&c->slabW, (size_t)c->chunksW * fw));
  const size_t n_slots = (size_t)c->chunksH * (c->nA / 16 / WG_WAVES);
  HIPCHK(dmalloc(&c->lossbuf, sizeof(double) * n_slots));
  HIPCHK(dmalloc(&c->lossfin, sizeof(double) * n_slots));
  if (int rc = fill_ll_empty(c)) return rc;
  return NBMF_OK;
}

// Drop whatever communicator is attached (the stream must be idle); the context is single-GPU again.
void comm_release(nbmf_ctx* c, bool recount = false) {
  // the column split replaced the per-row observed counts by their global sums: back to this shard's own
  if (recount && is_sharded(c) && c->shard_axis == 1 && c->data_kind >= 0) {
    hipLaunchKernelGGL(rowcount_kernel, dim3((unsigned)((c->m + 255) / 256)), dim3(256), 0, c->stream, c->dataB, c->maskB,
                       c->data_kind, (long long)(c->nA / 16), (long long)c->m, (long long)c->n, c->rowcnt);
    hipStreamSynchronize(c->stream);
  }
  if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
  c->comm = nullptr;
  c->host_reduce = nullptr;
  c->host_reduce_user = nullptr;
  if (c->peer) {
    c->Pbuf = c->Pbuf_own;
    c->sbuf = c->sbuf_own;
    c->Qbuf = c->Qbuf_own;
    c->Pbuf_own = c->sbuf_own = c->Qbuf_own = nullptr;
  }
  for (void* q : c->peer_mapped) hipIpcCloseMemHandle(q);
  c->peer_mapped.clear();
  c->peer = false;
  c->prior_src = c->prior;
  c->n_prior_src = c->n_prior_blocks;
  c->ll_ptr = nullptr;
  c->nranks = 1;
  c->rank = 0;
  c->shard_axis = 0;
  c->npanel = 1;
  c->n_obs_global = c->n_obs;
  c->n_div_global = (double)c->n;
}

// After a stream synchronisation: did a peer exchange give up waiting?
int peer_check(nbmf_ctx* c) {
  if (!c->peer) return NBMF_OK;
  unsigned long long err = 0;
  HIPCHK(hipMemcpy(&err, c->pflags + PF_ERR, sizeof err, hipMemcpyDeviceToHost));
  if (err)
    return fail(NBMF_ERR_COMM, "peer exchange %llu timed out on rank %d (a rank died, stalled for more than "
                               "NBMF_PEER_TIMEOUT_MS, or ran a different sequence of calls); detach the communicator", err, c->rank);
  return NBMF_OK;
}

int ready(nbmf_ctx* c) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (c->data_kind < 0) return fail(NBMF_ERR_STATE, "nbmf_upload has not been called");
  if (!c->have_factors) return fail(NBMF_ERR_STATE, "nbmf_set_factors has not been called");
  return NBMF_OK;
}

int set_device(nbmf_ctx* c) {
  HIPCHK(hipSetDevice(c->device));
  return NBMF_OK;
}

// One sweep over image A and its finalize, the result read back: the loss of the current factors (with_prior: the Beta
// log-prior sums recomputed first) or their log-likelihood.  collect_timing: fold any recorded sweep events into the
// totals (nbmf_timing_get).
int one_shot(nbmf_ctx* c, bool with_prior, int strict, int clip, bool collect_timing, double* out) {
  if (int rc = set_device(c)) return rc;
  if (int rc = ensure_losses(c, 1)) return rc;
  HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 8, c->stream));
  if (with_prior) {
    hipLaunchKernelGGL(prior_kernel, dim3(c->n_prior_blocks), dim3(256), 0, c->stream, c->Hn, c->prior, c->k, c->KP,
                       (long long)c->n, (long long)c->nA, c->eps);
    HIPCHK(hipGetLastError());
    c->prior_src = c->prior;
    c->n_prior_src = c->n_prior_blocks;
  }
  if (int rc = enqueue_a_sweep(c, /*with_products=*/false, strict, clip)) return rc;
  // (a pure log-likelihood has no prior term, and no pad term when strict: -(ll + 0 + 0) / -1 = ll)
  if (int rc = enqueue_finalize(c, 0, 0.0, /*loglik_only=*/!with_prior, strict)) return rc;
  HIPCHK(hipMemcpyAsync(out, c->losses_d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (collect_timing && c->timing) timing_collect(c);
  return peer_check(c);
}

// (also the single-launch engine's end-of-run guard: small_guard)
int loss_by_launches(nbmf_ctx* c, double* loss) { return one_shot(c, /*with_prior=*/true, 0, 0, /*collect_timing=*/true, loss); }

// ---- shared by the eight entry points that read Theta back: nbmf_predict_at, nbmf_predict_rows, nbmf_top_n, nbmf_score_rows,
// nbmf_theta_hist, nbmf_rank_rows, nbmf_theta_bits, nbmf_top_pairs
// (DESIGN.md 4.6).  Staging of one such call, from the pool: given back when the call returns, on every path, after the
// stream has drained (a pooled block may be handed to the next caller at once).
struct PredictStage {
  hipStream_t stream;
  std::vector<void*> blocks;
  template <typename T>
  hipError_t get(T** out, size_t bytes) {
    hipError_t e = dmalloc(out, bytes);
    if (e == hipSuccess) blocks.push_back((void*)*out);
    return e;
  }
  ~PredictStage() {
    if (blocks.empty()) return;
    (void)hipStreamSynchronize(stream);
    for (void* p : blocks) dfree(p);
  }
};

// The checks all six share, in the order the header gives them: factors, not data (so not ready()).
int predict_ready(nbmf_ctx* c) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (!c->have_factors) return fail(NBMF_ERR_STATE, "no factors on the device");
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "prediction runs on an unsharded context (nbmf_comm_detach first)");
  return NBMF_OK;
}

int check_rows(nbmf_ctx* c, int64_t row0, int64_t nrows) {   // the six row-slab entry points: all but nbmf_predict_at
  if (nrows < 0 || row0 < 0 || row0 > c->m || nrows > c->m - row0)
    return fail(NBMF_ERR_ARG, "rows [%lld, %lld + %lld) are not inside [0, %lld)", (long long)row0, (long long)row0, (long long)nrows,
                (long long)c->m);
  return NBMF_OK;
}

// rows x width bytes between a caller's rows and a staging panel: one flat copy where both sides are dense, else the 2D
// copy.  Only `width` bytes of a row are touched on either side, whatever its pitch: nothing of a caller's array beyond
// column n - 1 (slot top - 1) is read or written.
hipError_t copy_rows(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width, size_t rows, hipMemcpyKind kind,
                     hipStream_t stream) {
  if (dst_pitch == width && src_pitch == width) return hipMemcpyAsync(dst, src, rows * width, kind, stream);
  return hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width, rows, kind, stream);
}

// ---- bit-packed operands (NBMF_DATA_BITS / NBMF_MASK_BITS; nbmf_bits_kernels.inc) ---------------------------
inline long long packed_ld(long long n) { return (n + 7) / 8; }   // bytes of a packed row of n entries

// unpack_bits_kernel over rows x n entries, with the widest store that both the address of out_d and ldout are a multiple of.
hipError_t launch_unpack_bits(const unsigned char* bits_d, long long ldbits, long long rows, long long n, unsigned char* out_d,
                              long long ldout, hipStream_t stream) {
  if (rows <= 0 || n <= 0) return hipSuccess;
  const unsigned long long align = (unsigned long long)(uintptr_t)out_d | (unsigned long long)ldout;
  const int out_elt = align % 8 == 0 ? 8 : align % 4 == 0 ? 4 : 1;
  const long long spans = (n + out_elt - 1) / out_elt;
  dim3 grid((unsigned)((spans + UB_THREADS - 1) / UB_THREADS), (unsigned)std::min<long long>(rows, 65535));
  hipLaunchKernelGGL(unpack_bits_kernel, grid, dim3(UB_THREADS), 0, stream, bits_d, ldbits, rows, n, out_d, ldout, out_elt);
  return hipGetLastError();
}

// `rows` rows of a caller's operand into the staging panel dst (leading dimension ldp entries of elt bytes) -- what the
// upload and the four row-slab calls that take data do per chunk or panel.  An operand of elt bytes per entry (ld in
// entries) is copied (copy_rows).  A packed one (ld in bytes; elt is 1) goes up as it is into bits_d, a block of at least
// rows x packed_ld(n) bytes from the call's staging, and is unpacked into dst on the stream: the panel then holds the
// bytes the uint8 operand of the same values would have put there.
hipError_t stage_rows_as_bytes(unsigned char* bits_d, const void* src, bool packed, size_t elt, size_t ld, size_t n, size_t rows,
                               void* dst, size_t ldp, hipStream_t stream) {
  if (!packed) return copy_rows(dst, ldp * elt, src, ld * elt, n * elt, rows, hipMemcpyHostToDevice, stream);
  const size_t nb = (size_t)packed_ld((long long)n);
  hipError_t e = copy_rows(bits_d, nb, src, ld, nb, rows, hipMemcpyHostToDevice, stream);
  if (e != hipSuccess) return e;
  return launch_unpack_bits(bits_d, (long long)nb, (long long)rows, (long long)n, (unsigned char*)dst, (long long)ldp, stream);
}

// The leading-dimension rule of a row operand of a row-slab call, packed or not: NBMF_OK, or the error.
int check_row_ld(const char* what, int64_t ld, bool packed, int64_t n) {
  if (packed && ld < packed_ld(n))
    return fail(NBMF_ERR_ARG, "%s %lld is less than ceil(n / 8) = %lld", what, (long long)ld, (long long)packed_ld(n));
  if (!packed && ld < n) return fail(NBMF_ERR_ARG, "%s %lld is less than n = %lld", what, (long long)ld, (long long)n);
  return NBMF_OK;
}

// How a row-slab call walks its rows [row0, end), in panels that share one staging and end in a stream synchronise each:
//   for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) { pn = pl.rows_at(p0); ... }
// A panel is NBMF_PREDICT_PANEL_ROWS rows high, or else what 256 MiB of staging hold at row_bytes per panel row, rounded
// down to a multiple of 16 with a floor of 16.  With align16 the height is rounded up to 16 and the first panel is cut
// short by row0 % 16, so that every later panel starts on the absolute 16-row grid: a 16-row block of the product kernels
// never straddles two panels (nbmf_score_rows' column sums rely on it: DESIGN.md 4.8).
struct RowPanels {
  long long ldp;          // round_up(n, 4) (<= nA): a staged panel's leading dimension -- the kernels move 4 entries at a time
  long long col_groups;   // gridDim.y of a product kernel: PR_WAVES strips of PR_STRIP columns per workgroup
  long long row0, end, panel;
  bool align16;
  long long stage_rows() const { return std::min(panel, end - row0); }   // (no panel holds more rows than this)
  long long rows_at(long long p0) const { return std::min(align16 ? panel - p0 % 16 : panel, end - p0); }
  static long long blocks(long long p0, long long pn) { return (p0 + pn + 15) / 16 - p0 / 16; }
  dim3 grid(long long p0, long long pn) const { return dim3((unsigned)blocks(p0, pn), (unsigned)col_groups); }
};
inline long long panel_ld(const nbmf_ctx* c) { return round_up(c->n, 4); }

// The plan for a product whose right operand has n real columns on an image nA long (a multiple of PR_STRIP): Theta's
// (plan_row_panels) or the item-by-item product of nbmf_similarity / nbmf_neighbors, whose columns are the axis's items.
int plan_panels(const char* who, long long n, long long nA, int64_t row0, int64_t nrows, size_t row_bytes, bool align16,
                RowPanels* pl) {
  const long long col_groups = (nA + PR_WAVES * PR_STRIP - 1) / (PR_WAVES * PR_STRIP);
  if (col_groups > 65535) return fail(NBMF_ERR_ARG, "n = %lld is beyond what %s launches", n, who);
  const long long dflt = std::max<long long>(16, (long long)((256ull << 20) / row_bytes) / 16 * 16);
  const long long panel = std::max<long long>(1, env_int("NBMF_PREDICT_PANEL_ROWS", dflt));
  *pl = RowPanels{(long long)round_up(n, 4), col_groups, row0, row0 + nrows, align16 ? (long long)round_up(panel, 16) : panel, align16};
  return NBMF_OK;
}

int plan_row_panels(nbmf_ctx* c, const char* who, int64_t row0, int64_t nrows, size_t row_bytes, bool align16, RowPanels* pl) {
  return plan_panels(who, (long long)c->n, (long long)c->nA, row0, nrows, row_bytes, align16, pl);
}

// Rows [p0, p0 + pn) of the product of two natural-layout operand images -- left[k * leftA + i], right[k * rightA + j], the
// first c->k rows of each -- into the staging panel of leading dimension pl.ldp.  Theta is (c->Wn, c->mA, c->Hn, c->nA):
// what nbmf_predict_rows, nbmf_top_n and nbmf_rank_rows pass; nbmf_similarity / nbmf_neighbors pass the gathered queries
// and the prepared items.  leftA is a multiple of 16 that covers row p0 + pn - 1, rightA one of PR_STRIP.
hipError_t launch_theta_panel(nbmf_ctx* c, const RowPanels& pl, const double* left, long long leftA, const double* right,
                              long long rightA, long long p0, long long pn, int out_kind, int clip, double threshold, void* panel_d) {
  hipLaunchKernelGGL(out_kind == NBMF_PREDICT_U8 ? predict_rows_kernel<1> : predict_rows_kernel<0>, pl.grid(p0, pn),
                     dim3(PR_WAVES * 64), 0, c->stream, left, right, c->k, leftA, rightA, p0, pn, pl.ldp, clip != 0 ? 1 : 0, threshold,
                     panel_d);
  return hipGetLastError();
}

// The same rows of Theta scored against the staged data and mask panels (nbmf_score_rows).
hipError_t launch_score_panel(nbmf_ctx* c, const RowPanels& pl, long long p0, long long pn, int x_kind, int clip, double eps,
                              const void* x_d, const unsigned char* m_d, double* rpart_d, int* rcnt_d, double* cpart_d, int* ccnt_d) {
  hipLaunchKernelGGL(x_kind == NBMF_DATA_F64 ? score_rows_kernel<1> : score_rows_kernel<0>, pl.grid(p0, pn), dim3(PR_WAVES * 64), 0,
                     c->stream, (const double*)c->Wn, (const double*)c->Hn, c->k, (long long)c->mA, (long long)c->nA,
                     (long long)c->n, p0, pn, pl.ldp, clip != 0 ? 1 : 0, eps, x_d, m_d, rpart_d, rcnt_d, cpart_d, ccnt_d);
  return hipGetLastError();
}

// The same rows of Theta, clipped, counted by class and bin against the staged data and mask panels (nbmf_theta_hist).
hipError_t launch_hist_panel(nbmf_ctx* c, const RowPanels& pl, long long p0, long long pn, int bins, const unsigned char* x_d,
                             const unsigned char* m_d, int copies, unsigned long long* total_d) {
  const size_t lds = sizeof(unsigned int) * PR_WAVES * (2 * (size_t)bins + 2);   // a histogram per wave: <= 32 KiB + 32 bytes
  hipLaunchKernelGGL(theta_hist_kernel, pl.grid(p0, pn), dim3(PR_WAVES * 64), lds, c->stream, (const double*)c->Wn,
                     (const double*)c->Hn, c->k, (long long)c->mA, (long long)c->nA, (long long)c->n, p0, pn, pl.ldp, bins, x_d, m_d,
                     copies, total_d);
  return hipGetLastError();
}

// The same rows of Theta, clipped, summed by (row, column group) and by column against the staged data and mask panels
// (nbmf_moment_rows_v).  rtab_d (this panel's table, zeroed by the caller) or ctab_d may be null.
hipError_t launch_moment_panel(nbmf_ctx* c, const RowPanels& pl, long long p0, long long pn, int groups, const unsigned char* x_d,
                               const unsigned char* m_d, const int* grp_d, unsigned long long* rtab_d, int copies,
                               unsigned long long* ctab_d, unsigned long long* nan_d) {
  // a table of 16 rows x groups slots per wave: <= 32 KiB
  const size_t lds = rtab_d ? sizeof(unsigned long long) * PR_WAVES * 16 * (size_t)groups * MO_WORDS : 0;
  hipLaunchKernelGGL(moment_rows_kernel, pl.grid(p0, pn), dim3(PR_WAVES * 64), lds, c->stream, (const double*)c->Wn,
                     (const double*)c->Hn, c->k, (long long)c->mA, (long long)c->nA, (long long)c->n, p0, pn, pl.ldp, groups, x_d, m_d,
                     grp_d, rtab_d, copies, ctab_d, nan_d);
  return hipGetLastError();
}

}  // namespace

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------
extern "C" {

int nbmf_abi_version(void) { return 4; }   // 2: NBMF_PEER_HANDLE_BYTES 128 -> 192, nbmf_generate_slice, nbmf_set_storage; 3: nbmf_upload_v (uint8 / bool data), nbmf_selftest_mfma_peak, nbmf_engine_stats; 4: nbmf_source_hash, nbmf_comm_info, nbmf_cancel, nbmf_variant_stats, nbmf_device_bus_id; still 4 with nbmf_predict_at, nbmf_predict_rows, nbmf_top_n, nbmf_score_rows, nbmf_theta_hist, nbmf_rank_rows, nbmf_set_eval, nbmf_eval_loglik, nbmf_get_eval, nbmf_get_best_factors, the *_v forms and nbmf_selftest_unpack_bits, nbmf_theta_bits, nbmf_hold_out, nbmf_hold_out_undo, nbmf_get_eval_pairs, nbmf_top_pairs, nbmf_similarity, nbmf_neighbors: compatible additions, which a caller detects by the symbol
// The sources this binary was compiled from: first 12 hex digits of the SHA-256 over nbmf_hip.hip, the *.inc files (sorted
// by name) and include/nbmf_hip.h, put in by the Makefile (tools/src_hash.sh prints the same for the tree).  A profile or a
// bench line that quotes it can be tied to a commit; a library built by hand without the Makefile says "unstamped".
#ifndef NBMF_SRC_HASH
#define NBMF_SRC_HASH "unstamped"
#endif
const char* nbmf_source_hash(void) { return NBMF_SRC_HASH; }

const char* nbmf_last_error(void) { return g_err.c_str(); }

int nbmf_device_bus_id(int device, char* buf, int len) {
  if (!buf || len < 16) return fail(NBMF_ERR_ARG, "buffer of at least 16 bytes expected");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return fail(NBMF_ERR_HIP, "no HIP device %d", device);
  HIPCHK(hipDeviceGetPCIBusId(buf, len, device));
  return NBMF_OK;
}

int nbmf_device_count(int* count) {
  if (!count) return fail(NBMF_ERR_ARG, "count is NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(NBMF_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return NBMF_OK;
}

int nbmf_create(int64_t m, int64_t n, int k, int device, nbmf_ctx** out) {
  if (!out) return fail(NBMF_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (m < 1 || n < 1) return fail(NBMF_ERR_ARG, "m and n must be >= 1 (got %lld x %lld)", (long long)m, (long long)n);
  if (k < 1 || k > NBMF_MAX_K) return fail(NBMF_ERR_ARG, "n_components must be in [1, %d] (got %d)", NBMF_MAX_K, k);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev < 1)
    return fail(NBMF_ERR_HIP, "no HIP device available (%s): libnbmf_hip needs an MI355X (gfx950)",
                e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  if (device < 0 || device >= ndev) return fail(NBMF_ERR_ARG, "device %d out of range (have %d)", device, ndev);
  HIPCHK(hipSetDevice(device));
  DevInfo info;
  HIPCHK(device_info(device, &info));
  if (!info.gfx950) return fail(NBMF_ERR_HIP, "device %d is %s; this library is built for gfx950 only", device, info.arch);

  nbmf_ctx* c = new nbmf_ctx();
  c->cus = info.cus;
  struct CtxGuard {   // a failure below releases what has been allocated so far
    nbmf_ctx* p;
    ~CtxGuard() {
      if (p) nbmf_destroy(p);
    }
  } ctx_guard{c};
  c->device = device;
  c->m = m;
  c->n = n;
  c->k = k;
  c->mA = round_up(m, PAD);
  c->nA = round_up(n, PAD);
  c->KB = k <= 16 ? 1 : k <= 32 ? 2 : k <= 64 ? 4 : 8;
  c->KS = (k + SLICE_K - 1) / SLICE_K;
  c->KP = c->KS > 1 ? SLICE_K * c->KS : 16 * c->KB;
  if (c->KS > 1) HIPCHK(dmalloc(&c->theta, sizeof(double) * (size_t)c->mA * c->nA));
  HIPCHK(stream_acquire(device, &c->stream));
  HIPCHK(log_table_build(device, c->stream));   // (the general path's table: once per device, never in the launch path)

  const size_t fw = (size_t)c->KP * c->mA * sizeof(double), fh = (size_t)c->KP * c->nA * sizeof(double);
  HIPCHK(dmalloc(&c->Wn, fw));
  HIPCHK(dmalloc(&c->WT, fw + PASS_SLACK));   // (+ slack: the sweeps prefetch one stage past the end, see STAGE_DMA)
  HIPCHK(dmalloc(&c->WG, fw + PASS_SLACK));
  HIPCHK(dmalloc(&c->Hn, fh));
  HIPCHK(dmalloc(&c->HT, fh + PASS_SLACK));
  HIPCHK(dmalloc(&c->HG, fh + PASS_SLACK));
  // (the pass workspaces depend on the storage path: setup_workspaces, called by nbmf_upload)
  HIPCHK(dmalloc(&c->Pbuf, 2 * fh + 64));
  c->n_prior_blocks = (int)(((size_t)c->KP * c->nA + 255) / 256);
  HIPCHK(dmalloc(&c->prior, sizeof(double) * 2 * (size_t)c->n_prior_blocks));
  c->prior_src = c->prior;
  c->n_prior_src = c->n_prior_blocks;
  HIPCHK(dmalloc(&c->scal, sizeof(double) * 8));
  HIPCHK(dmalloc(&c->sbuf, sizeof(double) * 8));
  HIPCHK(dmalloc(&c->flags, sizeof(int) * 8));
  HIPCHK(dmalloc(&c->stats, sizeof(unsigned long long) * 8));
  HIPCHK(dmalloc(&c->rowcnt, sizeof(double) * (size_t)c->mA));
  HIPCHK(hipMemset(c->flags, 0, sizeof(int) * 8));
  HIPCHK(hipMemset(c->scal, 0, sizeof(double) * 8));
  c->stage_bytes = (fw > fh ? fw : fh);
  HIPCHK(dmalloc(&c->stage, c->stage_bytes));
  ctx_guard.p = nullptr;
  *out = c;
  return NBMF_OK;
}

int nbmf_destroy(nbmf_ctx* c) {
  if (!c) return NBMF_OK;
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  comm_release(c);
  if (c->host_buf) hipHostFree(c->host_buf);
  arena_release((ArenaSlot*)c->arena_slot.p);   // back to the pool, never to the allocator (see ArenaSlot)
  void* ptrs[] = {c->dataA, c->dataB, c->maskA, c->maskB, c->rowcnt, c->Wn, c->WT, c->WG, c->Hn, c->HT, c->HG,
                  c->slabH, c->slabW, c->Pbuf, c->lossbuf, c->lossfin, c->prior, c->scal, c->flags, c->losses_d, c->stage, c->stats,
                  c->sbuf, c->Qbuf, c->cstartH, c->cstartW, c->theta, c->small.slab, c->small_batch.slab, c->small_batch.table,
                  c->small_batch.io, c->bitsA, c->bitsB, c->eval.rows, c->eval.cols, c->eval.x, c->eval.Wk, c->eval.Hk,
                  c->eval.partials, c->eval.eval_ll_d, c->eval.bestW, c->eval.bestH};
  for (void* p : ptrs)
    if (p) dfree(p);
  for (hipEvent_t e : c->ev) hipEventDestroy(e);
  for (hipEvent_t e : {c->evH, c->evF, c->ev1})
    if (e) hipEventDestroy(e);
  if (c->stream2) {
    hipStreamSynchronize(c->stream2);
    hipStreamDestroy(c->stream2);
  }
  if (c->stream) stream_release(c->device, c->stream);   // (synchronised at the top of this function)
  delete c;
  return NBMF_OK;
}

int nbmf_set_hyper(nbmf_ctx* c, double alpha, double beta, double eps, int projection) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (projection != NBMF_PROJ_NORMALIZE && projection != NBMF_PROJ_DUCHI)
    return fail(NBMF_ERR_ARG, "unknown projection %d", projection);
  if (!(eps >= 2.2250738585072014e-308 && eps <= 1.7976931348623157e308))
    return fail(NBMF_ERR_ARG, "eps must be a positive normal number");
  c->alpha = alpha;
  c->beta = beta;
  c->eps = eps;
  c->projection = projection;
  return NBMF_OK;
}

int nbmf_upload(nbmf_ctx* c, const double* x, int64_t ldx, int transposed, const void* mask, int mask_kind,
                int64_t ldmask, int* out_flags) {
  return nbmf_upload_v(c, x, NBMF_DATA_F64, ldx, transposed, mask, mask_kind, ldmask, out_flags);
}

int nbmf_upload_v(nbmf_ctx* c, const void* xv, int x_kind, int64_t ldx, int transposed, const void* mask, int mask_kind,
                  int64_t ldmask, int* out_flags) {
  if (!c || !xv) return fail(NBMF_ERR_ARG, "null context or data");
  if (x_kind != NBMF_DATA_F64 && x_kind != NBMF_DATA_U8 && x_kind != NBMF_DATA_F32 && x_kind != NBMF_DATA_BITS)
    return fail(NBMF_ERR_ARG, "x_kind must be NBMF_DATA_F64, NBMF_DATA_U8, NBMF_DATA_F32 or NBMF_DATA_BITS");
  if (mask && (mask_kind < NBMF_MASK_NONE || mask_kind > NBMF_MASK_BITS)) return fail(NBMF_ERR_ARG, "unknown mask_kind %d", mask_kind);
  // A packed operand is unpacked on the device into the byte staging of the uint8 one: from there on it IS one
  const bool xbits = x_kind == NBMF_DATA_BITS, mbits = mask && mask_kind == NBMF_MASK_BITS;
  const size_t xsz = x_kind == NBMF_DATA_U8 || xbits ? 1 : (x_kind == NBMF_DATA_F32 ? 4 : 8);   // bytes per element of the staged rows
  const double* x = (const double*)xv;
  const unsigned char* xb = (const unsigned char*)xv;
  if (mask_kind != NBMF_MASK_NONE && !mask) return fail(NBMF_ERR_ARG, "mask_kind set but mask is NULL");
  if (!mask) mask_kind = NBMF_MASK_NONE;
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "upload before attaching a communicator");
  if (int rc = set_device(c)) return rc;
  const int64_t U = transposed ? c->n : c->m, V = transposed ? c->m : c->n;
  if (xbits && ldx < packed_ld(V))
    return fail(NBMF_ERR_ARG, "ldx %lld is less than ceil(n / 8) = %lld", (long long)ldx, (long long)packed_ld(V));
  if (mbits && ldmask < packed_ld(V))
    return fail(NBMF_ERR_ARG, "ldmask %lld is less than ceil(n / 8) = %lld", (long long)ldmask, (long long)packed_ld(V));
  if ((!xbits && ldx < V) || (mask && !mbits && ldmask < V)) return fail(NBMF_ERR_ARG, "leading dimension smaller than the row length");

  // cheap host-side guess of the storage path from a sample (the device pack verifies it exactly);
  // NBMF_FORCE_F64=1 keeps binary data on the 8-byte path (measurement only)
  bool guess_bin = c->storage == NBMF_STORAGE_AUTO && env_int("NBMF_FORCE_F64", 0) == 0;
  bool guess_mask_bin = true;   // a float64 mask holding only 0 and 1 is a binary mask
  {
    const int64_t rows = U < 8 ? U : 8;
    for (int64_t u = 0; u < rows && (guess_bin || guess_mask_bin); ++u) {
      const int64_t uu = (U - 1) * u / (rows > 1 ? rows - 1 : 1);
      for (int64_t v = 0; v < V && v < 4096; ++v) {
        const double xe = xbits ? 0.0   // (packed operands are binary by construction: not sampled)
                          : x_kind == NBMF_DATA_U8 ? (double)xb[uu * ldx + v]
                          : x_kind == NBMF_DATA_F32 ? (double)((const float*)xv)[uu * ldx + v] : x[uu * ldx + v];
        if (xe != 0.0 && xe != 1.0) guess_bin = false;
        if (mask_kind == NBMF_MASK_F64) {
          const double mk = ((const double*)mask)[uu * ldmask + v];
          if (mk != 0.0 && mk != 1.0) guess_mask_bin = false;
        }
      }
    }
    if (!guess_mask_bin) guess_bin = false;
  }

  // NBMF_UPLOAD_TRACE=1: where an upload's time goes, stage by stage (host clock, the stream drained at every mark)
  const bool up_trace = env_set("NBMF_UPLOAD_TRACE");
  auto up_t0 = std::chrono::steady_clock::now();
  double up_copy = 0, up_pack = 0;
  auto up_mark = [&](const char* what) {
    if (!up_trace) return;
    hipStreamSynchronize(c->stream);
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[nbmf upload] %-28s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(t - up_t0).count());
    up_t0 = t;
  };
  up_mark("host sample");
  const size_t tiles = (size_t)(c->mA / 16) * (c->nA / 16);
  // staging chunk: <= 256 MiB of raw rows and <= 32768 tile rows (grid.y limit of the pack launch)
  // (NBMF_UPLOAD_CHUNK_ROWS, a test hook, replaces the 256 MiB height: rounded up to a multiple of PAD, the grid limit stays)
  const int64_t chunk_rows_env = env_int<int64_t>("NBMF_UPLOAD_CHUNK_ROWS", 0);
  const int64_t chunk_rows_max = std::min<int64_t>(
      32768 * 16, chunk_rows_env > 0 ? round_up(std::min<int64_t>(chunk_rows_env, 32768 * 16), PAD)
                                     : std::max<int64_t>(PAD, ((int64_t)(256ll << 20) / (V * (int64_t)xsz)) / PAD * PAD));
  char* raw = nullptr;
  void* rawm = nullptr;
  struct StagingGuard {   // the raw staging buffers never outlive this call, whichever way it returns
    char*& a;
    void*& b;
    ~StagingGuard() {
      if (a) dfree(a);
      if (b) dfree(b);
    }
  } staging_guard{raw, rawm};
  const size_t msz = mask_kind == NBMF_MASK_F64 ? 8 : 1;
  const int64_t chunk_rows = std::min<int64_t>(round_up(U, PAD), chunk_rows_max);
  HIPCHK(dmalloc(&raw, (size_t)chunk_rows * V * xsz));
  if (mask) HIPCHK(dmalloc(&rawm, (size_t)chunk_rows * V * msz));
  PredictStage bit_stage{c->stream, {}};   // the packed rows of a chunk, as they came
  unsigned char *xbits_d = nullptr, *mbits_d = nullptr;
  if (xbits) HIPCHK(bit_stage.get(&xbits_d, (size_t)chunk_rows * packed_ld(V)));
  if (mbits) HIPCHK(bit_stage.get(&mbits_d, (size_t)chunk_rows * packed_ld(V)));

  up_mark("staging buffers");
  int rc = NBMF_OK;
  unsigned long long st[4] = {0, 0, 0, 0};
  // Storage paths, cheapest first: byte codes (binary data, binary or no mask); doubles with a binary (or no)
  // mask folded in as NaN; doubles plus weight tiles.  A path the sample suggested is dropped when the pack's
  // exact counts say otherwise, and the next one is packed.
  for (int kind : {DATA_BIN, DATA_F64, DATA_F64M}) {
    if (kind == DATA_BIN && !guess_bin) continue;
    if (kind == DATA_F64 && (!guess_mask_bin || c->storage == NBMF_STORAGE_F64_WEIGHTS)) continue;
    if (kind == DATA_F64M && mask_kind == NBMF_MASK_NONE && c->storage != NBMF_STORAGE_F64_WEIGHTS) continue;   // (no mask: all-ones weights)
    const bool binary = kind == DATA_BIN;
    for (void** p : {&c->dataA, &c->dataB, &c->maskA, &c->maskB}) {
      if (*p) dfree(*p);
      *p = nullptr;
    }
    c->data_kind = -1;
    c->eval.held_out = false;   // (new data: the list stays as a plain eval set)
    const size_t esz = binary ? 1 : 8;
    const size_t bytes = tiles * 256 * esz;
    HIPCHK(dmalloc(&c->dataA, bytes + PASS_SLACK));
    HIPCHK(dmalloc(&c->dataB, bytes + PASS_SLACK));
    // (the pack kernel writes every tile of the padded mA x nA grid, pad entries included)
    if (kind == DATA_F64M) {
      HIPCHK(dmalloc(&c->maskA, bytes + PASS_SLACK));   // (slack: the sweeps request the tile behind their last one)
      HIPCHK(dmalloc(&c->maskB, bytes + PASS_SLACK));
    }
    HIPCHK(hipMemsetAsync(c->stats, 0, sizeof(unsigned long long) * 8, c->stream));
    up_mark("image allocations");

    for (int64_t u0 = 0; u0 < round_up(U, PAD); u0 += chunk_rows) {
      const int64_t urows_pad = std::min<int64_t>(chunk_rows, round_up(U, PAD) - u0);
      const int64_t urows = std::max<int64_t>(0, std::min<int64_t>(U - u0, urows_pad));
      if (urows > 0) {
        if (xbits)
          HIPCHK(stage_rows_as_bytes(xbits_d, xb + (size_t)u0 * ldx, true, 1, (size_t)ldx, (size_t)V, (size_t)urows, raw, (size_t)V,
                                     c->stream));
        else
          HIPCHK(hipMemcpy2DAsync(raw, (size_t)V * xsz, xb + (size_t)u0 * ldx * xsz, (size_t)ldx * xsz, (size_t)V * xsz,
                                  (size_t)urows, hipMemcpyHostToDevice, c->stream));
        if (mbits)
          HIPCHK(stage_rows_as_bytes(mbits_d, (const char*)mask + (size_t)u0 * ldmask, true, 1, (size_t)ldmask, (size_t)V,
                                     (size_t)urows, rawm, (size_t)V, c->stream));
        else if (mask)
          HIPCHK(hipMemcpy2DAsync(rawm, (size_t)V * msz, (const char*)mask + (size_t)u0 * ldmask * msz,
                                  (size_t)ldmask * msz, (size_t)V * msz, (size_t)urows, hipMemcpyHostToDevice,
                                  c->stream));
      }
      if (up_trace) {
        hipStreamSynchronize(c->stream);
        const auto t = std::chrono::steady_clock::now();
        up_copy += std::chrono::duration<double, std::milli>(t - up_t0).count();
        up_t0 = t;
      }
      PackArgs a{};
      a.x = raw;
      a.x_kind = xbits ? NBMF_DATA_U8 : x_kind;
      a.mask = mask ? rawm : nullptr;
      a.mask_kind = mbits ? NBMF_MASK_U8 : mask_kind;
      a.ldx = V;
      a.ldmask = V;
      a.u0 = u0;
      a.urows = urows;
      a.U = U;
      a.V = V;
      a.transposed = transposed;
      a.binary = binary ? 1 : 0;
      a.fold_mask = kind == DATA_F64;
      a.dataA = c->dataA;
      a.dataB = c->dataB;
      a.maskA = c->maskA;
      a.maskB = c->maskB;
      a.RbA = c->mA / 16;
      a.RbB = c->nA / 16;
      a.stats = c->stats;
      const int64_t VA = transposed ? c->mA : c->nA;
      a.tile_rows = urows_pad / 16;
      dim3 grid((unsigned)(VA / 16 / 4), (unsigned)((a.tile_rows + PACK_TILE_ROWS - 1) / PACK_TILE_ROWS));
      hipLaunchKernelGGL(pack_kernel, grid, dim3(256), 0, c->stream, a);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));   // raw staging buffer is reused by the next chunk
      if (up_trace) {
        const auto t = std::chrono::steady_clock::now();
        up_pack += std::chrono::duration<double, std::milli>(t - up_t0).count();
        up_t0 = t;
      }
    }
    if (up_trace) fprintf(stderr, "[nbmf upload] host -> device copies %.3f ms, pack kernels %.3f ms\n", up_copy, up_pack);
    HIPCHK(hipMemcpy(st, c->stats, sizeof st, hipMemcpyDeviceToHost));
    if (st[1] != 0) {
      rc = fail(NBMF_ERR_RANGE, "X must be binary: %llu entries outside [0,1] or not finite", st[1]);
      break;
    }
    if (st[3] != 0) guess_mask_bin = false;   // exact now: weights that are not 0 or 1 need the weight tiles
    if (kind == DATA_BIN && (st[2] != 0 || st[3] != 0)) continue;   // sample guessed wrong: repack as doubles
    if (kind == DATA_F64 && st[3] != 0) continue;
    c->data_kind = kind;
    break;
  }
  if (rc != NBMF_OK) return rc;
  if (c->data_kind < 0) return fail(NBMF_ERR_STATE, "internal: pack did not settle on a storage path");
  up_mark("pack statistics");
  if (int rc2 = setup_workspaces(c)) return rc2;
  up_mark("workspaces + lane masks");
  c->n_obs = (mask_kind == NBMF_MASK_NONE) ? (double)c->m * (double)c->n : (double)st[0];
  if (int rc2 = mark_pad_rows_b(c)) return rc2;
  c->n_obs_global = c->n_obs;
  hipLaunchKernelGGL(rowcount_kernel, dim3((unsigned)((c->m + 255) / 256)), dim3(256), 0, c->stream, c->dataB, c->maskB,
                     c->data_kind, (long long)(c->nA / 16), (long long)c->m, (long long)c->n, c->rowcnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  up_mark("row counts");
  if (out_flags) *out_flags = (c->data_kind == DATA_BIN) ? NBMF_FLAG_BINARY_PATH : 0;
  return NBMF_OK;
}

int nbmf_generate_slice(nbmf_ctx* c, uint64_t seed, double density, double observed, int64_t row0, int64_t col0,
                        int64_t n_global) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (!(density >= 0.0 && density <= 1.0) || !(observed >= 0.0 && observed <= 1.0))
    return fail(NBMF_ERR_ARG, "density and observed must lie in [0, 1]");
  if (row0 < 0 || col0 < 0 || n_global < col0 + c->n)
    return fail(NBMF_ERR_ARG, "slice [%lld.., %lld..+%lld) does not fit a matrix %lld columns wide", (long long)row0, (long long)col0,
                (long long)c->n, (long long)n_global);
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "generate before attaching a communicator");
  if (int rc = set_device(c)) return rc;
  for (void** p : {&c->dataA, &c->dataB, &c->maskA, &c->maskB}) {
    if (*p) dfree(*p);
    *p = nullptr;
  }
  c->data_kind = -1;
  c->eval.held_out = false;   // (new data: the list stays as a plain eval set)
  const size_t tiles = (size_t)(c->mA / 16) * (c->nA / 16);
  HIPCHK(dmalloc(&c->dataA, tiles * 256 + PASS_SLACK));
  HIPCHK(dmalloc(&c->dataB, tiles * 256 + PASS_SLACK));
  HIPCHK(hipMemsetAsync(c->stats, 0, sizeof(unsigned long long) * 8, c->stream));
  const long long RbA = c->mA / 16;
  dim3 grid((unsigned)(c->nA / 16 / 4), (unsigned)std::min<long long>(RbA, 65535), (unsigned)((RbA + 65534) / 65535));
  hipLaunchKernelGGL(synth_kernel, grid, dim3(256), 0, c->stream, (uint32_t*)c->dataA, (uint32_t*)c->dataB,
                     RbA, (long long)(c->nA / 16), (long long)c->m, (long long)c->n,
                     SynthSlice{(long long)row0, (long long)col0, (long long)n_global}, (unsigned long long)seed, density, observed,
                     c->stats);
  HIPCHK(hipGetLastError());
  unsigned long long st[1] = {0};
  HIPCHK(hipMemcpyAsync(st, c->stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->data_kind = DATA_BIN;
  if (int rc2 = setup_workspaces(c)) return rc2;
  c->n_obs = (double)st[0];
  if (int rc2 = mark_pad_rows_b(c)) return rc2;
  c->n_obs_global = c->n_obs;
  hipLaunchKernelGGL(rowcount_kernel, dim3((unsigned)((c->m + 255) / 256)), dim3(256), 0, c->stream, c->dataB, c->maskB,
                     c->data_kind, (long long)(c->nA / 16), (long long)c->m, (long long)c->n, c->rowcnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBMF_OK;
}

int nbmf_generate(nbmf_ctx* c, uint64_t seed, double density, double observed) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  return nbmf_generate_slice(c, seed, density, observed, 0, 0, c->n);
}

int nbmf_set_storage(nbmf_ctx* c, int storage) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (storage < NBMF_STORAGE_AUTO || storage > NBMF_STORAGE_F64_WEIGHTS) return fail(NBMF_ERR_ARG, "unknown storage path %d", storage);
  c->storage = storage;
  return NBMF_OK;
}

int nbmf_upload_csr(nbmf_ctx* c, const int64_t* indptr, const int32_t* indices, int64_t nnz, int transposed,
                    const int64_t* mask_indptr, const int32_t* mask_indices, int64_t mask_nnz, int* out_flags) {
  if (!c || !indptr || (nnz > 0 && !indices)) return fail(NBMF_ERR_ARG, "null context or CSR arrays");
  if (nnz < 0 || mask_nnz < 0) return fail(NBMF_ERR_ARG, "negative entry count");
  const bool masked = mask_indptr != nullptr;
  if (masked && mask_nnz > 0 && !mask_indices) return fail(NBMF_ERR_ARG, "mask_indptr without mask_indices");
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "upload before attaching a communicator");
  if (int rc = set_device(c)) return rc;
  const int64_t U = transposed ? c->n : c->m, V = transposed ? c->m : c->n;   // the user's matrix is U x V
  if (indptr[0] != 0 || indptr[U] != nnz) return fail(NBMF_ERR_ARG, "indptr does not span the %lld stored entries", (long long)nnz);
  if (masked && (mask_indptr[0] != 0 || mask_indptr[U] != mask_nnz)) return fail(NBMF_ERR_ARG, "mask indptr does not span its entries");
  for (void** p : {&c->dataA, &c->dataB, &c->maskA, &c->maskB}) {
    if (*p) dfree(*p);
    *p = nullptr;
  }
  c->data_kind = -1;
  c->eval.held_out = false;   // (new data: the list stays as a plain eval set)
  const long long RbA = c->mA / 16, RbB = c->nA / 16;
  const size_t tiles = (size_t)RbA * RbB;
  HIPCHK(dmalloc(&c->dataA, tiles * 256 + PASS_SLACK));
  HIPCHK(dmalloc(&c->dataB, tiles * 256 + PASS_SLACK));
  HIPCHK(hipMemsetAsync(c->stats, 0, sizeof(unsigned long long) * 8, c->stream));
  const long long dwords = (long long)tiles * 64;
  hipLaunchKernelGGL(csr_fill_kernel, dim3((unsigned)((dwords + 255) / 256)), dim3(256), 0, c->stream, (uint32_t*)c->dataA,
                     (uint32_t*)c->dataB, RbA, RbB, (long long)c->m, (long long)c->n,
                     masked ? (unsigned)CB_VALID : (unsigned)(CB_VALID | CB_ZOBS));
  HIPCHK(hipGetLastError());
  // the two patterns, staged through the device in pieces of at most 64 M entries
  struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
      if (p) dfree(p);
    }
  } d_ptr, d_idx;
  HIPCHK(dmalloc(&d_ptr.p, sizeof(int64_t) * (size_t)(U + 1)));
  const int64_t piece = std::max<int64_t>(1, env_int<int64_t>("NBMF_CSR_PIECE", 64ll << 20));   // (tests: force several pieces)
  HIPCHK(dmalloc(&d_idx.p, sizeof(int32_t) * (size_t)std::max<int64_t>(1, std::min<int64_t>(piece, std::max(nnz, mask_nnz)))));
  for (int what = masked ? 0 : 1; what <= 1; ++what) {
    const int64_t* ip = what == 0 ? mask_indptr : indptr;
    const int32_t* ix = what == 0 ? mask_indices : indices;
    const int64_t cnt = what == 0 ? mask_nnz : nnz;
    HIPCHK(hipMemcpyAsync(d_ptr.p, ip, sizeof(int64_t) * (size_t)(U + 1), hipMemcpyHostToDevice, c->stream));
    for (int64_t e0 = 0; e0 < cnt; e0 += piece) {
      const int64_t ne = std::min(piece, cnt - e0);
      HIPCHK(hipMemcpyAsync(d_idx.p, ix + e0, sizeof(int32_t) * (size_t)ne, hipMemcpyHostToDevice, c->stream));
      // the kernel indexes entries from e0: shift the view of indices, keep indptr absolute
      hipLaunchKernelGGL(csr_scatter_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, c->stream,
                         (const long long*)d_ptr.p, (const int*)d_idx.p - e0, (long long)U, (long long)V, (long long)e0,
                         (long long)(e0 + ne), transposed, what, (unsigned char*)c->dataA, (unsigned char*)c->dataB, RbA, RbB, c->stats);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));   // the staging buffer is reused by the next piece
    }
  }
  if (masked) {
    hipLaunchKernelGGL(count_observed_kernel, dim3(1024), dim3(256), 0, c->stream, (const uint32_t*)c->dataA, dwords, c->stats);
    HIPCHK(hipGetLastError());
  }
  unsigned long long st[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(st, c->stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (st[1] != 0) return fail(NBMF_ERR_ARG, "%llu column indices outside [0, %lld)", st[1], (long long)V);
  c->data_kind = DATA_BIN;
  if (int rc2 = setup_workspaces(c)) return rc2;
  c->n_obs = masked ? (double)st[0] : (double)c->m * (double)c->n;
  if (int rc2 = mark_pad_rows_b(c)) return rc2;
  c->n_obs_global = c->n_obs;
  hipLaunchKernelGGL(rowcount_kernel, dim3((unsigned)((c->m + 255) / 256)), dim3(256), 0, c->stream, c->dataB, c->maskB,
                     c->data_kind, (long long)(c->nA / 16), (long long)c->m, (long long)c->n, c->rowcnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  if (out_flags) *out_flags = NBMF_FLAG_BINARY_PATH;
  return NBMF_OK;
}

int nbmf_get_n_obs(nbmf_ctx* c, double* n_obs) {
  if (!c || !n_obs) return fail(NBMF_ERR_ARG, "null argument");
  if (c->data_kind < 0) return fail(NBMF_ERR_STATE, "nbmf_upload has not been called");
  *n_obs = c->n_obs;
  return NBMF_OK;
}

// Are the factors on the device where a fit keeps them (tiny_a)?  flags[5] collects the violations; synchronises.
int check_factor_range(nbmf_ctx* c) {
  HIPCHK(hipMemsetAsync(c->flags + 5, 0, sizeof(int), c->stream));
  const long long tot = std::max((long long)c->mA, (long long)c->KP * c->nA);
  hipLaunchKernelGGL(factor_range_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, (const double*)c->Wn,
                     (const double*)c->Hn, c->k, (long long)c->m, (long long)c->mA, (long long)c->n, (long long)c->nA, c->flags + 5);
  HIPCHK(hipGetLastError());
  int out_of_range = 1;
  HIPCHK(hipMemcpyAsync(&out_of_range, c->flags + 5, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->factors_in_range = out_of_range == 0;
  return NBMF_OK;
}

int nbmf_set_factors(nbmf_ctx* c, const double* W, const double* H) {
  if (!c || !W || !H) return fail(NBMF_ERR_ARG, "null argument");
  if (int rc = set_device(c)) return rc;
  HIPCHK(hipMemcpyAsync(c->stage, W, sizeof(double) * (size_t)c->k * c->m, hipMemcpyHostToDevice, c->stream));
  launch_set_factor(c, /*h=*/false, c->stage, c->Wn, c->WT, c->WG);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpyAsync(c->stage, H, sizeof(double) * (size_t)c->k * c->n, hipMemcpyHostToDevice, c->stream));
  launch_set_factor(c, /*h=*/true, c->stage, c->Hn, c->HT, c->HG);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(prior_kernel, dim3(c->n_prior_blocks), dim3(256), 0, c->stream, c->Hn, c->prior, c->k, c->KP,
                     (long long)c->n, (long long)c->nA, c->eps);
  HIPCHK(hipGetLastError());
  if (int rc = check_factor_range(c)) return rc;
  c->prior_src = c->prior;
  c->n_prior_src = c->n_prior_blocks;
  c->have_factors = true;
  return NBMF_OK;
}

int nbmf_get_factors(nbmf_ctx* c, double* W, double* H) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (!c->have_factors) return fail(NBMF_ERR_STATE, "no factors on the device");
  if (int rc = set_device(c)) return rc;
  for (const bool h : {false, true}) {
    double* out = h ? H : W;
    if (!out) continue;
    launch_get_factor(c, h, h ? c->Hn : c->Wn, c->stage);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->stage, sizeof(double) * (size_t)c->k * (h ? c->n : c->m), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return NBMF_OK;
}

int nbmf_run(nbmf_ctx* c, int max_iter, double tol, double* losses, int* n_iter) {
  if (int rc = ready(c)) return rc;
  if (max_iter < 1) return fail(NBMF_ERR_ARG, "max_iter must be >= 1");
  if (!losses || !n_iter) return fail(NBMF_ERR_ARG, "null output");
  if (c->cancelled.load(std::memory_order_relaxed)) return fail(NBMF_ERR_STATE, "cancelled (nbmf_cancel)");
  if (int rc = set_device(c)) return rc;
  if (int rc = ensure_losses(c, max_iter)) return rc;
  HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->scal, 0, sizeof(double) * 8, c->stream));
  // An eval set (nbmf_set_eval) is evaluated between iterations by launches of its own: such a run is served by the
  // launch engine below, in batches of `every` iterations, and never replayed from a graph.
  auto& ev = c->eval;
  const bool evaling = ev.count > 0;
  ev.iters.clear();
  ev.logliks.clear();
  ev.best_iter = 0;
  ev.stopped_early = 0;
  ev.have_best = false;
  if (evaling)
    if (int rc = ensure_eval_slots(c, 3 + max_iter / ev.every)) return rc;
  if (!evaling) {
    bool handled = false;   // small problems: the whole run in one persistent launch
    if (int rc = run_small(c, max_iter, tol, losses, n_iter, &handled)) return rc;
    if (handled) return NBMF_OK;
  }
  g_engine_launches_served.fetch_add(1, std::memory_order_relaxed);

  // Timeline (N3 of SURVEY Appendix A): the H-pass of iteration t also yields the log-likelihood of
  // the factors after iteration t-1, so loss(t-1) and its stop test are settled before H-update(t).
  const bool progress = c->progress && c->progress_every > 0;
  const int batch = progress ? c->progress_every : (tol > 0.0) ? 8 : max_iter;
  int reported = 0;   // losses already handed to the progress callback
  std::vector<double> fresh;
  auto report = [&](int n_final) -> int {
    if (!progress || n_final <= reported) return NBMF_OK;
    fresh.resize((size_t)(n_final - reported));
    HIPCHK(hipMemcpy(fresh.data(), c->losses_d + reported, sizeof(double) * fresh.size(), hipMemcpyDeviceToHost));
    c->progress(c->progress_user, reported, n_final - reported, fresh.data());
    reported = n_final;
    return NBMF_OK;
  };
  int host_done = 0;
  int it = 0;
  // One iteration = five launches with identical arguments every time (the loss index is counted on the
  // device), so on a single GPU it can be captured once into a hipGraph and replayed.  Measured: no gain
  // (config 1, 100x500 K=6: 14.7k it/s replayed vs 16.5k it/s eager) -- tiny problems are bound by the
  // latency of the five dependent kernels, not by the host's launch rate -- so it is opt-in
  // (NBMF_USE_GRAPH=1), never used with a communicator or event timing.
  const bool use_graph = env_set("NBMF_USE_GRAPH") && !is_sharded(c) && !c->timing && !progress && max_iter >= 8 && !evaling;
  int limit = max_iter;     // the iterations this run makes at most: max_iter, or the evaluation the patience rule ended it at
  int since_best = 0;       // consecutive evaluations on a multiple of `every` that did not improve
  double ev_val = 0.0, ev_best = 0.0;
  bool fused_fin = fin_fusable(c) && !use_graph;
  int recoveries = 0;
  int fl[8];
  // The host's look at the run: the flags read back (the stream drained), the timing, the peer check.  A sweep whose loss
  // assembly ran out of time (PassFin: the chip is shared and this sweep's other workgroups were held back for seconds) has
  // assembled nothing, raised the stop flag -- every later kernel has returned at once, the factors are those that sweep
  // read -- and told the host (flags[6]).  `done` losses are in place (flags[1]): the run resumes (*resume) at iteration
  // done + 1, whose H sweep is the one that failed, with the loss and stop test in a launch of their own from here on (bit
  // for bit the fused form's losses: tested).  Slots that filled late are emptied first.  At most 4 recoveries, and at the
  // end of the run none once it has been cancelled.
  auto settle = [&](bool at_end, bool* resume) -> int {
    *resume = false;
    HIPCHK(hipMemcpyAsync(fl, c->flags, sizeof fl, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->timing) timing_collect(c);
    if (int rc = peer_check(c)) return rc;
    if (!fl[6] || !fused_fin || recoveries >= 4 || (at_end && c->cancelled.load(std::memory_order_relaxed))) return NBMF_OK;
    ++recoveries;
    g_loss_assembly_recoveries.fetch_add(1, std::memory_order_relaxed);
    if (env_set("NBMF_DEBUG")) fprintf(stderr, "[nbmf] loss %d could not be assembled inside its sweep within the bound: resuming with separate launches\n", fl[1]);
    fused_fin = false;
    if (int rc = fill_ll_empty(c)) return rc;
    HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(c->flags + 6, 0, sizeof(int), c->stream));
    it = fl[1] + 1;
    host_done = 0;
    *resume = true;
    return NBMF_OK;
  };
  hipGraph_t graph = nullptr;
  hipGraphExec_t gexec = nullptr;
  if (use_graph) {
    HIPCHK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    int rc = enqueue_a_sweep(c, /*with_products=*/true);
    if (!rc) rc = enqueue_finalize(c, -1, tol);
    if (!rc) rc = enqueue_h_update(c);
    if (!rc) rc = enqueue_w_step(c, c->projection);
    hipError_t e = hipStreamEndCapture(c->stream, &graph);
    if (rc) return rc;
    if (e != hipSuccess) return fail(NBMF_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
    HIPCHK(hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0));
  }
  struct GraphGuard {
    hipGraph_t g;
    hipGraphExec_t x;
    ~GraphGuard() {
      if (x) hipGraphExecDestroy(x);
      if (g) hipGraphDestroy(g);
    }
  } guard{graph, gexec};
  for (;;) {
    if (it < limit && !host_done) {
      // the next batch of iterations; behind it (stop rule, progress reports) a look at the flags.  With an eval set a
      // batch ends on the next multiple of `every` (also after a rewind has left `it` between two)
      const int end = evaling ? (int)std::min<long long>(limit, ((long long)it / ev.every + 1) * ev.every) : std::min(max_iter, it + batch);
      for (; it < end; ++it) {
        if (c->cancelled.load(std::memory_order_relaxed)) return fail(NBMF_ERR_STATE, "cancelled (nbmf_cancel)");
        c->timing_it = it;
        if (use_graph) {
          HIPCHK(hipGraphLaunch(gexec, c->stream));
          continue;
        }
        if (is_sharded(c) && c->shard_axis == 0) {
          if (int rc = enqueue_iteration_rows(c, it, tol)) return rc;
          continue;
        }
        if (fused_fin) {
          if (int rc = enqueue_a_sweep(c, true, 0, 0, it - 1, tol)) return rc;   // (with the loss and stop test of iteration it-1)
        } else {
          if (int rc = enqueue_a_sweep(c, /*with_products=*/true)) return rc;
          if (it > 0)
            if (int rc = enqueue_finalize(c, it - 1, tol)) return rc;
        }
        if (int rc = enqueue_h_update(c)) return rc;
        if (int rc = enqueue_w_step(c, c->projection)) return rc;
      }
      if (evaling) {
        // The factors have had `it` iterations -- or, where the tol rule has ended the run inside this batch, n_iter of
        // them: every later kernel has returned at once -- and the evaluation enqueued here sees exactly those.  The host
        // looks at it at once: recorded under its label (a label already recorded is the same factors again: dropped),
        // the snapshot taken if it improves, the patience rule applied.  A batch that settle() rewinds is made again,
        // and its evaluation with it.
        const int slot = 1 + (int)ev.iters.size();
        if (int rc = enqueue_eval(c, slot)) return rc;
        HIPCHK(hipMemcpyAsync(&ev_val, ev.eval_ll_d + slot, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        bool resume = false;
        if (int rc = settle(/*at_end=*/false, &resume)) return rc;
        if (!resume) {
          host_done = fl[0];
          if (int rc = report(fl[1])) return rc;
          const int label = host_done ? fl[1] : it;
          if (label >= 1 && (ev.iters.empty() || label != ev.iters.back())) {
            const bool improves = ev.iters.empty() || ev_val > ev_best;
            ev.iters.push_back(label);
            ev.logliks.push_back(ev_val);
            if (improves) {   // (the stream is drained and nothing is enqueued behind the evaluation: what it saw)
              HIPCHK(hipMemcpyAsync(ev.bestW, c->Wn, sizeof(double) * (size_t)c->KP * c->mA, hipMemcpyDeviceToDevice, c->stream));
              HIPCHK(hipMemcpyAsync(ev.bestH, c->Hn, sizeof(double) * (size_t)c->KP * c->nA, hipMemcpyDeviceToDevice, c->stream));
              HIPCHK(hipStreamSynchronize(c->stream));
              ev_best = ev_val;
              ev.best_iter = label;
              ev.have_best = true;
              since_best = 0;
            } else if (label % ev.every == 0) {
              ++since_best;
            }
            if (ev.patience > 0 && since_best >= ev.patience && !host_done) {
              limit = it;   // the run ends here as one with max_iter = it would: the last loss from the Theta-only sweep
              ev.stopped_early = 1;
            }
          }
        }
      } else if ((tol > 0.0 || progress) && it < max_iter) {
        bool resume = false;
        if (int rc = settle(/*at_end=*/false, &resume)) return rc;
        if (!resume) {
          host_done = fl[0];
          if (int rc = report(fl[1])) return rc;
        }
      }
      continue;
    }
    if (!host_done) {
      // loss of the last iteration (Theta-only sweep)
      if (fused_fin) {
        if (int rc = enqueue_a_sweep(c, false, 0, 0, limit - 1, tol)) return rc;
      } else {
        if (int rc = enqueue_a_sweep(c, /*with_products=*/false)) return rc;
        if (int rc = enqueue_finalize(c, use_graph ? -1 : limit - 1, tol)) return rc;
      }
    }
    bool resume = false;
    if (int rc = settle(/*at_end=*/true, &resume)) return rc;
    if (resume) continue;   // the iterations from the one whose sweep failed on (or, behind the last one, only the last loss)
    if (fl[6]) {   // the loss assembly inside a sweep gave up waiting for a partial (PassFin), and may not be retried
      if (int rc = fill_ll_empty(c)) return rc;
      HIPCHK(hipStreamSynchronize(c->stream));
      return fail(NBMF_ERR_STATE, "internal: a sweep's loss assembly timed out waiting for its workgroups' partials");
    }
    if (c->cancelled.load(std::memory_order_relaxed)) return fail(NBMF_ERR_STATE, "cancelled (nbmf_cancel)");
    const int nit = fl[1];
    if (nit < 1 || nit > limit) return fail(NBMF_ERR_STATE, "internal: device reported n_iter=%d", nit);
    if (evaling && (ev.iters.empty() || ev.iters.back() != nit))
      return fail(NBMF_ERR_STATE, "internal: the last evaluation is labelled %d, n_iter=%d", ev.iters.empty() ? 0 : ev.iters.back(), nit);
    if (int rc = report(nit)) return rc;
    HIPCHK(hipMemcpy(losses, c->losses_d, sizeof(double) * (size_t)nit, hipMemcpyDeviceToHost));
    *n_iter = nit;
    return NBMF_OK;
  }
}

int nbmf_run_batch(nbmf_ctx* c, int n_problems, const double* alpha, const double* beta, const double* W0, const double* H0,
                   int max_iter, double tol, double* losses, int* n_iter, double* W_out, double* H_out) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (c->data_kind < 0) return fail(NBMF_ERR_STATE, "nbmf_upload has not been called");
  if (n_problems < 1) return fail(NBMF_ERR_ARG, "n_problems must be >= 1");
  if (max_iter < 1) return fail(NBMF_ERR_ARG, "max_iter must be >= 1");
  if (!alpha || !beta || !W0 || !H0 || !losses || !n_iter || !W_out || !H_out) return fail(NBMF_ERR_ARG, "null argument");
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "nbmf_run_batch runs on an unsharded context (nbmf_comm_detach first)");
  if (c->eval.count > 0) return fail(NBMF_ERR_STATE, "nbmf_run_batch does not evaluate an eval set (nbmf_set_eval with count 0 first)");
  if (int rc = set_device(c)) return rc;
  {
    bool handled = false;
    if (int rc = run_small_batch(c, n_problems, alpha, beta, W0, H0, max_iter, tol, losses, n_iter, W_out, H_out, &handled)) return rc;
    if (handled) return NBMF_OK;
  }
  // problems too large for the persistent kernel (or a run that gave up): one after the other, each exactly the
  // nbmf_set_hyper / nbmf_set_factors / nbmf_run / nbmf_get_factors sequence
  const double a0 = c->alpha, b0 = c->beta;
  const size_t wsz = (size_t)c->k * c->m, hsz = (size_t)c->k * c->n;
  int rc = NBMF_OK;
  for (int p = 0; p < n_problems && rc == NBMF_OK; ++p) {
    c->alpha = alpha[p];
    c->beta = beta[p];
    rc = nbmf_set_factors(c, W0 + (size_t)p * wsz, H0 + (size_t)p * hsz);
    if (rc == NBMF_OK) rc = nbmf_run(c, max_iter, tol, losses + (size_t)p * max_iter, n_iter + p);
    if (rc == NBMF_OK) rc = nbmf_get_factors(c, W_out + (size_t)p * wsz, H_out + (size_t)p * hsz);
  }
  c->alpha = a0;
  c->beta = b0;
  return rc;
}

int nbmf_batch_stats(nbmf_ctx* c, int* launches, int* problems) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (launches) *launches = c->small_batch.launches;
  if (problems) *problems = c->small_batch.problems;
  return NBMF_OK;
}

int nbmf_sweep_info(nbmf_ctx* c, int* h_chunks, int* h_blocks, int* w_chunks, int* w_blocks) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (!c->cstartH) return fail(NBMF_ERR_STATE, "no data on the device yet");
  if (h_chunks) *h_chunks = c->chunksH;
  if (h_blocks) *h_blocks = c->CH_H;
  if (w_chunks) *w_chunks = c->chunksW;
  if (w_blocks) *w_blocks = c->CH_W;
  return NBMF_OK;
}

int nbmf_variant_stats(long long* full_w_launches, long long* ragged_k_launches, long long* loss_assembly_recoveries) {
  if (full_w_launches) *full_w_launches = g_full_w_launches.load(std::memory_order_relaxed);
  if (ragged_k_launches) *ragged_k_launches = g_ragged_launches.load(std::memory_order_relaxed);
  if (loss_assembly_recoveries) *loss_assembly_recoveries = g_loss_assembly_recoveries.load(std::memory_order_relaxed);
  return NBMF_OK;
}

int nbmf_w_only_steps(nbmf_ctx* c, int n_steps) {
  if (int rc = ready(c)) return rc;
  if (n_steps < 0) return fail(NBMF_ERR_ARG, "n_steps must be >= 0");
  if (int rc = set_device(c)) return rc;
  HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 8, c->stream));
  struct FreeW {
    nbmf_ctx* c;
    ~FreeW() { c->w_free = false; }
  } free_w{c};
  c->w_free = true;   // (W starts off the simplex, _base.py:175: Theta above 1 is possible)
  for (int s = 0; s < n_steps; ++s) {
    if (int rc = enqueue_w_step(c, NBMF_PROJ_NORMALIZE)) return rc;
    if (s == 0 && n_steps > 2) {
      // ... and is on it from the first step on: looked at once (a ~20 us kernel and a synchronisation), so that the
      // remaining steps can take the sweeps' plain variant if W has come out non-negative as well
      if (int rc = check_factor_range(c)) return rc;
      c->w_free = !c->factors_in_range;
    }
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->timing) timing_collect(c);
  return peer_check(c);
}

int nbmf_loss(nbmf_ctx* c, double* loss) {
  if (int rc = ready(c)) return rc;
  if (!loss) return fail(NBMF_ERR_ARG, "null output");
  return loss_by_launches(c, loss);
}
int nbmf_loglik(nbmf_ctx* c, int clip_theta, double* loglik) {
  if (int rc = ready(c)) return rc;
  if (!loglik) return fail(NBMF_ERR_ARG, "null output");
  return one_shot(c, /*with_prior=*/false, /*strict=*/0, clip_theta != 0, /*collect_timing=*/true, loglik);
}

int nbmf_loglik_strict(nbmf_ctx* c, double* loglik) {
  if (int rc = ready(c)) return rc;
  if (!loglik) return fail(NBMF_ERR_ARG, "null output");
  return one_shot(c, /*with_prior=*/false, /*strict=*/1, /*clip=*/0, /*collect_timing=*/false, loglik);
}

// ---- Theta handed back: index pairs and row slabs (nbmf_predict_kernels.inc) ----------------------------
int nbmf_predict_at(nbmf_ctx* c, const int64_t* rows, const int64_t* cols, int64_t count, int clip_theta, double* out) {
  if (int rc = predict_ready(c)) return rc;
  if (count < 0) return fail(NBMF_ERR_ARG, "count must be >= 0 (got %lld)", (long long)count);
  if (count == 0) return NBMF_OK;
  if (!rows || !cols || !out) return fail(NBMF_ERR_ARG, "null argument");
  if (int rc = set_device(c)) return rc;
  const long long chunk = std::min<long long>(count, std::max<long long>(1, env_int("NBMF_PREDICT_PAIRS", 1LL << 22)));
  const size_t K = (size_t)c->k;
  PredictStage st{c->stream, {}};
  double *Wk = nullptr, *Hk = nullptr, *out_d = nullptr;
  long long *rows_d = nullptr, *cols_d = nullptr;
  unsigned long long* bad_d = nullptr;
  HIPCHK(st.get(&Wk, sizeof(double) * K * (size_t)c->m));
  HIPCHK(st.get(&Hk, sizeof(double) * K * (size_t)c->n));
  HIPCHK(st.get(&rows_d, sizeof(long long) * (size_t)chunk));
  HIPCHK(st.get(&cols_d, sizeof(long long) * (size_t)chunk));
  HIPCHK(st.get(&out_d, sizeof(double) * (size_t)chunk));
  HIPCHK(st.get(&bad_d, sizeof(unsigned long long)));
  for (const bool h : {false, true}) {   // the k-major copies of the two factors, once per call
    const long long len = h ? c->n : c->m, lenA = h ? c->nA : c->mA;
    hipLaunchKernelGGL(k_major_kernel, dim3((unsigned)((len + PT_TILE - 1) / PT_TILE), (unsigned)((c->k + PT_TILE - 1) / PT_TILE)),
                       dim3(PT_TILE * 8), 0, c->stream, (const double*)(h ? c->Hn : c->Wn), h ? Hk : Wk, c->k, len, lenA);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemsetAsync(bad_d, 0xff, sizeof(unsigned long long), c->stream));
  for (long long base = 0; base < count; base += chunk) {
    const long long cnt = std::min(chunk, (long long)count - base);
    HIPCHK(hipMemcpyAsync(rows_d, rows + base, sizeof(long long) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(cols_d, cols + base, sizeof(long long) * (size_t)cnt, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(predict_at_kernel, dim3((unsigned)((cnt * PA_LANES + 255) / 256)), dim3(256), 0, c->stream, (const double*)Wk,
                       (const double*)Hk, c->k, (long long)c->m, (long long)c->n, (const long long*)rows_d, (const long long*)cols_d, cnt,
                       base, clip_theta != 0 ? 1 : 0, bad_d, out_d);
    HIPCHK(hipGetLastError());
    unsigned long long bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, bad_d, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad != ~0ull)   // (chunks run in ascending order: the first chunk that reports holds the lowest position of all)
      return fail(NBMF_ERR_ARG, "index pair at position %llu is outside [0, %lld) x [0, %lld)", bad, (long long)c->m,
                  (long long)c->n);
    HIPCHK(hipMemcpyAsync(out + base, out_d, sizeof(double) * (size_t)cnt, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return NBMF_OK;
}

// ---- held-out pairs resident on the device, their log-likelihood sum (nbmf_eval_kernels.inc) ------------
int nbmf_set_eval(nbmf_ctx* c, const int64_t* rows, const int64_t* cols, const uint8_t* x, int64_t count, int every, int patience) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (count < 0) return fail(NBMF_ERR_ARG, "count must be >= 0 (got %lld)", (long long)count);
  if (every < 1) return fail(NBMF_ERR_ARG, "every must be >= 1 (got %d)", every);
  if (patience < 0) return fail(NBMF_ERR_ARG, "patience must be >= 0 (got %d)", patience);
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "held-out evaluation runs on an unsharded context (nbmf_comm_detach first)");
  if (c->eval.held_out)
    return fail(NBMF_ERR_STATE, "the eval set is a hold-out in place, the only record of the entries it cleared: nbmf_hold_out_undo first");
  if (int rc = set_device(c)) return rc;
  auto& ev = c->eval;
  if (count == 0) {
    HIPCHK(hipStreamSynchronize(c->stream));
    eval_release(c);
    return NBMF_OK;
  }
  if (!rows || !cols || !x) return fail(NBMF_ERR_ARG, "null argument");
  if (c->m > 0x7fffffffLL || c->n > 0x7fffffffLL || count > (1LL << 35))
    return fail(NBMF_ERR_ARG, "an eval set holds at most 2^35 pairs of a matrix with fewer than 2^31 rows and columns");
  for (int64_t t = 0; t < count; ++t)   // before anything is kept: a refused set leaves the one in place working
    if (rows[t] < 0 || rows[t] >= c->m || cols[t] < 0 || cols[t] >= c->n)
      return fail(NBMF_ERR_ARG, "index pair at position %lld is outside [0, %lld) x [0, %lld)", (long long)t, (long long)c->m,
                  (long long)c->n);
  const size_t K = (size_t)c->k, cnt = (size_t)count;
  const size_t nparts = (cnt + EV_PAIRS - 1) / EV_PAIRS;
  PredictStage fresh{c->stream, {}};   // given back on every early return; emptied once the context owns the blocks
  int *rows_d = nullptr, *cols_d = nullptr;
  unsigned char* x_d = nullptr;
  double *Wk = nullptr, *Hk = nullptr, *partials = nullptr;
  HIPCHK(fresh.get(&rows_d, sizeof(int) * cnt));
  HIPCHK(fresh.get(&cols_d, sizeof(int) * cnt));
  HIPCHK(fresh.get(&x_d, cnt));
  HIPCHK(fresh.get(&Wk, sizeof(double) * K * (size_t)c->m));
  HIPCHK(fresh.get(&Hk, sizeof(double) * K * (size_t)c->n));
  HIPCHK(fresh.get(&partials, sizeof(double) * nparts));
  if (!ev.bestW) HIPCHK(dmalloc(&ev.bestW, sizeof(double) * (size_t)c->KP * c->mA));
  if (!ev.bestH) HIPCHK(dmalloc(&ev.bestH, sizeof(double) * (size_t)c->KP * c->nA));
  if (int rc = ensure_eval_slots(c, 1)) return rc;
  {
    std::vector<int> narrow(cnt);
    for (const bool col : {false, true}) {
      const int64_t* src = col ? cols : rows;
      for (size_t t = 0; t < cnt; ++t) narrow[t] = (int)src[t];
      HIPCHK(hipMemcpyAsync(col ? cols_d : rows_d, narrow.data(), sizeof(int) * cnt, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    HIPCHK(hipMemcpyAsync(x_d, x, cnt, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  eval_release(c);   // (the stream has just been drained)
  fresh.blocks.clear();
  ev.rows = rows_d;
  ev.cols = cols_d;
  ev.x = x_d;
  ev.Wk = Wk;
  ev.Hk = Hk;
  ev.partials = partials;
  ev.count = count;
  ev.every = every;
  ev.patience = patience;
  return NBMF_OK;
}

int nbmf_eval_loglik(nbmf_ctx* c, double* loglik) {
  if (int rc = predict_ready(c)) return rc;
  if (c->eval.count == 0) return fail(NBMF_ERR_STATE, "no eval set on the device (nbmf_set_eval)");
  if (!loglik) return fail(NBMF_ERR_ARG, "null output");
  if (int rc = set_device(c)) return rc;
  if (int rc = enqueue_eval(c, 0)) return rc;
  HIPCHK(hipMemcpyAsync(loglik, c->eval.eval_ll_d, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBMF_OK;
}

int nbmf_get_eval(nbmf_ctx* c, int cap, int* n_evals, int* iters, double* logliks, int* best_iter, int* stopped_early) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (cap < 0) return fail(NBMF_ERR_ARG, "cap must be >= 0 (got %d)", cap);
  const auto& ev = c->eval;
  const size_t have = ev.iters.size(), give = std::min(have, (size_t)cap);
  if (n_evals) *n_evals = (int)have;
  if (iters) std::copy(ev.iters.begin(), ev.iters.begin() + give, iters);
  if (logliks) std::copy(ev.logliks.begin(), ev.logliks.begin() + give, logliks);
  if (best_iter) *best_iter = ev.best_iter;
  if (stopped_early) *stopped_early = ev.stopped_early;
  return NBMF_OK;
}

int nbmf_get_best_factors(nbmf_ctx* c, double* W, double* H) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (!c->eval.have_best) return fail(NBMF_ERR_STATE, "the last nbmf_run made no evaluation: no best factors");
  if (int rc = set_device(c)) return rc;
  for (const bool h : {false, true}) {
    double* out = h ? H : W;
    if (!out) continue;
    launch_get_factor(c, h, h ? c->eval.bestH : c->eval.bestW, c->stage);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, c->stage, sizeof(double) * (size_t)c->k * (h ? c->n : c->m), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return NBMF_OK;
}

// ---- the held-out split drawn on the device (nbmf_holdout_kernels.inc) ----------------------------------
// Everything derived from the observed pattern, made again from the code images the way the tail of an upload makes it:
// the lane-mask images (which also drops image B's pad marks), the pad marks where everything is observed again, the
// observed counts and the per-row counts.  c->n_obs is the caller's.  Synchronises.
static int rebuild_observed_state(nbmf_ctx* c) {
  const long long n_tiles = (long long)(c->mA / 16) * (c->nA / 16);
  for (int image = 0; image < 2; ++image) {
    hipLaunchKernelGGL(mask_build_kernel, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, c->stream,
                       (const uint32_t*)(image == 0 ? c->dataA : c->dataB), image == 0 ? c->bitsA : c->bitsB, n_tiles);
    HIPCHK(hipGetLastError());
  }
  if (int rc = mark_pad_rows_b(c)) return rc;
  c->n_obs_global = c->n_obs;
  hipLaunchKernelGGL(rowcount_kernel, dim3((unsigned)((c->m + 255) / 256)), dim3(256), 0, c->stream, c->dataB, c->maskB,
                     c->data_kind, (long long)(c->nA / 16), (long long)c->m, (long long)c->n, c->rowcnt);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBMF_OK;
}

int nbmf_hold_out(nbmf_ctx* c, uint64_t seed, int transposed, double lo, double hi, int every, int patience, int64_t* count) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (!(lo >= 0.0 && lo < hi && hi <= 1.0)) return fail(NBMF_ERR_ARG, "the interval must satisfy 0 <= lo < hi <= 1 (got [%g, %g))", lo, hi);
  if (every < 1) return fail(NBMF_ERR_ARG, "every must be >= 1 (got %d)", every);
  if (patience < 0) return fail(NBMF_ERR_ARG, "patience must be >= 0 (got %d)", patience);
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "held-out evaluation runs on an unsharded context (nbmf_comm_detach first)");
  if (c->data_kind != DATA_BIN) return fail(NBMF_ERR_STATE, "hold-out needs binary data with a binary or no mask");
  auto& ev = c->eval;
  if (ev.held_out) return fail(NBMF_ERR_STATE, "a hold-out is already in place: undo it first (nbmf_hold_out_undo)");
  if (c->m > 0x7fffffffLL || c->n > 0x7fffffffLL)
    return fail(NBMF_ERR_ARG, "an eval set holds at most 2^35 pairs of a matrix with fewer than 2^31 rows and columns");
  if (int rc = set_device(c)) return rc;
  // (lo 2^53 and hi 2^53 are exact, and for the integer k of the uniform  lo <= k 2^-53 < hi  <=>  ceil(lo 2^53) <= k < ceil(hi 2^53))
  HoldOutRule h{(unsigned long long)seed, (unsigned long long)ceil(lo * 9007199254740992.0), (unsigned long long)ceil(hi * 9007199254740992.0),
                (long long)c->m, (long long)c->n, transposed ? 1 : 0};
  const long long RbA = c->mA / 16, RbB = c->nA / 16, strips = (c->m + 15) / 16, tiles_e = (c->n + 15) / 16;
  const long long nseg = (tiles_e + HO_SEG_TILES - 1) / HO_SEG_TILES, total = (long long)c->m * nseg;
  const long long nb = (total + HO_SCAN_BLOCK - 1) / HO_SCAN_BLOCK;
  const unsigned walk_grid = (unsigned)((strips * nseg + 3) / 4);
  PredictStage scratch{c->stream, {}};
  unsigned int* counts = nullptr;
  unsigned long long *bsum = nullptr, *offs = nullptr;
  HIPCHK(scratch.get(&counts, sizeof(unsigned int) * (size_t)total));
  HIPCHK(scratch.get(&bsum, sizeof(unsigned long long) * (size_t)(nb + 1)));
  // count first: a split that is refused has changed nothing
  hipLaunchKernelGGL(holdout_count_kernel, dim3(walk_grid), dim3(256), 0, c->stream, (const uint32_t*)c->dataB, RbB, strips, nseg,
                     tiles_e, h, counts);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(holdout_block_sum_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, (const unsigned int*)counts, total, bsum);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(holdout_scan_blocks_kernel, dim3(1), dim3(256), 0, c->stream, bsum, nb);
  HIPCHK(hipGetLastError());
  unsigned long long held = 0;
  HIPCHK(hipMemcpyAsync(&held, bsum + nb, sizeof held, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (held == 0) return fail(NBMF_ERR_ARG, "the split [%g, %g) with seed %llu holds out no entry", lo, hi, (unsigned long long)seed);
  if ((double)held >= c->n_obs)
    return fail(NBMF_ERR_ARG, "the split [%g, %g) with seed %llu leaves no observed entry", lo, hi, (unsigned long long)seed);
  if (held > (1ull << 35))
    return fail(NBMF_ERR_ARG, "an eval set holds at most 2^35 pairs of a matrix with fewer than 2^31 rows and columns");
  const size_t K = (size_t)c->k, cnt = (size_t)held;
  const size_t nparts = (cnt + EV_PAIRS - 1) / EV_PAIRS;
  PredictStage fresh{c->stream, {}};   // given back on every early return; emptied once the context owns the blocks
  int *rows_d = nullptr, *cols_d = nullptr;
  unsigned char* x_d = nullptr;
  double *Wk = nullptr, *Hk = nullptr, *partials = nullptr;
  HIPCHK(scratch.get(&offs, sizeof(unsigned long long) * (size_t)total));
  HIPCHK(fresh.get(&rows_d, sizeof(int) * cnt));
  HIPCHK(fresh.get(&cols_d, sizeof(int) * cnt));
  HIPCHK(fresh.get(&x_d, cnt));
  HIPCHK(fresh.get(&Wk, sizeof(double) * K * (size_t)c->m));
  HIPCHK(fresh.get(&Hk, sizeof(double) * K * (size_t)c->n));
  HIPCHK(fresh.get(&partials, sizeof(double) * nparts));
  if (!ev.bestW) HIPCHK(dmalloc(&ev.bestW, sizeof(double) * (size_t)c->KP * c->mA));
  if (!ev.bestH) HIPCHK(dmalloc(&ev.bestH, sizeof(double) * (size_t)c->KP * c->nA));
  if (int rc = ensure_eval_slots(c, 1)) return rc;
  // nothing below can be refused: the images change from here on
  hipLaunchKernelGGL(holdout_scan_final_kernel, dim3((unsigned)nb), dim3(256), 0, c->stream, (const unsigned int*)counts, total,
                     (const unsigned long long*)bsum, offs);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(holdout_scatter_kernel, dim3(walk_grid), dim3(256), 0, c->stream, (unsigned char*)c->dataA,
                     (unsigned char*)c->dataB, RbA, RbB, strips, nseg, tiles_e, h, (const unsigned long long*)offs, rows_d, cols_d, x_d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  eval_release(c);   // (the stream has just been drained)
  fresh.blocks.clear();
  ev.rows = rows_d;
  ev.cols = cols_d;
  ev.x = x_d;
  ev.Wk = Wk;
  ev.Hk = Hk;
  ev.partials = partials;
  ev.count = (int64_t)held;
  ev.every = every;
  ev.patience = patience;
  ev.held_out = true;
  c->n_obs -= (double)held;
  if (int rc = rebuild_observed_state(c)) return rc;
  if (count) *count = (int64_t)held;
  return NBMF_OK;
}

int nbmf_hold_out_undo(nbmf_ctx* c) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  auto& ev = c->eval;
  if (!ev.held_out) return fail(NBMF_ERR_STATE, "no hold-out in place (nbmf_hold_out)");
  if (int rc = set_device(c)) return rc;
  hipLaunchKernelGGL(holdout_restore_kernel, dim3((unsigned)((ev.count + 255) / 256)), dim3(256), 0, c->stream,
                     (unsigned char*)c->dataA, (unsigned char*)c->dataB, (long long)(c->mA / 16), (long long)(c->nA / 16),
                     (const int*)ev.rows, (const int*)ev.cols, (const unsigned char*)ev.x, (long long)ev.count);
  HIPCHK(hipGetLastError());
  c->n_obs += (double)ev.count;
  ev.held_out = false;
  if (int rc = rebuild_observed_state(c)) return rc;
  eval_release(c);   // (rebuild_observed_state has drained the stream)
  return NBMF_OK;
}

int nbmf_get_eval_pairs(nbmf_ctx* c, int64_t cap, int64_t* count, int64_t* rows, int64_t* cols, uint8_t* x) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (cap < 0) return fail(NBMF_ERR_ARG, "cap must be >= 0 (got %lld)", (long long)cap);
  const auto& ev = c->eval;
  if (count) *count = ev.count;
  const size_t give = (size_t)std::min<int64_t>(cap, ev.count);
  if (give == 0 || (!rows && !cols && !x)) return NBMF_OK;
  if (int rc = set_device(c)) return rc;
  std::vector<int> narrow(give);
  for (const bool col : {false, true}) {
    int64_t* dst = col ? cols : rows;
    if (!dst) continue;
    HIPCHK(hipMemcpyAsync(narrow.data(), col ? ev.cols : ev.rows, sizeof(int) * give, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t t = 0; t < give; ++t) dst[t] = narrow[t];
  }
  if (x) {
    HIPCHK(hipMemcpyAsync(x, ev.x, give, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return NBMF_OK;
}

int nbmf_predict_rows(nbmf_ctx* c, int64_t row0, int64_t nrows, int clip_theta, int out_kind, double threshold, void* out,
                      int64_t ldout) {
  if (int rc = predict_ready(c)) return rc;
  if (int rc = check_rows(c, row0, nrows)) return rc;
  if (ldout < c->n) return fail(NBMF_ERR_ARG, "ldout %lld is less than n = %lld", (long long)ldout, (long long)c->n);
  if (out_kind != NBMF_PREDICT_F64 && out_kind != NBMF_PREDICT_U8) return fail(NBMF_ERR_ARG, "unknown out_kind %d", out_kind);
  if (out_kind == NBMF_PREDICT_U8 && threshold != threshold) return fail(NBMF_ERR_ARG, "threshold is NaN");
  if (nrows == 0) return NBMF_OK;
  if (!out) return fail(NBMF_ERR_ARG, "null output");
  if (int rc = set_device(c)) return rc;
  const size_t elt = out_kind == NBMF_PREDICT_U8 ? 1 : sizeof(double);
  RowPanels pl;
  if (int rc = plan_row_panels(c, "nbmf_predict_rows", row0, nrows, (size_t)panel_ld(c) * elt, false, &pl)) return rc;
  PredictStage st{c->stream, {}};
  char* panel_d = nullptr;
  HIPCHK(st.get(&panel_d, (size_t)pl.stage_rows() * pl.ldp * elt));
  for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    HIPCHK(launch_theta_panel(c, pl, c->Wn, (long long)c->mA, c->Hn, (long long)c->nA, p0, pn, out_kind, clip_theta, threshold, panel_d));
    HIPCHK(copy_rows((char*)out + (size_t)(p0 - row0) * ldout * elt, ldout * elt, panel_d, pl.ldp * elt, c->n * elt, pn,
                     hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  return NBMF_OK;
}

// ---- Theta decided per entry, as bits (theta_bits_kernel in nbmf_theta_bits_kernels.inc) ---------------------
// The shape of nbmf_predict_rows: per panel one launch into a staging panel of nA / 8 bytes per row (a multiple of 16: the
// kernel stores 8 aligned bytes per wave and row), then ceil(n / 8) bytes of each row back to the caller.
int nbmf_theta_bits(nbmf_ctx* c, int64_t row0, int64_t nrows, int clip_theta, int mode, double threshold, uint64_t seed,
                    uint8_t* out, int64_t ldout) {
  if (int rc = predict_ready(c)) return rc;
  if (int rc = check_rows(c, row0, nrows)) return rc;
  if (int rc = check_row_ld("ldout", ldout, true, c->n)) return rc;
  if (mode != NBMF_BITS_THRESHOLD && mode != NBMF_BITS_SAMPLE) return fail(NBMF_ERR_ARG, "unknown mode %d", mode);
  if (mode == NBMF_BITS_THRESHOLD && threshold != threshold) return fail(NBMF_ERR_ARG, "threshold is NaN");
  if (nrows == 0) return NBMF_OK;
  if (!out) return fail(NBMF_ERR_ARG, "null output");
  if (int rc = set_device(c)) return rc;
  const long long ldb = (long long)c->nA / 8;   // (nA is a multiple of 128)
  RowPanels pl;
  if (int rc = plan_row_panels(c, "nbmf_theta_bits", row0, nrows, (size_t)ldb, false, &pl)) return rc;
  PredictStage st{c->stream, {}};
  unsigned char* panel_d = nullptr;
  HIPCHK(st.get(&panel_d, (size_t)pl.stage_rows() * ldb));
  const size_t width = (size_t)packed_ld(c->n);
  for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    hipLaunchKernelGGL(mode == NBMF_BITS_SAMPLE ? theta_bits_kernel<TB_SAMPLE> : theta_bits_kernel<TB_THRESHOLD>, pl.grid(p0, pn),
                       dim3(PR_WAVES * 64), 0, c->stream, (const double*)c->Wn, (const double*)c->Hn, c->k, (long long)c->mA,
                       (long long)c->nA, (long long)c->n, p0, pn, ldb, clip_theta != 0 ? 1 : 0, threshold,
                       (unsigned long long)seed, panel_d);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_rows(out + (size_t)(p0 - row0) * ldout, (size_t)ldout, panel_d, (size_t)ldb, width, pn, hipMemcpyDeviceToHost,
                     c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  return NBMF_OK;
}

// ---- Theta ranked on the device: the top columns of each row (top_n_kernel) --------------------------------
// Per panel: the product kernel of nbmf_predict_rows, unchanged, into the staging panel (so a score is bit for bit the
// entry nbmf_predict_rows returns), then the selection, then top entries per row back to the host instead of n.
int nbmf_top_n(nbmf_ctx* c, int64_t row0, int64_t nrows, int top, int clip_theta, const uint8_t* exclude, int64_t ldx,
               int64_t* out_cols, double* out_scores, int64_t ldout) {
  return nbmf_top_n_v(c, row0, nrows, top, clip_theta, exclude, NBMF_DATA_U8, ldx, out_cols, out_scores, ldout);
}

int nbmf_top_n_v(nbmf_ctx* c, int64_t row0, int64_t nrows, int top, int clip_theta, const void* exclude, int exclude_kind,
                 int64_t ldx, int64_t* out_cols, double* out_scores, int64_t ldout) {
  if (int rc = predict_ready(c)) return rc;
  if (top < 1 || top > NBMF_TOP_N_MAX) return fail(NBMF_ERR_ARG, "top must be in [1, %d] (got %d)", NBMF_TOP_N_MAX, top);
  if (int rc = check_rows(c, row0, nrows)) return rc;
  if (ldout < top) return fail(NBMF_ERR_ARG, "ldout %lld is less than top = %d", (long long)ldout, top);
  if (exclude_kind != NBMF_DATA_U8 && exclude_kind != NBMF_DATA_BITS) return fail(NBMF_ERR_ARG, "unknown exclude_kind %d", exclude_kind);
  const bool exbits = exclude_kind == NBMF_DATA_BITS;
  if (exclude)
    if (int rc = check_row_ld("ldx", ldx, exbits, c->n)) return rc;
  if (nrows == 0) return NBMF_OK;
  if (!out_cols) return fail(NBMF_ERR_ARG, "null output");
  if (int rc = set_device(c)) return rc;
  static_assert(NBMF_TOP_N_MAX == TN_MAX, "the kernel's entry list holds NBMF_TOP_N_MAX slots");
  const long long n = c->n;
  RowPanels pl;   // (the panel of nbmf_predict_rows, float64)
  const size_t exb = exclude && exbits ? (size_t)packed_ld(n) : 0;   // a packed exclude row's share of the staging
  if (int rc = plan_row_panels(c, "nbmf_top_n", row0, nrows, (size_t)panel_ld(c) * sizeof(double) + exb, false, &pl)) return rc;
  const size_t rows = (size_t)pl.stage_rows(), w64 = sizeof(int64_t) * (size_t)top, pitch = sizeof(int64_t) * (size_t)ldout;
  PredictStage st{c->stream, {}};
  double *panel_d = nullptr, *scores_d = nullptr;
  long long* cols_d = nullptr;
  unsigned char *ex_d = nullptr, *exbits_d = nullptr;
  HIPCHK(st.get(&panel_d, sizeof(double) * rows * pl.ldp));
  HIPCHK(st.get(&cols_d, rows * w64));
  if (out_scores) HIPCHK(st.get(&scores_d, rows * w64));
  if (exclude) HIPCHK(st.get(&ex_d, rows * n));
  if (exb) HIPCHK(st.get(&exbits_d, rows * exb));
  for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    const size_t done = (size_t)(p0 - row0);
    if (exclude)
      HIPCHK(stage_rows_as_bytes(exbits_d, (const char*)exclude + done * ldx, exbits, 1, ldx, n, pn, ex_d, n, c->stream));
    HIPCHK(launch_theta_panel(c, pl, c->Wn, (long long)c->mA, c->Hn, (long long)c->nA, p0, pn, NBMF_PREDICT_F64, clip_theta, 0.0,
                              panel_d));
    hipLaunchKernelGGL(top_n_kernel<0>, dim3((unsigned)pn), dim3(TN_THREADS), 0, c->stream, (const double*)panel_d, pl.ldp, n,
                       (const unsigned char*)ex_d, n, top, cols_d, scores_d, (const long long*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_rows(out_cols + done * ldout, pitch, cols_d, w64, w64, pn, hipMemcpyDeviceToHost, c->stream));
    if (out_scores) HIPCHK(copy_rows(out_scores + done * ldout, pitch, scores_d, w64, w64, pn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  return NBMF_OK;
}

// ---- similar items: one side of the matrix against itself (nbmf_neighbors_kernels.inc) --------------------
// Per call: the two operand images of the metric (DOT: the factor itself, twice; COSINE: the factor scaled by its items'
// norms, twice; PROFILE: F d^(-1/2) and (G F) d^(-1/2) with G the other factor's Gram matrix and d = diag(F^T G F)), the
// query items' columns of the left one gathered into a compact image, and then per panel of query rows the product kernel
// of nbmf_predict_rows without a clip -- and for nbmf_neighbors the selection of nbmf_top_n with the row's own item
// ineligible.  Both entry points run the same kernels on the same operands up to the panel: a neighbour's score is the
// slab's entry by construction.
}  // extern "C"
namespace {

struct SimCall {
  long long L = 0, LA = 0, nqA = 0;   // items of the axis, their image length, the gathered image's length
  const double* right = nullptr;      // [KP][LA]
  double* left = nullptr;             // [KP][nqA]: the gathered queries
  long long* query_d = nullptr;       // nq indices (the self column of each row)
};

int sim_check(nbmf_ctx* c, int axis, int metric, const int64_t* query, int64_t nq, long long* L_out) {
  if (int rc = predict_ready(c)) return rc;
  if (axis != 0 && axis != 1) return fail(NBMF_ERR_ARG, "axis must be 0 (samples) or 1 (features) (got %d)", axis);
  if (metric != NBMF_SIM_DOT && metric != NBMF_SIM_COSINE && metric != NBMF_SIM_PROFILE)
    return fail(NBMF_ERR_ARG, "unknown metric %d", metric);
  const long long L = axis == 0 ? c->m : c->n;
  if (nq < 0) return fail(NBMF_ERR_ARG, "nq must be >= 0 (got %lld)", (long long)nq);
  if (!query && nq > L) return fail(NBMF_ERR_ARG, "nq = %lld without a query list is more than the %lld items", (long long)nq, L);
  if (query)
    for (int64_t t = 0; t < nq; ++t)
      if (query[t] < 0 || query[t] >= L)
        return fail(NBMF_ERR_ARG, "query index at position %lld is outside [0, %lld)", (long long)t, L);
  *L_out = L;
  return NBMF_OK;
}

// The operands of one call on the stream, from the call's staging.
int sim_prepare(nbmf_ctx* c, int axis, int metric, const int64_t* query, int64_t nq, PredictStage& st, SimCall* sc) {
  const int K = c->k, KP = c->KP;
  const double* F = axis == 0 ? c->Wn : c->Hn;
  const double* C = axis == 0 ? c->Hn : c->Wn;
  const long long L = axis == 0 ? c->m : c->n, LA = axis == 0 ? c->mA : c->nA;
  const long long lenC = axis == 0 ? c->n : c->m, lenCA = axis == 0 ? c->nA : c->mA;
  const size_t img = sizeof(double) * (size_t)KP * LA;
  const unsigned item_blocks = (unsigned)((L + NB_THREADS - 1) / NB_THREADS), image_blocks = (unsigned)(LA / NB_THREADS + (LA % NB_THREADS != 0));
  const double *left = F, *right = F;
  if (metric == NBMF_SIM_COSINE) {
    double *d = nullptr, *U = nullptr;
    HIPCHK(st.get(&d, sizeof(double) * (size_t)L));
    HIPCHK(st.get(&U, img));
    hipLaunchKernelGGL(item_dot_kernel, dim3(item_blocks), dim3(NB_THREADS), 0, c->stream, F, F, K, L, LA, d);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(item_scale_kernel, dim3(image_blocks, (unsigned)KP), dim3(NB_THREADS), 0, c->stream, F, (const double*)d, K, KP,
                       L, LA, U);
    HIPCHK(hipGetLastError());
    left = right = U;
  } else if (metric == NBMF_SIM_PROFILE) {
    // the chunks of the Gram sum: at most NB_GRAM_BLOCKS of them, each a multiple of NB_GX items -- a function of lenC only
    const long long want = std::min<long long>(NB_GRAM_BLOCKS, (lenC + 4 * NB_GX - 1) / (4 * NB_GX));
    const long long chunk = round_up((lenC + want - 1) / want, NB_GX);
    const int chunks = (int)((lenC + chunk - 1) / chunk);
    const unsigned tiles = (unsigned)((K + NB_GT - 1) / NB_GT);
    double *part = nullptr, *G = nullptr, *B = nullptr, *d = nullptr, *P = nullptr, *Q = nullptr;
    HIPCHK(st.get(&part, sizeof(double) * (size_t)chunks * K * K));
    HIPCHK(st.get(&G, sizeof(double) * (size_t)K * K));
    HIPCHK(st.get(&B, sizeof(double) * (size_t)K * LA));
    HIPCHK(st.get(&d, sizeof(double) * (size_t)L));
    HIPCHK(st.get(&P, img));
    HIPCHK(st.get(&Q, img));
    hipLaunchKernelGGL(gram_partial_kernel, dim3((unsigned)chunks, tiles, tiles), dim3(NB_GT * NB_GT), 0, c->stream, C, K, lenC, lenCA,
                       chunk, part);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(gram_sum_kernel, dim3((unsigned)((K * K + NB_THREADS - 1) / NB_THREADS)), dim3(NB_THREADS), 0, c->stream,
                       (const double*)part, K, chunks, G);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(gram_apply_kernel, dim3(item_blocks, (unsigned)((K + NB_BT - 1) / NB_BT)), dim3(NB_THREADS), 0, c->stream,
                       (const double*)G, F, K, L, LA, B);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(item_dot_kernel, dim3(item_blocks), dim3(NB_THREADS), 0, c->stream, F, (const double*)B, K, L, LA, d);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(item_scale_kernel, dim3(image_blocks, (unsigned)KP), dim3(NB_THREADS), 0, c->stream, F, (const double*)d, K, KP,
                       L, LA, P);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(item_scale_kernel, dim3(image_blocks, (unsigned)KP), dim3(NB_THREADS), 0, c->stream, (const double*)B,
                       (const double*)d, K, KP, L, LA, Q);
    HIPCHK(hipGetLastError());
    left = P;
    right = Q;
  }
  sc->L = L;
  sc->LA = LA;
  sc->right = right;
  sc->nqA = round_up(nq, 16);
  HIPCHK(st.get(&sc->query_d, sizeof(long long) * (size_t)nq));
  HIPCHK(st.get(&sc->left, sizeof(double) * (size_t)KP * sc->nqA));
  std::vector<long long> iota;   // (a NULL query: the items 0 .. nq - 1)
  if (!query) {
    iota.resize((size_t)nq);
    for (int64_t t = 0; t < nq; ++t) iota[(size_t)t] = t;
  }
  static_assert(sizeof(long long) == sizeof(int64_t), "the query list goes up as it is");
  HIPCHK(hipMemcpyAsync(sc->query_d, query ? (const void*)query : (const void*)iota.data(), sizeof(long long) * (size_t)nq,
                        hipMemcpyHostToDevice, c->stream));
  if (!query) HIPCHK(hipStreamSynchronize(c->stream));   // (iota leaves scope with this function)
  hipLaunchKernelGGL(gather_items_kernel, dim3((unsigned)((sc->nqA + NB_THREADS - 1) / NB_THREADS), (unsigned)KP), dim3(NB_THREADS), 0,
                     c->stream, left, LA, (const long long*)sc->query_d, K, (long long)nq, sc->nqA, sc->left);
  HIPCHK(hipGetLastError());
  return NBMF_OK;
}

}  // namespace
extern "C" {

int nbmf_similarity(nbmf_ctx* c, int axis, int metric, const int64_t* query, int64_t nq, double* out, int64_t ldout) {
  long long L = 0;
  if (int rc = sim_check(c, axis, metric, query, nq, &L)) return rc;
  if (ldout < L) return fail(NBMF_ERR_ARG, "ldout %lld is less than the %lld items", (long long)ldout, L);
  if (nq == 0) return NBMF_OK;
  if (!out) return fail(NBMF_ERR_ARG, "null output");
  if (int rc = set_device(c)) return rc;
  RowPanels pl;
  if (int rc = plan_panels("nbmf_similarity", L, axis == 0 ? c->mA : c->nA, 0, nq, (size_t)round_up(L, 4) * sizeof(double), false, &pl))
    return rc;
  PredictStage st{c->stream, {}};
  SimCall sc;
  if (int rc = sim_prepare(c, axis, metric, query, nq, st, &sc)) return rc;
  double* panel_d = nullptr;
  HIPCHK(st.get(&panel_d, sizeof(double) * (size_t)pl.stage_rows() * pl.ldp));
  for (long long p0 = 0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    HIPCHK(launch_theta_panel(c, pl, sc.left, sc.nqA, sc.right, sc.LA, p0, pn, NBMF_PREDICT_F64, 0, 0.0, panel_d));
    HIPCHK(copy_rows(out + (size_t)p0 * ldout, sizeof(double) * (size_t)ldout, panel_d, sizeof(double) * (size_t)pl.ldp,
                     sizeof(double) * (size_t)L, pn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  return NBMF_OK;
}

int nbmf_neighbors(nbmf_ctx* c, int axis, int metric, const int64_t* query, int64_t nq, int top, int skip_self, int64_t* out_idx,
                   double* out_scores, int64_t ldout) {
  long long L = 0;
  if (int rc = sim_check(c, axis, metric, query, nq, &L)) return rc;
  if (top < 1 || top > NBMF_TOP_N_MAX) return fail(NBMF_ERR_ARG, "top must be in [1, %d] (got %d)", NBMF_TOP_N_MAX, top);
  if (ldout < top) return fail(NBMF_ERR_ARG, "ldout %lld is less than top = %d", (long long)ldout, top);
  if (nq == 0) return NBMF_OK;
  if (!out_idx) return fail(NBMF_ERR_ARG, "null output");
  if (int rc = set_device(c)) return rc;
  RowPanels pl;
  if (int rc = plan_panels("nbmf_neighbors", L, axis == 0 ? c->mA : c->nA, 0, nq, (size_t)round_up(L, 4) * sizeof(double), false, &pl))
    return rc;
  PredictStage st{c->stream, {}};
  SimCall sc;
  if (int rc = sim_prepare(c, axis, metric, query, nq, st, &sc)) return rc;
  const size_t rows = (size_t)pl.stage_rows(), w64 = sizeof(int64_t) * (size_t)top, pitch = sizeof(int64_t) * (size_t)ldout;
  double *panel_d = nullptr, *scores_d = nullptr;
  long long* idx_d = nullptr;
  HIPCHK(st.get(&panel_d, sizeof(double) * rows * pl.ldp));
  HIPCHK(st.get(&idx_d, rows * w64));
  if (out_scores) HIPCHK(st.get(&scores_d, rows * w64));
  for (long long p0 = 0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    HIPCHK(launch_theta_panel(c, pl, sc.left, sc.nqA, sc.right, sc.LA, p0, pn, NBMF_PREDICT_F64, 0, 0.0, panel_d));
    if (skip_self)
      hipLaunchKernelGGL(top_n_kernel<1>, dim3((unsigned)pn), dim3(TN_THREADS), 0, c->stream, (const double*)panel_d, pl.ldp, L,
                         (const unsigned char*)nullptr, 0LL, top, idx_d, scores_d, (const long long*)(sc.query_d + p0));
    else
      hipLaunchKernelGGL(top_n_kernel<0>, dim3((unsigned)pn), dim3(TN_THREADS), 0, c->stream, (const double*)panel_d, pl.ldp, L,
                         (const unsigned char*)nullptr, 0LL, top, idx_d, scores_d, (const long long*)nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(copy_rows(out_idx + (size_t)p0 * ldout, pitch, idx_d, w64, w64, pn, hipMemcpyDeviceToHost, c->stream));
    if (out_scores) HIPCHK(copy_rows(out_scores + (size_t)p0 * ldout, pitch, scores_d, w64, w64, pn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  return NBMF_OK;
}

// ---- Theta judged against data: log-likelihood per row and per column (nbmf_score_kernels.inc) -------------
// Per panel: the caller's data and mask rows up into staging panels (copy_rows), the fused product-and-score kernel, then
// the finishing steps -- the strips of a row in ascending order, the 16-row blocks of a column in ascending order onto
// accumulators that stay on the device for the whole call.  The panels are 16-aligned (RowPanels), so a 16-row block never
// straddles two of them and a column's chain of additions is the same whatever the panel height.
int nbmf_score_rows(nbmf_ctx* c, int64_t row0, int64_t nrows, int clip_theta, double eps, const void* x, int x_kind, int64_t ldx,
                    const uint8_t* mask, int64_t ldmask, double* row_ll, int64_t* row_obs, double* col_ll, int64_t* col_obs) {
  return nbmf_score_rows_v(c, row0, nrows, clip_theta, eps, x, x_kind, ldx, mask, mask ? NBMF_MASK_U8 : NBMF_MASK_NONE, ldmask, row_ll,
                           row_obs, col_ll, col_obs);
}

int nbmf_score_rows_v(nbmf_ctx* c, int64_t row0, int64_t nrows, int clip_theta, double eps, const void* x, int x_kind, int64_t ldx,
                      const void* mask, int mask_kind, int64_t ldmask, double* row_ll, int64_t* row_obs, double* col_ll,
                      int64_t* col_obs) {
  if (int rc = predict_ready(c)) return rc;
  if (int rc = check_rows(c, row0, nrows)) return rc;
  if (x_kind != NBMF_DATA_U8 && x_kind != NBMF_DATA_F64 && x_kind != NBMF_DATA_BITS) return fail(NBMF_ERR_ARG, "unknown x_kind %d", x_kind);
  if (mask_kind != NBMF_MASK_NONE && mask_kind != NBMF_MASK_U8 && mask_kind != NBMF_MASK_BITS)
    return fail(NBMF_ERR_ARG, "unknown mask_kind %d", mask_kind);
  if (mask_kind != NBMF_MASK_NONE && !mask) return fail(NBMF_ERR_ARG, "mask_kind set but mask is NULL");
  if (mask_kind == NBMF_MASK_NONE) mask = nullptr;
  const bool xbits = x_kind == NBMF_DATA_BITS, mbits = mask_kind == NBMF_MASK_BITS;
  if (int rc = check_row_ld("ldx", ldx, xbits, c->n)) return rc;
  if (mask)
    if (int rc = check_row_ld("ldmask", ldmask, mbits, c->n)) return rc;
  if (!(eps >= 0.0)) return fail(NBMF_ERR_ARG, "eps must be >= 0 (got %g)", eps);
  if (!row_ll && !row_obs && !col_ll && !col_obs) return fail(NBMF_ERR_ARG, "no output requested");
  const long long n = c->n;
  if (nrows == 0) {   // nothing is read; the sums over no rows
    if (col_ll) std::fill(col_ll, col_ll + n, 0.0);
    if (col_obs) std::fill(col_obs, col_obs + n, (int64_t)0);
    return NBMF_OK;
  }
  if (!x) return fail(NBMF_ERR_ARG, "null data");
  if (int rc = set_device(c)) return rc;
  const bool want_rows = row_ll || row_obs, want_cols = col_ll || col_obs;
  const size_t elt = x_kind == NBMF_DATA_F64 ? sizeof(double) : 1;
  const long long ldp = panel_ld(c);
  const long long strips = (n + PR_STRIP - 1) / PR_STRIP;      // the strips that hold a real column
  // the budget of nbmf_predict_rows over everything a panel row stages: data, mask, its strip partials, its share of a block's
  // (and the packed rows as they came, where an operand is packed)
  const size_t per_row = (size_t)ldp * (elt + (mask ? 1 : 0)) + (want_rows ? (size_t)strips * 12 + 16 : 0) +
                         (want_cols ? ((size_t)ldp * 12 + 15) / 16 : 0) + (size_t)packed_ld(n) * ((xbits ? 1 : 0) + (mbits ? 1 : 0));
  RowPanels pl;
  if (int rc = plan_row_panels(c, "nbmf_score_rows", row0, nrows, per_row, true, &pl)) return rc;
  const long long stage_rows = pl.stage_rows(), max_blocks = stage_rows / 16 + 2;   // (no panel touches more 16-row blocks)
  PredictStage st{c->stream, {}};
  char* x_d = nullptr;
  unsigned char *m_d = nullptr, *xbits_d = nullptr, *mbits_d = nullptr;
  double *rpart_d = nullptr, *cpart_d = nullptr, *row_ll_d = nullptr, *col_ll_d = nullptr;
  int *rcnt_d = nullptr, *ccnt_d = nullptr;
  long long *row_obs_d = nullptr, *col_obs_d = nullptr;
  HIPCHK(st.get(&x_d, (size_t)stage_rows * ldp * elt));
  if (mask) HIPCHK(st.get(&m_d, (size_t)stage_rows * ldp));
  if (xbits) HIPCHK(st.get(&xbits_d, (size_t)stage_rows * packed_ld(n)));
  if (mbits) HIPCHK(st.get(&mbits_d, (size_t)stage_rows * packed_ld(n)));
  if (want_rows) {
    HIPCHK(st.get(&rpart_d, sizeof(double) * (size_t)strips * stage_rows));
    HIPCHK(st.get(&rcnt_d, sizeof(int) * (size_t)strips * stage_rows));
    HIPCHK(st.get(&row_ll_d, sizeof(double) * (size_t)stage_rows));
    HIPCHK(st.get(&row_obs_d, sizeof(long long) * (size_t)stage_rows));
  }
  if (want_cols) {
    HIPCHK(st.get(&cpart_d, sizeof(double) * (size_t)max_blocks * ldp));
    HIPCHK(st.get(&ccnt_d, sizeof(int) * (size_t)max_blocks * ldp));
    HIPCHK(st.get(&col_ll_d, sizeof(double) * (size_t)n));
    HIPCHK(st.get(&col_obs_d, sizeof(long long) * (size_t)n));
    HIPCHK(hipMemsetAsync(col_ll_d, 0, sizeof(double) * (size_t)n, c->stream));
    HIPCHK(hipMemsetAsync(col_obs_d, 0, sizeof(long long) * (size_t)n, c->stream));
  }
  for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);   // (p0 + pn is a multiple of 16, or the end)
    const size_t done = (size_t)(p0 - row0);
    HIPCHK(stage_rows_as_bytes(xbits_d, (const char*)x + done * ldx * elt, xbits, elt, ldx, n, pn, x_d, ldp, c->stream));
    if (mask) HIPCHK(stage_rows_as_bytes(mbits_d, (const char*)mask + done * ldmask, mbits, 1, ldmask, n, pn, m_d, ldp, c->stream));
    HIPCHK(launch_score_panel(c, pl, p0, pn, xbits ? NBMF_DATA_U8 : x_kind, clip_theta, eps, x_d, m_d, rpart_d, rcnt_d, cpart_d, ccnt_d));
    if (want_rows) {
      hipLaunchKernelGGL(score_rows_finish_kernel, dim3((unsigned)((pn + 255) / 256)), dim3(256), 0, c->stream,
                         (const double*)rpart_d, (const int*)rcnt_d, pn, strips, row_ll_d, row_obs_d);
      HIPCHK(hipGetLastError());
      if (row_ll) HIPCHK(hipMemcpyAsync(row_ll + done, row_ll_d, sizeof(double) * (size_t)pn, hipMemcpyDeviceToHost, c->stream));
      if (row_obs)
        HIPCHK(hipMemcpyAsync(row_obs + done, row_obs_d, sizeof(int64_t) * (size_t)pn, hipMemcpyDeviceToHost, c->stream));
    }
    if (want_cols) {
      hipLaunchKernelGGL(score_cols_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                         (const double*)cpart_d, (const int*)ccnt_d, RowPanels::blocks(p0, pn), ldp, n, col_ll_d, col_obs_d);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  if (col_ll) HIPCHK(hipMemcpyAsync(col_ll, col_ll_d, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (col_obs) HIPCHK(hipMemcpyAsync(col_obs, col_obs_d, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  if (want_cols) HIPCHK(hipStreamSynchronize(c->stream));
  return NBMF_OK;
}

// ---- Theta counted against data: class histograms (nbmf_hist_kernels.inc) ----------------------------------
// Per panel: the caller's data and mask rows up into staging panels (copy_rows), then the fused product-and-count kernel,
// whose waves add onto an accumulator of 2 * bins + 2 integers that stays on the device for the whole call -- in
// NBMF_HIST_COPIES copies (environment; default 64), which the finishing kernel adds up at the end -- and comes down once.
// Integer adds: the panels need no alignment (a 16-row block that straddles two of them is formed twice, and each of
// its rows counted in the panel that holds it).
int nbmf_theta_hist(nbmf_ctx* c, int64_t row0, int64_t nrows, int bins, const uint8_t* x, int64_t ldx, const uint8_t* mask,
                    int64_t ldmask, int64_t* hist, int64_t* nan_count) {
  return nbmf_theta_hist_v(c, row0, nrows, bins, x, NBMF_DATA_U8, ldx, mask, mask ? NBMF_MASK_U8 : NBMF_MASK_NONE, ldmask, hist, nan_count);
}

int nbmf_theta_hist_v(nbmf_ctx* c, int64_t row0, int64_t nrows, int bins, const void* x, int x_kind, int64_t ldx, const void* mask,
                      int mask_kind, int64_t ldmask, int64_t* hist, int64_t* nan_count) {
  if (int rc = predict_ready(c)) return rc;
  if (int rc = check_rows(c, row0, nrows)) return rc;
  if (bins < 1 || bins > NBMF_HIST_MAX_BINS) return fail(NBMF_ERR_ARG, "bins must be in [1, %d] (got %d)", NBMF_HIST_MAX_BINS, bins);
  if (x_kind != NBMF_DATA_U8 && x_kind != NBMF_DATA_BITS) return fail(NBMF_ERR_ARG, "unknown x_kind %d", x_kind);
  if (mask_kind != NBMF_MASK_NONE && mask_kind != NBMF_MASK_U8 && mask_kind != NBMF_MASK_BITS)
    return fail(NBMF_ERR_ARG, "unknown mask_kind %d", mask_kind);
  if (mask_kind != NBMF_MASK_NONE && !mask) return fail(NBMF_ERR_ARG, "mask_kind set but mask is NULL");
  if (mask_kind == NBMF_MASK_NONE) mask = nullptr;
  const bool xbits = x_kind == NBMF_DATA_BITS, mbits = mask_kind == NBMF_MASK_BITS;
  if (int rc = check_row_ld("ldx", ldx, xbits, c->n)) return rc;
  if (mask)
    if (int rc = check_row_ld("ldmask", ldmask, mbits, c->n)) return rc;
  if (!hist) return fail(NBMF_ERR_ARG, "null output");
  if (nrows > 0 && !x) return fail(NBMF_ERR_ARG, "null data");
  const size_t slots = 2 * (size_t)bins;
  std::fill(hist, hist + slots, (int64_t)0);   // (nrows == 0: nothing is read; the counts over no rows)
  if (nan_count) nan_count[0] = nan_count[1] = 0;
  if (nrows == 0) return NBMF_OK;
  if (int rc = set_device(c)) return rc;
  const long long n = c->n, ldp = panel_ld(c);
  RowPanels pl;
  const size_t bit_bytes = (size_t)packed_ld(n) * ((xbits ? 1 : 0) + (mbits ? 1 : 0));   // the packed rows as they came
  if (int rc = plan_row_panels(c, "nbmf_theta_hist", row0, nrows, (size_t)ldp * (mask ? 2 : 1) + bit_bytes, false, &pl)) return rc;
  PredictStage st{c->stream, {}};
  unsigned char *x_d = nullptr, *m_d = nullptr, *xbits_d = nullptr, *mbits_d = nullptr;
  const int copies = (int)std::min<long long>(1024, std::max<long long>(1, env_int("NBMF_HIST_COPIES", 64)));
  unsigned long long *total_d = nullptr, *sum_d = nullptr;
  HIPCHK(st.get(&x_d, (size_t)pl.stage_rows() * ldp));
  if (mask) HIPCHK(st.get(&m_d, (size_t)pl.stage_rows() * ldp));
  if (xbits) HIPCHK(st.get(&xbits_d, (size_t)pl.stage_rows() * packed_ld(n)));
  if (mbits) HIPCHK(st.get(&mbits_d, (size_t)pl.stage_rows() * packed_ld(n)));
  HIPCHK(st.get(&total_d, sizeof(unsigned long long) * (slots + 2) * copies));
  HIPCHK(st.get(&sum_d, sizeof(unsigned long long) * (slots + 2)));
  HIPCHK(hipMemsetAsync(total_d, 0, sizeof(unsigned long long) * (slots + 2) * copies, c->stream));
  for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    const size_t done = (size_t)(p0 - row0);
    HIPCHK(stage_rows_as_bytes(xbits_d, (const char*)x + done * ldx, xbits, 1, ldx, n, pn, x_d, ldp, c->stream));
    if (mask) HIPCHK(stage_rows_as_bytes(mbits_d, (const char*)mask + done * ldmask, mbits, 1, ldmask, n, pn, m_d, ldp, c->stream));
    HIPCHK(launch_hist_panel(c, pl, p0, pn, bins, x_d, m_d, copies, total_d));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "the counters come down as they are");
  hipLaunchKernelGGL(theta_hist_finish_kernel, dim3((unsigned)((slots + 2 + 255) / 256)), dim3(256), 0, c->stream,
                     (const unsigned long long*)total_d, copies, (int)(slots + 2), sum_d);
  HIPCHK(hipGetLastError());
  int64_t nan[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(hist, sum_d, sizeof(int64_t) * slots, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(nan, sum_d + slots, sizeof nan, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (nan_count) nan_count[0] = nan[0], nan_count[1] = nan[1];
  return NBMF_OK;
}

// ---- Theta summed against data: expected counts by (row, column group) and by column (nbmf_moment_kernels.inc)
// nbmf_theta_hist_v's walk: per panel the caller's data and mask rows up into staging panels, then the fused
// product-and-sum kernel.  The panel's row table is zeroed before the launch and comes down after it; the column table
// (NBMF_MOMENT_COPIES copies of it -- environment; default 32, fewer where n is so large that they would pass 64 MiB --
// which theta_hist_finish_kernel adds up at the end) and the NaN counts stay on the device for the whole call.  The labels
// go up once, padded to nA entries with -1.  Integer adds: the panels need no alignment.
int nbmf_moment_rows_v(nbmf_ctx* c, int64_t row0, int64_t nrows, const void* x, int x_kind, int64_t ldx, const void* mask, int mask_kind,
                       int64_t ldmask, const int32_t* col_group, int groups, int64_t* row_tab, int64_t* col_tab, int64_t* nan_count) {
  if (int rc = predict_ready(c)) return rc;
  if (int rc = check_rows(c, row0, nrows)) return rc;
  if (nrows > (1ll << 30)) return fail(NBMF_ERR_ARG, "nrows must be at most 2^30 (got %lld)", (long long)nrows);
  if (groups < 1 || groups > NBMF_MOMENT_MAX_GROUPS)
    return fail(NBMF_ERR_ARG, "groups must be in [1, %d] (got %d)", NBMF_MOMENT_MAX_GROUPS, groups);
  if (x_kind != NBMF_DATA_U8 && x_kind != NBMF_DATA_BITS) return fail(NBMF_ERR_ARG, "unknown x_kind %d", x_kind);
  if (mask_kind != NBMF_MASK_NONE && mask_kind != NBMF_MASK_U8 && mask_kind != NBMF_MASK_BITS)
    return fail(NBMF_ERR_ARG, "unknown mask_kind %d", mask_kind);
  if (mask_kind != NBMF_MASK_NONE && !mask) return fail(NBMF_ERR_ARG, "mask_kind set but mask is NULL");
  if (mask_kind == NBMF_MASK_NONE) mask = nullptr;
  const bool xbits = x_kind == NBMF_DATA_BITS, mbits = mask_kind == NBMF_MASK_BITS;
  if (int rc = check_row_ld("ldx", ldx, xbits, c->n)) return rc;
  if (mask)
    if (int rc = check_row_ld("ldmask", ldmask, mbits, c->n)) return rc;
  if (!row_tab && !col_tab) return fail(NBMF_ERR_ARG, "no output requested");
  if (nrows > 0 && !x) return fail(NBMF_ERR_ARG, "null data");
  const long long n = c->n, ldp = panel_ld(c);
  if (col_group)
    for (long long j = 0; j < n; ++j)
      if (col_group[j] < -1 || col_group[j] >= groups)
        return fail(NBMF_ERR_ARG, "the group of column %lld is %d, outside [-1, %d)", j, (int)col_group[j], groups);
  static_assert(MO_FIELDS == NBMF_MOMENT_FIELDS && sizeof(int64_t) == sizeof(unsigned long long), "the tables come down as they are");
  const size_t row_words = (size_t)groups * MO_FIELDS, col_words = (size_t)n * MO_FIELDS;
  RowPanels pl;
  const size_t bit_bytes = (size_t)packed_ld(n) * ((xbits ? 1 : 0) + (mbits ? 1 : 0));   // the packed rows as they came
  const size_t per_row = (size_t)ldp * (mask ? 2 : 1) + bit_bytes + (row_tab ? sizeof(int64_t) * row_words : 0);
  if (int rc = plan_row_panels(c, "nbmf_moment_rows", row0, nrows, per_row, false, &pl)) return rc;
  if (col_tab) std::fill(col_tab, col_tab + (size_t)n * MO_FIELDS, (int64_t)0);   // (nrows == 0: nothing is read; the sums over no rows)
  if (nan_count) nan_count[0] = nan_count[1] = 0;
  if (nrows == 0) return NBMF_OK;
  if (int rc = set_device(c)) return rc;
  std::vector<int> labels((size_t)c->nA, -1);   // (the pad columns: in no group)
  for (long long j = 0; j < n; ++j) labels[(size_t)j] = col_group ? (int)col_group[j] : 0;
  const long long fit = std::max<long long>(1, (long long)((64ull << 20) / (sizeof(int64_t) * col_words)));
  const int copies = (int)std::min<long long>(fit, std::min<long long>(1024, std::max<long long>(1, env_int("NBMF_MOMENT_COPIES", 32))));
  PredictStage st{c->stream, {}};
  unsigned char *x_d = nullptr, *m_d = nullptr, *xbits_d = nullptr, *mbits_d = nullptr;
  int* grp_d = nullptr;
  unsigned long long *rtab_d = nullptr, *ctab_d = nullptr, *csum_d = nullptr, *nan_d = nullptr;
  HIPCHK(st.get(&x_d, (size_t)pl.stage_rows() * ldp));
  if (mask) HIPCHK(st.get(&m_d, (size_t)pl.stage_rows() * ldp));
  if (xbits) HIPCHK(st.get(&xbits_d, (size_t)pl.stage_rows() * packed_ld(n)));
  if (mbits) HIPCHK(st.get(&mbits_d, (size_t)pl.stage_rows() * packed_ld(n)));
  HIPCHK(st.get(&grp_d, sizeof(int) * labels.size()));
  HIPCHK(st.get(&nan_d, sizeof(unsigned long long) * 2));
  if (row_tab) HIPCHK(st.get(&rtab_d, sizeof(unsigned long long) * (size_t)pl.stage_rows() * row_words));
  if (col_tab) {
    HIPCHK(st.get(&ctab_d, sizeof(unsigned long long) * col_words * copies));
    HIPCHK(st.get(&csum_d, sizeof(unsigned long long) * col_words));
    HIPCHK(hipMemsetAsync(ctab_d, 0, sizeof(unsigned long long) * col_words * copies, c->stream));
  }
  HIPCHK(hipMemsetAsync(nan_d, 0, sizeof(unsigned long long) * 2, c->stream));
  HIPCHK(hipMemcpyAsync(grp_d, labels.data(), sizeof(int) * labels.size(), hipMemcpyHostToDevice, c->stream));
  for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    const size_t done = (size_t)(p0 - row0);
    HIPCHK(stage_rows_as_bytes(xbits_d, (const char*)x + done * ldx, xbits, 1, ldx, n, pn, x_d, ldp, c->stream));
    if (mask) HIPCHK(stage_rows_as_bytes(mbits_d, (const char*)mask + done * ldmask, mbits, 1, ldmask, n, pn, m_d, ldp, c->stream));
    if (row_tab) HIPCHK(hipMemsetAsync(rtab_d, 0, sizeof(unsigned long long) * (size_t)pn * row_words, c->stream));
    HIPCHK(launch_moment_panel(c, pl, p0, pn, groups, x_d, m_d, grp_d, rtab_d, copies, ctab_d, nan_d));
    if (row_tab)
      HIPCHK(hipMemcpyAsync(row_tab + done * row_words, rtab_d, sizeof(int64_t) * (size_t)pn * row_words, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  if (col_tab) {
    hipLaunchKernelGGL(theta_hist_finish_kernel, dim3((unsigned)((col_words + 255) / 256)), dim3(256), 0, c->stream,
                       (const unsigned long long*)ctab_d, copies, (int)col_words, csum_d);   // (n < 2^24: col_words fits an int)
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(col_tab, csum_d, sizeof(int64_t) * col_words, hipMemcpyDeviceToHost, c->stream));
  }
  int64_t nan[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(nan, nan_d, sizeof nan, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (nan_count) nan_count[0] = nan[0], nan_count[1] = nan[1];
  return NBMF_OK;
}

// ---- the best entries of Theta over a row range, as (row, column) pairs (nbmf_pairs_kernels.inc) ----------
// The operands go up once and stay staged for the whole call (no panels: every pass sees all rows).  Then a radix selection
// on the 64-bit key, PAIRS_DIGIT_BITS at a time from the top, each pass a fused product-and-count whose PAIRS_BINS counters
// come down to be scanned here; it ends as soon as the entries at or above the current bin's lower edge fit the candidate
// buffer (top plus a slack), which one collecting pass then fills and this function sorts.  Only where the passes run to
// the last digit and more entries equal the threshold key than the buffer holds does the tie pass run: the ties per row,
// the boundary row from their prefix sum, the boundary column from that one row's ties, and a collecting pass that takes
// exactly `top` entries.
struct PairsCall {
  nbmf_ctx* c;
  dim3 grid;
  long long row0, nrows, ldp;
  int clip, kind;
  const unsigned char *x_d, *m_d;
};

static unsigned long long host_pairs_key(double s, int kind) {   // pairs_key of an eligible entry, from its score
  if (s != s) return 0ull;
  unsigned long long k;
  if (s == 0.0) {
    k = 1ull << 63;
  } else {
    unsigned long long b;
    memcpy(&b, &s, sizeof b);
    k = (b >> 63) ? ~b : (b | (1ull << 63));
  }
  return kind == NBMF_PAIRS_LIKELIHOOD ? ~k : k;
}

// One collecting pass over the rows [p0, p0 + pn) of the request into the candidate arrays; *count = the entries taken.
static int pairs_collect(const PairsCall& pc, long long p0, long long pn, unsigned long long lo, unsigned long long T, long long rs,
                  long long cs, int row_only, unsigned long long cap, unsigned long long* counter_d, long long* rows_d,
                  long long* cols_d, double* scores_d, unsigned long long* count) {
  nbmf_ctx* c = pc.c;
  HIPCHK(hipMemsetAsync(counter_d, 0, sizeof(unsigned long long), c->stream));
  const dim3 grid((unsigned)RowPanels::blocks(p0, pn), pc.grid.y);
  hipLaunchKernelGGL(pairs_collect_kernel, grid, dim3(PR_WAVES * 64), 0, c->stream, (const double*)c->Wn, (const double*)c->Hn, c->k,
                     (long long)c->mA, (long long)c->nA, (long long)c->n, p0, pn, pc.row0, pc.ldp, pc.clip, pc.kind, pc.x_d, pc.m_d, lo,
                     T, rs, cs, row_only, cap, counter_d, rows_d, cols_d, scores_d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(count, counter_d, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (*count > cap) return fail(NBMF_ERR_HIP, "nbmf_top_pairs: %llu candidates for a buffer of %llu (internal error)", *count, cap);
  return NBMF_OK;
}

int nbmf_top_pairs(nbmf_ctx* c, int64_t row0, int64_t nrows, int64_t top, int clip_theta, int kind, const void* x, int x_kind,
                   int64_t ldx, const void* mask, int mask_kind, int64_t ldmask, int64_t* out_rows, int64_t* out_cols,
                   double* out_scores, int64_t* out_count) {
  if (int rc = predict_ready(c)) return rc;
  if (top < 1 || top > NBMF_TOP_PAIRS_MAX)
    return fail(NBMF_ERR_ARG, "top must be in [1, %d] (got %lld)", NBMF_TOP_PAIRS_MAX, (long long)top);
  if (int rc = check_rows(c, row0, nrows)) return rc;
  if (kind != NBMF_PAIRS_THETA && kind != NBMF_PAIRS_LIKELIHOOD) return fail(NBMF_ERR_ARG, "unknown kind %d", kind);
  if (x_kind != NBMF_DATA_U8 && x_kind != NBMF_DATA_BITS) return fail(NBMF_ERR_ARG, "unknown x_kind %d", x_kind);
  if (mask_kind != NBMF_MASK_NONE && mask_kind != NBMF_MASK_U8 && mask_kind != NBMF_MASK_BITS)
    return fail(NBMF_ERR_ARG, "unknown mask_kind %d", mask_kind);
  if (kind == NBMF_PAIRS_THETA && (mask_kind != NBMF_MASK_NONE || mask))
    return fail(NBMF_ERR_ARG, "NBMF_PAIRS_THETA takes an exclude matrix, not a mask");
  if (mask_kind != NBMF_MASK_NONE && !mask) return fail(NBMF_ERR_ARG, "mask_kind set but mask is NULL");
  if (mask_kind == NBMF_MASK_NONE) mask = nullptr;
  const bool xbits = x_kind == NBMF_DATA_BITS, mbits = mask_kind == NBMF_MASK_BITS;
  if (x)
    if (int rc = check_row_ld("ldx", ldx, xbits, c->n)) return rc;
  if (mask)
    if (int rc = check_row_ld("ldmask", ldmask, mbits, c->n)) return rc;
  if (!out_rows || !out_cols || !out_count) return fail(NBMF_ERR_ARG, "null output");
  if (kind == NBMF_PAIRS_LIKELIHOOD && nrows > 0 && !x) return fail(NBMF_ERR_ARG, "null data");
  *out_count = 0;
  if (nrows == 0) return NBMF_OK;
  if (int rc = set_device(c)) return rc;

  const long long n = c->n, ldp = panel_ld(c);
  const long long col_groups = (c->nA + PR_WAVES * PR_STRIP - 1) / (PR_WAVES * PR_STRIP);
  if (col_groups > 65535) return fail(NBMF_ERR_ARG, "n = %lld is beyond what nbmf_top_pairs launches", (long long)n);
  // the candidate buffer: `top` and a slack that lets the selection end early, and never less than one row (the boundary row's ties)
  // (NBMF_PAIRS_SLACK: the slack in entries, for tests -- 0 makes the selection run to the last digit and through the tie pass)
  const unsigned long long slack = (unsigned long long)std::min<long long>(
      1ll << 24, std::max<long long>(0, env_int("NBMF_PAIRS_SLACK", std::max<long long>(1ll << 16, (long long)top / 8))));
  const unsigned long long cap = std::max<unsigned long long>((unsigned long long)top + slack, (unsigned long long)ldp);
  const int copies = (int)std::min<long long>(1024, std::max<long long>(1, env_int("NBMF_HIST_COPIES", 64)));

  PredictStage st{c->stream, {}};
  unsigned char *x_d = nullptr, *m_d = nullptr, *xbits_d = nullptr, *mbits_d = nullptr;
  unsigned long long *total_d = nullptr, *sum_d = nullptr, *counter_d = nullptr, *ties_d = nullptr;
  long long *rows_d = nullptr, *cols_d = nullptr;
  double* scores_d = nullptr;
  const size_t panel_bytes = (size_t)nrows * ldp, bits_bytes = (size_t)nrows * packed_ld(n);
  const size_t need_bytes = panel_bytes * ((x ? 1 : 0) + (mask ? 1 : 0)) + bits_bytes * ((x && xbits ? 1 : 0) + (mask && mbits ? 1 : 0)) +
                            (size_t)cap * 24 + sizeof(unsigned long long) * PAIRS_BINS * ((size_t)copies + 1);
  {
    hipError_t e = hipSuccess;
    if (x) e = st.get(&x_d, panel_bytes);
    if (e == hipSuccess && mask) e = st.get(&m_d, panel_bytes);
    if (e == hipSuccess && x && xbits) e = st.get(&xbits_d, bits_bytes);
    if (e == hipSuccess && mask && mbits) e = st.get(&mbits_d, bits_bytes);
    if (e == hipSuccess) e = st.get(&rows_d, sizeof(long long) * (size_t)cap);
    if (e == hipSuccess) e = st.get(&cols_d, sizeof(long long) * (size_t)cap);
    if (e == hipSuccess) e = st.get(&scores_d, sizeof(double) * (size_t)cap);
    if (e == hipSuccess) e = st.get(&total_d, sizeof(unsigned long long) * PAIRS_BINS * (size_t)copies);
    if (e == hipSuccess) e = st.get(&sum_d, sizeof(unsigned long long) * PAIRS_BINS);
    if (e == hipSuccess) e = st.get(&counter_d, sizeof(unsigned long long));
    if (e != hipSuccess)
      return fail(NBMF_ERR_HIP,
                  "nbmf_top_pairs keeps its operands on the device for the whole call and the %.1f MiB it needs for %lld rows do not "
                  "fit (%s): ask for fewer rows per call and merge the results",
                  (double)need_bytes / (1 << 20), (long long)nrows, hipGetErrorString(e));
  }
  if (x) HIPCHK(stage_rows_as_bytes(xbits_d, x, xbits, 1, ldx, n, nrows, x_d, ldp, c->stream));
  if (mask) HIPCHK(stage_rows_as_bytes(mbits_d, mask, mbits, 1, ldmask, n, nrows, m_d, ldp, c->stream));

  const PairsCall pc{c, dim3((unsigned)RowPanels::blocks(row0, nrows), (unsigned)col_groups), row0, nrows, ldp, clip_theta != 0 ? 1 : 0,
                     kind, x_d, m_d};
  const long long NO_ROW = 0x7fffffffffffffffLL;

  // 1. select
  unsigned long long prefix = 0, fixed = 0, need = (unsigned long long)top, n_gt = 0, in_bin = 0;
  bool all = false, fits = false;
  int passes = 0;
  std::vector<unsigned long long> h(PAIRS_BINS);
  for (int shift = 64 - PAIRS_DIGIT_BITS; !all && !fits && fixed != ~0ull; shift = std::max(0, shift - PAIRS_DIGIT_BITS)) {
    const int bits = shift > 0 || passes == 0 ? PAIRS_DIGIT_BITS : 64 - passes * PAIRS_DIGIT_BITS;   // the last digit is what is left
    const int bins = 1 << bits;
    HIPCHK(hipMemsetAsync(total_d, 0, sizeof(unsigned long long) * PAIRS_BINS * (size_t)copies, c->stream));
    hipLaunchKernelGGL(pairs_digit_kernel, pc.grid, dim3(PR_WAVES * 64), 0, c->stream, (const double*)c->Wn, (const double*)c->Hn,
                       c->k, (long long)c->mA, (long long)c->nA, n, (long long)row0, (long long)nrows, (long long)row0, ldp, pc.clip,
                       kind, (const unsigned char*)x_d, (const unsigned char*)m_d, prefix, fixed, shift, bins, copies, total_d);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(theta_hist_finish_kernel, dim3((unsigned)((PAIRS_BINS + 255) / 256)), dim3(256), 0, c->stream,
                       (const unsigned long long*)total_d, copies, PAIRS_BINS, sum_d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h.data(), sum_d, sizeof(unsigned long long) * (size_t)bins, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    ++passes;
    unsigned long long above = 0;
    int d = bins - 1;
    for (; d >= 0 && above + h[d] < need; --d) above += h[d];   // from the best bin down
    if (d < 0) {   // (first pass only: fewer eligible entries than `top`) -- every one of them is taken
      all = true;
      n_gt = above;
      break;
    }
    n_gt += above;
    need -= above;
    in_bin = h[d];
    prefix |= (unsigned long long)d << shift;
    fixed |= (unsigned long long)(bins - 1) << shift;
    fits = n_gt + in_bin <= cap;
  }

  // 2. collect
  unsigned long long count = 0;
  bool tie_pass = false;
  if (all) {
    if (n_gt > 0)
      if (int rc = pairs_collect(pc, row0, nrows, 1ull, 1ull, NO_ROW, 0, 0, cap, counter_d, rows_d, cols_d, scores_d, &count)) return rc;
  } else if (fits) {   // everything at or above the bin's lower edge
    if (int rc = pairs_collect(pc, row0, nrows, prefix, prefix, NO_ROW, 0, 0, cap, counter_d, rows_d, cols_d, scores_d, &count)) return rc;
  } else {   // prefix is the threshold key T in full, and more entries equal it than the buffer holds
    tie_pass = true;
    const unsigned long long T = prefix;
    HIPCHK(st.get(&ties_d, sizeof(unsigned long long) * (size_t)nrows));
    HIPCHK(hipMemsetAsync(ties_d, 0, sizeof(unsigned long long) * (size_t)nrows, c->stream));
    hipLaunchKernelGGL(pairs_ties_kernel, pc.grid, dim3(PR_WAVES * 64), 0, c->stream, (const double*)c->Wn, (const double*)c->Hn, c->k,
                       (long long)c->mA, (long long)c->nA, n, (long long)row0, (long long)nrows, (long long)row0, ldp, pc.clip, kind,
                       (const unsigned char*)x_d, (const unsigned char*)m_d, T, ties_d);
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> ties((size_t)nrows);
    HIPCHK(hipMemcpyAsync(ties.data(), ties_d, sizeof(unsigned long long) * (size_t)nrows, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    long long r = 0;
    unsigned long long before = 0;
    for (; r < nrows && before + ties[(size_t)r] < need; ++r) before += ties[(size_t)r];
    if (r >= nrows) return fail(NBMF_ERR_HIP, "nbmf_top_pairs: the tie counts do not reach the threshold (internal error)");
    const long long rs = row0 + r;
    const unsigned long long kth = need - before;   // the boundary row gives its first kth ties (>= 1)
    if (int rc = pairs_collect(pc, rs, 1, T, T, rs, 0, 1, cap, counter_d, rows_d, cols_d, scores_d, &count)) return rc;
    if (count < kth) return fail(NBMF_ERR_HIP, "nbmf_top_pairs: the boundary row has too few ties (internal error)");
    std::vector<long long> tie_cols((size_t)count);
    HIPCHK(hipMemcpy(tie_cols.data(), cols_d, sizeof(long long) * (size_t)count, hipMemcpyDeviceToHost));
    std::nth_element(tie_cols.begin(), tie_cols.begin() + (size_t)(kth - 1), tie_cols.end());
    const long long cs = tie_cols[(size_t)(kth - 1)];
    if (int rc = pairs_collect(pc, row0, nrows, T, T, rs, cs, 0, cap, counter_d, rows_d, cols_d, scores_d, &count)) return rc;
  }
  if (env_set("NBMF_PAIRS_TRACE"))
    fprintf(stderr, "nbmf_top_pairs: top %lld rows %lld digit_passes %d tie_pass %d collected %llu device_bytes %zu\n", (long long)top,
            (long long)nrows, passes, tie_pass ? 1 : 0, count, need_bytes + (tie_pass ? sizeof(unsigned long long) * (size_t)nrows : 0));

  // 3. sort: key descending, then row, then column -- the arrival order of the candidates does not survive this
  struct Cand {
    unsigned long long key;
    long long row, col;
    double score;
  };
  std::vector<Cand> cand((size_t)count);
  if (count > 0) {
    std::vector<long long> hr((size_t)count), hc((size_t)count);
    std::vector<double> hs((size_t)count);
    HIPCHK(hipMemcpy(hr.data(), rows_d, sizeof(long long) * (size_t)count, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hc.data(), cols_d, sizeof(long long) * (size_t)count, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(hs.data(), scores_d, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    for (size_t q = 0; q < (size_t)count; ++q) cand[q] = Cand{host_pairs_key(hs[q], kind), hr[q], hc[q], hs[q]};
  }
  const auto first = [](const Cand& a, const Cand& b) {
    return a.key != b.key ? a.key > b.key : a.row != b.row ? a.row < b.row : a.col < b.col;
  };
  const size_t keep = (size_t)std::min<unsigned long long>((unsigned long long)top, count);
  if (keep < cand.size()) {
    std::nth_element(cand.begin(), cand.begin() + keep, cand.end(), first);
    cand.resize(keep);
  }
  std::sort(cand.begin(), cand.end(), first);
  for (size_t q = 0; q < keep; ++q) {
    out_rows[q] = cand[q].row;
    out_cols[q] = cand[q].col;
    if (out_scores) out_scores[q] = cand[q].score;
  }
  *out_count = (int64_t)keep;
  return NBMF_OK;
}

// ---- Theta ranked at given entries: where held-out columns stand in top_n's order (nbmf_rank_kernels.inc) ---
// Per panel: the product kernel of nbmf_predict_rows, unchanged, into the staging panel (as nbmf_top_n: a score is bit for
// bit the entry nbmf_predict_rows returns), the panel's slice of indptr and its range of indices up, the counting kernel,
// and the same range of every output that was asked for back: a few integers per target instead of n doubles per row.
// The target staging holds the most targets any one panel has, found from indptr before the loop.
int nbmf_rank_rows(nbmf_ctx* c, int64_t row0, int64_t nrows, int clip_theta, const int64_t* indptr, const int32_t* indices,
                   const uint8_t* exclude, int64_t ldx, int64_t* out_rank, int64_t* out_above, int64_t* out_tied, double* out_scores,
                   int64_t* out_eligible) {
  return nbmf_rank_rows_v(c, row0, nrows, clip_theta, indptr, indices, exclude, NBMF_DATA_U8, ldx, out_rank, out_above, out_tied,
                          out_scores, out_eligible);
}

int nbmf_rank_rows_v(nbmf_ctx* c, int64_t row0, int64_t nrows, int clip_theta, const int64_t* indptr, const int32_t* indices,
                     const void* exclude, int exclude_kind, int64_t ldx, int64_t* out_rank, int64_t* out_above, int64_t* out_tied,
                     double* out_scores, int64_t* out_eligible) {
  if (int rc = predict_ready(c)) return rc;
  if (int rc = check_rows(c, row0, nrows)) return rc;
  if (exclude_kind != NBMF_DATA_U8 && exclude_kind != NBMF_DATA_BITS) return fail(NBMF_ERR_ARG, "unknown exclude_kind %d", exclude_kind);
  const bool exbits = exclude_kind == NBMF_DATA_BITS;
  if (exclude)
    if (int rc = check_row_ld("ldx", ldx, exbits, c->n)) return rc;
  if (nrows == 0) return NBMF_OK;
  if (!out_rank && !out_above && !out_tied && !out_scores && !out_eligible) return fail(NBMF_ERR_ARG, "no output requested");
  if (!indptr) return fail(NBMF_ERR_ARG, "null indptr");
  if (indptr[0] < 0) return fail(NBMF_ERR_ARG, "indptr[0] = %lld is negative", (long long)indptr[0]);
  for (int64_t r = 0; r < nrows; ++r)
    if (indptr[r + 1] < indptr[r])
      return fail(NBMF_ERR_ARG, "indptr decreases at row %lld (%lld after %lld)", (long long)(row0 + r), (long long)indptr[r + 1],
                  (long long)indptr[r]);
  const long long n = c->n;
  const int64_t first = indptr[0], last = indptr[nrows];
  if (last > first && !indices) return fail(NBMF_ERR_ARG, "null indices");
  for (int64_t p = first; p < last; ++p)
    if (indices[p] < 0 || indices[p] >= n)
      return fail(NBMF_ERR_ARG, "target column %d at position %lld is outside [0, %lld)", (int)indices[p], (long long)p, n);
  if (int rc = set_device(c)) return rc;
  RowPanels pl;   // (the panel of nbmf_predict_rows, float64)
  const size_t exb = exclude && exbits ? (size_t)packed_ld(n) : 0;   // a packed exclude row's share of the staging
  if (int rc = plan_row_panels(c, "nbmf_rank_rows", row0, nrows, (size_t)panel_ld(c) * sizeof(double) + exb, false, &pl)) return rc;
  long long most = 1;   // targets of the fullest panel (1: no empty staging block)
  for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    most = std::max<long long>(most, indptr[p0 - row0 + pn] - indptr[p0 - row0]);
  }
  static_assert(sizeof(int64_t) == sizeof(long long), "indptr and the integer outputs travel as they are");
  const size_t rows = (size_t)pl.stage_rows();
  PredictStage st{c->stream, {}};
  double *panel_d = nullptr, *scores_d = nullptr;
  long long *indptr_d = nullptr, *rank_d = nullptr, *above_d = nullptr, *tied_d = nullptr, *elig_d = nullptr;
  int* indices_d = nullptr;
  unsigned char *ex_d = nullptr, *exbits_d = nullptr;
  HIPCHK(st.get(&panel_d, sizeof(double) * rows * pl.ldp));
  HIPCHK(st.get(&indptr_d, sizeof(long long) * (rows + 1)));
  HIPCHK(st.get(&indices_d, sizeof(int) * (size_t)most));
  if (out_rank) HIPCHK(st.get(&rank_d, sizeof(long long) * (size_t)most));
  if (out_above) HIPCHK(st.get(&above_d, sizeof(long long) * (size_t)most));
  if (out_tied) HIPCHK(st.get(&tied_d, sizeof(long long) * (size_t)most));
  if (out_scores) HIPCHK(st.get(&scores_d, sizeof(double) * (size_t)most));
  if (out_eligible) HIPCHK(st.get(&elig_d, sizeof(long long) * rows));
  if (exclude) HIPCHK(st.get(&ex_d, rows * n));
  if (exb) HIPCHK(st.get(&exbits_d, rows * exb));
  for (long long p0 = row0, pn; p0 < pl.end; p0 += pn) {
    pn = pl.rows_at(p0);
    const size_t done = (size_t)(p0 - row0);
    const long long base = indptr[done];
    const size_t cnt = (size_t)(indptr[done + pn] - base);   // <= most
    if (exclude)
      HIPCHK(stage_rows_as_bytes(exbits_d, (const char*)exclude + done * ldx, exbits, 1, ldx, n, pn, ex_d, n, c->stream));
    HIPCHK(hipMemcpyAsync(indptr_d, indptr + done, sizeof(long long) * (size_t)(pn + 1), hipMemcpyHostToDevice, c->stream));
    if (cnt) HIPCHK(hipMemcpyAsync(indices_d, indices + base, sizeof(int) * cnt, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_theta_panel(c, pl, c->Wn, (long long)c->mA, c->Hn, (long long)c->nA, p0, pn, NBMF_PREDICT_F64, clip_theta, 0.0,
                              panel_d));
    hipLaunchKernelGGL(rank_rows_kernel, dim3((unsigned)pn), dim3(RK_THREADS), 0, c->stream, (const double*)panel_d, pl.ldp, n,
                       (const unsigned char*)ex_d, n, (const long long*)indptr_d, (const int*)indices_d, base, rank_d, above_d,
                       tied_d, scores_d, elig_d);
    HIPCHK(hipGetLastError());
    if (cnt) {
      const size_t w64 = sizeof(int64_t) * cnt;
      if (out_rank) HIPCHK(hipMemcpyAsync(out_rank + base, rank_d, w64, hipMemcpyDeviceToHost, c->stream));
      if (out_above) HIPCHK(hipMemcpyAsync(out_above + base, above_d, w64, hipMemcpyDeviceToHost, c->stream));
      if (out_tied) HIPCHK(hipMemcpyAsync(out_tied + base, tied_d, w64, hipMemcpyDeviceToHost, c->stream));
      if (out_scores) HIPCHK(hipMemcpyAsync(out_scores + base, scores_d, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
    }
    if (out_eligible)
      HIPCHK(hipMemcpyAsync(out_eligible + done, elig_d, sizeof(int64_t) * (size_t)pn, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (the next panel reuses the staging)
  }
  return NBMF_OK;
}

int nbmf_comm_unique_id(void* id128) {
  if (!id128) return fail(NBMF_ERR_ARG, "null id");
  if (int rc = load_rccl()) return rc;
  NCCLCHK(g_rccl.GetUniqueId(id128));
  return NBMF_OK;
}

// Shared tail of the two comm-init entry points: exchange buffers for the chosen axis and the global
// quantities the update formulas need.
static int comm_finish_init(nbmf_ctx* c, int nranks, int rank, int shard_axis) {
  HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 8, c->stream));   // a stop flag left by an earlier run must not mute the exchanges below
  c->nranks = nranks;
  c->rank = rank;
  c->shard_axis = shard_axis;
  // row split: panels of the K x N exchange (see enqueue_iteration_rows).  Two panels (NBMF_OVERLAP=1)
  // hide half of the exchange but cost ~35 us per iteration in extra launches and a split W-pass (measured
  // with one rank, where there is nothing to hide); the break-even is an all-reduce of ~70 us, which cannot
  // be timed on a one-GPU box, so the default stays one panel.
  const bool two = c->panels_wanted ? c->panels_wanted == 2 : env_int("NBMF_OVERLAP", 0) != 0;
  c->npanel = (shard_axis == 0 && c->KS == 1 && c->chunksW >= 2 && two) ? 2 : 1;
  c->wsplit = c->npanel == 2 ? c->chunksW / 2 : c->chunksW;
  c->pc0[0] = 0;
  c->pc0[1] = c->npanel == 2 ? (long long)c->bW_host[c->wsplit] * 16 : c->nA;
  c->pc0[2] = c->nA;
  c->pbase[0] = 0;
  c->ll_index = 2 * (size_t)c->KP * c->pc0[1];
  c->pbase[1] = c->ll_index + 2;
  if (env_set("NBMF_DEBUG"))
    fprintf(stderr, "[nbmf] rank %d/%d axis %d: %d exchange panel(s), columns split at %lld of %lld, W-pass chunks %d + %d, %s\n",
            rank, nranks, shard_axis, c->npanel, c->pc0[1], (long long)c->nA, c->wsplit, c->chunksW - c->wsplit,
            c->comm ? "RCCL" : c->peer ? "peer (xGMI)" : "host transport");
  if (c->npanel == 2 && (c->comm || c->peer) && !c->stream2) {
    HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->evH, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->evF, hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&c->ev1, hipEventDisableTiming));
  }
  if (c->peer && shard_axis == 0) {
    // the slice of each panel's columns this rank reduces and updates, in 16-column blocks
    for (int p = 0; p < c->npanel; ++p) {
      const long long b_lo = c->pc0[p] / 16, nb = (c->pc0[p + 1] - c->pc0[p]) / 16;
      const long long b0 = nb * rank / nranks, b1 = nb * (rank + 1) / nranks;
      c->psl_c0[p] = 16 * (b_lo + b0);
      c->psl_wp[p] = 16 * (b1 - b0);
    }
  }
  if (shard_axis == 1 && !c->Qbuf) HIPCHK(dmalloc(&c->Qbuf, sizeof(double) * (size_t)c->KP * c->mA));
  // global observed count (the divisor of _solver.py:162) and, when the columns are split, the global
  // column count (the "/ n" of :54) and the per-row observed counts of the Duchi extension
  double h[2] = {c->n_obs, (double)c->n};
  HIPCHK(hipMemcpyAsync(c->sbuf, h, sizeof h, hipMemcpyHostToDevice, c->stream));
  if (int rc = all_reduce_inplace(c, c->sbuf, 2)) return rc;
  HIPCHK(hipMemcpyAsync(h, c->sbuf, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->n_obs_global = h[0];
  c->n_div_global = (shard_axis == 1) ? h[1] : (double)c->n;
  if (shard_axis == 1) {
    HIPCHK(hipMemsetAsync(c->rowcnt + c->m, 0, sizeof(double) * (size_t)(c->mA - c->m), c->stream));
    if (c->peer) {   // the peer exchange works on the arena only
      HIPCHK(hipMemcpyAsync(c->arena, c->rowcnt, sizeof(double) * (size_t)c->mA, hipMemcpyDeviceToDevice, c->stream));
      if (int rc = all_reduce_inplace(c, c->arena, (size_t)c->mA)) return rc;
      HIPCHK(hipMemcpyAsync(c->rowcnt, c->arena, sizeof(double) * (size_t)c->mA, hipMemcpyDeviceToDevice, c->stream));
    } else {
      if (int rc = all_reduce_inplace(c, c->rowcnt, (size_t)c->mA)) return rc;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  return NBMF_OK;
}

static int comm_check_args(nbmf_ctx* c, int nranks, int rank, int shard_axis) {
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(NBMF_ERR_ARG, "bad rank %d / nranks %d", rank, nranks);
  if (shard_axis != 0 && shard_axis != 1) return fail(NBMF_ERR_ARG, "shard_axis must be 0 (rows of Y) or 1 (columns of Y)");
  if (c->data_kind < 0) return fail(NBMF_ERR_STATE, "call nbmf_upload before attaching a communicator (global counts are reduced there)");
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "a communicator is already attached (nbmf_comm_detach first)");
  if (c->eval.count > 0) return fail(NBMF_ERR_STATE, "the context holds an eval set (nbmf_set_eval with count 0 first): held-out evaluation runs unsharded");
  return NBMF_OK;
}

int nbmf_comm_init(nbmf_ctx* c, const void* id128, int nranks, int rank, int shard_axis) {
  if (!c || !id128) return fail(NBMF_ERR_ARG, "null argument");
  if (int rc = comm_check_args(c, nranks, rank, shard_axis)) return rc;
  if (int rc = set_device(c)) return rc;
  if (int rc = load_rccl()) return rc;
  Uid uid;
  memcpy(uid.internal, id128, 128);
  NCCLCHK(g_rccl.CommInitRank(&c->comm, nranks, uid, rank));
  return comm_finish_init(c, nranks, rank, shard_axis);
}

int nbmf_comm_init_host(nbmf_ctx* c, nbmf_host_allreduce_fn fn, void* user, int nranks, int rank, int shard_axis) {
  if (!c || !fn) return fail(NBMF_ERR_ARG, "null argument");
  if (int rc = comm_check_args(c, nranks, rank, shard_axis)) return rc;
  if (int rc = set_device(c)) return rc;
  const size_t cnt = std::max<size_t>(2 * (size_t)c->KP * c->nA + 1, (size_t)c->KP * c->mA);
  if (!c->host_buf) {
    HIPCHK(hipHostMalloc((void**)&c->host_buf, cnt * sizeof(double), hipHostMallocDefault));
    c->host_buf_count = cnt;
  }
  c->host_reduce = fn;
  c->host_reduce_user = user;
  return comm_finish_init(c, nranks, rank, shard_axis);
}

// Cooperative cancellation from ANOTHER thread (the only entry point that may be called on a context while its owner is
// inside a call): the flag is sticky; what is already enqueued is cut short on the device by raising the run's own stop
// flag -- the word every kernel of an iteration (the exchange kernels included) looks at before it does anything, as after
// convergence -- through a stream of its own.  The owner's nbmf_run then returns NBMF_ERR_STATE ("cancelled").
int nbmf_cancel(nbmf_ctx* c) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  c->cancelled.store(1, std::memory_order_relaxed);
  int* flags = c->flags;
  if (!flags) return NBMF_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  static const int one = 1;
  hipError_t e = hipMemcpyAsync(flags, &one, sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  hipStreamDestroy(st);
  if (e != hipSuccess) return fail(NBMF_ERR_HIP, "nbmf_cancel: %s", hipGetErrorString(e));
  return NBMF_OK;
}

int nbmf_set_peer_timeout_ms(nbmf_ctx* c, double ms) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (!(ms >= 0.0)) return fail(NBMF_ERR_ARG, "timeout must be >= 0 ms");
  c->peer_timeout_ms = ms;
  return NBMF_OK;
}

int nbmf_set_exchange_panels(nbmf_ctx* c, int panels) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (panels < 0 || panels > 2) return fail(NBMF_ERR_ARG, "panels must be 0 (default), 1 or 2");
  c->panels_wanted = panels;
  return NBMF_OK;
}

int nbmf_comm_detach(nbmf_ctx* c) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (int rc = set_device(c)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->stream2) HIPCHK(hipStreamSynchronize(c->stream2));
  comm_release(c, /*recount=*/true);
  return NBMF_OK;
}

// What the attached transport ITSELF says about the job (as opposed to what the caller told it): for RCCL the
// communicator's own rank count and device (ncclCommCount / ncclCommCuDevice: -1 where this librccl lacks them), for the
// peer transport the number of arenas it has mapped (its own included) and how many of those it reaches over IPC or peer
// access -- i.e. outside this context's own device memory.
int nbmf_comm_info(nbmf_ctx* c, int* kind, int* nranks_seen, int* remote) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  int k = 0, n = 0, rem = 0;
  if (c->comm) {
    k = 1;
    n = -1;
    rem = -1;
    if (g_rccl.CommCount) NCCLCHK(g_rccl.CommCount(c->comm, &n));
    if (g_rccl.CommCuDevice) NCCLCHK(g_rccl.CommCuDevice(c->comm, &rem));
  } else if (c->peer) {
    k = 2;
    for (int j = 0; j < c->pv.nranks; ++j)
      if (c->pv.arena[j] && c->pv.flag[j]) {
        ++n;
        if (j != c->pv.rank) ++rem;
      }
  } else if (c->host_reduce) {
    k = 3;
    n = c->nranks;
    rem = c->nranks - 1;
  }
  if (kind) *kind = k;
  if (nranks_seen) *nranks_seen = n;
  if (remote) *remote = rem;
  return NBMF_OK;
}

// Arena layout in doubles (same on every rank for a given axis, because the unsplit extent is):
//   axis 0   X = [P1 | P2 | loglik .. 8]   HX = H' staging [KP][nA]   PR = 2 x prior partial pairs   SC = 64 scalars
//   axis 1   X = [Q (KP x mA) .. 8]        SC = 64 scalars
static void peer_layout(nbmf_ctx* c, int axis) {
  const long long fh = (long long)c->KP * c->nA, fw = (long long)c->KP * c->mA;
  if (axis == 0) {
    c->x_doubles = 2 * fh + 8;
    c->offHX = c->x_doubles;
    c->offPR = c->offHX + fh;
    c->offSC = c->offPR + 2LL * 2 * 2 * PEER_H_WGS * PEER_MAX_RANKS;   // [parity][panel][workgroup of every rank][2]
  } else {
    c->x_doubles = fw + 8;
    c->offHX = c->offPR = c->offSC = c->x_doubles;
  }
}

int nbmf_peer_export(nbmf_ctx* c, int shard_axis, void* handle) {
  if (!c || !handle) return fail(NBMF_ERR_ARG, "null argument");
  if (shard_axis != 0 && shard_axis != 1) return fail(NBMF_ERR_ARG, "shard_axis must be 0 or 1");
  if (is_sharded(c)) return fail(NBMF_ERR_STATE, "a communicator is already attached (nbmf_comm_detach first)");
  if (int rc = set_device(c)) return rc;
  // Epochs restart at zero on all ranks together: arena and flag block are cleared on every export (the
  // ranks synchronise on the handle exchange before anyone signals).  The memory comes from the process-wide
  // pool and keeps its IPC handles for the life of the process.
  if (!c->arena || c->arena_axis != shard_axis) {
    arena_release((ArenaSlot*)c->arena_slot.p);
    c->arena_slot.p = nullptr;
    c->arena = nullptr;
    c->pflags = nullptr;
    peer_layout(c, shard_axis);
    ArenaSlot* slot = nullptr;
    if (int rc = arena_acquire(c->device, (size_t)(c->offSC + 64), &slot)) return rc;
    c->arena_slot.p = slot;
    c->arena = slot->arena;
    c->pflags = slot->flags;
    c->arena_doubles = slot->doubles;
    c->arena_axis = shard_axis;
  }
  HIPCHK(hipMemset(c->arena, 0, c->arena_doubles * sizeof(double)));
  HIPCHK(hipMemset(c->pflags, 0, PF_WORDS * sizeof(unsigned long long)));
  HIPCHK(hipDeviceSynchronize());
  c->epoch = 0;
  c->hseq = 0;
  memcpy(handle, ((ArenaSlot*)c->arena_slot.p)->handles, NBMF_PEER_HANDLE_BYTES);
  return NBMF_OK;
}

int nbmf_comm_init_peer(nbmf_ctx* c, const void* handles, int nranks, int rank, int shard_axis) {
  if (!c || !handles) return fail(NBMF_ERR_ARG, "null argument");
  if (int rc = comm_check_args(c, nranks, rank, shard_axis)) return rc;
  if (nranks > PEER_MAX_RANKS) return fail(NBMF_ERR_ARG, "the peer transport supports at most %d ranks", PEER_MAX_RANKS);
  if (!c->arena || c->arena_axis != shard_axis)
    return fail(NBMF_ERR_STATE, "call nbmf_peer_export(ctx, %d, ...) on every rank first", shard_axis);
  if (shard_axis == 0 && c->nA / 16 < nranks) return fail(NBMF_ERR_ARG, "too few columns to slice the H-step over %d ranks", nranks);
  if (int rc = set_device(c)) return rc;
  PeerView pv{};
  pv.nranks = nranks;
  pv.rank = rank;
  double ms = std::max(1.0, env_double("NBMF_PEER_TIMEOUT_MS", 30000.0));
  if (c->peer_timeout_ms > 0) ms = c->peer_timeout_ms;
  pv.timeout = (unsigned long long)(ms * 1e5);   // wall_clock64 ticks at 100 MHz
  struct Undo {   // any failure below leaves the context unattached
    nbmf_ctx* c;
    bool armed = true;
    ~Undo() {
      if (armed) {
        hipStreamSynchronize(c->stream);
        comm_release(c, /*recount=*/true);
      }
    }
  } undo{c};
  for (int j = 0; j < nranks; ++j) {
    if (j == rank) {
      pv.arena[j] = c->arena;
      pv.flag[j] = c->pflags;
      continue;
    }
    hipIpcMemHandle_t h[2];
    PeerOrigin origin;
    memcpy(h, (const char*)handles + (size_t)j * NBMF_PEER_HANDLE_BYTES, sizeof h);
    memcpy(&origin, (const char*)handles + (size_t)j * NBMF_PEER_HANDLE_BYTES + sizeof h, sizeof origin);
    if (origin.pid == process_nonce()) {
      // a rank of THIS process (several contexts, one host thread each): its arena is plain device memory here;
      // if it lives on another GPU of this process, peer access makes it addressable (pooled arenas are never freed,
      // so the address stays valid for the life of the process)
      if (origin.device != c->device) {
        const hipError_t e = hipDeviceEnablePeerAccess(origin.device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
          return fail(NBMF_ERR_HIP, "hipDeviceEnablePeerAccess(%d) from device %d: %s", origin.device, c->device, hipGetErrorString(e));
        (void)hipGetLastError();
      }
      pv.arena[j] = (double*)origin.arena;
      pv.flag[j] = (unsigned long long*)origin.flags;
      continue;
    }
    void *a = nullptr, *f = nullptr;
    HIPCHK(hipIpcOpenMemHandle(&a, h[0], hipIpcMemLazyEnablePeerAccess));
    c->peer_mapped.push_back(a);
    HIPCHK(hipIpcOpenMemHandle(&f, h[1], hipIpcMemLazyEnablePeerAccess));
    c->peer_mapped.push_back(f);
    pv.arena[j] = (double*)a;
    pv.flag[j] = (unsigned long long*)f;
  }
  c->pv = pv;
  c->peer = true;
  c->Pbuf_own = c->Pbuf;
  c->sbuf_own = c->sbuf;
  c->Qbuf_own = c->Qbuf;
  c->Pbuf = c->arena;
  c->Qbuf = c->arena;
  c->sbuf = c->arena + c->offSC;
  if (shard_axis == 0) {
    // column slices of the fused H-step, in 16-column blocks
    const long long nb = c->nA / 16;
    const long long b0 = nb * rank / nranks, b1 = nb * (rank + 1) / nranks;
    c->sl_c0 = 16 * b0;
    c->sl_wp = 16 * (b1 - b0);
  }
  // Known-answer exchanges before anything depends on the transport (also the first rendezvous of the ranks):
  // rank r contributes (r+1)*((i+7t)%1021+1)+t, all exact in binary64; FOUR epochs are queued back to back, each
  // filling, reducing and checking on the device with no host synchronisation in between, so the arena and the
  // flag words are reused exactly as consecutive iterations of a run reuse them.
  {
    const long long cnt = std::min<long long>(c->x_doubles, 1 << 20);
    const unsigned long long full = c->pv.timeout;
    c->pv.timeout = std::min<unsigned long long>(full, 10ull * 100000000ull);
    unsigned long long* bad = c->stats + 4;
    // (the exchange kernels return at once while the run's stop flag is up -- and a run that ended by its stop rule
    //  leaves it up: clear it, or the known-answer epochs of a re-attach find nothing exchanged)
    HIPCHK(hipMemsetAsync(c->flags, 0, sizeof(int) * 8, c->stream));
    HIPCHK(hipMemsetAsync(bad, 0, sizeof(unsigned long long), c->stream));
    for (int t = 0; t < 4; ++t) {
      hipLaunchKernelGGL(peer_selftest_fill_kernel, dim3(256), dim3(256), 0, c->stream, c->arena, cnt, rank, t);
      HIPCHK(hipGetLastError());
      if (int rc = all_reduce_inplace(c, c->arena, (size_t)cnt)) return rc;
      hipLaunchKernelGGL(peer_selftest_check_kernel, dim3(256), dim3(256), 0, c->stream, (const double*)c->arena, cnt, nranks, t, bad);
      HIPCHK(hipGetLastError());
    }
    unsigned long long n_bad = 0;
    HIPCHK(hipMemcpyAsync(&n_bad, bad, sizeof n_bad, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (int rc = peer_check(c)) return rc;
    if (n_bad) return fail(NBMF_ERR_COMM, "peer transport self-test failed: %llu wrong elements over four back-to-back exchanges", n_bad);
    c->pv.timeout = full;
    HIPCHK(hipMemsetAsync(c->arena, 0, (size_t)cnt * sizeof(double), c->stream));
  }
  if (int rc = comm_finish_init(c, nranks, rank, shard_axis)) return rc;
  if (int rc = peer_check(c)) return rc;
  undo.armed = false;
  return NBMF_OK;
}

int nbmf_timing_enable(nbmf_ctx* c, int enable) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  c->timing = enable != 0;
  c->timing_stride = enable > 1 ? enable : 1;
  c->timing_it = 0;
  c->ev_used = 0;
  c->t_ms[0] = c->t_ms[1] = 0;
  c->t_n[0] = c->t_n[1] = 0;
  return NBMF_OK;
}

int nbmf_timing_get(nbmf_ctx* c, double* hpass_ms, int* hpass_launches, double* wpass_ms, int* wpass_launches) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (hpass_ms) *hpass_ms = c->t_ms[0];
  if (hpass_launches) *hpass_launches = c->t_n[0];
  if (wpass_ms) *wpass_ms = c->t_ms[1];
  if (wpass_launches) *wpass_launches = c->t_n[1];
  return NBMF_OK;
}

int nbmf_set_progress(nbmf_ctx* c, nbmf_progress_fn fn, void* user, int every) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (fn && every < 1) return fail(NBMF_ERR_ARG, "every must be >= 1");
  c->progress = fn;
  c->progress_user = user;
  c->progress_every = fn ? every : 0;
  return NBMF_OK;
}

int nbmf_small_stats(nbmf_ctx* c, int* runs, int* aborted) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (runs) *runs = c->small.runs;
  if (aborted) *aborted = c->small.aborted;
  return NBMF_OK;
}

int nbmf_device_synchronize(int device) {
  if (device < 0) return fail(NBMF_ERR_ARG, "device index must be >= 0");   // (before anything touches the runtime)
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipDeviceSynchronize());
  return NBMF_OK;
}

int nbmf_synchronize(nbmf_ctx* c) {
  if (!c) return fail(NBMF_ERR_ARG, "null context");
  if (int rc = set_device(c)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return NBMF_OK;
}

int nbmf_selftest_unary(int device, int op, int n, const double* x, double* y) {
  if (!x || !y || n < 1 || op < 0 || op > 7) return fail(NBMF_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(device));
  const double2* ltab10 = nullptr;
  HIPCHK(log_table_build(device, nullptr));   // (a self-test entry, no context: the null stream)
  HIPCHK(log_table_device(&ltab10));
  double *d = nullptr, *o = nullptr;
  HIPCHK(dmalloc(&d, sizeof(double) * (size_t)n));
  HIPCHK(dmalloc(&o, sizeof(double) * (size_t)n));
  HIPCHK(hipMemcpy(d, x, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(unary_test_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, d, o, n, ltab10);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(y, o, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
  dfree(d);
  dfree(o);
  return NBMF_OK;
}

// unpack_bits_kernel on the caller's arrays (a test hook): `out` goes up whole, the kernel runs over it, and it comes back
// whole, so a test sees every byte the kernel did not write.  All checks come before the first device call.
int nbmf_selftest_unpack_bits(int device, const uint8_t* bits, int64_t ldbits, int64_t rows, int64_t n, uint8_t* out, int64_t ldout) {
  if (!bits || !out) return fail(NBMF_ERR_ARG, "null bits or out");
  if (rows < 0 || n < 0) return fail(NBMF_ERR_ARG, "rows and n must be >= 0 (got %lld and %lld)", (long long)rows, (long long)n);
  if (ldbits < packed_ld(n))
    return fail(NBMF_ERR_ARG, "ldbits %lld is less than ceil(n / 8) = %lld", (long long)ldbits, (long long)packed_ld(n));
  if (ldout < n) return fail(NBMF_ERR_ARG, "ldout %lld is less than n = %lld", (long long)ldout, (long long)n);
  if (rows == 0 || n == 0) return NBMF_OK;
  HIPCHK(hipSetDevice(device));
  // (bits ends with the last byte of its last row; out is rows x ldout bytes, all of them the caller's)
  const size_t bits_bytes = (size_t)(rows - 1) * ldbits + (size_t)packed_ld(n), out_bytes = (size_t)rows * ldout;
  PredictStage st{nullptr, {}};   // (a self-test entry, no context: the null stream)
  unsigned char *bits_d = nullptr, *out_d = nullptr;
  HIPCHK(st.get(&bits_d, bits_bytes));
  HIPCHK(st.get(&out_d, out_bytes));
  HIPCHK(hipMemcpy(bits_d, bits, bits_bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(out_d, out, out_bytes, hipMemcpyHostToDevice));
  HIPCHK(launch_unpack_bits(bits_d, ldbits, rows, n, out_d, ldout, nullptr));
  HIPCHK(hipMemcpy(out, out_d, out_bytes, hipMemcpyDeviceToHost));
  return NBMF_OK;
}

int nbmf_engine_stats(long long* persistent_served, long long* persistent_aborted, long long* launches_served) {
  if (persistent_served) *persistent_served = g_engine_persistent_served.load(std::memory_order_relaxed);
  // (a fit declined because the context's kernel gave up earlier counts as given up: it ran on the other engine)
  if (persistent_aborted)
    *persistent_aborted = g_engine_persistent_aborted.load(std::memory_order_relaxed) + g_engine_persistent_declined.load(std::memory_order_relaxed);
  if (launches_served) *launches_served = g_engine_launches_served.load(std::memory_order_relaxed);
  return NBMF_OK;
}

int nbmf_selftest_mfma_peak(int device, double target_ms, double* tflops, double* cycles_per_mfma, double* launch_ms) {
  if (!(target_ms > 0.0 && target_ms <= 2000.0)) return fail(NBMF_ERR_ARG, "target_ms must be in (0, 2000]");
  HIPCHK(hipSetDevice(device));
  DevInfo di;
  HIPCHK(device_info(device, &di));
  if (!di.gfx950) return fail(NBMF_ERR_HIP, "device %d is %s, not gfx950", device, di.arch);
  const int wgs = di.cus * 2;   // 4 waves each: two waves per SIMD (one does as well: the pipe is the limit)
  double* out = nullptr;
  HIPCHK(dmalloc(&out, sizeof(double) * (size_t)wgs * 256));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  struct Cleanup {   // (every return below, the HIPCHK ones included, frees what has been made)
    double*& out;
    hipEvent_t &e0, &e1;
    ~Cleanup() {
      if (e0) hipEventDestroy(e0);
      if (e1) hipEventDestroy(e1);
      if (out) dfree(out);
    }
  } cleanup{out, e0, e1};
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  auto timed = [&](int iters, float* ms) -> hipError_t {
    hipError_t e;
    if ((e = hipEventRecord(e0, 0)) != hipSuccess) return e;
    hipLaunchKernelGGL(mfma_peak_kernel, dim3(wgs), dim3(256), 0, 0, out, iters, 1.0, 0.5);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipEventRecord(e1, 0)) != hipSuccess) return e;
    if ((e = hipEventSynchronize(e1)) != hipSuccess) return e;
    return hipEventElapsedTime(ms, e0, e1);
  };
  // a trip is 8 MFMAs of 64 cycles on each of two waves of a SIMD: ~0.43 us at 2.4 GHz.  Warm up and calibrate with a
  // short launch, then one launch of about target_ms (long enough for the power management to act).
  float ms = 0;
  hipError_t e = timed(2000, &ms);
  if (e == hipSuccess) e = timed(2000, &ms);
  int iters = 2000;
  if (e == hipSuccess) {
    iters = (int)std::min(4.0e6, std::max(2000.0, 2000.0 * target_ms / std::max((double)ms, 1e-3)));
    e = timed(iters, &ms);
  }
  if (e != hipSuccess) return fail(NBMF_ERR_HIP, "MFMA peak self-test failed: %s", hipGetErrorString(e));
  const double mfmas_per_simd = 2.0 * 8.0 * (double)iters;                    // two waves per SIMD
  const double flop = (double)wgs * 4.0 * 8.0 * (double)iters * 2048.0;       // 16 x 16 x 4 multiply-adds per MFMA and wave
  if (tflops) *tflops = flop / ((double)ms * 1e-3) * 1e-12;
  if (cycles_per_mfma) *cycles_per_mfma = (double)ms * 1e-3 * 2.4e9 / mfmas_per_simd;
  if (launch_ms) *launch_ms = ms;
  return NBMF_OK;
}

}  // extern "C"

