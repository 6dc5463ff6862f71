// nbmf_predict_kernels.inc -- Theta = W^T H handed back to the caller (nbmf_predict_at, nbmf_predict_rows; DESIGN.md 4.6)
// and ranked on the device (nbmf_top_n: top_n_kernel at the end of this file; DESIGN.md 4.7); and THETA_TILE, the 16 x 64
// strip of Theta that predict_rows_kernel here and score_rows_kernel (nbmf_score_kernels.inc; DESIGN.md 4.8) both open with.
// Included by nbmf_hip.hip after the other kernel files, before nbmf_score_kernels.inc.  The kernels that form products
// read the natural padded factor images Wn[k * mA + i], Hn[k * nA + j] (what get_factor_kernel reads) and nothing else of
// the context; none relies on what the images hold in rows k >= K or in columns beyond m / n: components k >= K are
// replaced by exact zeros in registers, and pad rows / columns of a tile only reach results that are never stored.

constexpr int PR_WAVES = 4;          // waves per workgroup of predict_rows_kernel: 4 strips of 64 columns, one 16-row tile
constexpr int PR_STRIP = 64;         // columns per wave: four 16-column MFMA tiles on four accumulators
constexpr int PA_LANES = 8;          // lanes that share one pair in predict_at_kernel
constexpr int PT_TILE = 32;          // k_major_kernel: 32 x 32 transpose tiles
constexpr int TN_THREADS = 256;      // top_n_kernel: one workgroup per panel row, 256 columns per ordered chunk
constexpr int TN_MAX = 256;          // most slots per row (NBMF_TOP_N_MAX): what the LDS entry list holds

// The 16 x 64 strip of Theta = W^T H that one wave of a product kernel owns: what predict_rows_kernel and score_rows_kernel
// (nbmf_score_kernels.inc) have in common, written once, so that the Theta one of them scores is the Theta the other
// stores by construction.  The strip is rows i0 .. i0+15 on the image's 16-grid (blockIdx.x counts 16-row tiles from the
// one that holds prow0) and columns j0 .. j0+63 (blockIdx.y, wave).  A wave whose strip starts at or beyond column JEND
// (<= nA) leaves the kernel at once -- a whole wave, and no product kernel has a barrier.  What follows the macro is the
// kernel's epilogue, which finds lr = l >> 4, lc = l & 15, i0, j0, jc = j0 + 4 lc and the finished accumulators acc[4].
// A statement macro (as STAGE_DMA and MASKS_REQUEST of the sweeps), not a function: the tile is then the same statements
// in both kernels, and the compiler's output for them is instruction for instruction what it was when each kernel
// spelled them out (a function filling or returning acc changed the register assignment, by reference the counts too).
//
// The four MFMA tiles of a strip are INTERLEAVED over it -- column c of tile t is j0 + 4c + t -- so that
//   - the four B operands of a lane are 4 consecutive doubles of one row of Hn: one 32-byte load, 512 contiguous bytes
//     per group of 16 lanes (A: Wn[(k0 + (l >> 4)) * mA + i0 + (l & 15)], 128 contiguous bytes per group);
//   - result register r of a lane holds Theta[i0 + (l >> 4) + 4r, jc + t] for t = 0..3 (the f64 C/D map: row =
//     (l >> 4) + 4r, column = l & 15): 4 consecutive entries of one row, which an epilogue stores, or reads data for, as
//     one 32-byte (doubles) or one 4-byte (bytes) access -- 512 resp. 64 contiguous bytes per row and instruction.
// The k blocks are added in ascending order, one chain per tile: an entry's value depends on its row, its column and the
// factors only, not on the kernel, the panel or the request it was computed in.  Lanes whose k is >= K supply 0.0 to both
// operands (the loop stops at the first multiple of 4 >= K, which is <= KP: no row of the images beyond KP is read).
#define THETA_TILE(Wn, Hn, K, mA, nA, prow0, JEND)                                                                    \
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                                         \
  const int lr = lane >> 4, lc = lane & 15;                                                                           \
  const long long i0 = ((prow0) / 16 + blockIdx.x) * 16; /* < mA: the host sizes the grid */                          \
  const long long j0 = ((long long)blockIdx.y * PR_WAVES + wave) * PR_STRIP;                                          \
  if (j0 >= (JEND)) return;                                                                                           \
  const long long jc = j0 + 4 * lc; /* this lane's four columns: jc .. jc+3 (< nA, a multiple of 128) */              \
  d4 acc[4];                                                                                                          \
  _Pragma("unroll") for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};                                      \
  for (int k0 = 0; k0 < (K); k0 += 4) {                                                                               \
    const int k = k0 + lr;                                                                                            \
    double a = 0.0;                                                                                                   \
    d4 b = d4{0.0, 0.0, 0.0, 0.0};                                                                                    \
    if (k < (K)) {                                                                                                    \
      a = (Wn)[(size_t)k * (mA) + i0 + lc];                                                                           \
      b = *(const d4*)((Hn) + (size_t)k * (nA) + jc);                                                                 \
    }                                                                                                                 \
    _Pragma("unroll") for (int t = 0; t < 4; ++t) acc[t] = NBMF_MFMA(a, b[t], acc[t], 0, 0, 0);                       \
  }

// Rows [prow0, prow0 + pnrows) of Theta, all n columns, into a staging panel whose row 0 is row prow0 and whose leading
// dimension ldd is a multiple of 4 (doubles for OUT_U8 == 0, bytes otherwise): the tile, then a lane's 4 x 4 entries
// clipped, compared where bytes are asked for, and stored where their row is inside the panel.
template <int OUT_U8>
__global__ __launch_bounds__(PR_WAVES * 64) void predict_rows_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long prow0,
    long long pnrows, long long ldd, int clip, double threshold, void* __restrict__ out) {
  THETA_TILE(Wn, Hn, K, mA, nA, prow0, nA)

  if (jc >= ldd) return;   // ldd is a multiple of 4: jc .. jc+3 are inside the panel's row or all outside
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long prow = i0 + lr + 4 * r - prow0;
    if (prow < 0 || prow >= pnrows) continue;
    double v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      v[t] = acc[t][r];
      if (clip) v[t] = v[t] < 0.0 ? 0.0 : (v[t] > 1.0 ? 1.0 : v[t]);   // np.clip: a NaN stays a NaN
    }
    if (OUT_U8) {
      uint32_t w = 0;
#pragma unroll
      for (int t = 0; t < 4; ++t) w |= (v[t] > threshold ? 1u : 0u) << (8 * t);
      *(uint32_t*)((unsigned char*)out + (size_t)prow * ldd + jc) = w;
    } else {
      *(d4*)((double*)out + (size_t)prow * ldd + jc) = d4{v[0], v[1], v[2], v[3]};
    }
  }
}

// Natural padded [.][lenA] -> k-major true-size [len][K]: dst[x * K + k] = Fn[k * lenA + x], through a 32 x 33 LDS tile so
// that both sides move whole rows.  Made once per nbmf_predict_at call for each factor: a pair's K operands are then
// K consecutive doubles instead of K doubles lenA apart.
__global__ __launch_bounds__(PT_TILE * 8) void k_major_kernel(const double* __restrict__ Fn, double* __restrict__ dst, int K,
                                                              long long len, long long lenA) {
  __shared__ double tile[PT_TILE][PT_TILE + 1];
  const int tx = threadIdx.x & (PT_TILE - 1), ty = threadIdx.x / PT_TILE;
  const long long x0 = (long long)blockIdx.x * PT_TILE;
  const int k0 = blockIdx.y * PT_TILE;
#pragma unroll
  for (int r = 0; r < PT_TILE; r += 8) {
    const int k = k0 + ty + r;
    const long long x = x0 + tx;
    tile[ty + r][tx] = (k < K && x < len) ? Fn[(size_t)k * lenA + x] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < PT_TILE; r += 8) {
    const long long x = x0 + ty + r;
    const int k = k0 + tx;
    if (x < len && k < K) dst[(size_t)x * K + k] = tile[tx][ty + r];
  }
}

// Theta at one index pair, from the k-major copies: sum_k Wk[i * K + k] * Hk[j * K + k].  PA_LANES consecutive lanes share
// the pair: lane q adds the products of k = q, q + 8, q + 16, ... in ascending order (consecutive lanes read consecutive
// doubles), then the 8 partial sums are folded by the xor butterfly 4, 2, 1 -- a fixed order, so the value at (i, j)
// depends on (i, j) and the factors only, and every lane of the pair ends with it.  A pair that is not `live` loads
// nothing and yields 0; all 64 lanes of the wave must call.  predict_at_kernel and eval_pairs_kernel
// (nbmf_eval_kernels.inc) both take their Theta from here: the same bits by construction.
__device__ __forceinline__ double theta_at_pair(const double* __restrict__ Wk, const double* __restrict__ Hk, int K,
                                                long long i, long long j, int q, bool live) {
  double s = 0.0;
  if (live) {
    const double* __restrict__ w = Wk + (size_t)i * K;
    const double* __restrict__ h = Hk + (size_t)j * K;
    for (int k = q; k < K; k += PA_LANES) s = __builtin_fma(w[k], h[k], s);
  }
#pragma unroll
  for (int off = PA_LANES / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  return s;
}

// out[t] = theta_at_pair(rows[t], cols[t]) for the `count` pairs of one chunk (Wk, Hk: k_major_kernel).
// A pair whose row is outside [0, m) or whose column is outside [0, n) is never used for an address: its lanes load
// nothing, its output is 0, and the lowest such position (base + t) is left in *bad_pos by an atomicMin.
__global__ __launch_bounds__(256) void predict_at_kernel(const double* __restrict__ Wk, const double* __restrict__ Hk, int K,
                                                         long long m, long long n, const long long* __restrict__ rows,
                                                         const long long* __restrict__ cols, long long count, long long base,
                                                         int clip, unsigned long long* bad_pos, double* __restrict__ out) {
  const long long t = ((long long)blockIdx.x * blockDim.x + threadIdx.x) / PA_LANES;
  const int q = threadIdx.x & (PA_LANES - 1);
  bool live = t < count;
  long long i = 0, j = 0;
  if (live) {
    i = rows[t];
    j = cols[t];
    if (i < 0 || i >= m || j < 0 || j >= n) {
      live = false;
      if (q == 0) atomicMin(bad_pos, (unsigned long long)(base + t));
    }
  }
  double s = theta_at_pair(Wk, Hk, K, i, j, q, live);
  if (t < count && q == 0) {
    if (clip) s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    out[t] = s;
  }
}

// ---- the top columns of every panel row (nbmf_top_n; DESIGN.md 4.7) ----------------------------------------------------
// The order-preserving 64-bit key of one panel entry: a larger Theta has a larger key, equal Thetas have equal keys
// (-0.0 and +0.0 compare equal, so they share one), and 0 is the key of an entry that may not be chosen: an excluded
// one or a NaN.  No finite or infinite value maps to 0 (the smallest key, that of -inf, is 0x000fffffffffffff).
__device__ __forceinline__ unsigned long long top_n_key(double v, bool skip) {
  if (skip || v != v) return 0ull;
  if (v == 0.0) return 1ull << 63;
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// One workgroup per row of the staging panel predict_rows_kernel<0> has just written (row stride ldd doubles, n real
// columns; ex: one byte per entry, row stride ldx, nonzero = skip, or null).  Slot s < top of the row's output gets the
// column with the s-th largest Theta among the eligible ones -- ties to the lower column -- and its Theta, read back from
// the panel; slots beyond the last eligible column get -1 and NaN.  out_cols / out_scores (may be null) are dense,
// `top` entries per row.  Only columns j < n are ever read: what the panel holds in its pad columns does not matter.
//
//   1. select: eight passes over the row, 8 bits of the key at a time from the top.  Each pass counts, in a 256-bin LDS
//      histogram (integer atomics: a count does not depend on the order), the keys that carry the digits found so far,
//      and wave 0 scans the bins from the highest down to the one in which the running count reaches what is still
//      needed.  The end is the key T of the last entry that gets a slot, and how many entries equal to T do (n_eq); the
//      n_gt entries above T all do.  A row with fewer than `top` nonzero keys takes every one of them (T = 0).
//   2. collect: one pass in ascending chunks of 256 columns with a workgroup prefix count per chunk (ballots inside a
//      wave, wave totals through LDS), so that the entries equal to T that are taken are the n_eq FIRST ones in column
//      order: the tie rule.  Entry lists in LDS: keys above T in slots [0, n_gt), the ties in [n_gt, n_gt + n_eq).
//   3. sort: a bitonic network over the smallest power of two >= top, key descending, then column ascending.
// LDS: 1 KiB of bins, 3 KiB of entries and a few counters, whatever n is.  Every branch around a barrier is uniform.
//
// SELF = 0 is nbmf_top_n's kernel (`self` is not read).  SELF = 1 is nbmf_neighbors' (nbmf_neighbors_kernels.inc; DESIGN.md
// 4.16): column self[row] of the row is ineligible -- by index, whatever its value -- on top of the rest: the key of that
// one entry is 0, and everything downstream is the same statements.
template <int SELF>
__global__ __launch_bounds__(TN_THREADS) void top_n_kernel(const double* __restrict__ panel, long long ldd, long long n,
                                                           const unsigned char* __restrict__ ex, long long ldx, int top,
                                                           long long* __restrict__ out_cols, double* __restrict__ out_scores,
                                                           const long long* __restrict__ self) {
  __shared__ unsigned long long ent_key[TN_MAX];
  __shared__ int ent_col[TN_MAX];
  __shared__ unsigned int hist[256];
  __shared__ unsigned int wave_cnt[2][TN_THREADS / 64][2];
  __shared__ unsigned int sel[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* __restrict__ row = panel + (size_t)blockIdx.x * ldd;
  const unsigned char* __restrict__ exr = ex ? ex + (size_t)blockIdx.x * ldx : nullptr;
  long long self_j = -1;
  if constexpr (SELF != 0) self_j = self[blockIdx.x];
  auto key_at = [&](long long j) {
    if constexpr (SELF != 0) return top_n_key(row[j], (exr && exr[j] != 0) || j == self_j);
    else return top_n_key(row[j], exr && exr[j] != 0);   // (nbmf_top_n's statement, as it was)
  };

  // 1. select
  unsigned long long prefix = 0, fixed = 0;   // the digits found so far, and the bits they occupy
  unsigned int need = (unsigned int)top;      // slots still to fill from the keys that carry `prefix`: >= 1 throughout
  unsigned int n_gt = 0;                      // keys above every key that carries `prefix`
  bool all = false;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[tid] = 0;
    __syncthreads();
    for (long long j = tid; j < n; j += TN_THREADS) {
      const unsigned long long k = key_at(j);
      if (k != 0 && (k & fixed) == prefix) atomicAdd(&hist[(unsigned int)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (wave == 0) {   // lane l owns bins 255 - 4l .. 252 - 4l, the highest first
      unsigned int h[4], own = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        h[q] = hist[255 - 4 * lane - q];
        own += h[q];
      }
      unsigned int incl = own;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const unsigned int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
      }
      unsigned int above = incl - own;   // keys in the bins above this lane's
      if (lane == 63 && incl < need) {   // (first pass only: later passes scan a bin that held at least `need` keys)
        sel[0] = 256u;
        sel[1] = incl;
      }
      if (above < need && incl >= need) {   // exactly one lane: the running count reaches `need` in one of its bins
        int d = -1;
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (d < 0) {
            if (above + h[q] >= need) d = 255 - 4 * lane - q;
            else above += h[q];
          }
        sel[0] = (unsigned int)d;
        sel[1] = above;
      }
    }
    __syncthreads();
    const unsigned int d = sel[0], above = sel[1];   // (sel is rewritten two barriers from here at the earliest)
    n_gt += above;
    if (d == 256u) {
      all = true;
      break;
    }
    need -= above;
    prefix |= (unsigned long long)d << shift;
    fixed |= 0xffull << shift;
  }
  const unsigned long long T = all ? 0ull : prefix;
  const unsigned int n_eq = all ? 0u : need;
  const unsigned int cnt = n_gt + n_eq;   // = top, or every nonzero key of a short row

  // 2. collect
  if ((unsigned int)tid >= cnt) {   // the pads of the sort: behind every real entry
    ent_key[tid] = 0ull;
    ent_col[tid] = 0x7fffffff;
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned int run_gt = 0, run_eq = 0;   // taken in the chunks before this one (the same in every thread)
  int buf = 0;
  for (long long c0 = 0; c0 < n; c0 += TN_THREADS, buf ^= 1) {
    const long long j = c0 + tid;
    const unsigned long long k = j < n ? key_at(j) : 0ull;
    const bool gt = k > T, eq = n_eq != 0 && k == T;
    const unsigned long long bg = __ballot(gt), be = __ballot(eq);
    if (lane == 0) {
      wave_cnt[buf][wave][0] = (unsigned int)__popcll(bg);
      wave_cnt[buf][wave][1] = (unsigned int)__popcll(be);
    }
    __syncthreads();   // (one barrier per chunk: the next chunk writes the other half of wave_cnt)
    unsigned int pg = run_gt + (unsigned int)__popcll(bg & below), pe = run_eq + (unsigned int)__popcll(be & below);
#pragma unroll
    for (int w = 0; w < TN_THREADS / 64; ++w) {
      const unsigned int g = wave_cnt[buf][w][0], e = wave_cnt[buf][w][1];
      if (w < wave) {
        pg += g;
        pe += e;
      }
      run_gt += g;
      run_eq += e;
    }
    if (gt && pg < n_gt) {
      ent_key[pg] = k;
      ent_col[pg] = (int)j;
    } else if (eq && pe < n_eq) {
      ent_key[n_gt + pe] = k;
      ent_col[n_gt + pe] = (int)j;
    }
    if (run_gt >= n_gt && run_eq >= n_eq) break;   // every slot has its entry
  }
  __syncthreads();

  // 3. sort and write
  int P = 2;
  while (P < top) P <<= 1;   // <= TN_MAX
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
      const int p = tid ^ j2;
      if (tid < P && p > tid) {
        const unsigned long long ka = ent_key[tid], kb = ent_key[p];
        const int ca = ent_col[tid], cb = ent_col[p];
        const bool a_first = ka > kb || (ka == kb && ca < cb);
        if (((tid & k2) == 0) != a_first) {
          ent_key[tid] = kb;
          ent_key[p] = ka;
          ent_col[tid] = cb;
          ent_col[p] = ca;
        }
      }
      __syncthreads();
    }
  if (tid < top) {
    const size_t o = (size_t)blockIdx.x * top + tid;
    long long col = -1;
    double score = __longlong_as_double(0x7ff8000000000000ll);   // NaN
    if ((unsigned int)tid < cnt) {   // (a real entry: its column is < n)
      col = ent_col[tid];
      score = row[col];
    }
    out_cols[o] = col;
    if (out_scores) out_scores[o] = score;
  }
}
