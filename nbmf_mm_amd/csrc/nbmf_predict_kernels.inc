// nbmf_predict_kernels.inc -- Theta = W^T H handed back to the caller (nbmf_predict_at, nbmf_predict_rows; DESIGN.md 4.6).
// Included by nbmf_hip.hip after the other kernel files.  Both kernels read the natural padded factor images
// Wn[k * mA + i], Hn[k * nA + j] (what get_factor_kernel reads) and nothing else of the context; neither relies on what
// the images hold in rows k >= K or in columns beyond m / n: components k >= K are replaced by exact zeros in registers,
// and pad rows / columns of a tile only reach results that are never stored.

constexpr int PR_WAVES = 4;          // waves per workgroup of predict_rows_kernel: 4 strips of 64 columns, one 16-row tile
constexpr int PR_STRIP = 64;         // columns per wave: four 16-column MFMA tiles on four accumulators
constexpr int PA_LANES = 8;          // lanes that share one pair in predict_at_kernel
constexpr int PT_TILE = 32;          // k_major_kernel: 32 x 32 transpose tiles

// Rows [prow0, prow0 + pnrows) of Theta, all n columns, into a staging panel whose row 0 is row prow0 and whose leading
// dimension ldd is a multiple of 4 (doubles for OUT_U8 == 0, bytes otherwise).
//
// One wave owns a 16 x 64 strip: rows i0 .. i0+15 on the image's 16-grid, columns j0 .. j0+63.  Its four MFMA tiles are
// INTERLEAVED over the strip -- column c of tile t is j0 + 4c + t -- so that
//   - the four B operands of a lane are 4 consecutive doubles of one row of Hn: one 32-byte load, 512 contiguous bytes
//     per group of 16 lanes (A: Wn[(k0 + (l >> 4)) * mA + i0 + (l & 15)], 128 contiguous bytes per group);
//   - result register r of a lane holds Theta[i0 + (l >> 4) + 4r, j0 + 4(l & 15) + t] for t = 0..3 (the f64 C/D map:
//     row = (l >> 4) + 4r, column = l & 15): 4 consecutive entries of one output row, stored as one 32-byte (doubles) or
//     one 4-byte (bytes) access -- a store instruction writes 512 resp. 64 contiguous bytes per output row.
// The k blocks are added in ascending order, one chain per tile: an entry's value depends on its row, its column and the
// factors only, not on the panel or the request it was computed in.  Lanes whose k is >= K supply 0.0 to both operands
// (the loop stops at the first multiple of 4 >= K, which is <= KP: no row of the images beyond KP is read).
template <int OUT_U8>
__global__ __launch_bounds__(PR_WAVES * 64) void predict_rows_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long prow0,
    long long pnrows, long long ldd, int clip, double threshold, void* __restrict__ out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lr = lane >> 4, lc = lane & 15;
  const long long i0 = (prow0 / 16 + blockIdx.x) * 16;                                  // < mA: the host sizes the grid
  const long long j0 = ((long long)blockIdx.y * PR_WAVES + wave) * PR_STRIP;
  if (j0 >= nA) return;   // (no barrier below)
  const long long jc = j0 + 4 * lc;   // this lane's four columns: jc .. jc+3 (< nA, a multiple of 128)

  d4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < K; k0 += 4) {
    const int k = k0 + lr;
    double a = 0.0;
    d4 b = d4{0.0, 0.0, 0.0, 0.0};
    if (k < K) {
      a = Wn[(size_t)k * mA + i0 + lc];
      b = *(const d4*)(Hn + (size_t)k * nA + jc);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = NBMF_MFMA(a, b[t], acc[t], 0, 0, 0);
  }

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

// out[t] = sum_k Wk[rows[t] * K + k] * Hk[cols[t] * K + k] for the `count` pairs of one chunk (Wk, Hk: k_major_kernel).
// PA_LANES consecutive lanes share a pair: lane q adds the products of k = q, q + 8, q + 16, ... in ascending order
// (consecutive lanes read consecutive doubles), then the 8 partial sums are folded by the xor butterfly 4, 2, 1 -- a fixed
// order, so the value at (i, j) depends on (i, j) and the factors only.
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
  double s = 0.0;
  if (live) {
    const double* __restrict__ w = Wk + (size_t)i * K;
    const double* __restrict__ h = Hk + (size_t)j * K;
    for (int k = q; k < K; k += PA_LANES) s = __builtin_fma(w[k], h[k], s);
  }
#pragma unroll
  for (int off = PA_LANES / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (t < count && q == 0) {
    if (clip) s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    out[t] = s;
  }
}
