// nbmf_theta_bits_kernels.inc -- a yes / no decision per entry of Theta = W^T H, leaving the device as bits
// (nbmf_theta_bits; DESIGN.md 4.13).  Included by nbmf_hip.hip after nbmf_predict_kernels.inc (THETA_TILE) and
// nbmf_pack_kernels.inc (splitmix64).  The output is np.packbits' layout, the one nbmf_bits_kernels.inc unpacks: entry j of
// a row is bit 7 - j % 8 of its byte j / 8, so what this kernel writes is an operand of every call that takes bits.

constexpr int TB_THRESHOLD = 0;   // NBMF_BITS_THRESHOLD: theta > threshold
constexpr int TB_SAMPLE = 1;      // NBMF_BITS_SAMPLE:    u(i, j) < theta

// x of the lane CTRL names inside this lane's DPP row -- the 16 lanes lane >> 4 of the wave, which is a group of THETA_TILE.
// Every lane of the wave must be active: a DPP read of a lane that is switched off leaves the destination as it was.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_row(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}

// The OR of x over the 16 lanes of the DPP row, in every one of them: rotations by 8, 4, 2 and 1 lanes (row_ror).
__device__ __forceinline__ uint32_t or_over_row(uint32_t x) {
  x |= dpp_row<0x128>(x);
  x |= dpp_row<0x124>(x);
  x |= dpp_row<0x122>(x);
  x |= dpp_row<0x121>(x);
  return x;
}

// Rows [prow0, prow0 + pnrows) of the decision, columns [0, n), into a staging panel whose row 0 is row prow0 and whose
// leading dimension ldb (bytes) is a multiple of 8 and at least nA / 8: the tile -- Theta is bit for bit what
// predict_rows_kernel stores -- then, after the same clip, per entry
//   TB_THRESHOLD: theta > threshold, strictly, as predict_rows_kernel<1>; a NaN theta gives 0;
//   TB_SAMPLE:    u < theta with u the uniform of synth_code (nbmf_pack_kernels.inc) at row0 = col0 = 0, n_global = n:
//                 the top 53 bits of splitmix64(seed * 0x100000001B3 + i * n + j) times 2^-53.  u is in [0, 1): theta = 0
//                 never gives a one, theta >= 1 always does, a NaN theta gives 0.
// A column j >= n decides 0.  A lane holds 4 consecutive columns of 4 rows: per row one nibble, the high one of byte
// lc >> 1 of the wave's 8 bytes where lc is even, the low one otherwise.  The nibbles of a row are ORed over its 16 lanes
// in registers (two dwords), and lane lc == 0 stores the 8 bytes at once where the row is inside the panel: the strip starts
// at a multiple of 64 columns, so the store is 8-byte aligned.  Strips that start at or beyond n are not computed; the last
// strip that is writes zeros for its columns >= n, so bytes [0, ceil(n / 8)) of a panel row are all written and the pad
// bits of the last one are 0.  No LDS, no barrier, no atomics; no branch diverges before the last cross-lane operation.
template <int MODE>
__global__ __launch_bounds__(PR_WAVES * 64) void theta_bits_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long n, long long prow0,
    long long pnrows, long long ldb, int clip, double threshold, unsigned long long seed, unsigned char* __restrict__ out) {
  THETA_TILE(Wn, Hn, K, mA, nA, prow0, n)

  const unsigned long long base = seed * 0x100000001B3ull;
  const int shift = 8 * ((lc >> 1) & 3) + ((lc & 1) ? 0 : 4);   // this lane's nibble inside its dword (byte b: bits 8b .. 8b+7)
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long i = i0 + lr + 4 * r, prow = i - prow0;
    uint32_t nib = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double v = acc[t][r];
      if (clip) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);   // np.clip: a NaN stays a NaN
      const long long j = jc + t;
      bool one;
      if (MODE == TB_SAMPLE) {
        const unsigned long long idx = (unsigned long long)i * (unsigned long long)n + (unsigned long long)j;
        const double u = (double)(splitmix64(base + idx) >> 11) * (1.0 / 9007199254740992.0);
        one = u < v;
      } else {
        one = v > threshold;
      }
      nib |= (one && j < n) ? (8u >> t) : 0u;   // column jc + t is bit 3 - t of the nibble
    }
    const uint32_t lo = or_over_row(lc < 8 ? nib << shift : 0u);    // bytes 0 .. 3 of the row's 8
    const uint32_t hi = or_over_row(lc < 8 ? 0u : nib << shift);    // bytes 4 .. 7
    if (lc == 0 && prow >= 0 && prow < pnrows)
      *(unsigned long long*)(out + (size_t)prow * ldb + (j0 >> 3)) = ((unsigned long long)hi << 32) | lo;
  }
}
