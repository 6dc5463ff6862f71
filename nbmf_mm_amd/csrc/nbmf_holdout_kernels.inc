// nbmf_holdout_kernels.inc -- the held-out split drawn on the device (nbmf_hold_out, nbmf_hold_out_undo; DESIGN.md 4.14).
// Included by nbmf_hip.hip after nbmf_pack_kernels.inc (splitmix64, the code bytes and the two images' tile order).
// The observed entries of the resident code images whose counter-based uniform falls in [lo, hi) leave the images (their
// byte becomes "valid, unobserved" in both) and are listed as (row, col, truth) triples in row-major order of the internal
// matrix, columns ascending: the order np.nonzero gives on the host.  Integers only: the uniform is compared as the
// 53-bit integer it is made from, positions come from ballots and population counts, the sums are integer sums.
//
// The walk is over image B, where a lane's dword holds four entries of ONE internal row: tile (ib, jb) is 64 dwords, lane
// (q, c) holds row 16 ib + c at columns 16 jb + 4 r + q, r = 0 .. 3 its bytes.  A wave owns 16 rows x one SEGMENT of
// HO_SEG_TILES tiles (512 columns); the count of a (row, segment) is one 32-bit word at counts[row * nseg + segment], so
// the exclusive prefix sum over the flat array IS the list position of the segment's first entry.

constexpr int HO_SEG_TILES = 32;       // tiles of 16 columns per segment
constexpr int HO_SCAN_BLOCK = 2048;    // counts per workgroup of the two outer scan kernels (256 threads x 8)
constexpr unsigned long long HO_SALT = 0xA0761D6478BD642Full;

struct HoldOutRule {
  unsigned long long seed;       // as given
  unsigned long long klo, khi;   // held out iff klo <= (hash >> 11) < khi: ceil(lo 2^53), ceil(hi 2^53)
  long long m, n;                // internal shape
  int transposed;                // the user's matrix is n x m: the counter is j * m + i
};

// Is entry (i, j) of the internal matrix inside the split's interval?  (Whether it is observed is the caller's test.)
__device__ __forceinline__ bool ho_in_interval(const HoldOutRule& h, long long i, long long j) {
  const unsigned long long idx = h.transposed ? (unsigned long long)j * (unsigned long long)h.m + (unsigned long long)i
                                              : (unsigned long long)i * (unsigned long long)h.n + (unsigned long long)j;
  const unsigned long long k = splitmix64((h.seed * 0x100000001B3ull + idx) ^ HO_SALT) >> 11;
  return k >= h.klo && k < h.khi;
}

// The wave of (strip ib, segment s): which one this is, and the segment's tiles.  Waves beyond the last return false.
__device__ __forceinline__ bool ho_wave(long long strips, long long nseg, long long tiles_e, long long* ib, long long* s,
                                        long long* jb0, long long* jb1) {
  const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= strips * nseg) return false;
  *ib = w / nseg;
  *s = w % nseg;
  *jb0 = *s * HO_SEG_TILES;
  *jb1 = min(*jb0 + HO_SEG_TILES, tiles_e);
  return true;
}

// Step 1: counts[i * nseg + s] = held-out entries of row i in segment s.  Reads image B once; writes nothing else.
__global__ __launch_bounds__(256) void holdout_count_kernel(const uint32_t* __restrict__ dataB, long long RbB, long long strips,
                                                            long long nseg, long long tiles_e, HoldOutRule h,
                                                            unsigned int* __restrict__ counts) {
  long long ib, s, jb0, jb1;
  if (!ho_wave(strips, nseg, tiles_e, &ib, &s, &jb0, &jb1)) return;   // (uniform over the wave)
  const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  const long long i = ib * 16 + c;
  unsigned int cnt = 0;
#pragma unroll 4
  for (long long jb = jb0; jb < jb1; ++jb) {
    const uint32_t code = dataB[((size_t)ib * RbB + jb) * 64 + lane];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (((code >> (8 * r)) & (CB_YM | CB_ZOBS)) && ho_in_interval(h, i, jb * 16 + 4 * r + q)) ++cnt;
  }
  cnt += __shfl_xor(cnt, 16, 64);   // the row's four lanes
  cnt += __shfl_xor(cnt, 32, 64);
  if (q == 0 && i < h.m) counts[i * nseg + s] = cnt;
}

// Step 2, the exclusive prefix sum of counts[0 .. total) in 64 bits, three launches:
//   holdout_block_sum_kernel    bsum[b] = sum of block b's HO_SCAN_BLOCK counts
//   holdout_scan_blocks_kernel  one workgroup: bsum becomes its own exclusive prefix sum, bsum[nb] the grand total
//   holdout_scan_final_kernel   offs[e] = bsum[block of e] + the counts before e in its block
__global__ __launch_bounds__(256) void holdout_block_sum_kernel(const unsigned int* __restrict__ counts, long long total,
                                                                unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long sh[4];
  const long long base = (long long)blockIdx.x * HO_SCAN_BLOCK + threadIdx.x * 8;
  unsigned long long v = 0;
  for (int e = 0; e < 8; ++e)
    if (base + e < total) v += counts[base + e];
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) bsum[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// Exclusive scan of the 256 values the threads of a workgroup hold (Hillis-Steele in LDS); every thread reaches the barriers.
__device__ __forceinline__ unsigned long long ho_scan256(unsigned long long v, unsigned long long* sh, unsigned long long* all) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const unsigned long long add = tid >= off ? sh[tid - off] : 0ull;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  const unsigned long long incl = sh[tid];
  if (all) *all = sh[255];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(256) void holdout_scan_blocks_kernel(unsigned long long* __restrict__ bsum, long long nb) {
  __shared__ unsigned long long sh[256];
  const long long per = (nb + 255) / 256, b0 = threadIdx.x * per, b1 = min(b0 + per, nb);
  unsigned long long v = 0, all = 0;
  for (long long b = b0; b < b1; ++b) v += bsum[b];
  unsigned long long run = ho_scan256(v, sh, &all);
  for (long long b = b0; b < b1; ++b) {
    const unsigned long long mine = bsum[b];
    bsum[b] = run;
    run += mine;
  }
  if (threadIdx.x == 0) bsum[nb] = all;
}

__global__ __launch_bounds__(256) void holdout_scan_final_kernel(const unsigned int* __restrict__ counts, long long total,
                                                                 const unsigned long long* __restrict__ bsum,
                                                                 unsigned long long* __restrict__ offs) {
  __shared__ unsigned long long sh[256];
  const long long base = (long long)blockIdx.x * HO_SCAN_BLOCK + threadIdx.x * 8;
  unsigned int mine[8];
  unsigned long long v = 0;
  for (int e = 0; e < 8; ++e) {
    mine[e] = base + e < total ? counts[base + e] : 0u;
    v += mine[e];
  }
  unsigned long long run = bsum[blockIdx.x] + ho_scan256(v, sh, nullptr);
  for (int e = 0; e < 8; ++e) {
    if (base + e < total) offs[base + e] = run;
    run += mine[e];
  }
}

// Step 3: the same walk as step 1.  Entry r of the wave's tile is held out in the lanes of the ballot; row c's lanes are
// bits c, 16 + c, 32 + c, 48 + c of it, in ascending column order within r (column 4 r + q), and r ascends in the loop:
// the position of an entry is the row's running position plus the row's set bits below its own lane.  The entry's byte in
// image B (this lane's dword) and in image A becomes "valid, unobserved": one byte per image, this thread alone.
__global__ __launch_bounds__(256) void holdout_scatter_kernel(unsigned char* __restrict__ dataA, unsigned char* __restrict__ dataB,
                                                              long long RbA, long long RbB, long long strips, long long nseg,
                                                              long long tiles_e, HoldOutRule h,
                                                              const unsigned long long* __restrict__ offs, int* __restrict__ rows,
                                                              int* __restrict__ cols, unsigned char* __restrict__ x) {
  long long ib, s, jb0, jb1;
  if (!ho_wave(strips, nseg, tiles_e, &ib, &s, &jb0, &jb1)) return;   // (uniform over the wave: the ballots below are whole)
  const int lane = threadIdx.x & 63, q = lane >> 4, c = lane & 15;
  const long long i = ib * 16 + c;
  const unsigned long long rowmask = 0x0001000100010001ull << c;
  const unsigned long long below = rowmask & ((1ull << (16 * q)) - 1ull);   // the row's lanes with a smaller q
  unsigned long long pos = i < h.m ? offs[i * nseg + s] : 0ull;
  for (long long jb = jb0; jb < jb1; ++jb) {
    const size_t dwB = ((size_t)ib * RbB + jb) * 64 + lane;
    const uint32_t code = ((const uint32_t*)dataB)[dwB];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const uint32_t b = (code >> (8 * r)) & 0xffu;
      const long long j = jb * 16 + 4 * r + q;
      const bool held = (b & (CB_YM | CB_ZOBS)) && ho_in_interval(h, i, j);
      const unsigned long long row_bits = __ballot(held) & rowmask;
      if (held) {
        const unsigned long long t = pos + (unsigned long long)__popcll(row_bits & below);
        rows[t] = (int)i;
        cols[t] = (int)j;
        x[t] = (b & CB_YM) ? 1 : 0;
        dataB[dwB * 4 + r] = (unsigned char)CB_VALID;
        const int rj = 4 * r + q;   // image A: strip jb, block ib, lane (c & 3, rj), byte c >> 2
        dataA[(((size_t)jb * RbA + ib) * 64 + (c & 3) * 16 + rj) * 4 + (c >> 2)] = (unsigned char)CB_VALID;
      }
      pos += (unsigned long long)__popcll(row_bits);
    }
  }
}

// The undo: one thread per listed triple puts the entry's byte back in both images, an observed one or an observed zero
// as x[t] says (the addresses of csr_scatter_kernel).
__global__ __launch_bounds__(256) void holdout_restore_kernel(unsigned char* __restrict__ dataA, unsigned char* __restrict__ dataB,
                                                              long long RbA, long long RbB, const int* __restrict__ rows,
                                                              const int* __restrict__ cols, const unsigned char* __restrict__ x,
                                                              long long count) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= count) return;
  const long long i = rows[t], j = cols[t];
  const long long ib = i >> 4, jb = j >> 4;
  const int ri = (int)(i & 15), rj = (int)(j & 15);
  const unsigned char code = (unsigned char)(CB_VALID | (x[t] ? CB_YM : CB_ZOBS));
  dataA[(((size_t)jb * RbA + ib) * 64 + (ri & 3) * 16 + rj) * 4 + (ri >> 2)] = code;
  dataB[(((size_t)ib * RbB + jb) * 64 + (rj & 3) * 16 + ri) * 4 + (rj >> 2)] = code;
}
