// nbmf_pairs_kernels.inc -- the best entries of Theta = W^T H over a whole row range, as one list of (row, column) pairs
// (nbmf_top_pairs; DESIGN.md 4.15).  Included by nbmf_hip.hip after nbmf_hist_kernels.inc: the three kernels here open with
// THETA_TILE, the very statements predict_rows_kernel opens with, so the Theta they select from is bit for bit the entry
// predict_rows_kernel<0> stores -- but no Theta panel is ever written.  A radix selection over an order-preserving 64-bit
// key forms the product again on every pass: what leaves a digit pass are integer adds onto PAIRS_BINS counters, what
// leaves the tie pass are integer adds onto one counter per row, and what leaves the collecting pass are the chosen
// entries.  No floating-point atomics, no workgroup barrier (THETA_TILE lets whole waves leave early).

constexpr int PAIRS_DIGIT_BITS = 11;                 // bits of the key fixed per digit pass
constexpr int PAIRS_BINS = 1 << PAIRS_DIGIT_BITS;    // counters per wave histogram: 8 KiB of LDS per wave, 32 KiB per workgroup

// What one entry is to the selection.  `live`: its row is inside the request and its column is < n.  xb / mb: its bytes in
// the staged operand panels (0 and 1 where there is none).
//   NBMF_PAIRS_THETA       score = theta,                     eligible unless xb != 0 (the exclude byte)
//   NBMF_PAIRS_LIKELIHOOD  score = xb ? theta : 1.0 - theta,  eligible where mb != 0 (observed)
// The key is 0 for an entry that is not eligible or whose score is NaN, and otherwise orders the entries best first by
// DESCENDING key: top_n_key for the theta kind (largest first), its complement for the likelihood kind (smallest first;
// the complement of a nonzero top_n_key is nonzero: no key is all ones).  Scores that compare equal share a key.
__device__ __forceinline__ unsigned long long pairs_key(double v, int clip, int kind, bool live, unsigned int xb, unsigned int mb,
                                                        double* score) {
  if (clip) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);   // np.clip: a NaN stays a NaN
  double s = v;
  bool skip = !live;
  if (kind == NBMF_PAIRS_LIKELIHOOD) {
    if (xb == 0) s = 1.0 - v;   // one rounded subtraction
    skip = skip || mb == 0;
  } else {
    skip = skip || xb != 0;
  }
  *score = s;
  const unsigned long long k = top_n_key(s, skip);
  return (kind == NBMF_PAIRS_LIKELIHOOD && k != 0ull) ? ~k : k;
}

// The epilogue all three kernels share: the 16 keys (and scores) of a lane, key[r][t] for row i0 + lr + 4r, column jc + t.
// The staged panels xd / md (either may be null) hold the request's rows from row srow0 on, ldp bytes per row (a multiple
// of 4 >= n): one 4-byte word per lane and row, as theta_hist_kernel reads them.  Rows outside [prow0, prow0 + pnrows) and
// columns >= n do not exist: key 0.
#define PAIRS_KEYS(xd, md)                                                                                            \
  unsigned long long key[4][4];                                                                                       \
  double score[4][4];                                                                                                 \
  {                                                                                                                   \
    const bool in_panel = jc < ldp; /* ldp is a multiple of 4: jc .. jc+3 are inside the panel's row or all outside */ \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                   \
      const long long row = i0 + lr + 4 * r;                                                                          \
      const bool in_rows = in_panel && row >= prow0 && row < prow0 + pnrows;                                          \
      uint32_t xw = 0, mw = 0x01010101u;                                                                              \
      if (in_rows) {                                                                                                  \
        const size_t at = (size_t)(row - srow0) * ldp + jc;                                                           \
        if (xd) xw = *(const uint32_t*)((xd) + at);                                                                   \
        if (md) mw = *(const uint32_t*)((md) + at);                                                                   \
      }                                                                                                               \
      _Pragma("unroll") for (int t = 0; t < 4; ++t) key[r][t] =                                                       \
          pairs_key(acc[t][r], clip, kind, in_rows && jc + t < n, (xw >> (8 * t)) & 0xffu, (mw >> (8 * t)) & 0xffu,   \
                    &score[r][t]);                                                                                    \
    }                                                                                                                 \
  }

// One digit pass.  Every entry with a nonzero key that carries the digits found so far -- (key & fixed) == prefix -- adds 1
// to the bin (key >> shift) & (bins - 1) of its next digit (bins <= PAIRS_BINS, a power of two).  Per wave a histogram of
// its own in LDS, then no-return 64-bit integer adds of the nonzero bins onto the copy of the accumulator the wave's number
// picks, total[copy * PAIRS_BINS + bin]: the three steps and their ordering inside the wave are theta_hist_kernel's.
__global__ __launch_bounds__(PR_WAVES * 64) void pairs_digit_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long n,
    long long prow0, long long pnrows, long long srow0, long long ldp, int clip, int kind,
    const unsigned char* __restrict__ xd, const unsigned char* __restrict__ md, unsigned long long prefix,
    unsigned long long fixed, int shift, int bins, int copies, unsigned long long* __restrict__ total) {
  __shared__ unsigned int pairs_lds[PR_WAVES * PAIRS_BINS];
  THETA_TILE(Wn, Hn, K, mA, nA, prow0, ldp)   // (ldp <= nA)

  unsigned int* mine = pairs_lds + wave * PAIRS_BINS;
  for (int s = lane; s < bins; s += 64) mine[s] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  PAIRS_KEYS(xd, md)
  (void)score;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const unsigned long long k = key[r][t];
      if (k != 0ull && (k & fixed) == prefix)
        (void)__hip_atomic_fetch_add(mine + ((unsigned int)(k >> shift) & (unsigned int)(bins - 1)), 1u, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  const unsigned int wave_no = (blockIdx.y * gridDim.x + blockIdx.x) * PR_WAVES + wave;   // (may wrap: any number picks a copy)
  total += (size_t)(wave_no % (unsigned int)copies) * PAIRS_BINS;
  for (int s = lane; s < bins; s += 64) {
    const unsigned int cnt = mine[s];
    if (cnt != 0u)
      (void)__hip_atomic_fetch_add(total + s, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The tie pass: row_ties[row - prow0] += the entries of the row whose key equals T (nonzero).  A lane's four entries of a
// row are added up, then the 16 lanes that share the row (lc = 0..15) by the xor butterfly, and lane lc = 0 adds a nonzero
// sum with one no-return integer atomic.
__global__ __launch_bounds__(PR_WAVES * 64) void pairs_ties_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long n,
    long long prow0, long long pnrows, long long srow0, long long ldp, int clip, int kind,
    const unsigned char* __restrict__ xd, const unsigned char* __restrict__ md, unsigned long long T,
    unsigned long long* __restrict__ row_ties) {
  THETA_TILE(Wn, Hn, K, mA, nA, prow0, ldp)
  PAIRS_KEYS(xd, md)
  (void)score;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    unsigned int cnt = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) cnt += key[r][t] == T ? 1u : 0u;
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    const long long row = i0 + lr + 4 * r;
    if (lc == 0 && cnt != 0u)   // (a nonzero count: the row is inside the request)
      (void)__hip_atomic_fetch_add(row_ties + (row - prow0), (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The collecting pass.  An entry is TAKEN where its key is nonzero and
//   row_only == 0:  key > T, or key == T and (row, column) <= (rs, cs) in row-major order.  T = `lo`, rs = LLONG_MAX takes
//                   every entry at or above a lower edge `lo`; T = 0 takes nothing extra (keys are nonzero).
//   row_only != 0:  key == T and row == rs: the ties of the boundary row, for the host to find the boundary column in.
// and entries below `lo` are never taken.  Every taken entry is appended to the candidate arrays: a lane counts its taken
// entries, the wave forms the lanes' exclusive prefix and total by shuffles, ONE lane makes one returning integer atomic
// on the slot counter for the whole wave, and each lane stores its entries behind the base it is handed.  The order of
// arrival is arbitrary; the set is not.  A slot at or beyond `cap` is counted and never stored.
__global__ __launch_bounds__(PR_WAVES * 64) void pairs_collect_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long n,
    long long prow0, long long pnrows, long long srow0, long long ldp, int clip, int kind,
    const unsigned char* __restrict__ xd, const unsigned char* __restrict__ md, unsigned long long lo, unsigned long long T,
    long long rs, long long cs, int row_only, unsigned long long cap, unsigned long long* __restrict__ slot_counter,
    long long* __restrict__ c_rows, long long* __restrict__ c_cols, double* __restrict__ c_scores) {
  THETA_TILE(Wn, Hn, K, mA, nA, prow0, ldp)
  PAIRS_KEYS(xd, md)
  unsigned int taken = 0, mine = 0;   // bit 4r + t: entry (r, t) is taken
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long row = i0 + lr + 4 * r;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const unsigned long long k = key[r][t];
      const long long col = jc + t;
      bool take;
      if (row_only) take = k == T && row == rs;
      else take = k >= lo && (k > T || row < rs || (row == rs && col <= cs));
      take = take && k != 0ull;
      if (take) {
        taken |= 1u << (4 * r + t);
        ++mine;
      }
    }
  }
  unsigned int incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned int up = __shfl_up(incl, off, 64);
    if (lane >= off) incl += up;
  }
  const unsigned int wave_total = __shfl(incl, 63, 64);
  if (wave_total == 0u) return;   // (the whole wave)
  unsigned long long base = 0;
  if (lane == 63) base = __hip_atomic_fetch_add(slot_counter, (unsigned long long)wave_total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  base = __shfl(base, 63, 64);
  unsigned long long at = base + (incl - mine);
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (taken & (1u << (4 * r + t))) {
        if (at < cap) {
          c_rows[at] = i0 + lr + 4 * r;
          c_cols[at] = jc + t;
          c_scores[at] = score[r][t];
        }
        ++at;
      }
}
