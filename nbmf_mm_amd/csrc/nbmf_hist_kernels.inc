// nbmf_hist_kernels.inc -- the observed zeros and the observed ones of the data, counted by the Theta = W^T H they got
// (nbmf_theta_hist; DESIGN.md 4.9): the two integer histograms that ROC AUC and calibration are functions of.  Included by
// nbmf_hip.hip after nbmf_predict_kernels.inc and nbmf_score_kernels.inc: theta_hist_kernel opens with THETA_TILE, the very
// statements predict_rows_kernel and score_rows_kernel open with, so the Theta it bins is bit for bit the entry
// predict_rows_kernel<0> stores with the clip on -- but no Theta panel is ever written: what leaves the kernel are integer
// adds onto 2 * bins + 2 counters.  No floating-point atomics, no workgroup barrier.

// The bin of a Theta already clipped to [0, 1] and not NaN: p = theta * bins is ONE rounded multiplication (there is
// nothing next to it to contract), truncated towards zero, and bins - 1 where that reaches bins (theta = 1).  A theta
// exactly on an edge is in the upper bin.  0 <= p <= 1024, so the 32-bit conversion is the 64-bit one of the header.
__device__ __forceinline__ int theta_bin(double th, int bins) {
  const double p = th * (double)bins;
  int b = (int)p;
  if (b >= bins) b = bins - 1;
  return b < 0 ? 0 : b;   // (never taken for a clipped theta: the slot index stays inside the wave's histogram by itself)
}

// Rows [prow0, prow0 + pnrows) of Theta, clipped to [0, 1], against the staged data panel xd (bytes, row 0 = row prow0,
// leading dimension ldp, a multiple of 4 >= n; nonzero means class 1) and the staged mask panel md (bytes, leading
// dimension ldp, nonzero = observed; null: every entry is).  What the panels hold in columns n .. ldp-1 is read and never
// used.  An entry is LIVE where its panel row is inside [0, pnrows), its column is < n and it is observed -- the rules of
// score_rows_kernel.  Every live entry adds 1 to one slot of the call's accumulator of 2 * bins + 2 counters:
//   slot c * bins + b    hist[c][b], c = (data byte != 0), b = theta_bin(theta)
//   slot 2 * bins + c    nan_count[c]: a NaN theta is in no bin
// The accumulator is kept in `copies` copies, total[copy * slots + slot]: a wave adds onto the copy its number in the grid
// picks (modulo), so that the waves in flight at one time -- consecutive numbers -- spread over all of them instead of
// queueing on the cache lines of one 16 KiB array (DESIGN.md 4.9: measured), and theta_hist_finish_kernel adds the copies
// up at the end of the call.
//
// Each wave counts its 16 x 64 strip in a histogram of its own in LDS (slots + 0 .. 2 * bins + 1 of its quarter of the
// dynamic LDS, 4 bytes each: 32 KiB + 32 bytes per workgroup at bins = 1024): it zeroes the slots, adds its 16 entries per
// lane with LDS integer atomics (lanes of one wave do meet in a slot), reads the slots back, lane l the slots l, l + 64,
// ..., and adds every nonzero one onto its copy of the accumulator with a no-return 64-bit integer atomic -- consecutive
// lanes, consecutive counters.  The three steps are ordered INSIDE the wave only: a wave's LDS instructions are carried out in the order
// it issues them, and the wavefront-scope fences keep the compiler from moving one across a step's end.  No other wave
// ever touches these slots, so there is no __syncthreads() -- and there must be none: THETA_TILE lets the waves whose
// strip lies wholly beyond ldp leave before the k loop.  A wave that stays keeps all its 64 lanes (lanes whose columns
// are >= ldp, rows outside the panel: they count nothing, and zero and read back like the others).
// Integer adds commute: the sums over the copies do not depend on the order the waves arrive in, on which copy a wave
// adds to, on the panels or on prow0.
__global__ __launch_bounds__(PR_WAVES * 64) void theta_hist_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long n,
    long long prow0, long long pnrows, long long ldp, int bins, const unsigned char* __restrict__ xd,
    const unsigned char* __restrict__ md, int copies, unsigned long long* __restrict__ total) {
  extern __shared__ unsigned int hist_lds[];   // PR_WAVES * (2 * bins + 2) words
  THETA_TILE(Wn, Hn, K, mA, nA, prow0, ldp)   // (ldp <= nA)

  const int slots = 2 * bins + 2;
  unsigned int* mine = hist_lds + wave * slots;
  for (int s = lane; s < slots; s += 64) mine[s] = 0u;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();

  const bool in_panel = jc < ldp;   // ldp is a multiple of 4: jc .. jc+3 are inside the panel's row or all outside
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long prow = i0 + lr + 4 * r - prow0;
    const bool live = in_panel && prow >= 0 && prow < pnrows;
    uint32_t xw = 0, mw = 0;
    if (live) {
      const size_t at = (size_t)prow * ldp + jc;
      xw = *(const uint32_t*)(xd + at);
      mw = md ? *(const uint32_t*)(md + at) : 0x01010101u;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double v = acc[t][r];
      v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);   // np.clip: a NaN stays a NaN
      const bool obs = live && jc + t < n && ((mw >> (8 * t)) & 0xffu) != 0;
      if (obs) {
        const int c = ((xw >> (8 * t)) & 0xffu) != 0 ? 1 : 0;
        const int s = v != v ? 2 * bins + c : c * bins + theta_bin(v, bins);
        (void)__hip_atomic_fetch_add(mine + s, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();

  const unsigned int wave_no = (blockIdx.y * gridDim.x + blockIdx.x) * PR_WAVES + wave;   // (may wrap: any number picks a copy)
  total += (size_t)(wave_no % (unsigned int)copies) * slots;
  for (int s = lane; s < slots; s += 64) {
    const unsigned int cnt = mine[s];
    if (cnt != 0u)
      (void)__hip_atomic_fetch_add(total + s, (unsigned long long)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The `copies` copies of the accumulator, added up in ascending order into out[0 .. slots): one thread per slot.
__global__ __launch_bounds__(256) void theta_hist_finish_kernel(const unsigned long long* __restrict__ total, int copies, int slots,
                                                                 unsigned long long* __restrict__ out) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= slots) return;
  unsigned long long sum = 0;
  for (int q = 0; q < copies; ++q) sum += total[(size_t)q * slots + s];
  out[s] = sum;
}
