// nbmf_eval_kernels.inc -- the Bernoulli log-likelihood of the factors at a resident list of held-out index pairs, summed
// on the device (nbmf_set_eval, nbmf_eval_loglik and the evaluations nbmf_run makes between iterations; DESIGN.md 4.11).
// Included by nbmf_hip.hip after nbmf_predict_kernels.inc (theta_at_pair, PA_LANES) and nbmf_score_kernels.inc
// (score_term_u8).  Two launches per evaluation: one partial per workgroup of 32 pairs, then one workgroup that folds
// the partials.  Every sum has a fixed order: no floating-point atomics, no hand-off between workgroups, and the two
// barriers are reached by every thread.

constexpr int EV_THREADS = 256;                     // eval_pairs_kernel: 4 waves, PA_LANES lanes per pair
constexpr int EV_PAIRS = EV_THREADS / PA_LANES;     // 32 pairs per workgroup
constexpr int EV_FOLD = 256;                        // eval_fold_kernel: one workgroup

// partials[blockIdx.x] = the sum of the terms of pairs [32 blockIdx.x, 32 blockIdx.x + 32) that are below `count`.
// Theta at pair t is theta_at_pair(rows[t], cols[t]) -- bit for bit what predict_at_kernel stores without its clip -- and
// the term score_term_u8(theta, x[t] != 0, eps), which the 8 lanes of the pair all hold.  A wave's 8 terms are folded by
// the xor butterfly 8, 16, 32 (pair p with p ^ 1, then ^ 2, then ^ 4: the same tree in every lane, an addition's operands
// commute), the four wave sums through LDS as (w0 + w1) + (w2 + w3).  Pairs at or beyond `count` load nothing and add
// +0.0.  rows / cols were checked against [0, m) x [0, n) on the host before they were uploaded (nbmf_set_eval).
__global__ __launch_bounds__(EV_THREADS) void eval_pairs_kernel(const double* __restrict__ Wk, const double* __restrict__ Hk,
                                                                int K, const int* __restrict__ rows,
                                                                const int* __restrict__ cols,
                                                                const unsigned char* __restrict__ x, long long count,
                                                                double eps, double* __restrict__ partials) {
  __shared__ double wave_sum[EV_THREADS / 64];
  const long long t = (long long)blockIdx.x * EV_PAIRS + threadIdx.x / PA_LANES;
  const int q = threadIdx.x & (PA_LANES - 1);
  const bool live = t < count;
  long long i = 0, j = 0;
  bool one = false;
  if (live) {
    i = rows[t];
    j = cols[t];
    one = x[t] != 0;
  }
  const double th = theta_at_pair(Wk, Hk, K, i, j, q, live);
  double s = live ? score_term_u8(th, one, eps) : 0.0;
#pragma unroll
  for (int off = PA_LANES; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
}

// *out = the sum of partials[0 .. nparts): thread t adds partials[t], [t + 256], ... in ascending order, then the 256
// thread sums are halved in LDS, 128, 64, ..., 1 -- a fixed order whatever nparts is.  One workgroup.
__global__ __launch_bounds__(EV_FOLD) void eval_fold_kernel(const double* __restrict__ partials, long long nparts,
                                                            double* __restrict__ out) {
  __shared__ double sh[EV_FOLD];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long p = tid; p < nparts; p += EV_FOLD) s += partials[p];
  sh[tid] = s;
  __syncthreads();
  for (int w = EV_FOLD / 2; w >= 1; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  if (tid == 0) *out = sh[0];
}
