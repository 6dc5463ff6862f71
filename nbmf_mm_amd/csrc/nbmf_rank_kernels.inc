// nbmf_rank_kernels.inc -- where given columns of a row of Theta stand in top_n's order (nbmf_rank_rows; DESIGN.md 4.10).
// Included by nbmf_hip.hip after nbmf_predict_kernels.inc, whose top_n_key fixes what "ranked above" means: the kernel here
// counts keys, it never compares doubles, so a rank is by construction the slot top_n_kernel gives the column.

constexpr int RK_THREADS = 256;   // rank_rows_kernel: one workgroup per panel row, 256 columns per stride
constexpr int RK_GROUP = 8;       // targets answered by one pass over the row

// One workgroup per row of the staging panel predict_rows_kernel<0> has just written (row stride ldd doubles, n real
// columns; ex: one byte per entry, row stride ldx, nonzero = skip, or null).  The TARGETS of panel row r are the columns
// indices[indptr[r] - base .. indptr[r + 1] - base): indptr holds positions of the caller's array, `indices` is staged
// from position `base` on, and so are the four per-target outputs (any may be null).  With key(j) = top_n_key(row[j],
// ex[j]) over the real columns j' < n only -- what the panel holds in its pad columns does not matter --
//   eligible[r] = #{j' : key(j') != 0}                                        (out_eligible, may be null)
// and for a target j with key(j) != 0
//   above = #{j' : key(j') > key(j)},  tied = #{j' != j : key(j') == key(j)},  rank = above + #{j' < j : key(j') == key(j)},
// score = row[j]; a target with key(j) == 0 (excluded or NaN) gets rank = above = tied = -1 and its panel entry as score.
//
// Targets are taken in groups of RK_GROUP.  The group's columns and keys are the same in every thread (read through
// uniform addresses); a thread strides over the columns, forms key(j') once per column and group, and keeps 3 x RK_GROUP
// integer counters in registers, plus the eligible count in the first group.  The counters are added up inside a wave by
// the xor butterfly, across the waves by LDS integer atomics: integer adds only, so no result depends on an order.  The
// cost of a row is ceil(targets / RK_GROUP) passes over it (one pass for a row without targets when eligible is asked
// for; such a row's workgroup leaves at once otherwise).  LDS: 3 * RK_GROUP + 1 counters, whatever n and the number of
// targets are.  Every branch around a barrier is uniform: the group count is the row's.
__global__ __launch_bounds__(RK_THREADS) void rank_rows_kernel(const double* __restrict__ panel, long long ldd, long long n,
                                                               const unsigned char* __restrict__ ex, long long ldx,
                                                               const long long* __restrict__ indptr,
                                                               const int* __restrict__ indices, long long base,
                                                               long long* __restrict__ out_rank, long long* __restrict__ out_above,
                                                               long long* __restrict__ out_tied, double* __restrict__ out_scores,
                                                               long long* __restrict__ out_eligible) {
  __shared__ unsigned int total[3 * RK_GROUP + 1];   // [q]: above, [RK_GROUP + q]: equal (the target included), [2 RK_GROUP + q]: equal and left of it
  const int tid = threadIdx.x, lane = tid & 63;
  const double* __restrict__ row = panel + (size_t)blockIdx.x * ldd;
  const unsigned char* __restrict__ exr = ex ? ex + (size_t)blockIdx.x * ldx : nullptr;
  auto key_at = [&](long long j) { return top_n_key(row[j], exr && exr[j] != 0); };

  const bool per_target = out_rank || out_above || out_tied || out_scores;
  const long long t0 = indptr[blockIdx.x] - base;
  const long long t1 = per_target ? indptr[blockIdx.x + 1] - base : t0;
  long long groups = (t1 - t0 + RK_GROUP - 1) / RK_GROUP;
  if (groups == 0 && out_eligible) groups = 1;   // (a pass for the eligible count alone)

  for (long long g = 0; g < groups; ++g) {
    const long long tg = t0 + g * RK_GROUP;
    int tcol[RK_GROUP];                   // the group's columns (-1 beyond the row's last target) and keys: uniform
    unsigned long long tkey[RK_GROUP];
#pragma unroll
    for (int q = 0; q < RK_GROUP; ++q) {
      const bool live = tg + q < t1;
      tcol[q] = live ? indices[tg + q] : -1;   // (inside [0, n): checked on the host)
      tkey[q] = live ? key_at(tcol[q]) : 0ull;
    }
    if (tid < 3 * RK_GROUP + 1) total[tid] = 0u;
    __syncthreads();

    unsigned int above[RK_GROUP], equal[RK_GROUP], left[RK_GROUP], eligible = 0u;
#pragma unroll
    for (int q = 0; q < RK_GROUP; ++q) above[q] = equal[q] = left[q] = 0u;
    for (long long j = tid; j < n; j += RK_THREADS) {
      const unsigned long long k = key_at(j);
      eligible += k != 0ull ? 1u : 0u;
#pragma unroll
      for (int q = 0; q < RK_GROUP; ++q) {
        const bool eq = k == tkey[q];
        above[q] += k > tkey[q] ? 1u : 0u;
        equal[q] += eq ? 1u : 0u;
        left[q] += eq && j < tcol[q] ? 1u : 0u;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
      for (int q = 0; q < RK_GROUP; ++q) {
        above[q] += __shfl_xor(above[q], off, 64);
        equal[q] += __shfl_xor(equal[q], off, 64);
        left[q] += __shfl_xor(left[q], off, 64);
      }
      eligible += __shfl_xor(eligible, off, 64);
    }
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < RK_GROUP; ++q) {
        atomicAdd(&total[q], above[q]);
        atomicAdd(&total[RK_GROUP + q], equal[q]);
        atomicAdd(&total[2 * RK_GROUP + q], left[q]);
      }
      atomicAdd(&total[3 * RK_GROUP], eligible);
    }
    __syncthreads();

    if (tid < RK_GROUP && tg + tid < t1) {
      int col = -1;                       // (this thread's target, picked without indexing the register arrays)
      unsigned long long key = 0ull;
#pragma unroll
      for (int q = 0; q < RK_GROUP; ++q)
        if (q == tid) {
          col = tcol[q];
          key = tkey[q];
        }
      const bool ranked = key != 0ull;    // then the target itself is one of the `equal`
      const long long a = ranked ? (long long)total[tid] : -1;
      const long long t = ranked ? (long long)total[RK_GROUP + tid] - 1 : -1;
      const long long r = ranked ? a + (long long)total[2 * RK_GROUP + tid] : -1;
      if (out_rank) out_rank[tg + tid] = r;
      if (out_above) out_above[tg + tid] = a;
      if (out_tied) out_tied[tg + tid] = t;
      if (out_scores) out_scores[tg + tid] = row[col];
    }
    if (g == 0 && tid == RK_GROUP && out_eligible) out_eligible[blockIdx.x] = (long long)total[3 * RK_GROUP];
    __syncthreads();   // (the next group clears the counters)
  }
}
