// nbmf_moment_kernels.inc -- expected counts of the data under Theta = W^T H, by (row, feature group) and by feature
// (nbmf_moment_rows_v; DESIGN.md 4.17): per slot the five integer sums N_OBS, N_ONES, S1, S2, S1_ONES that the expected
// count, its variance, the z-score of the observed count, the Brier score and Tjur's coefficient are functions of.
// Included by nbmf_hip.hip after nbmf_hist_kernels.inc: moment_rows_kernel opens with THETA_TILE, the very statements
// predict_rows_kernel, score_rows_kernel and theta_hist_kernel open with, so the Theta it sums is bit for bit the entry
// predict_rows_kernel<0> stores with the clip on -- but no Theta panel is ever written: what leaves the kernel are integer
// adds.  No floating-point atomics, no workgroup barrier.

constexpr int MO_FIELDS = 5;   // NBMF_MOMENT_FIELDS: N_OBS, N_ONES, S1, S2, S1_ONES
constexpr int MO_WORDS = 4;    // 64-bit words of a slot in LDS: the two counts share one (N_OBS low, N_ONES high)

// rint(v) as an integer for an integral-after-rounding v in [0, 2^32]: v + 2^52 is ONE rounded addition whose result lies
// in [2^52, 2^53), where a double's spacing is 1 -- the addition rounds v to the nearest integer, ties to even, exactly
// rint -- and whose low 52 bits are that integer.  (Nothing next to the addition to contract with: v is a product by a
// power of two, exact, so an fma of the two is the same value.)
__device__ __forceinline__ unsigned long long moment_rint(double v) {
  return (unsigned long long)__double_as_longlong(v + 4503599627370496.0) & 0x000fffffffffffffull;
}

// Rows [prow0, prow0 + pnrows) of Theta, clipped to [0, 1], against the staged data panel xd and the staged mask panel md
// (bytes, exactly as theta_hist_kernel takes them: row 0 = row prow0, leading dimension ldp, a multiple of 4 >= n; nonzero
// = class 1 / observed; md null: every entry is observed) and the labels col_group[0 .. nA): the group of a column in
// [0, G), or -1 for "in no group"; the pad columns are -1.  An entry is LIVE where its panel row is inside [0, pnrows), its
// column is < n and it is observed -- the rules of score_rows_kernel.  With Q = 2^32 (NBMF_MOMENT_FRAC_BITS),
//   q1 = rint(theta * Q)              (the product is exact)
//   q2 = rint((theta * theta) * Q)    (one rounded product, then an exact one)
// a live entry whose theta is not NaN adds (1, x != 0, q1, q2, x != 0 ? q1 : 0) to
//   row_tab[(row - prow0) * G + g][0 .. 5)        where g = col_group[column] is not -1 (row_tab may be null), and to
//   col_tab[copy][column][0 .. 5)                 whatever its group (col_tab may be null);
// one whose theta is NaN adds 1 to nan_count[x != 0] and nothing else.  row_tab is the table of THIS panel (the host
// zeroes it before the launch); col_tab and nan_count run over all panels of the call.  col_tab is kept in `copies`
// copies of n * 5 words: a workgroup adds onto the copy blockIdx.x picks (modulo) -- the workgroups in flight at one time
// are consecutive 16-row tiles of the SAME columns, which would otherwise queue on the same words -- and
// theta_hist_finish_kernel adds the copies up at the end of the call.
//
// Rows: each wave keeps a table of its own 16 rows x G slots x MO_WORDS words in LDS (its quarter of the dynamic LDS:
// G * 2 KiB per workgroup, 32 KiB at G = 16).  It zeroes the words; every lane walks its four consecutive columns of a row,
// sums while the group stays the same and adds the run with 64-bit LDS integer atomics (the 16 lanes of a row do meet in a
// slot); then the wave reads the words back, lane l the words l, l + 64, ..., and adds every nonzero one onto row_tab with
// no-return agent-scope 64-bit integer atomics (the strips of a row are other waves and other workgroups).  The three
// steps are ordered INSIDE the wave only, by wavefront-scope fences and wave_barrier, as in theta_hist_kernel: no other
// wave touches these words, and there must be no __syncthreads() -- THETA_TILE lets whole waves leave before the k loop.
// Columns: register sums over a lane's 4 rows, the xor butterfly 16, 32 over the four lane groups (score_rows_kernel's),
// then lanes 0 .. 15 add their four columns' nonzero words onto the copy.
// Every sum is an integer and integer adds commute: nothing depends on the panels, on prow0, on the copies or on the
// order the waves arrive in.  A slot sums at most max(n, nrows) <= 2^30 entries of at most 2^32 each: below 2^63.
__global__ __launch_bounds__(PR_WAVES * 64) void moment_rows_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long n,
    long long prow0, long long pnrows, long long ldp, int G, const unsigned char* __restrict__ xd,
    const unsigned char* __restrict__ md, const int* __restrict__ col_group, unsigned long long* __restrict__ row_tab,
    int copies, unsigned long long* __restrict__ col_tab, unsigned long long* __restrict__ nan_count) {
  extern __shared__ unsigned long long moment_lds[];   // PR_WAVES * 16 * G * MO_WORDS words (none without row_tab)
  THETA_TILE(Wn, Hn, K, mA, nA, prow0, ldp)   // (ldp <= nA)

  const int words = 16 * G * MO_WORDS;
  unsigned long long* mine = moment_lds + wave * words;
  if (row_tab) {
    for (int s = lane; s < words; s += 64) mine[s] = 0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }

  const bool in_panel = jc < ldp;   // ldp is a multiple of 4: jc .. jc+3 are inside the panel's row or all outside
  const int4 grp = *(const int4*)(col_group + jc);   // (jc + 3 < nA: the labels are nA long)
  const int g4[4] = {grp.x, grp.y, grp.z, grp.w};
  unsigned long long cs1[4] = {0, 0, 0, 0}, cs2[4] = {0, 0, 0, 0}, cs1o[4] = {0, 0, 0, 0};
  unsigned int ccnt[4] = {0, 0, 0, 0};   // per column: observed entries in the low half, ones in the high half (<= 16 each)
  unsigned int nan[2] = {0, 0};
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
    // the run of consecutive columns that share a group: counts (N_OBS low, N_ONES high), S1, S2, S1_ONES
    int run_g = -1;
    unsigned long long rc = 0, r1 = 0, r2 = 0, r1o = 0;
    auto flush = [&]() {
      if (rc == 0ull) return;   // (run_g is a group then: rc only grows inside one)
      unsigned long long* slot = mine + ((lr + 4 * r) * G + run_g) * MO_WORDS;
      (void)__hip_atomic_fetch_add(slot + 0, rc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      (void)__hip_atomic_fetch_add(slot + 1, r1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      (void)__hip_atomic_fetch_add(slot + 2, r2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (r1o != 0ull) (void)__hip_atomic_fetch_add(slot + 3, r1o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      rc = r1 = r2 = r1o = 0ull;
    };
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double v = acc[t][r];
      v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);   // np.clip: a NaN stays a NaN
      const bool obs = live && jc + t < n && ((mw >> (8 * t)) & 0xffu) != 0;
      if (!obs) continue;
      const unsigned int one = ((xw >> (8 * t)) & 0xffu) != 0 ? 1u : 0u;
      if (v != v) {
        nan[one] += 1u;
        continue;
      }
      const unsigned long long q1 = moment_rint(v * 4294967296.0), q2 = moment_rint((v * v) * 4294967296.0);
      const unsigned long long q1o = one ? q1 : 0ull;
      ccnt[t] += 1u + (one << 16);
      cs1[t] += q1;
      cs2[t] += q2;
      cs1o[t] += q1o;
      const int g = g4[t];
      if (row_tab && (unsigned int)g < (unsigned int)G) {   // (-1, and anything the host's check would have refused: nowhere)
        if (g != run_g) {
          flush();
          run_g = g;
        }
        rc += 1ull + ((unsigned long long)one << 32);
        r1 += q1;
        r2 += q2;
        r1o += q1o;
      }
    }
    flush();
  }

  if (nan[0] != 0u) (void)__hip_atomic_fetch_add(nan_count + 0, (unsigned long long)nan[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (nan[1] != 0u) (void)__hip_atomic_fetch_add(nan_count + 1, (unsigned long long)nan[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

  if (row_tab) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int s = lane; s < words; s += 64) {
      const unsigned long long w = mine[s];
      if (w == 0ull) continue;   // (a nonzero word belongs to a live entry: its row is inside the panel)
      const int slot = s / MO_WORDS, f = s % MO_WORDS;
      const long long prow = i0 + slot / G - prow0;
      unsigned long long* out = row_tab + ((size_t)prow * G + slot % G) * MO_FIELDS;
      if (f == 0) {
        (void)__hip_atomic_fetch_add(out + 0, w & 0xffffffffull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((w >> 32) != 0ull) (void)__hip_atomic_fetch_add(out + 1, w >> 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      } else {
        (void)__hip_atomic_fetch_add(out + f + 1, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }

  if (col_tab) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        ccnt[t] += (unsigned int)__shfl_xor((int)ccnt[t], off, 64);
        cs1[t] += (unsigned long long)__shfl_xor((long long)cs1[t], off, 64);
        cs2[t] += (unsigned long long)__shfl_xor((long long)cs2[t], off, 64);
        cs1o[t] += (unsigned long long)__shfl_xor((long long)cs1o[t], off, 64);
      }
    }
    if (lr == 0 && in_panel) {
      unsigned long long* copy = col_tab + (size_t)(blockIdx.x % (unsigned int)copies) * (size_t)n * MO_FIELDS;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (ccnt[t] == 0u) continue;   // (no live entry without a NaN theta in this block's column -- or the column is >= n)
        unsigned long long* out = copy + (size_t)(jc + t) * MO_FIELDS;
        (void)__hip_atomic_fetch_add(out + 0, (unsigned long long)(ccnt[t] & 0xffffu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((ccnt[t] >> 16) != 0u)
          (void)__hip_atomic_fetch_add(out + 1, (unsigned long long)(ccnt[t] >> 16), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(out + 2, cs1[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(out + 3, cs2[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cs1o[t] != 0ull) (void)__hip_atomic_fetch_add(out + 4, cs1o[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}
