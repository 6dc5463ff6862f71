// nbmf_score_kernels.inc -- the Bernoulli log-likelihood of Theta = W^T H against data, per row and per column
// (nbmf_score_rows; DESIGN.md 4.8).  Included by nbmf_hip.hip after nbmf_predict_kernels.inc: score_rows_kernel opens with
// that file's THETA_TILE, the very statements predict_rows_kernel opens with, so the Theta it scores is bit for bit the
// entry predict_rows_kernel<0> stores -- but no Theta panel is ever written: what leaves the kernel is one partial sum and
// one count per (row, 64-column strip) and per (16-row block, column).  No floating-point atomics, no LDS, no barrier.

// The term of one observed entry, its logarithm's argument formed in exactly the order the header gives (additions only
// around it: nothing to contract), with the device library's log (<= 1 ulp), not the sweeps' table logarithm.
__device__ __forceinline__ double score_term_u8(double th, bool one, double eps) {
  return log(one ? th + eps : (1.0 - th) + eps);
}

// x in [0, 1]: x log(theta + eps) + (1 - x) log((1 - theta) + eps) -- two products, each rounded, then their sum, as NumPy
// evaluates the expression: no FMA contraction.
__device__ __forceinline__ double score_term_f64(double th, double x, double eps) {
#pragma clang fp contract(off)
  const double la = log(th + eps), lb = log((1.0 - th) + eps);
  const double pa = x * la, pb = (1.0 - x) * lb;
  return pa + pb;
}

// Rows [prow0, prow0 + pnrows) of Theta against the staged data panel xd (row 0 = row prow0; leading dimension ldp, a
// multiple of 4 >= n: bytes for X_F64 == 0, where nonzero means x = 1, doubles otherwise) and the staged mask panel md
// (bytes, leading dimension ldp, nonzero = observed; null: every entry is).  What the panels hold in columns n .. ldp-1 is
// read and never used.
//
// After THETA_TILE (nbmf_predict_kernels.inc) register r of a lane's acc[t] holds Theta[i0 + (l >> 4) + 4r, jc + t],
// t = 0..3, jc = j0 + 4 (l & 15) -- 4 rows x 4 consecutive columns, whose data are one 4-byte word (one 32-byte
// access for doubles) per row, and the mask likewise.  term[r][t] is the entry's term, or nothing (+0.0, count 0) where
// the entry is unobserved, its column is >= n or its row is outside the panel.
//   rows:    ((term[r][0] + term[r][1]) + term[r][2]) + term[r][3], then the xor butterfly 1, 2, 4, 8 over the 16 lanes
//            that share the row: row_part / row_cnt [strip * pnrows + (row - prow0)], strip = j0 / 64.
//   columns: ((term[0][t] + term[1][t]) + term[2][t]) + term[3][t] (rows ascending), then the xor butterfly 16, 32 over
//            the four lane groups: col_part / col_cnt [block * ldp + column], block = blockIdx.x, the 16-row block of the
//            ABSOLUTE row grid counted from the panel's first.
// Every step has a fixed order, so a row partial depends on that row, the factors, its data and its mask bytes only, and
// a column partial on the block's rows inside the panel.  The counts travel through the butterflies four to a word, one
// byte each (a row partial counts at most 64 entries, a column partial at most 16).
// row_part or col_part may be null: that half is then not reduced or stored.  Strips that lie wholly beyond the panel's
// leading dimension leave at once (a whole wave: there is no barrier anywhere).
template <int X_F64>
__global__ __launch_bounds__(PR_WAVES * 64) void score_rows_kernel(
    const double* __restrict__ Wn, const double* __restrict__ Hn, int K, long long mA, long long nA, long long n,
    long long prow0, long long pnrows, long long ldp, int clip, double eps, const void* __restrict__ xd,
    const unsigned char* __restrict__ md, double* __restrict__ row_part, int* __restrict__ row_cnt,
    double* __restrict__ col_part, int* __restrict__ col_cnt) {
  THETA_TILE(Wn, Hn, K, mA, nA, prow0, ldp)   // (ldp <= nA)

  const bool in_panel = jc < ldp;   // ldp is a multiple of 4: jc .. jc+3 are inside the panel's row or all outside
  double term[4][4];
  unsigned int rcnt = 0, ccnt = 0;   // byte r: observed entries of row r; byte t: of column t
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const long long prow = i0 + lr + 4 * r - prow0;
    const bool live = in_panel && prow >= 0 && prow < pnrows;
    uint32_t xw = 0, mw = 0;
    d4 xv = d4{0.0, 0.0, 0.0, 0.0};
    if (live) {
      const size_t at = (size_t)prow * ldp + jc;
      if (X_F64) xv = *(const d4*)((const double*)xd + at);
      else xw = *(const uint32_t*)((const unsigned char*)xd + at);
      mw = md ? *(const uint32_t*)(md + at) : 0x01010101u;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      double v = acc[t][r];
      if (clip) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);   // np.clip: a NaN stays a NaN
      const bool obs = live && jc + t < n && ((mw >> (8 * t)) & 0xffu) != 0;
      double s = 0.0;
      if (obs) {
        s = X_F64 ? score_term_f64(v, xv[t], eps) : score_term_u8(v, ((xw >> (8 * t)) & 0xffu) != 0, eps);
        rcnt += 1u << (8 * r);
        ccnt += 1u << (8 * t);
      }
      term[r][t] = s;
    }
  }

  if (row_part) {
    double rs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rs[r] = ((term[r][0] + term[r][1]) + term[r][2]) + term[r][3];
#pragma unroll
    for (int off = 1; off <= 8; off <<= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) rs[r] += __shfl_xor(rs[r], off, 64);
      rcnt += (unsigned int)__shfl_xor((int)rcnt, off, 64);   // (<= 64 per byte: no carry between the bytes)
    }
    if (lc == 0) {
      const size_t strip = (size_t)(j0 / PR_STRIP);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long prow = i0 + lr + 4 * r - prow0;
        if (prow < 0 || prow >= pnrows) continue;
        row_part[strip * (size_t)pnrows + prow] = rs[r];
        row_cnt[strip * (size_t)pnrows + prow] = (int)((rcnt >> (8 * r)) & 0xffu);
      }
    }
  }

  if (col_part) {
    double cs[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) cs[t] = ((term[0][t] + term[1][t]) + term[2][t]) + term[3][t];
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
#pragma unroll
      for (int t = 0; t < 4; ++t) cs[t] += __shfl_xor(cs[t], off, 64);
      ccnt += (unsigned int)__shfl_xor((int)ccnt, off, 64);
    }
    if (lr == 0 && in_panel) {   // 16 lanes: 512 contiguous bytes of sums, 256 of counts
      const size_t at = (size_t)blockIdx.x * ldp + jc;
      *(d4*)(col_part + at) = d4{cs[0], cs[1], cs[2], cs[3]};
      *(int4*)(col_cnt + at) =
          make_int4((int)(ccnt & 0xffu), (int)((ccnt >> 8) & 0xffu), (int)((ccnt >> 16) & 0xffu), (int)(ccnt >> 24));
    }
  }
}

// The partials of one panel row, strip after strip in ascending order: its log-likelihood sum and its observed count.
__global__ __launch_bounds__(256) void score_rows_finish_kernel(const double* __restrict__ row_part,
                                                                 const int* __restrict__ row_cnt, long long pnrows,
                                                                 long long strips, double* __restrict__ row_ll,
                                                                 long long* __restrict__ row_obs) {
  const long long prow = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (prow >= pnrows) return;
  double s = 0.0;
  long long c = 0;
  for (long long q = 0; q < strips; ++q) {
    s += row_part[(size_t)q * pnrows + prow];
    c += row_cnt[(size_t)q * pnrows + prow];
  }
  row_ll[prow] = s;
  row_obs[prow] = c;
}

// The column partials of one panel, 16-row block after block in ascending order, onto the running per-column accumulators
// of the call (zeroed before its first panel): one chain per column over all the blocks of the call, whatever the panels.
__global__ __launch_bounds__(256) void score_cols_finish_kernel(const double* __restrict__ col_part,
                                                                 const int* __restrict__ col_cnt, long long blocks,
                                                                 long long ldp, long long n, double* __restrict__ col_ll,
                                                                 long long* __restrict__ col_obs) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s = col_ll[j];
  long long c = col_obs[j];
  for (long long b = 0; b < blocks; ++b) {
    s += col_part[(size_t)b * ldp + j];
    c += col_cnt[(size_t)b * ldp + j];
  }
  col_ll[j] = s;
  col_obs[j] = c;
}
