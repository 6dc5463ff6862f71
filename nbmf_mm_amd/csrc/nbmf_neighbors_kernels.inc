// nbmf_neighbors_kernels.inc -- similarity within one side of the matrix (nbmf_similarity, nbmf_neighbors; DESIGN.md 4.16).
// Included by nbmf_hip.hip after the other kernel files.  The kernels here PREPARE the two operands of an item-by-item
// product and GATHER the query items; the product itself is predict_rows_kernel<0> and the ranking top_n_kernel<1>
// (nbmf_predict_kernels.inc).  Every image is natural layout, [KP][lenA] with element (k, x) at k * lenA + x, like the
// factor images Wn / Hn they are made from; of those only rows k < K and columns x < len are ever read, and an image made
// here is written whole: rows k >= K and columns x >= len are exactly zero.  K is the true component count, whatever
// KP is (sliced K > 128 and ragged K alike): no kernel has a special case for either.  Every sum runs in one fixed order
// and none uses a floating-point atomic: the same factors give the same bits.

constexpr int NB_THREADS = 256;     // the per-item and per-element kernels: one thread per item or element
constexpr int NB_GT = 16;           // gram_partial_kernel: a 16 x 16 tile of G per workgroup, one entry per thread
constexpr int NB_GX = 64;           // ... and 64 items per LDS stage
constexpr int NB_GRAM_BLOCKS = 32;  // most item chunks (partials per entry of G)
constexpr int NB_BT = 8;            // gram_apply_kernel: rows of B per thread

// d[x] = sum_k A[k, x] * B[k, x] for the items x < len, k ascending on one chain, one thread per item (consecutive threads
// read consecutive doubles of a row).  A == B: the squared norm of an item (COSINE); A = F, B = G F: f^T G f (PROFILE).
__global__ __launch_bounds__(NB_THREADS) void item_dot_kernel(const double* __restrict__ A, const double* __restrict__ B, int K,
                                                              long long len, long long lenA, double* __restrict__ d) {
  const long long x = (long long)blockIdx.x * NB_THREADS + threadIdx.x;
  if (x >= len) return;
  double s = 0.0;
  for (int k = 0; k < K; ++k) s = __builtin_fma(A[(size_t)k * lenA + x], B[(size_t)k * lenA + x], s);
  d[x] = s;
}

// out[k, x] = in[k, x] / sqrt(d[x]) for k < K and x < len, and 0 everywhere else on the [KP][lenA] image.  An item with
// d == 0 gets a zero column (its score with everything is 0, not NaN); a NaN d stays NaN.
__global__ __launch_bounds__(NB_THREADS) void item_scale_kernel(const double* __restrict__ in, const double* __restrict__ d, int K,
                                                                int KP, long long len, long long lenA, double* __restrict__ out) {
  const long long x = (long long)blockIdx.x * NB_THREADS + threadIdx.x;
  const int k = blockIdx.y;   // < KP: the grid
  if (x >= lenA) return;
  double v = 0.0;
  if (k < K && x < len) {
    const double dx = d[x];
    if (dx != 0.0) v = in[(size_t)k * lenA + x] / sqrt(dx);
  }
  out[(size_t)k * lenA + x] = v;
}

// The Gram matrix G = C C^T of the OTHER factor over its len items, in two ordered steps.  Step 1: workgroup (blockIdx.x =
// item chunk, blockIdx.y = tile row, blockIdx.z = tile column) adds, for its 16 x 16 tile, the products of the chunk's items
// in ascending order -- thread (ta, tb) owns entry (a0 + ta, b0 + tb); the 2 x 16 rows of C involved pass through LDS 64
// items at a time -- and stores the tile into part[chunk][K][K].  Step 2: gram_sum_kernel adds the chunks of an entry in
// ascending order.  The chunk length depends on len only (the host: a multiple of NB_GX), so G depends on C only.
__global__ __launch_bounds__(NB_GT * NB_GT) void gram_partial_kernel(const double* __restrict__ C, int K, long long len,
                                                                     long long lenA, long long chunk, double* __restrict__ part) {
  __shared__ double sa[NB_GT][NB_GX + 1], sb[NB_GT][NB_GX + 1];
  const int tid = threadIdx.x, ta = tid / NB_GT, tb = tid % NB_GT;
  const int a0 = blockIdx.y * NB_GT, b0 = blockIdx.z * NB_GT;
  const long long x0 = (long long)blockIdx.x * chunk, x1 = x0 + chunk < len ? x0 + chunk : len;
  double s = 0.0;
  for (long long xs = x0; xs < x1; xs += NB_GX) {   // (uniform bounds: every thread meets every barrier)
#pragma unroll
    for (int r = 0; r < NB_GT * NB_GX / (NB_GT * NB_GT); ++r) {   // 4 loads per thread and operand: row r * 4 + tid / 64
      const int row = r * (NB_GT * NB_GT / NB_GX) + tid / NB_GX, col = tid % NB_GX;
      const long long x = xs + col;
      const bool in = x < x1;
      sa[row][col] = in && a0 + row < K ? C[(size_t)(a0 + row) * lenA + x] : 0.0;
      sb[row][col] = in && b0 + row < K ? C[(size_t)(b0 + row) * lenA + x] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int q = 0; q < NB_GX; ++q) s = __builtin_fma(sa[ta][q], sb[tb][q], s);   // (a zero product past x1 adds +0.0: no change)
    __syncthreads();
  }
  if (a0 + ta < K && b0 + tb < K) part[((size_t)blockIdx.x * K + a0 + ta) * K + b0 + tb] = s;
}

__global__ __launch_bounds__(NB_THREADS) void gram_sum_kernel(const double* __restrict__ part, int K, int chunks,
                                                              double* __restrict__ G) {
  const int e = blockIdx.x * NB_THREADS + threadIdx.x;
  if (e >= K * K) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(size_t)c * K * K + e];
  G[e] = s;
}

// B = G F on the [K][lenA] part of an image: B[a, x] = sum_b G[a, b] F[b, x], b ascending on one chain.  One thread per item
// and NB_BT rows of B (blockIdx.y): a row of F is read once per NB_BT rows; G's entries are the same for the whole wave.
__global__ __launch_bounds__(NB_THREADS) void gram_apply_kernel(const double* __restrict__ G, const double* __restrict__ F, int K,
                                                                long long len, long long lenA, double* __restrict__ B) {
  const long long x = (long long)blockIdx.x * NB_THREADS + threadIdx.x;
  const int a0 = blockIdx.y * NB_BT;
  if (x >= len) return;
  double acc[NB_BT];
#pragma unroll
  for (int r = 0; r < NB_BT; ++r) acc[r] = 0.0;
  for (int b = 0; b < K; ++b) {
    const double f = F[(size_t)b * lenA + x];
#pragma unroll
    for (int r = 0; r < NB_BT; ++r) {
      const int a = a0 + r < K ? a0 + r : K - 1;   // (a clamped row is computed and not stored)
      acc[r] = __builtin_fma(G[(size_t)a * K + b], f, acc[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < NB_BT; ++r)
    if (a0 + r < K) B[(size_t)(a0 + r) * lenA + x] = acc[r];
}

// The query items' columns of the left operand as a compact [KP][nqA] image: out[k, t] = left[k, query[t]] for k < K and
// t < nq, and 0 everywhere else.  The product kernel then sees plain rows 0 .. nq - 1, whatever the list repeats or how it
// is ordered.  The indices were checked on the host: every query[t] is in [0, len).
__global__ __launch_bounds__(NB_THREADS) void gather_items_kernel(const double* __restrict__ left, long long lenA,
                                                                  const long long* __restrict__ query, int K, long long nq,
                                                                  long long nqA, double* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NB_THREADS + threadIdx.x;
  const int k = blockIdx.y;   // < KP: the grid
  if (t >= nqA) return;
  out[(size_t)k * nqA + t] = (k < K && t < nq) ? left[(size_t)k * lenA + query[t]] : 0.0;
}
