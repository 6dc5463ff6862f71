// Part of libnbmf_hip (see nbmf_hip.hip for the overview).  Included into the single translation unit
// nbmf_hip.hip; everything here lives in its anonymous namespace.
// The fused sweep: pass_kernel<KB, DATA, MODE> (DESIGN.md 4.1).

#define NBMF_DIV(y_, d_) ((y_) * rcp_nr(d_))   // within 1.5 ulp of the quotient (tests: op 2 of nbmf_selftest_unary)
// The two quotients of an entry, ya / (Theta + eps) and yb / (1 - Theta + eps), from ONE reciprocal, that of the product
// of the two denominators (they add up to 1 + 2 eps, so the product cannot underflow): a v_rcp_f64 issues at a quarter
// of the rate and drags three Newton FMAs behind it.  Each quotient within ~2.5 ulp.
#define NBMF_DIV2(ya_, da_, yb_, db_, qa_, qb_) \
  {                                             \
    const double it_ = rcp_nr((da_) * (db_));   \
    qa_ = (ya_) * (it_ * (db_));                \
    qb_ = (yb_) * (it_ * (da_));                \
  }

// ------------------------------------------------------------------------------------------
// The fused pass kernel.
//   D      data matrix of this pass, R row blocks x C column strips of 16x16 tiles
//   L      the factor indexed by D's rows (streamed through LDS):  LT = Theta operand, LG = back operand
//   Rf     the factor indexed by D's columns (stationary in registers, T form)
//   MODE_H: out1 = L (R1), out2 = L (R2)                  (P1, P2 of _solver.py:42-43)
//   MODE_W: out1 = L (S1 - S2) + column sums of S2         (the bracket of _solver.py:53)
//   MODE_L: no products; strictly masked log-likelihood only (held-out perplexity, evaluation)
//   MODE_T: Theta only, stored (or added to what is stored) in tile order -- n_components > 128 runs as slices
//           of 128 components: all slices but the last add their part of Theta with a MODE_T sweep; the LAST
//           slice's H/W/L sweep (template parameter TH = 2) adds its own part to what is stored, stores the
//           total and goes on with its products; the other slices' sweeps (TH = 1) read the total instead of
//           computing anything
// Workgroup = 4 waves; wave w owns column strip 4*blockIdx.x + w and sweeps row blocks
// [chunk*CH, chunk*CH + CH).  Partial results go to per-chunk slabs (ordered reduction later: no
// atomics, bitwise reproducible).
// ------------------------------------------------------------------------------------------
// The f64 MFMA of the sweeps.  NBMF_NO_MFMA=1 (measurement builds only, results are garbage) swaps it for a stub that
// keeps its operands alive but issues nothing: what is left is the sweep's skeleton -- staging, LDS reads, the ratio
// arithmetic -- whose time per tile is what the real kernel spends besides its MFMAs if nothing overlaps (DESIGN.md 4.1).
#if NBMF_NO_MFMA
__device__ __forceinline__ d4 mfma_stub(double a, double b, d4 c) {
  __asm__ volatile("" : "+v"(c) : "v"(a), "v"(b));
  return c;
}
#define NBMF_MFMA(a_, b_, c_, x_, y_, z_) mfma_stub((a_), (b_), (c_))
#else
#define NBMF_MFMA(a_, b_, c_, x_, y_, z_) __builtin_amdgcn_mfma_f64_16x16x4f64((a_), (b_), (c_), (x_), (y_), (z_))
#endif

// A wave's run of an operand image, HBM/L2 -> LDS by LDS-DMA: PPW pieces of 1 KiB (16 bytes per lane), told apart by
// the instruction's immediate offset, which the hardware adds to the memory address and to the LDS address alike.
typedef __attribute__((address_space(3))) char lds_char;
typedef const __attribute__((address_space(1))) char glb_char;
typedef const __attribute__((address_space(1))) uint32_t glb_u32;
template <int PPW>
__device__ __forceinline__ void dma_run(glb_char* g, lds_char* l) {
  static_assert(PPW == 2 || PPW == 4, "2 KiB or 4 KiB per wave and image");
  __builtin_amdgcn_global_load_lds(g, l, 16, 0, 0);
  __builtin_amdgcn_global_load_lds(g, l, 16, 1024, 0);
  if (PPW == 4) {
    __builtin_amdgcn_global_load_lds(g, l, 16, 2048, 0);
    __builtin_amdgcn_global_load_lds(g, l, 16, 3072, 0);
  }
}
// The other split of a stage over the four waves (round 3): piece u of wave w is bytes
// [4096 u + 1024 w, + 1024) of the image, so the four waves' simultaneous requests cover 4 KiB of consecutive
// addresses.  4096 does not fit the immediate offset: the second piece takes a second lane-offset register and a
// second M0 write.
__device__ __forceinline__ void dma_pair_interleaved(glb_char* base, unsigned lane_off, unsigned lane_off_4k, lds_char* l) {
  __builtin_amdgcn_global_load_lds(base + lane_off, l, 16, 0, 0);
  __builtin_amdgcn_global_load_lds(base + lane_off_4k, l + 4096, 16, 0, 0);
}

// Binary path: what a sweep reads of the data is the LANE-MASK image (round 3), one 64-byte record per 16x16 tile:
//   word r     (r = 0..3): bit l set <=> entry r of lane l (row 4r + l/16, column l%16 of the tile) is an observed one
//   word 4 + r           : ...                                                              is an observed zero
// built once from the byte codes (mask_build_kernel).  A wave fetches its tile's record with ONE scalar load into the
// SGPR pairs its v_cndmask_b32 selects read directly: no code dword per lane, no byte compares (4 per H tile, 8 per W
// tile) and no masking ANDs -- vector instructions that each cost an issue slot beside the f64 MFMAs (configs[1]:
// W-pass -8 %, H-pass -3 %; configs[2]: -1 %) -- and a quarter of the bytes.  The byte codes stay for the kernels that
// work per lane (single-launch path, row counts, sparse upload).
typedef const __attribute__((address_space(4))) unsigned long long tile_masks_t;

// Loss assembly + stop rule of the iteration a sweep has scored, inside that sweep (single GPU: no launch of its own
// between the H-pass and the H-update).  Round 4: THE VALUE IS THE MESSAGE.  Every workgroup hands in its log-likelihood
// partial with ONE agent-scope atomic 64-bit store into its slot of a buffer that holds LL_EMPTY -- a NaN bit pattern no
// computation produces -- in every slot between sweeps, and is done.  The sweep's last workgroup IN LAUNCH ORDER (it
// starts in the final round) finishes its own work, then reads the slots with agent-scope atomic loads until none is
// empty, sums them in the fixed order finalize_kernel uses -- the losses do not depend on timing -- and empties the slots
// again for the next sweep.  A slot's arrival IS its data: no second location whose order against the first would need
// a release / acquire pair (round 3's ticket counter: a drained store, an atomic and its round trip in every workgroup's
// epilogue -- 9 us of a 200 us sweep at configs[1] against the W sweep's 2.6 -- plus an acquire whose necessity rested
// on a litmus run).  The wait is bounded (PassFin::wait_ticks, 3 s) -- never a hung grid.  On expiry (round 6: a GPU shared
// with a tenant that saturates it holds a 64 ms sweep's workgroups back for longer than that; tests/test_gpu_configs.py)
// nothing is assembled, the run's stop flag goes up so that every later kernel returns at once, and nbmf_run RESUMES from
// the factors this sweep read with the loss in a launch of its own for the rest of the run (counted: nbmf_variant_stats;
// tested with a workgroup that withholds its partial: NBMF_PASSFIN_FAULT).
constexpr unsigned long long LL_EMPTY = 0x7FF8DEADC0DE0001ull;
constexpr unsigned long long LL_WAIT_TICKS = 300000000ull;   // 3 s of the 100 MHz wall clock
struct PassFin {
  int on;               // 0 = the caller launches finalize_kernel itself; 2 = (tests: NBMF_PASSFIN_FAULT) workgroup (0, 0) never hands in its partial
  unsigned long long wait_ticks;   // bound of the assembling workgroup's wait, in 100 MHz ticks
  int t;                // index of the loss
  int n_ll, n_prior;
  double ll_pad, am1, bm1, n_obs, tol;
  const double* prior;
  double* losses;
  double* scal;
  int* flags;
};
template <bool SC1>
__device__ __forceinline__ void finalize_block(const double* ll_src, int n_ll, double ll_pad, const double* prior, int n_prior,
                                               double am1, double bm1, double n_obs, double* __restrict__ losses, int t,
                                               double tol, double* __restrict__ scal, int* __restrict__ flags, double (*sh)[4]);

struct PassArgs {
  const void* data;     // BIN: lane masks, uint64 [C strips][Rb][8] (see below) ; F64: double [C strips][Rb][64][4]
  const void* mask;     // F64M only, same indexing as data
  const double2* ltab_g;   // general path: the device's 1024-entry logarithm table (log_table_device)
  const double* LT;     // [Rb][K/4][64]
  const double* LG;     // [Rb][K/16][4][64]
  const double* RfT;    // [Cb][K/4][64]
  double* out1;         // [chunks][K][C_alloc]
  double* out2;         // MODE_H only
  double* lossbuf;      // MODE_H/L: [chunks][Cb/4] per-workgroup log-likelihood partials
  const int* done;      // device stop flag: skip all work when set
  int Rb;               // row blocks of D (multiple of 8)
  int Cb;               // column strips of D (multiple of 4)
  const int* chunk_start;   // [chunks + 1] row-block boundaries of the chunks
  int chunk0;               // first chunk of this launch (a sweep may be launched in two parts)
  long long C_alloc;    // 16*Cb
  double eps;
  int strict;           // MODE_L: 1 = only observed entries enter the likelihood; 0 = the loss's semantics (as MODE_H)
  int clip;             // MODE_L: 1 = clip Theta to [0, 1] first (NBMFMM.inverse_transform, _base.py:210)
  double* theta;        // MODE_T / TH = 1: Theta in tile order [C strips][Rb][64 lanes][4]
  int accum;            // MODE_T: 1 = add to the stored Theta (second and later slices), 0 = overwrite
  int tiny_eps;         // BIN loss: eps so small that a product of four entries could underflow -> frexp per entry
  int ksteps, kblocks;  // Theta k-steps (ceil(k / 4)) and 16-blocks of components (ceil(k / 16)) that hold real components: the RAG variant skips the rest
  int full;             // MODE_W, binary path: every entry of the matrix is observed and the swept dimension has no pad rows -> the FULL (two-state) variant
  PassFin fin;          // MODE_H / MODE_L: the loss of the scored iteration, assembled by the last workgroup
  unsigned long long* trace;   // diagnosis (NBMF_PASS_TRACE=1): [workgroup][8] wall-clock ticks at entry, at the loop's top, at its end, at exit; HW_ID of wave 0; ticks behind the loss block and behind the slab stores; shader clocks over the loop
};

// index bits of the general path's logarithm table (log_tab)
constexpr int pass_log_bits(int KB) { return KB == 8 ? 8 : 10; }
// LDS of a workgroup: two stages of 16 KiB (K <= 64; 32 KiB at K = 128) [+ the general path's logarithm table]
constexpr int pass_lds_bytes(int KB, int DATA, int MODE) {
  return (KB <= 4 ? STAGE_BYTES : 2 * STAGE_BYTES) + ((DATA != DATA_BIN && MODE != MODE_W && MODE != MODE_T) ? (16 << pass_log_bits(KB)) : 0);
}
// Workgroups per CU a sweep is compiled for (= waves per SIMD: the register budget is 512 / this per lane).  One line per
// case; tests/test_isa_hazards.py holds every instantiation to zero scratch, whatever is chosen here.
constexpr int pass_wgs_per_cu(int KB, int DATA, int MODE) {
  if (KB == 8) return (MODE == MODE_H && DATA != DATA_BIN) ? 1 : 2;   // K = 128: the general H sweep needs the 512-register form
  if (DATA != DATA_BIN && MODE == MODE_H) return 2;                    // general H sweep, K <= 64: 3 needs <= 168 registers and spills
  if (DATA == DATA_F64 && MODE == MODE_L && KB == 1) return 2;         // general likelihood sweep, K = 16: four tiles per stage in flight, 144 bytes of scratch at 3
  return 3;                                                             // K <= 64, everything else: 16 KiB stages, three workgroups
}
// RAG ("ragged K", round 5): fewer components than the layout holds (k = 10 in the K = 16 layout, 40 in the K = 64 one,
// 100 in the K = 128 one).  The padding rows of both factors are exact zeros, so the Theta k-steps and the back-products'
// 16-blocks that hold nothing but padding multiply zeros onto zeros: this variant skips them behind uniform branches
// (scalar instructions cost nothing beside the MFMAs) -- the same bits, k = 8: two of an H tile's twelve MFMAs fewer,
// k = 40: fourteen of 48.  A variant of its own so that the full-K code is untouched.
// FULL (round 6): W sweeps of the binary path over a matrix whose every entry is observed and whose swept dimension has no
// pad rows -- two states per entry instead of three: no "observed" factor, four words of lane masks instead of eight.
template <int KB, int DATA, int MODE, int TH = 0, bool TINY = false, bool RAG = false, bool FULL = false>
__global__ __launch_bounds__(64 * WG_WAVES, pass_wgs_per_cu(KB, DATA, MODE)) void pass_kernel(PassArgs a) {
  static_assert(TH == 0 || MODE != MODE_T, "a Theta sweep does not read Theta");
  static_assert(!FULL || (MODE == MODE_W && DATA == DATA_BIN && TH == 0 && !TINY), "the two-state variant: W sweeps of the binary path's plain variant");
  // TINY: eps below 1e-70, where a product of four denominators could underflow -- the reciprocals are then taken one
  // by one and the likelihood product is renormalised per entry.  A compile-time variant: as a run-time flag it cost
  // every tile two compares, four branches and a multiplication the compiler could no longer share.
  static_assert(!TINY || MODE != MODE_T, "eps does not change the code of the Theta sweeps");
  static_assert(!RAG || (TH == 0 && !TINY && MODE != MODE_T && KB <= 4), "the ragged-K variant: one slice, plain variant, fused sweeps, up to the K = 64 layout");
  [[maybe_unused]] const int ksteps = a.ksteps, kblocks = a.kblocks;
  constexpr bool PRODUCTS = (MODE == MODE_H || MODE == MODE_W);   // back-products and slabs
  constexpr int K = 16 * KB;
  constexpr int S = K / 4;            // Theta k-steps
  constexpr int NB = (KB >= 4) ? 1 : 4 / KB;   // row blocks per LDS stage: 16 KiB stages (32 KiB at K = 128)
  constexpr int BLK = K * 16;         // doubles per block per operand image
  constexpr int STAGE_D = 2 * NB * BLK;   // doubles per stage: [NB][T image] then [NB][G image]
  constexpr int N2 = NB * BLK / 2;    // double2 per image per stage (512, or 1024 at K = 128)
  extern __shared__ __attribute__((aligned(16))) double lds[];   // two stages (double buffer) [+ the log table]

  [[maybe_unused]] unsigned long long tr0 = 0, tr1 = 0, tr2 = 0, trc = 0;   // (trc: shader clocks over the loop)
  if (a.trace) tr0 = wall_clock64();
  const int stop_now = *a.done;   // (read together with the chunk's bounds below: one trip to memory, not two)
  // general path: the logarithm's table sits behind the stages (first use is after a barrier): 1024 entries copied from
  // the device's one copy in memory (a.ltab_g), which leaves the series a term shorter; at K = 128, where LDS decides how
  // many workgroups a CU holds, the 256 entries the workgroup computes itself
  constexpr bool GEN = DATA != DATA_BIN && MODE != MODE_T;
  constexpr int TB = pass_log_bits(KB);
  // (addressed by its absolute LDS byte offset: this kernel has no static LDS -- checked right here, folded away by the
  //  compiler when true -- so the dynamic region starts at address 0)
  constexpr uint32_t LTAB_BYTE = 2u * STAGE_D * 8u;
  if (GEN && __builtin_amdgcn_groupstaticsize() != 0) return;
  if (GEN && MODE != MODE_W) {
    if (TB == 8) {
      log_table_fill((double2*)(lds + 2 * STAGE_D));
    } else {
      for (int i = threadIdx.x; i < (1 << TB); i += 64 * WG_WAVES) ((double2*)(lds + 2 * STAGE_D))[i] = a.ltab_g[i];
    }
  }
  // Sweeps that compute Theta themselves start its accumulator at eps (see the ratio blocks): the MFMAs deliver
  // t1 = Theta + eps, and (1 + 2 eps) - t1 is 1 - Theta + eps.  General path always; binary path (round 4)
  // in the plain variant, where the host guarantees eps < 2^-22 (the high word of 1 + 2 eps is that of 1.0: tiny_a).
  // W sweeps (round 6, ZE_W): the same start, with a SIGNED z (see the ratio block).  Their sums must keep their EXACT zeros
  // where nothing is observed (a row nobody observed gives 0 / 0 = NaN in the reference, _solver.py:57, and so it does
  // here): an unobserved entry's ratio is multiplied by an exact zero, as before.
  constexpr bool ZE_K = DATA == DATA_BIN && !TINY && TH == 0 && (MODE == MODE_H || MODE == MODE_L);
  constexpr bool ZE_W = DATA == DATA_BIN && !TINY && TH == 0 && MODE == MODE_W;
  constexpr bool EPSACC = (GEN && TH == 0) || ZE_K || ZE_W;
  [[maybe_unused]] const double c12 = (1.0 + a.eps) + a.eps;
  // (evaluation sweeps that clip Theta, and on the binary path the strictly masked ones, keep the reference's own form)
  [[maybe_unused]] const bool l_plain = MODE == MODE_L && (a.clip || (DATA == DATA_BIN && a.strict));
  [[maybe_unused]] const double addeps = (MODE == MODE_L && a.clip) ? a.eps : 0.0;
  const double acc0 = (EPSACC && !l_plain) ? a.eps : 0.0;

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // scalar: LDS-DMA bases stay in SGPRs
  // Workgroup -> (strip group, chunk).  Workgroups go to the 8 XCDs round-robin in launch order, and every
  // strip group of a chunk streams the SAME rows of the L factor: when the chunk count allows, each XCD is given
  // whole chunks, so a panel is pulled into one L2 instead of all eight (H-pass at c3: 1.24 -> 1.00 GB of HBM
  // traffic per launch; the speed does not depend on it).
  unsigned bx = blockIdx.x, by = blockIdx.y;
  if ((gridDim.y & 7u) == 0u) {
    const unsigned id = blockIdx.x + gridDim.x * blockIdx.y;
    const unsigned xcd = id & 7u, slot = id >> 3;   // the slot-th workgroup of that XCD
    bx = slot % gridDim.x;
    by = xcd + 8u * (slot / gridDim.x);
  }
  const int cb = (int)bx * WG_WAVES + wave;   // this wave's strip
  const int chunk = (int)by + a.chunk0;
  const int rb0 = a.chunk_start[chunk];
  const int rb1 = a.chunk_start[chunk + 1];
  if (stop_now) return;
  const double eps = a.eps;

  // stationary operand: Rf in T form for this strip
  double rf[S];
  if (TH != 1) {
#pragma unroll
    for (int s = 0; s < S; ++s) rf[s] = a.RfT[((size_t)cb * S + s) * 64 + lane];
  }

  d4 acc1[KB], acc2[KB];
#pragma unroll
  for (int i = 0; i < KB; ++i) {
    acc1[i] = d4{0, 0, 0, 0};
    acc2[i] = d4{0, 0, 0, 0};
  }
  double prod = 1.0;   // BIN loss: running product of the per-entry Bernoulli probabilities
  int pexp = 0;        //           and its binary exponent
  bool negative = false;   // MODE_L, BIN: some Theta > 1 + eps -> log of a negative number -> NaN, as in NumPy
  int t2hmin = 0x3FF00000;   // general path: smallest high word of a 1 - Theta + eps met, as a signed integer (negative <=> a negative double)
  double llsum = 0.0;  // general path: the sum of the Ym log(t1 / t2)
  double s2 = 0.0;     // MODE_W: column sums of S2

  // this strip's lane-mask records (binary path): uniform address, scalar loads
  [[maybe_unused]] tile_masks_t* tmask = (tile_masks_t*)a.data + (size_t)cb * a.Rb * 8;
  const d4* yv = (const d4*)a.data + (size_t)cb * a.Rb * 64 + lane;
  const d4* mv = (const d4*)a.mask + (size_t)cb * a.Rb * 64 + lane;
  [[maybe_unused]] unsigned lane32 = (unsigned)lane * 32u;   // general path: the lane's 32 bytes of a data tile
  d4* thp = (d4*)a.theta + (size_t)cb * a.Rb * 64 + lane;   // MODE_T / TH: this strip's Theta tiles
  const bool th_in = (TH != 0) || (MODE == MODE_T && a.accum != 0);

  // ---- staging: the operand images of NB row blocks are contiguous in HBM in exactly the LDS order, so a stage is a
  //      linear copy, HBM/L2 -> LDS by LDS-DMA (global_load_lds, 1 KiB per wave-instruction, no VGPRs), issued one stage
  //      ahead into the other buffer and retired by the vmcnt(0) + barrier that ends the stage.
  d4 tnext[NB];   // MODE_T / TH: Theta tiles of the next stage
  [[maybe_unused]] d4 ybuf[2], mbuf[2];   // general path: data (and weight) tile in use / of the next row block
  unsigned lane16 = (unsigned)lane * 16u;   // (not const: see STAGE_DMA)
  // Every wave copies ONE contiguous run of each operand image of the stage (PW_BYTES = 2 KiB, 4 KiB at K = 128), in
  // 1 KiB pieces that differ only in the instruction's immediate offset -- which global_load_lds adds to the memory
  // AND to the LDS address -- so a piece costs no scalar instruction: one M0 write per image and stage.  The stage's
  // source addresses are two scalar pointers carried through the loop and advanced by a constant (pT, pG: T image,
  // G image), not recomputed from the block index.  (Every instruction of the loop,
  // scalar or vector, costs the SIMD an issue slot of ~4 cycles next to the f64 MFMAs -- profiles/r3_*: the sweep's
  // non-MFMA time is its instruction count -- so the ~20 scalar instructions per stage this saves are worth as much as
  // 20 vector ones.)
  constexpr int PPW = N2 * 16 / WG_WAVES / 1024;       // pieces per wave and image
  constexpr bool ILV = PPW == 2;   // waves interleaved piece by piece (see dma_pair_interleaved; c3 W-pass 2.15 -> 2.13 ms)
  constexpr int PW_BYTES = ILV ? 1024 : N2 * 16 / WG_WAVES;   // byte offset between the waves' first pieces
  [[maybe_unused]] unsigned lane16b = (unsigned)lane * 16u + 4096u;
  constexpr unsigned long long STRIDE_TG = (unsigned long long)NB * BLK * 8;
  // (uniform by construction; said so explicitly, half by half, because the pointers are pinned to scalar registers below)
  auto scalar64 = [](unsigned long long v) {
    return ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
           (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  };
  unsigned long long pT = scalar64((unsigned long long)(a.LT + (size_t)rb0 * BLK) + (unsigned long long)wave * PW_BYTES);
  unsigned long long pG = scalar64((unsigned long long)(a.LG + (size_t)rb0 * BLK) + (unsigned long long)wave * PW_BYTES);
#define STAGE_DMA(RB, BUF)                                                                         \
  {                                                                                                \
    lds_char* lT_ = (lds_char*)(lds + (BUF) * STAGE_D) + wave * PW_BYTES;                          \
    /* scalar base + 32-bit lane offset is an addressing mode of its own (no vector add) -- which instruction     */ \
    /* selection only finds while the zero-extension of the offset sits in this block: the lane offsets are made  */ \
    /* opaque IN PLACE each stage (no copy), or hipcc hoists a 64-bit offset and spends a 64-bit vector add per load */ \
    __asm__ volatile("" : "+s"(pT), "+s"(pG));                                                     \
    __asm__ volatile("" : "+v"(lane16));                                                           \
    if (ILV) __asm__ volatile("" : "+v"(lane16b));                                                 \
    const unsigned l16_ = lane16;                                                                  \
    if (TH != 1) { /* Theta read whole from memory: no T image */                                  \
      if (ILV) dma_pair_interleaved((glb_char*)pT, l16_, lane16b, lT_);                            \
      else dma_run<PPW>((glb_char*)pT + l16_, lT_);                                                \
    }                                                                                              \
    if (PRODUCTS) { /* the Theta-only sweeps never read the G image */                             \
      if (ILV) dma_pair_interleaved((glb_char*)pG, l16_, lane16b, lT_ + N2 * 16);                  \
      else dma_run<PPW>((glb_char*)pG + l16_, lT_ + N2 * 16);                                      \
    }                                                                                              \
    if (TH != 0 || MODE == MODE_T) {                                                               \
      if (th_in) {                                                                                 \
        _Pragma("unroll") for (int b_ = 0; b_ < NB; ++b_) tnext[b_] = thp[(size_t)((RB) + b_) * 64]; \
      }                                                                                            \
    }                                                                                              \
  }

  d4 tcurT[NB];
  if (DATA != DATA_BIN && MODE != MODE_T) {
    ybuf[0] = yv[(size_t)rb0 * 64];
    if (DATA == DATA_F64M) mbuf[0] = mv[(size_t)rb0 * 64];
  }
  STAGE_DMA(rb0, 0);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    tcurT[b] = tnext[b];
  }
  __syncthreads();

  // binary path: the lane masks of the tile in hand (lmcur) and of the next one (lmnxt), carried in scalar registers.
  // The record of tile i+1 is requested when tile i's ratio block starts: scalar loads return out of order and share
  // their counter with the LDS reads, so whatever LDS wait comes next also waits for them -- behind the ratio block
  // that is a few hundred cycles away, enough for the record's trip from L2 (a request at the top of the tile, right
  // in front of the first operand wait, stalled every tile for it: H-pass +2 %).
  [[maybe_unused]] lanemask_t lm[2][8];   // [which of the two register sets][word]
#define MASKS_REQUEST(DST, PTR)                                                           \
  if (DATA == DATA_BIN && MODE != MODE_T) {                                               \
    tile_masks_t* rec_ = (PTR);                                                           \
    _Pragma("unroll") for (int r_ = 0; r_ < (((MODE == MODE_W && !FULL) || MODE == MODE_L) ? 8 : 4); ++r_) DST[r_] = rec_[r_]; \
  }
  // (the record pointer is carried and advanced by a constant, not recomputed and clamped per tile: the request of a
  //  sweep's last tile reads the record behind the chunk -- the next chunk's, the next strip's or the image's slack)
  [[maybe_unused]] tile_masks_t* pM = tmask + (size_t)rb0 * 8;
  MASKS_REQUEST(lm[0], pM);
  pM += 8;
  // ... and a software prefetch for them: a scalar load that misses the L2 takes the better part of a microsecond, which
  // no ratio block covers.  Once per stage the wave's 64 lanes read the 256 bytes that hold the records of the four tiles
  // eight blocks ahead (one vector load, consumed a stage later by an XOR into a register nobody looks at): the records
  // are in the L2 when the scalar loads come for them.
  // (its pointer is carried too and runs MASK_PREFETCH + 4 records past the strip's end: slack again.  The value is
  //  consumed at the top of the next stage, in front of the load that replaces it: one XOR, no copy.)
  constexpr int MASK_PREFETCH = 8;   // row blocks ahead of the tile in hand at which the lane-mask records are pulled into the L2
  [[maybe_unused]] double zc[4] = {0.0, 0.0, 0.0, 0.0}, cc[4] = {0.0, 0.0, 0.0, 0.0};   // (H and W sweeps: see the ratio block)
  if ((MODE == MODE_H || MODE == MODE_W || ZE_K) && DATA == DATA_BIN && !TINY) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      // (ZE_K: the low word of z is that of 1 + 2 eps for good -- z is then 1 + 2 eps, or a subnormal that vanishes next to
      //  Theta + eps >= eps; see the ratio block)
      if (ZE_K || ZE_W) zc[r] = mk_double((uint32_t)__double2loint(c12), 0u);
      __asm__ volatile("" : "+v"(zc[r]));
      if (MODE == MODE_W) __asm__ volatile("" : "+v"(cc[r]));
    }
  }
  [[maybe_unused]] uint32_t pf_val = 0, pf_sink = 0;
  [[maybe_unused]] unsigned lane4 = (unsigned)lane * 4u;
  [[maybe_unused]] unsigned long long pPF = 0;
  if (DATA == DATA_BIN && MODE != MODE_T)
    pPF = scalar64((unsigned long long)((const unsigned long long*)a.data + ((size_t)cb * a.Rb + rb0 + MASK_PREFETCH) * 8));
  // Two stages per trip (by hand, a loop with barriers is not unrolled on request): the LDS
  // buffer index is then a constant of each copy and the lane-mask registers change hands by renaming instead of
  // moves; a chunk with an odd number of stages leaves from the middle.
  constexpr int UNR = (MODE != MODE_T && TH == 0 && NB <= 2) ? 2 : 1;   // (more tiles per trip only cost registers)
  // general path: the data tiles are requested through a carried scalar pointer + the lane's offset (no vector address
  // arithmetic), one tile ahead; the request of a sweep's last tile reads the tile behind the chunk (slack again)
  [[maybe_unused]] unsigned long long pY = 0, pMk = 0;
  typedef const __attribute__((address_space(1))) d4 glb_d4;
  if (GEN) {
    pY = scalar64((unsigned long long)((const d4*)a.data + ((size_t)cb * a.Rb + rb0 + 1) * 64));
    if (DATA == DATA_F64M) pMk = scalar64((unsigned long long)((const d4*)a.mask + ((size_t)cb * a.Rb + rb0 + 1) * 64));
  }
  // (constants the general path's vector instructions read from registers: two literals do not fit one instruction,
  //  and left to itself hipcc rebuilds them per use -- a move per logarithm, four per tile for the accumulator's start)
  [[maybe_unused]] double third = 0.33333333333333331483, mquarter = -0.25;
  [[maybe_unused]] d4 acc0q = {acc0, acc0, acc0, acc0};
  if (GEN) __asm__ volatile("" : "+v"(third), "+v"(mquarter));
  if (EPSACC) __asm__ volatile("" : "+v"(acc0q));
  // The running product of the likelihood is renormalised once per trip, not per tile, where that is safe: a trip has at
  // most four tiles, and outside the TINY variant (eps >= 1e-12 and factors in range) every factor is
  // >= eps, so sixteen of them stay above 1e-192.  frexp is exact: the schedule does not change a bit of the result.
  constexpr bool RENORM_TRIP = !TINY && UNR * NB <= 4 && (MODE == MODE_H || MODE == MODE_L);
  [[maybe_unused]] int bufv = 0;
  if (a.trace) {
    tr1 = wall_clock64();
    trc = (unsigned long long)clock64();
  }
  for (int rbo = rb0; rbo < rb1; rbo += UNR * NB) {
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const int rb = rbo + u * NB;
    if (u > 0 && rb >= rb1) break;
    const int buf = (UNR == 2) ? u : bufv;
    if (DATA == DATA_BIN && MODE != MODE_T) {
      pf_sink ^= pf_val;
      __asm__ volatile("" : "+v"(pf_sink));   // (in front of the load, or hipcc issues the load first and copies the old value)
      __asm__ volatile("" : "+s"(pPF));
      __asm__ volatile("" : "+v"(lane4));
      pf_val = *(glb_u32*)((glb_char*)pPF + lane4);
      pPF += 64ull * NB;
    }
    // issue next stage's global loads now; they land while this stage computes (clamped: the last
    // stage re-reads an in-range block, harmlessly)
    // (straight-line on purpose, and with nothing to decide: the fetch of the sweep's last stage runs one stage past
    //  the chunk -- into the next chunk's blocks or, at the very end of an image, into the slack every image is
    //  allocated with (PASS_SLACK) -- and lands in the buffer nobody reads any more.  A branch around it made hipcc's
    //  wait-count insertion put an s_waitcnt vmcnt(0) behind the join, so that every stage waited for the DMA it had
    //  just issued (W-pass +2.5 %); a clamp or a select costs scalar instructions per stage.  Nobody reads buf^1
    //  between the last barrier and the next.)
    pT += STRIDE_TG;
    pG += STRIDE_TG;
    STAGE_DMA(min(rb + NB, a.Rb - NB), buf ^ 1);
    __builtin_amdgcn_sched_barrier(0);   // keep the loads here: hipcc otherwise sinks each one next to its ds_write
    const double* base = lds + buf * STAGE_D;

    // Operand fragments are pulled from LDS in groups of (at most) 8, one group ahead of the MFMAs that
    // use them (8 x 64 cycles of MFMA cover the LDS latency); keeps the fragment registers at 4 x 16.
    constexpr int GRP = 2;   // (8: 2.5 % slower, more registers)
    constexpr int GT = (S < GRP) ? S : GRP;          // Theta k-steps per group
    constexpr int NGT = S / GT;
    constexpr int PB = 4 * KB;                   // back-product operands per tile, order p = r*KB + kb
    constexpr int GB = (PB < GRP) ? PB : GRP;
    constexpr int NGB = PB / GB;
    double tcur[GT];
    if (TH != 1) {
#pragma unroll
      for (int i = 0; i < GT; ++i) tcur[i] = base[i * 64 + lane];
    }

#pragma unroll
    for (int b = 0; b < NB; ++b) {
      // lane masks: this tile's register set and the set the next tile's record is requested into.  The two alternate
      // statically -- by the tile's index in the stage when a stage has an even number of tiles, by the stage's index
      // in the trip otherwise -- so nothing is moved; with one single-tile stage per trip the next set is copied
      // into the current one behind the ratio block.
      constexpr bool LM_ALT = (NB % 2 == 0) || (UNR == 2);
      const int lm_i = (NB % 2 == 0) ? (b & 1) : u;
      [[maybe_unused]] lanemask_t(&lmcur)[8] = lm[LM_ALT ? lm_i : 0];
      [[maybe_unused]] lanemask_t(&lmnxt)[8] = lm[LM_ALT ? (lm_i ^ 1) : 1];
      [[maybe_unused]] d4& ycur = ybuf[LM_ALT ? lm_i : 0];   // (general path: the data tiles alternate the same way)
      [[maybe_unused]] d4& ynx = ybuf[LM_ALT ? (lm_i ^ 1) : 1];
      [[maybe_unused]] d4& mcur = mbuf[LM_ALT ? lm_i : 0];
      [[maybe_unused]] d4& mnx = mbuf[LM_ALT ? (lm_i ^ 1) : 1];
      const double* ldsT = base + b * BLK;
      const double* ldsG = base + NB * BLK + b * BLK;

      // ---- Theta tile: rows 16(rb+b)+4r+q, column 16cb+c in register r of lane (q,c).
      // (two interleaved accumulation chains: a dependent f64 MFMA issues ~10 % slower than an
      //  independent one when the SIMD's other wave is not there to fill the gap)
      constexpr bool DUAL = KB == 8 && MODE == MODE_H && DATA != DATA_BIN;   // only where one wave owns the SIMD (everywhere: -0.6 % at c3, -1.3 % at K = 32 -- the four additions cost more than the dependent issue they avoid)
      d4 th = EPSACC ? acc0q : d4{0, 0, 0, 0}, th2 = {0, 0, 0, 0};
      if (DATA != DATA_BIN && MODE != MODE_T) {
        // general path: the data tile of the NEXT row block is requested now and lands during this tile's
        // arithmetic (the last one of a sweep re-reads an in-range block, harmlessly)
        __asm__ volatile("" : "+s"(pY));
        __asm__ volatile("" : "+v"(lane32));
        ynx = *(glb_d4*)((glb_char*)pY + lane32);
        pY += 2048ull;
        if (DATA == DATA_F64M) {
          __asm__ volatile("" : "+s"(pMk));
          mnx = *(glb_d4*)((glb_char*)pMk + lane32);
          pMk += 2048ull;
        }
      }
      if (TH != 0 || MODE == MODE_T) {
        if (th_in) th = tcurT[b];   // TH = 1: the whole Theta; TH = 2 / MODE_T: what the earlier slices have added up
      }
#pragma unroll
      for (int g = 0; g < NGT && TH != 1; ++g) {
        double tnxt[GT];
        if (g + 1 < NGT) {
#pragma unroll
          for (int i = 0; i < GT; ++i) tnxt[i] = ldsT[((g + 1) * GT + i) * 64 + lane];
          __builtin_amdgcn_sched_barrier(0);   // keep the reads ahead of the MFMAs that hide them
        }
#pragma unroll
        for (int i = 0; i < GT; i += 2) {
          if (RAG) {
            if (g * GT + i < ksteps) th = NBMF_MFMA(tcur[i], rf[g * GT + i], th, 0, 0, 0);
            if (g * GT + i + 1 < ksteps) th = NBMF_MFMA(tcur[i + 1], rf[g * GT + i + 1], th, 0, 0, 0);
            continue;
          }
          th = NBMF_MFMA(tcur[i], rf[g * GT + i], th, 0, 0, 0);
          if (DUAL) {
            th2 = NBMF_MFMA(tcur[i + 1], rf[g * GT + i + 1], th2, 0, 0, 0);
          } else {
            th = NBMF_MFMA(tcur[i + 1], rf[g * GT + i + 1], th, 0, 0, 0);
          }
        }
        if (g + 1 < NGT) {
#pragma unroll
          for (int i = 0; i < GT; ++i) tcur[i] = tnxt[i];
        }
      }
      if (DUAL) th += th2;
      if (TH == 2) thp[(size_t)(rb + b) * 64] = th;   // the total, for the other slices' sweeps
      if (MODE == MODE_T) {
        thp[(size_t)(rb + b) * 64] = th;
        if (b + 1 < NB) {
#pragma unroll
          for (int i = 0; i < GT; ++i) tcur[i] = base[(b + 1) * BLK + i * 64 + lane];
        }
        continue;
      }
      if (MODE == MODE_L && a.clip) {
#pragma unroll
        for (int r = 0; r < 4; ++r) th[r] = fmin(fmax(th[r], 0.0), 1.0);
      }

      // first back-product operand group: issued now, lands during the ratio arithmetic
      double gcur[GB];
      if (PRODUCTS) {
#pragma unroll
        for (int i = 0; i < GB; ++i) gcur[i] = ldsG[((i % KB) * 4 + (i / KB)) * 64 + lane];
      } else if (b + 1 < NB && TH != 1) {
#pragma unroll
        for (int i = 0; i < GT; ++i) tcur[i] = base[(b + 1) * BLK + i * 64 + lane];
      }
      __builtin_amdgcn_sched_barrier(0);

      // Wave priority by phase: a wave in its (short) vector phase issues ahead of the SIMD's other waves, so that it
      // is back at its MFMAs sooner -- where MFMAs are scarce: K <= 32 (configs[1] +1.2 %) and the W sweep at K = 64
      // (-0.5 %); the H sweep at K = 64 and everything at K = 128 lose 0.3 % by it (the other way round,
      // MFMA phases first: no effect anywhere)
      constexpr bool PRIO = KB <= 2 || (MODE == MODE_W && KB == 4);
      if (PRIO) __builtin_amdgcn_s_setprio(1);
      // ---- ratios
      double R1[4], R2[4];
      {
      if (DATA == DATA_BIN) {
        // f64 MFMAs and every other instruction share the SIMD's issue slots on this chip, so the instruction count of
        // this block is the lever that is left (DESIGN.md 4.1).  The tile's lane masks arrive by ONE scalar load
        // (tile_masks_t above: observed ones, observed zeros, 64 lanes each per entry r), requested at the top of the
        // tile, and are read by the selects as they are.
        {   // (the next tile's record; pinned here: hipcc otherwise sinks the request towards its use)
          MASKS_REQUEST(lmnxt, pM);
          pM += 8;
          __builtin_amdgcn_sched_barrier(0);
        }
        lanemask_t ym[4], zo[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ym[r] = lmcur[r];
          zo[r] = lmcur[((MODE == MODE_W && !FULL) || MODE == MODE_L) ? 4 + r : r];
        }
        double dd[4];
        if (MODE == MODE_L) {
          // d = ym ? Theta+eps : (1-Theta)+eps -- the reference's own expressions, also for Theta > 1 (which the
          // un-normalised start of transform() can produce).  strict: only observed entries (ones or zeros) enter the
          // product; otherwise every entry does, exactly as in MODE_H (pad entries are divided out later)
          if (ZE_K && !l_plain) {
            // (the loss's semantics on factors a fit keeps: the H sweep's own denominators, bit for bit -- the last
            //  iteration's loss comes from this sweep, every other one from the next H sweep)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              zc[r] = mk_double((uint32_t)__double2loint(zc[r]), __builtin_amdgcn_inverse_ballot_w64(ym[r]) ? 0u : 0x3FF00000u);
              dd[r] = __builtin_fabs(th[r] - zc[r]);
            }
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const double dr = sel64(ym[r], th[r], 1.0 - th[r]) + eps;
              dd[r] = a.strict ? sel64(ym[r] | zo[r], dr, 1.0) : dr;
            }
          }
        } else {
          // the four entries' dependent chains (select -> +eps -> reciprocal) written side by side, so that each
          // step of one entry issues in the shadow of the same step of the others
          double d[4], r0[4], e[4], rr[4];
          // H sweeps of a fit (Theta < 1: W on the simplex, H <= 1 - eps; the host sends everything else to the TINY
          // variant): with z = 0 for an observed one and 1 otherwise, |Theta - z| IS the selected Theta or 1 - Theta,
          // bit for bit, and r z, r - r z ARE the two ratios -- one select per entry instead of four
          constexpr bool ZT = (MODE == MODE_H || MODE == MODE_W) && !TINY;
          [[maybe_unused]] double z[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            if (ZT) {
              // (the low word of z is always zero: four register pairs live through the sweep, only their high words
              //  are written, or hipcc copies a zero into a fresh pair per entry and tile)
              // (W sweeps: z = 1 for an OBSERVED ZERO and 0 for everything else -- an unobserved entry or a pad then gets
              //  Theta + eps for a denominator, any positive number doing for a ratio that is multiplied by zero below)
              // (W sweeps that compute Theta themselves, ZE_W, round 6: a SIGNED z -- -(1 + 2 eps) for an observed zero, the
              //  subnormal for everything else -- so that d = t1 + z is Theta + eps or -(1 - Theta + eps): the reciprocal
              //  then carries the sign S1 - S2 needs, and r z is (1 + 2 eps) S2 or ~0.  FULL: "not an observed one" IS an
              //  observed zero.)
              const uint32_t zhi = ZE_W ? (FULL ? (__builtin_amdgcn_inverse_ballot_w64(ym[r]) ? 0u : 0xBFF00000u)
                                                : (__builtin_amdgcn_inverse_ballot_w64(zo[r]) ? 0xBFF00000u : 0u))
                                   : (MODE == MODE_W) ? (__builtin_amdgcn_inverse_ballot_w64(zo[r]) ? 0x3FF00000u : 0u)
                                                      : (__builtin_amdgcn_inverse_ballot_w64(ym[r]) ? 0u : 0x3FF00000u);
              zc[r] = mk_double((uint32_t)__double2loint(zc[r]), zhi);
              z[r] = zc[r];
              // ZE_K: Theta's accumulator started at eps and z is 0' (a subnormal) or 1 + 2 eps: |t1 - z| is t1 = Theta + eps
              // or 1 - Theta + eps in ONE instruction (the absolute value rides on its readers as a source modifier) --
              // to rounding: what is exact in the other form, 1 - Theta, is here a difference of two numbers rounded at
              // the size of 1, as Theta itself is
              d[r] = ZE_W ? th[r] + z[r] : ZE_K ? __builtin_fabs(th[r] - z[r]) : __builtin_fabs(th[r] - z[r]) + eps;
            } else {
              d[r] = sel64(ym[r], th[r], 1.0 - th[r]) + eps;
            }
          }
          constexpr bool batch = !TINY;
          if (batch) {
            // The four reciprocals of a lane from ONE: 1/d0 = d1 (d2 d3) / (d0 d1 d2 d3), ...  (batch inversion).
            // v_rcp_f64 issues at a quarter of the rate and drags three Newton FMAs behind it; six multiplications
            // replace three such chains, and the H-mode needs the product anyway for the likelihood: 60 (H) / 48 (W)
            // issue cycles fewer per tile.  Each reciprocal is then within ~2.5 ulp instead of 1 (three roundings on top
            // of the reciprocal's); eps below 1e-70, where the product of four could underflow, keeps the chains.
            const double p01 = d[0] * d[1], p23 = d[2] * d[3];
            const double ip = rcp_nr(p01 * p23);
            const double i01 = ip * p23, i23 = ip * p01;
            rr[0] = i01 * d[1];
            rr[1] = i01 * d[0];
            rr[2] = i23 * d[3];
            rr[3] = i23 * d[2];
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) r0[r] = __builtin_amdgcn_rcp(d[r]);
#pragma unroll
            for (int r = 0; r < 4; ++r) e[r] = __builtin_fma(-d[r], r0[r], 1.0);
#pragma unroll
            for (int r = 0; r < 4; ++r) e[r] = __builtin_fma(e[r], e[r], e[r]);
#pragma unroll
            for (int r = 0; r < 4; ++r) rr[r] = __builtin_fma(r0[r], e[r], r0[r]);   // = rcp_nr(d[r])
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            dd[r] = d[r];
            if (ZT && MODE == MODE_H) {
              double rr_ = rr[r];
              __asm__("" : "+v"(rr_));   // (keeps the product that formed rr out of an FMA with the next one)
              if (ZE_K) {
                // z is (1 + 2 eps) or ~0: the second operand is (1 + 2 eps) R2, the first simply r = R1 + R2 -- the two
                // products are linear in their operands, and the H-update undoes both maps on the K x N sums (pform:
                // P2 = P2' / (1 + 2 eps), P1 = P1' - P2): two instructions fewer per entry here
                R2[r] = rr_ * z[r];
                R1[r] = rr_;
              } else {
                R2[r] = rr_ * z[r];        // exact: z is 0 or 1
                R1[r] = rr_ - R2[r];       // exact: one of the two is zero
              }
            } else if (MODE == MODE_H) {
              // Every entry that is not an observed one acts as an observed zero here (SURVEY Q3, Q4);
              // pad entries have Theta == 0 exactly and their operand rows/columns are zero, so they only
              // touch the loss product, by the constant (1+eps) that is divided out before the loss.
              R1[r] = sel64_or0(ym[r], rr[r]);       // ym ? rr : 0
              // ym ? 0 : rr -- the difference is exact, one of the two being zero, PROVIDED it is a difference of the
              // rounded reciprocal: fused with the multiplication that formed rr (hipcc contracts by default) it would
              // leave that product's rounding error where an exact zero belongs; the empty asm keeps them apart
              double rr_ = rr[r];
              __asm__("" : "+v"(rr_));
              R2[r] = rr_ - R1[r];
            } else if (ZE_W) {
              // W sweeps of a fit (round 6): rr = 1 / d is +1 / (Theta + eps) for an observed one and -1 / (1 - Theta + eps)
              // for an observed zero: S1 - S2 as it stands.  An unobserved entry or a pad (d = Theta + eps there) is taken
              // out by an exact zero, o = 0.0 (one v_cndmask_b32 on the high word; FULL has no such entries and no such
              // factor); the column sums take (S1 - S2) z = (1 + 2 eps) S2 for a zero, ~1e-300 for a one, an exact 0 for
              // the rest -- the factor 1 + 2 eps is taken off in the epilogue.  5 (FULL: 3) instructions per entry, from 6.
              double rr_ = rr[r];
              __asm__("" : "+v"(rr_));
              if (FULL) {
                R1[r] = rr_;
              } else {
                const uint32_t ohi = __builtin_amdgcn_inverse_ballot_w64(ym[r] | zo[r]) ? 0x3FF00000u : 0u;
                cc[r] = mk_double((uint32_t)__double2loint(cc[r]), ohi);
                R1[r] = rr_ * cc[r];
              }
              s2 = __builtin_fma(R1[r], z[r], s2);
            } else if (ZT) {
              // W sweeps whose Theta is read from memory (more than 128 components): S2 = r z adds to the column sums by one FMA, and S1 - S2 = r c with c = +1 for an
              // observed one, -z (-1 or -0) otherwise -- exact products, the same numbers as the selects below give
              double rr_ = rr[r];
              __asm__("" : "+v"(rr_));
              s2 = __builtin_fma(rr_, z[r], s2);
              uint32_t chi;
              const uint32_t zhi = (uint32_t)__double2hiint(z[r]);
              // (one v_cndmask_b32 with the sign flip as a source modifier: hipcc spends a v_xor_b32 on it.  The result
              //  feeds a v_mul_f64, not an MFMA: no wait states to mind)
              __asm__("v_cndmask_b32_e64 %0, -%1, %2, %3" : "=v"(chi) : "v"(zhi), "v"(0x3FF00000u), "s"(ym[r]));
              cc[r] = mk_double((uint32_t)__double2loint(cc[r]), chi);
              R1[r] = rr_ * cc[r];
            } else {
              const double nr = sel64_or0(zo[r], rr[r]);   // S2
              s2 += nr;
              R1[r] = sel64_neg(ym[r], rr[r], nr);      // S1 - S2: +rr, -rr or 0
            }
          }
        }
        if (MODE == MODE_H || MODE == MODE_L) {
          // The sign of a product forgets an even number of negative factors; only the evaluation sweeps can
          // meet them (Theta > 1 + eps needs factors off the simplex: in a fit every scored sweep comes after a
          // W-update, so Theta <= 1 - eps there).
          if (MODE == MODE_L) negative |= fmin(fmin(dd[0], dd[1]), fmin(dd[2], dd[3])) < 0.0;
          if (TINY) {
            // eps < 1e-70: four factors of size eps could underflow before the renormalisation
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int e;
              prod = frexp(prod * dd[r], &e);
              pexp += e;
            }
          } else {
            prod *= (dd[0] * dd[1]) * (dd[2] * dd[3]);   // each >= eps >= 1e-70: no underflow before frexp
            if (!RENORM_TRIP) {
              int e;
              prod = frexp(prod, &e);
              pexp += e;
            }
          }
        }
      } else {
        // General path, _solver.py:30-32,42-43,53,150-154, with no selects in the product sweeps:
        //   DATA_F64   real-valued data, binary or no mask.  Image A (H and likelihood sweeps) stores an unobserved or pad
        //              entry as -0.0: it acts as the zero Y*mask has there (_solver.py:30) in every product, and its sign
        //              bit tells it from an observed zero where only observed entries count (strict).  Image B (W sweeps)
        //              stores it as NaN, and max(y, 0) / max(1 - y, 0) make the zeros Y.T*mask.T and (1-Y).T*mask.T
        //              have there (:31-32);
        //   DATA_F64M  real weights in tiles of their own; pad entries hold y = 0, weight 0.
        // Either way a pad adds only the constant log(1 + eps) to the likelihood (removed on the host, as on the
        // binary path), and every product with a pad row or column of a factor is 0.
        const d4 y4 = ycur;
        d4 m4 = {1, 1, 1, 1};
        if (DATA == DATA_F64M) m4 = mcur;
        if (!LM_ALT) {
          ycur = ynx;
          if (DATA == DATA_F64M) mcur = mnx;
        }
        // The two denominators of every entry.  Sweeps that compute Theta (TH = 0) start its accumulator at eps, so the
        // MFMAs deliver t1 = Theta + eps themselves and t2 = (1 + 2 eps) - t1 is one subtraction: one instruction per
        // entry instead of three (Theta + eps, 1 - Theta, + eps), each an issue slot beside the f64 MFMAs.  What it
        // changes is rounding: t2 carries the absolute error of a sum of size 1 (1e-16) instead of Theta's alone --
        // Theta's own rounding error, which depends on the summation order, is of that size already.
        double t1v[4], t2v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (EPSACC) {
            t1v[r] = (MODE == MODE_L) ? th[r] + addeps : th[r];   // (evaluation sweeps that clip Theta add eps behind the clip)
            t2v[r] = (MODE == MODE_L && a.clip) ? (1.0 - th[r]) + eps : c12 - t1v[r];
          } else {
            t1v[r] = th[r] + eps;
            t2v[r] = (1.0 - th[r]) + eps;
          }
        }
        // 1 / (t1 t2) per entry -- both quotients of an entry and the likelihood's t1 / t2 come from it -- for the lane's
        // four entries from ONE reciprocal: that of the product of all eight denominators, as the
        // binary path does with its four (each pair's product is >= eps, so the product of four pairs cannot underflow
        // while eps >= 1e-70; below that every pair keeps its own).  Three v_rcp_f64 -- quarter rate, three Newton FMAs
        // each -- become six multiplications; each quotient within ~4 ulp.
        double ipp[4];
        constexpr bool B4 = true;   // (round 5: at K <= 16 too -- four tiles per stage, but the general sweeps there are compiled for two workgroups per CU and have the registers: K = 16 H sweep +3 %)
        {
          double pp[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) pp[r] = t1v[r] * t2v[r];
          if (B4 && !TINY) {
            const double q01 = pp[0] * pp[1], q23 = pp[2] * pp[3];
            const double iq = rcp_nr(q01 * q23);
            const double i01 = iq * q23, i23 = iq * q01;
            ipp[0] = i01 * pp[1];
            ipp[1] = i01 * pp[0];
            ipp[2] = i23 * pp[3];
            ipp[3] = i23 * pp[2];
          } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) ipp[r] = rcp_nr(pp[r]);
          }
        }
        if (MODE == MODE_L || MODE == MODE_H) {
          // log-likelihood, _solver.py:150,154: per entry Ym log t1 + (1 - Ym) log t2 = log t2 + Ym log(t1 / t2).  The
          // first terms are the logarithm of a running product (ONE logarithm per lane and sweep, as on the binary
          // path), t1 / t2 = t1 (1 / t2) is one multiplication away from the quotients' own reciprocal: ONE table
          // logarithm per entry instead of two (each: 11-12 vector instructions and a 16-byte gather from LDS).
          // 1 - Theta + eps <= 0 -- factors off the simplex -- is noticed on the high words (a negative double is a
          // negative integer there, zero and subnormals are below 0x00100000): two v_min3_i32 per tile.
          // (TINY only: in the plain variant the host has checked the factors -- W on the simplex, H <= 1 - 1e-9, and the
          //  updates keep them there: tiny_a -- so 1 - Theta + eps > 0 throughout and the two instructions are saved)
          if (TINY) {
            t2hmin = min(min(t2hmin, __double2hiint(t2v[0])), __double2hiint(t2v[1]));
            t2hmin = min(min(t2hmin, __double2hiint(t2v[2])), __double2hiint(t2v[3]));
          }
        }
        [[maybe_unused]] double t2p[4];   // what of t2 enters the running product
        // (PHASED: the four table gathers of a tile are issued together, the arithmetic that does not need them
        //  -- ratios, mantissas and exponents, the running product -- runs while they are in flight, the series last;
        //  left to itself hipcc waits for each gather a few instructions behind its issue)
        constexpr bool PHASED = (MODE == MODE_L || MODE == MODE_H) && !(DATA == DATA_F64M && MODE == MODE_L);
        if (PHASED) {
          typedef double d2raw __attribute__((ext_vector_type(2)));
          double uu[4], it1v[4], it2v[4];
          d2raw ev[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            it1v[r] = ipp[r] * t2v[r];
            it2v[r] = ipp[r] * t1v[r];
            uu[r] = t1v[r] * it2v[r];
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint32_t off = ((uint32_t)__double2hiint(uu[r]) >> (16 - TB)) & (((1u << TB) - 1u) << 4);
            ev[r] = *(const __attribute__((address_space(3))) d2raw*)(uintptr_t)(off + LTAB_BYTE);
          }
          __builtin_amdgcn_sched_barrier(0);
          double ymv[4], mm[4], kk[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double y = y4[r];
            if (MODE == MODE_L && a.strict) {   // (DATA_F64 only, see PHASED)
              ymv[r] = y;
              t2p[r] = __double2hiint(y) >= 0 ? t2v[r] : 1.0;
            } else {
              ymv[r] = (DATA == DATA_F64M) ? y * m4[r] : y;
              t2p[r] = t2v[r];
            }
            if (MODE == MODE_H) {
              R1[r] = ymv[r] * it1v[r];                       // :42
              R2[r] = __builtin_fma(-ymv[r], it2v[r], it2v[r]);   // :43
            }
            mm[r] = __builtin_amdgcn_frexp_mant(uu[r]);
            kk[r] = (double)__builtin_amdgcn_frexp_exp(uu[r]);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double rr_ = __builtin_fma(mm[r], ev[r][0], -1.0);
            double p = __builtin_fma(rr_, mquarter, third);
            if (TB == 8) {
              p = __builtin_fma(rr_, 0.2, -0.25);
              p = __builtin_fma(rr_, p, third);
            }
            p = __builtin_fma(rr_, p, -0.5);
            p = __builtin_fma(rr_, p, 1.0);
            const double lg = __builtin_fma(rr_, p, __builtin_fma(kk[r], 0.69314718055994530942, ev[r][1]));
            llsum = __builtin_fma(ymv[r], lg, llsum);
          }
        } else
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double y = y4[r];
          const double it1 = ipp[r] * t2v[r];   // 1 / (Theta + eps)
          const double it2 = ipp[r] * t1v[r];   // 1 / (1 - Theta + eps)
          if (MODE == MODE_L || MODE == MODE_H) {
            double ym;   // the weight of log(t1 / t2)
            if (MODE == MODE_L && a.strict) {
              // mask * (Y log(Theta+eps) + (1-Y) log(1-Theta+eps)): examples/reproduce_magron2022.py:40-47
              if (DATA == DATA_F64M) {
                ym = y * m4[r];
                llsum = __builtin_fma(m4[r], log_tab<false, TB, true>(t2v[r], LTAB_BYTE, third, mquarter), llsum);   // real weights: a logarithm of its own
                t2p[r] = 1.0;
              } else {
                ym = y;                                             // -0.0 where unobserved
                t2p[r] = __double2hiint(y) >= 0 ? t2v[r] : 1.0;     // observed entries only
              }
            } else {
              ym = (DATA == DATA_F64M) ? y * m4[r] : y;   // Y*mask, _solver.py:30; unobserved entries act as observed zeros (Q3, Q4)
              t2p[r] = t2v[r];
            }
            if (MODE == MODE_H) {
              R1[r] = ym * it1;                          // :42
              R2[r] = __builtin_fma(-ym, it2, it2);      // :43, (1 - Ym) / t2 with one rounding
            }
            llsum = __builtin_fma(ym, log_tab<false, TB, true>(t1v[r] * it2, LTAB_BYTE, third, mquarter), llsum);
          } else {
            const double yo = (DATA == DATA_F64M) ? y * m4[r] : max0(y);                  // Y.T*mask.T, :31
            double s2e;
            if (DATA == DATA_F64M) {
              s2e = ((1.0 - y) * m4[r]) * it2;                                            // (1-Y).T*mask.T / (1 - Theta + eps), :32, :53
              // (a product that is then ADDED to the running sum: hipcc contracts the two into an FMA in some instantiations
              //  of this kernel and not in others -- found as a last-bit difference between the full and the ragged-K variant
              //  on weighted data, round 5 -- so the product is kept a value of its own, as the byte-code path keeps its)
              __asm__("" : "+v"(s2e));
            } else {
              // (1 - y) / t2 = it2 - y it2 in one FMA (>= 0 for y <= 1); an unobserved entry's NaN becomes the zero
              // (1-Y).T*mask.T has there by the same v_max_f64 -- two instructions instead of three.
              // ">= 0" needs t2 > 0.  The select variant also serves factors off the simplex -- transform's start,
              // _base.py:175: Theta = 8 ... 88 there -- whose t2 = 1 - Theta + eps is NEGATIVE: a max over the quotient
              // threw every observed zero's (negative) ratio away, S1 - S2 came out as S1 alone and the step missed the
              // reference by 1e-2 absolute (tests/test_gpu_transform_start.py).  There the max goes where the reference has
              // its zero, on (1 - y), and the quotient keeps its sign.
              if (TINY) {
                s2e = max0(1.0 - y) * it2;
                __asm__("" : "+v"(s2e));   // (kept a value of its own, as on the weighted path above)
              } else {
                s2e = max0(__builtin_fma(-y, it2, it2));
              }
            }
            R1[r] = __builtin_fma(yo, it1, -s2e);   // S1 - S2
            s2 += s2e;
          }
        }
        if (MODE == MODE_L || MODE == MODE_H) {
          if (TINY) {   // eps < 1e-70: four factors of that size could underflow before the renormalisation
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              int e;
              prod = frexp(prod * t2p[r], &e);
              pexp += e;
            }
          } else {
            prod *= (t2p[0] * t2p[1]) * (t2p[2] * t2p[3]);
            if (!RENORM_TRIP) {
              int e;
              prod = frexp(prod, &e);
              pexp += e;
            }
          }
        }
      }
      }
      if (DATA == DATA_BIN && !LM_ALT) {
#pragma unroll
        for (int r = 0; r < 8; ++r) lmcur[r] = lmnxt[r];
      }

      if (PRIO) __builtin_amdgcn_s_setprio(0);
      // ---- back-products: accumulator registers of Theta are the B operands (rows 4r..4r+3)
      if (PRODUCTS) {
#pragma unroll
      for (int g = 0; g < NGB; ++g) {
        double gnxt[GB];
        if (g + 1 < NGB) {
#pragma unroll
          for (int i = 0; i < GB; ++i) {
            const int p = (g + 1) * GB + i;
            gnxt[i] = ldsG[((p % KB) * 4 + (p / KB)) * 64 + lane];
          }
          __builtin_amdgcn_sched_barrier(0);
        } else if (b + 1 < NB && TH != 1) {
          // last group: fetch the first Theta group of the next tile of this stage
#pragma unroll
          for (int i = 0; i < GT; ++i) tcur[i] = base[(b + 1) * BLK + i * 64 + lane];
          __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < GB; ++i) {
          const int p = g * GB + i, r = p / KB, kb = p % KB;
          if (RAG && KB >= 4 && kb >= kblocks) continue;   // (a 16-block of components that is all padding: its products stay the zeros they are; up to K = 32 every block holds components)
          acc1[kb] = NBMF_MFMA(gcur[i], R1[r], acc1[kb], 0, 0, 0);
          if (MODE == MODE_H) acc2[kb] = NBMF_MFMA(gcur[i], R2[r], acc2[kb], 0, 0, 0);
        }
        if (g + 1 < NGB) {
#pragma unroll
          for (int i = 0; i < GB; ++i) gcur[i] = gnxt[i];
        }
      }
      }
    }

    // (the prefetched stage has landed in the other buffer by the vmcnt(0) hipcc puts in front of this barrier; its last
    //  readers finished before the previous barrier, and this stage's readers use `buf`)
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      tcurT[b] = tnext[b];
    }
    __syncthreads();
    bufv ^= 1;
  }
    if (RENORM_TRIP) {
      int e;
      prod = frexp(prod, &e);
      pexp += e;
    }
  }
  if (DATA == DATA_BIN && MODE != MODE_T && (pf_sink ^ pf_val) == 0x5A17C0DEu && a.Rb < 0)   // (never true: keeps the prefetch loads alive)
    ((uint32_t*)a.out1)[lane] = pf_sink;

#undef STAGE_DMA
#undef MASKS_REQUEST
  if (a.trace) {
    tr2 = wall_clock64();
    trc = (unsigned long long)clock64() - trc;
  }
  // ---- the workgroup's log-likelihood partial: one atomic store into its slot (see PassFin)
  constexpr bool LOSS = (MODE == MODE_H || MODE == MODE_L);
  if (LOSS && a.lossbuf) {   // (sliced runs: only the first slice's sweep reports it)
    double ll;
    if (DATA == DATA_BIN)
      ll = negative ? __builtin_nan("") : log_of_product(prod, pexp);
    else   // Theta > 1 + eps (factors off the simplex): NumPy's log gives NaN there, -inf at exactly 0
      ll = t2hmin < 0 ? __builtin_nan("") : (t2hmin < 0x00100000 ? -__builtin_inf() : llsum + log_of_product(prod, pexp));
    ll = wave_sum(ll);
    // one partial per workgroup: the four waves in wave order (fixed -> reproducible)
    __syncthreads();                       // all waves are done with the staging buffers
    if (lane == 0) lds[wave] = ll;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = lds[0];
#pragma unroll
      for (int w_ = 1; w_ < WG_WAVES; ++w_) t += lds[w_];
      if (!(a.fin.on == 2 && blockIdx.x == 0 && blockIdx.y == 0))
        __hip_atomic_store(a.lossbuf + (size_t)chunk * gridDim.x + bx, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }

  [[maybe_unused]] unsigned long long tr3 = 0, tr4 = 0;
  if (a.trace) tr3 = wall_clock64();
  // ---- epilogue: slabs [chunk][k][column]
  const int q = lane >> 4, c = lane & 15;
  {
    if (MODE == MODE_W) {
      s2 += __shfl_xor(s2, 16, 64);
      s2 += __shfl_xor(s2, 32, 64);
    }
    [[maybe_unused]] const double inv12 = 1.0 / c12;
    double* o1 = a.out1 + (size_t)chunk * K * a.C_alloc + (size_t)cb * 16 + c;
    double* o2 = (MODE == MODE_H) ? a.out2 + (size_t)chunk * K * a.C_alloc + (size_t)cb * 16 + c : nullptr;
    if (PRODUCTS) {
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const size_t k = 16 * kb + 4 * r + q;
          if (MODE == MODE_H) {
            o1[k * a.C_alloc] = acc1[kb][r];
            o2[k * a.C_alloc] = acc2[kb][r];
          } else {
            // (ZE_W: the running sum is (1 + 2 eps) times the column sum of S2)
            o1[k * a.C_alloc] = ZE_W ? __builtin_fma(s2, inv12, acc1[kb][r]) : acc1[kb][r] + s2;
          }
        }
      }
    }
  }
  if (a.trace) tr4 = wall_clock64();
  if (LOSS && a.lossbuf && a.fin.on && blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1) {
    // the sweep's last workgroup in launch order: wait for every slot, assemble, empty the slots (see PassFin)
    const unsigned long long* slots = (const unsigned long long*)a.lossbuf;
    const unsigned long long t0 = (unsigned long long)wall_clock64();
    for (;;) {
      int missing = 0;
      for (int j = threadIdx.x; j < a.fin.n_ll; j += 64 * WG_WAVES)
        missing |= __hip_atomic_load(slots + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == LL_EMPTY;
      const bool expired = (unsigned long long)wall_clock64() - t0 > a.fin.wait_ticks;
      // (the workgroup's verdict through the dynamic LDS: __syncthreads_or brings static LDS of its own, and this kernel
      //  must have none -- see LTAB_BYTE)
      volatile int* again = (volatile int*)lds + 17;
      volatile int* some_missing = (volatile int*)lds + 18;   // (the verdict is the WORKGROUP's: `missing` is each thread's view of its own slots)
      __syncthreads();
      if (threadIdx.x == 0) {
        *again = 0;
        *some_missing = 0;
      }
      __syncthreads();
      if (missing) {
        *some_missing = 1;
        if (!expired) *again = 1;
      }
      __syncthreads();
      if (!*again) {   // every slot has arrived -- or the wait is over (a GPU shared with another tenant can hold this sweep's
        if (*some_missing) {   // other workgroups back for seconds): NOTHING is assembled; the run is stopped -- every later
          if (threadIdx.x == 0) {   // kernel returns at once, so the factors stay those this sweep read -- and the host is told
            a.fin.flags[0] = 1;     // (flags[6]): it resumes from exactly here with the loss in a launch of its own
            a.fin.flags[6] = 1;     // (nbmf_run: recover)
          }
          return;
        }
        break;
      }
      __builtin_amdgcn_s_sleep(32);
    }
    finalize_block<true>(a.lossbuf, a.fin.n_ll, a.fin.ll_pad, a.fin.prior, a.fin.n_prior, a.fin.am1, a.fin.bm1, a.fin.n_obs,
                         a.fin.losses, a.fin.t, a.fin.tol, a.fin.scal, a.fin.flags, (double (*)[4])(lds + 32));
    __syncthreads();   // (everybody has read the slots)
    for (int j = threadIdx.x; j < a.fin.n_ll; j += 64 * WG_WAVES)
      __hip_atomic_store((unsigned long long*)a.lossbuf + j, LL_EMPTY, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (a.trace) {
    __syncthreads();   // (the workgroup's last wave: its stores are issued)
    if (threadIdx.x == 0) {
      unsigned long long* t = a.trace + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 8;
      t[5] = tr3;
      t[6] = tr4;
      t[7] = trc;   // shader clocks (s_memtime) between the loop's top and its end: with t[2] - t[1] (100 MHz) the clock the chip held
      t[0] = tr0;
      t[1] = tr1;
      t[2] = tr2;
      t[3] = wall_clock64();
      t[4] = __builtin_amdgcn_s_getreg((4 /* HW_REG_HW_ID */) | (0 << 6) | (31 << 11));   // where wave 0 ran: wave slot, SIMD, CU, SE, ...
    }
  }
}

