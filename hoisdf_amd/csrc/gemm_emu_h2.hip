// f16x2 form ("h2"): the same contractions from TWO f16 pieces per operand and THREE products.
//   x s = hi + lo + r,  hi = f16(x s), lo = f16(x s - hi), |r| <= max(2^-22 |x s|, 2^-25) (on average 2^-24 |x s|): with the operand
//   scaled by a power of two s so that max |x s| lies in [2^13, 2^14) every element within 2^-16 of the largest keeps 22 bits; below
//   that lo is an f16 subnormal: an ABSOLUTE error of 2^-38 max |x|.  x y is accumulated in f32 from lo hi + hi lo + hi hi (each f16 x f16 product
//   is exact in f32); the dropped lo lo term is <= 2^-22 |x y|, on average 2^-26 |x y| with a random sign - the rounding of an f32
//   multiply-add.  Half the MFMA work of the bf16x3 form at the same matrix-pipe rate; the price is the scale: the largest
//   magnitude of every operand has to be known when its contraction is launched (weights: found while the image is built;
//   activations / gradients: magnitude words written by the producing kernel's epilogue, or by hoisdf's own magnitude pass).
// Tile 256 x 256 x 16, 4 waves as 2 x 2, wave tile 128 x 128 = 4 x 4 MFMA blocks (256 accumulators in AGPRs, one workgroup per CU):
// with half the MFMA work per byte the 256 x 128 tile of emu_kc2_kernel would ask the vector memory pipe for ~100 GB/s per CU.
// Staging (gemm_emu.h), LDS layout and the rotated, pinned phase are emu_kc2_kernel's (gemm_emu_b3.hip; tools/gen/h2_phase.py -> h2_phase.inc).
// Weight image: column tile tn (256 columns), slab s (16 k), plane p (hi, lo), chunk c (8 k), row r: 16 bytes at
// ((((tn * nslab + s) * 2 + p) * 2 + c) * 256 + r) * 16; behind the last tile a 128-byte trailer: 16 magnitude words, then {s, 1 / s}.
#include "gemm_emu.h"

namespace hoisdf {

// ---- weight -> f16x2 image.  Pass 1: 16 magnitude words per weight into the trailer; pass 2: scale, split, write (+ {s, 1 / s}).
__device__ __forceinline__ void h2_weight_amax_unit(const float* __restrict__ W, int ldw, int N, int K, int part, uint32_t* trailer, uint32_t* red4) {
  uint32_t m = 0u;
  const long n = (long)N * K;
  for (long i = (long)part * 256 + threadIdx.x; i < n; i += 16 * 256) {
    const long r = i / K;
    m = max(m, __builtin_bit_cast(uint32_t, W[r * ldw + (i - r * K)]) & 0x7fffffffu);
  }
  m = block_max_u32(m, red4);
  if (threadIdx.x == 0) trailer[part] = m;
}
__device__ __forceinline__ void h2_prep_weight_unit(const float* __restrict__ W, int ldw, int R, int Kc, int transpose, int nslab,
                                                    long idx, u32x4* __restrict__ img) {
  uint32_t* tr = h2_trailer(img, R, Kc);
  uint32_t am = 0u;
#pragma unroll
  for (int i = 0; i < 16; ++i) am = max(am, tr[i]);
  const float sc = h2_scale(am);
  if (idx == 0) {                                  // (the whole trailer is defined: images compare equal byte for byte)
    reinterpret_cast<float*>(tr)[16] = sc; reinterpret_cast<float*>(tr)[17] = h2_inv_scale(am);
#pragma unroll
    for (int i = 18; i < H_TRAILER / 4; ++i) tr[i] = 0u;
  }
  const int r = (int)(idx % HTN);
  const int c = (int)((idx / HTN) % 2);
  const int s = (int)((idx / (2 * HTN)) % nslab);
  const int tn = (int)(idx / ((long)2 * HTN * nslab));
  const int row = tn * HTN + r;
  const int k0 = s * KS + c * 8;
  f16x8 hi, lo;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + i;
    float v = 0.f;
    if (row < R && k < Kc) v = transpose ? W[(size_t)k * ldw + row] : W[(size_t)row * ldw + k];
    v *= sc;
    hi[i] = (_Float16)v;
    lo[i] = (_Float16)(v - (float)hi[i]);
  }
  const size_t base = ((size_t)(tn * nslab + s) * 2) * 2 * HTN;
  img[base + (0 * 2 + c) * HTN + r] = __builtin_bit_cast(u32x4, hi);
  img[base + (1 * 2 + c) * HTN + r] = __builtin_bit_cast(u32x4, lo);
}
__global__ __launch_bounds__(256) void h2_weight_amax_kernel(const float* __restrict__ W, int ldw, int N, int K, int R, int Kc, void* image) {
  __shared__ uint32_t red4[4];
  h2_weight_amax_unit(W, ldw, N, K, blockIdx.x, h2_trailer(image, R, Kc), red4);
}
__global__ __launch_bounds__(256) void h2_weight_amax_batch_kernel(const hoisdf_emu_prep_item* __restrict__ items) {
  __shared__ uint32_t red4[4];
  const hoisdf_emu_prep_item it = items[blockIdx.x >> 4];
  const int R = it.transpose ? it.K : it.N, Kc = it.transpose ? it.N : it.K;
  h2_weight_amax_unit(it.W, it.ldw, it.N, it.K, blockIdx.x & 15, h2_trailer(it.image, R, Kc), red4);
}
__global__ __launch_bounds__(256) void h2_prep_weight_kernel(const float* __restrict__ W, int ldw, int R, int Kc, int transpose, int nslab,
                                                             long total, u32x4* __restrict__ img) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < total) h2_prep_weight_unit(W, ldw, R, Kc, transpose, nslab, idx, img);
}
__global__ __launch_bounds__(256) void h2_prep_weight_batch_kernel(const hoisdf_emu_prep_item* __restrict__ items, int n) {
  EMU_PREP_FIND(items, n, lo)
  const hoisdf_emu_prep_item it = items[lo];
  const int R = it.transpose ? it.K : it.N, Kc = it.transpose ? it.N : it.K;
  const int nslab = ((Kc + KS - 1) / KS);
  const long total = (long)((R + HTN - 1) / HTN) * nslab * 2 * HTN;
  const long idx = ((long)blockIdx.x - it.first_block) * 256 + threadIdx.x;
  if (idx < total) h2_prep_weight_unit(it.W, it.ldw, R, Kc, it.transpose, nslab, idx, static_cast<u32x4*>(it.image));
}

// NJ = 4: tile 256 x 256 (one workgroup per CU); NJ = 2: tile 256 x 128, wave tile 128 x 64, two workgroups per CU (few or narrow
// tiles: the prologue / epilogue of one workgroup under the main loop of the other) - it reads one half of the image's 256-row blocks
template <bool MASK, bool KTAIL, int NJ>
__global__ __launch_bounds__(NT, NJ == 4 ? 1 : 2) void emu_h2_kernel(EmuArgs g) {
  constexpr int TN_ = 64 * NJ;                                        // tile width
  constexpr int BST = 2 * 2 * TN_;                                    // 16-byte units of the weight operand per stage
  constexpr int STG = HA_U4 + BST;
  constexpr int EPI = (4 * 32 * (TN_ / 2 + 4) * 4 + 64) / 16;         // the epilogue's four transposition slices + a few words
  __shared__ __attribute__((aligned(16))) u32x4 st0[EPI > STG ? EPI : STG];
  __shared__ __attribute__((aligned(16))) u32x4 st1[STG];
  __shared__ __attribute__((aligned(16))) float rpost[HTM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int t = xcd_remap(blockIdx.x, g.tiles_m * g.tiles_n);
  const int tm = t / g.tiles_n, tn = t - tm * g.tiles_n;
  const int m0 = tm * HTM, n0 = tn * TN_;
  const int nslab = (g.K + KS - 1) / KS;
  const int last = nslab - 1;
  const int rl = lane >> 2, qd = lane & 3, cq = qd >> 1;

  // operand scales: ONE PER ROW of A from its row magnitudes (common.h; a row's rounding depends on that row alone), the weight's from
  // the image trailer.  The staging thread keeps the scales of its four rows; every output row's factor (1 / row scale, 1 / weight
  // scale, 1 / keep) waits in LDS for the epilogue.  f16 conversions saturate (a word below the row's true maximum clips, no Inf).
  // (the five words are REQUESTED here, ahead of the first slab's loads, and used behind them: no load round trip of its own per tile)
  f16_saturate_on();
  const uint32_t wpost = m0 + tid < g.M ? g.a_amax[m0 + tid] : 0u;
  uint32_t wrow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = m0 + i * 64 + wave * 16 + rl;
    wrow[i] = row < g.M ? g.a_amax[row] : 0u;
  }
  float sAr[4];

  f32x16 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // staging roles, descriptors and LDS slots: gemm_emu.h (item i = row i * 64 + wave * 16 + lane / 4, quad lane % 4)
#ifdef H2_ABL_NOLOADA                 /* (tools/ablate_h2.sh: every tile reads the FIRST tile's rows - the same loads, served by the caches) */
  EMU_A_DESCRIPTORS(HTM, 0)
#else
  EMU_A_DESCRIPTORS(HTM, m0)
#endif
  // the image is laid out in 256-row blocks (HB_U4 units per slab): a 128-wide tile reads rows (tn & 1) * 128 .. + 127 of its block
  const int tb = NJ == 4 ? tn : tn >> 1, r0 = NJ == 4 ? 0 : (tn & 1) * 128;
  const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u32x4*>(g.Bimg + (size_t)tb * nslab * HB_U4), 0, nslab * HB_U4 * 16, 0x00020000);
  const int boff = NJ == 4 ? tid * 16 : ((tid >> 7) * HTN + r0 + (tid & 127)) * 16;     // piece q: + q * (NJ == 4 ? NT : 2 * HTN) units
  EMU_A_SLOTS(HTM)
  f32x2 rp[8], fu[8];
  uint32_t t0[8], t1[8];
  u32x4 rb[NJ];
  uint32_t rm[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, mb = 0xfu;
  bool kin = true;
#define HLDGA(i, sl) EMU_LDGA(i, sl)
#define HLDGB(q, sl) rb[q] = __builtin_amdgcn_raw_buffer_load_b128(rsb, boff + (q) * ((NJ == 4 ? NT : 2 * HTN) * 16), min((sl), last) * (HB_U4 * 16), 0)
#define HUI(i, sl) EMU_UI(i, sl)
// pair p = 2 i + j of item i: HC1 sign bitmap / k tail / scale, hi plane (v_cvt_pk_f16_f32, round to nearest) and its f32 image;
// HC2 residual, lo plane
#define HC1(p)                                                                                                         \
  do {                                                                                                                 \
    f32x2 v_ = rp[p];                                                                                                  \
    EMU_MASK_KTAIL(v_, p);                                                                                             \
    v_ *= sAr[(p) >> 1];                                                                                               \
    const f16x2 h_ = __builtin_convertvector(v_, f16x2);                                                               \
    t0[p] = __builtin_bit_cast(uint32_t, h_); rp[p] = v_;                                                              \
    fu[p] = __builtin_convertvector(h_, f32x2);                                                                        \
  } while (0)
#define HC2(p) do { f32x2 w_; PK_SUB(w_, rp[p], fu[p]); t1[p] = __builtin_bit_cast(uint32_t, __builtin_convertvector(w_, f16x2)); } while (0)
#define HSTA(st, i, tp, pl) reinterpret_cast<u32x2*>(st)[wslot + (i) * 128 + (pl) * 4 * HTM] = u32x2{tp[2 * (i)], tp[2 * (i) + 1]}
#define HSTB(st, q) (st)[HA_U4 + tid + (q) * NT] = rb[q]
#define HLA(st, p, i) __builtin_bit_cast(f16x8, (st)[aread + ((p) * 2 + kh) * HTM + (i) * 32])
#define HLB(st, p, j) __builtin_bit_cast(f16x8, (st)[HA_U4 + wn * (TN_ / 2) + l31 + ((p) * 2 + kh) * TN_ + (j) * 32])
#define HM1(ax, bx, i, j, work) do { acc[i][j] = MFH(ax[i], bx[j], acc[i][j]); work; SB(); } while (0)
#define HMM(ax, bx) _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < NJ; ++j) acc[i][j] = MFH(ax[i], bx[j], acc[i][j])
#include "h2_phase.inc"
#define HSTAGE_ALL(st, sl)                                                                                             \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                    \
      HUI(i, sl);                                                                                                      \
      HC1(2 * i); HC2(2 * i); HC1(2 * i + 1); HC2(2 * i + 1);                                                          \
      HSTA(st, i, t0, 0); HSTA(st, i, t1, 1);                                                                          \
    }                                                                                                                  \
    _Pragma("unroll") for (int q = 0; q < NJ; ++q) HSTB(st, q);                                                        \
  } while (0)
#define HLOAD_ALL(sl)                                                                                                  \
  do {                                                                                                                 \
    /* issue order pinned to a phase's (B pieces, then the items): the vmcnt waits inside the loop count BOTH histories */ \
    SB();                                                                                                              \
    _Pragma("unroll") for (int q = 0; q < NJ; ++q) { HLDGB(q, sl); SB(); }                                             \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) { HLDGA(i, sl); SB(); }                                              \
  } while (0)

  const int nslab2 = (nslab + 1) & ~1;
  f16x8 aH[4], aL[4], bP[NJ], bQ[NJ], bL[NJ];
  HLOAD_ALL(0);
#pragma unroll
  for (int i = 0; i < 4; ++i) sAr[i] = h2_scale(wrow[i]);
  HSTAGE_ALL(st0, 0);
  HLOAD_ALL(1);
  rpost[tid] = h2_inv_scale(wpost) * g.b_scale[1] * (MASK ? g.ascale : 1.f);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) { aL[i] = HLA(st0, 1, i); aH[i] = HLA(st0, 0, i); }
#pragma unroll
  for (int j = 0; j < NJ; ++j) { bP[j] = HLB(st0, 0, j); bL[j] = HLB(st0, 1, j); }
  HMM(aL, bP); HMM(aH, bL);                                    // lo hi, hi lo of slab 0
  HSTAGE_ALL(st1, 1);
  HLOAD_ALL(2);
  SYNC();                                                      // aH / bP = hi fragments of slab 0
#define HPH(cur, nxt, s, bC, bN) do { if constexpr (NJ == 4) { HPHASE(cur, nxt, s, bC, bN); } else { HPHASE2(cur, nxt, s, bC, bN); } } while (0)
  for (int s = 1; s + 1 < nslab2; s += 2) {
    HPH(st1, st0, s, bP, bQ);
    SYNC();
    HPH(st0, st1, s + 1, bQ, bP);
    SYNC();
  }
  HPH(st1, st0, nslab2 - 1, bP, bQ);
  SB();
  HMM(aH, bQ);                                                 // hi hi of the last slab
  __syncthreads();
#undef HLDGA
#undef HLDGB
#undef HUI
#undef HC1
#undef HC2
#undef HSTA
#undef HSTB
#undef HLA
#undef HLB
#undef HM1
#undef HMM
#undef HPHASE
#undef HPHASE2
#undef HPH
#undef HSTAGE_ALL
#undef HLOAD_ALL
  emu_epilogue<HTM, TN_, NJ>(g, acc, st0, m0, n0, wm, wn, wave, lane, l31, kh, 1.f, rpost);
}

int emu_h2_prepare(const float* W, int ldw, int N, int K, int transpose, void* image, hipStream_t st) {
  const int R = transpose ? K : N, Kc = transpose ? N : K;
  const int nslab = cdiv(Kc, KS);
  const long total = (long)cdiv(R, HTN) * nslab * 2 * HTN;
  hipLaunchKernelGGL(h2_weight_amax_kernel, dim3(16), dim3(256), 0, st, W, ldw, N, K, R, Kc, image);
  hipLaunchKernelGGL(h2_prep_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, ldw, R, Kc, transpose, nslab, total,
                     static_cast<u32x4*>(image));
  return check_launch("linear_emu_prepare (f16x2)");
}

int emu_h2_prepare_batch(const hoisdf_emu_prep_item* d_items, int n, long total_blocks, hipStream_t st) {
  hipLaunchKernelGGL(h2_weight_amax_batch_kernel, dim3((unsigned)n * 16), dim3(256), 0, st, d_items);
  hipLaunchKernelGGL(h2_prep_weight_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, d_items, n);
  return check_launch("linear_emu_prepare_batch (f16x2)");
}

int emu_h2_launch(EmuArgs g, hipStream_t st) {
  // tile width: 256 x 128, two workgroups per CU (the prologue / epilogue of one under the main loop of the other; finer tiles for
  // the 16 384 / 49 152-row shapes) except for the masked grad-input over a long contraction, where the 256 x 256 tile's halved
  // staging work per MFMA wins (profiles/r05_h2_tile_widths.txt: 65536 x 1024 x 256 forward + ReLU + dropout
  // 180 vs 149 TF, 49152 x 512 x 512 247 vs 212, 65536 x 256 x 256 176 vs 159; masked grad-input over 1024: 172 vs 181).
  const bool wide_ok = cdiv(g.M, HTM) * cdiv(g.N, HTN) >= 208 && g.N % HTN == 0;
  const bool narrow = !(g.abits && g.K >= 768 && wide_ok);
  g.tiles_m = cdiv(g.M, HTM);
  g.tiles_n = cdiv(g.N, narrow ? 128 : HTN);
  g.b_scale = reinterpret_cast<const float*>(h2_trailer(const_cast<u32x4*>(g.Bimg), g.N, g.K)) + 16;
  const bool kt = g.K % KS != 0 || (cdiv(g.K, KS) & 1);
  static void (*const kernel[2][2][2])(EmuArgs) = {      // [wide][MASK][KTAIL]
      {{emu_h2_kernel<false, false, 2>, emu_h2_kernel<false, true, 2>}, {emu_h2_kernel<true, false, 2>, emu_h2_kernel<true, true, 2>}},
      {{emu_h2_kernel<false, false, 4>, emu_h2_kernel<false, true, 4>}, {emu_h2_kernel<true, false, 4>, emu_h2_kernel<true, true, 4>}}};
  hipLaunchKernelGGL(kernel[!narrow][g.abits != nullptr][kt], dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(NT), 0, st, g);
  return check_launch("linear_emu (f16x2)");
}

}  // namespace hoisdf
