// fp32 linear layers EMULATED on the bf16 MFMA pipe ("bf16x3"): forward and grad-input of common/nets/layer.py:168-201
// (MLP), common/nets/transformer.py:286-302 (in / out projections, feed-forward), main/model.py:56-90 (input MLPs, heads).
//
// Every f32 operand is split EXACTLY into three bf16 pieces, x = x0 + x1 + x2 (8 + 8 + 8 significand bits; bf16 has the f32
// exponent range, so - unlike an f16 hi / lo pair - nothing has to be scaled and nothing is lost: x0 = bf16(x),
// x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), every subtraction exact).  A product x y is accumulated in f32 from six
// v_mfma_f32_32x32x16_bf16 products, x0y0 + x0y1 + x1y0 + x1y1 + x0y2 + x2y0 (each bf16 x bf16 product is exact in f32); the
// three dropped terms are <= 2^-24 |x y|, below the rounding of an f32 fused multiply-add.  Against fp64 the result has the
// error of an f32 GEMM (measured next to the exact-f32 MFMA kernel: tools/ubench/gemm_emu_lab.hip, tests/test_gpu_emu.py),
// while the bf16 pipe runs 16 x the f32 MFMA rate: 2.67 x after six products.
//
//   A (activations x, or dy) is read as f32, k-contiguous, and split on its way into LDS (thread = tile row; the forward's
//   ReLU / dropout sign bitmap and 1 / keep are applied to dy before the split).  B (the weight) is pre-split ONCE per weight
//   update into a "slab image": for column tile tn (128 output columns), slab s (16 k), plane p, k-chunk c (8 k), row r the
//   16 bytes at ((((tn * nslab + s) * 3 + p) * 2 + c) * 128 + r) * 16 - exactly the LDS image of the slab, so staging it is
//   three fully coalesced 16-byte loads and three ds_write_b128 per thread (hoisdf_linear_emu_prepare; transposed for grad-input).
//   LDS image of a plane slab: [chunk][row][16 B]: the MFMA fragment read (32 consecutive rows of one chunk per half-wave,
//   ds_read_b128) and the staging write (consecutive rows) are both bank-conflict free without padding.
// Tile 256 x 128, 4 waves as 2 x 2, wave tile 128 x 64 = 4 x 2 MFMA blocks (128 accumulators), 16-deep slabs double-buffered
// in LDS (72 KB), two workgroups per CU (<= 256 VGPRs); one barrier per slab; the next slab is converted / parked and the one
// after it requested at the top of every slab.  Epilogue = gemm.hip's (bias, ReLU, dropout, 1-bit sign map, accumulate-into,
// LDS-transposed 16-byte stores).
#include "gemm_emu.h"

namespace hoisdf {

// ---- weight -> slab image.  transpose = 0: image row n, contraction k = W[n][k] (forward);  1: image row k, contraction
// n = W[n][k] (grad-input: dx = dy . W).  One thread per (tile, slab, chunk, row): 8 source values -> 3 x 16 bytes.
__device__ __forceinline__ void emu_prep_weight_unit(const float* __restrict__ W, int ldw, int R, int Kc, int transpose, int nslab,
                                                     long idx, u32x4* __restrict__ img) {
  const int r = (int)(idx % TN);
  const int c = (int)((idx / TN) % 2);
  const int s = (int)((idx / (2 * TN)) % nslab);
  const int tn = (int)(idx / ((long)2 * TN * nslab));
  const int row = tn * TN + r;
  const int k0 = s * KS + c * 8;
  float e[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + i;
    float v = 0.f;
    if (row < R && k < Kc) v = transpose ? W[(size_t)k * ldw + row] : W[(size_t)row * ldw + k];
    e[i] = v;
  }
  bf16x8 p0, p1, p2;
  split3x8(make_float4(e[0], e[1], e[2], e[3]), make_float4(e[4], e[5], e[6], e[7]), p0, p1, p2);
  const size_t base = ((size_t)(tn * nslab + s) * 3) * 2 * TN;
  img[base + (0 * 2 + c) * TN + r] = __builtin_bit_cast(u32x4, p0);
  img[base + (1 * 2 + c) * TN + r] = __builtin_bit_cast(u32x4, p1);
  img[base + (2 * 2 + c) * TN + r] = __builtin_bit_cast(u32x4, p2);
}

__global__ __launch_bounds__(256) void emu_prep_weight_kernel(const float* __restrict__ W, int ldw, int R, int Kc, int transpose,
                                                              int nslab, long total, u32x4* __restrict__ img) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx < total) emu_prep_weight_unit(W, ldw, R, Kc, transpose, nslab, idx, img);
}

// many images in one launch (all weights of a model after an optimizer step)
__global__ __launch_bounds__(256) void emu_prep_weight_batch_kernel(const hoisdf_emu_prep_item* __restrict__ items, int n) {
  EMU_PREP_FIND(items, n, lo)
  const hoisdf_emu_prep_item it = items[lo];
  const int R = it.transpose ? it.K : it.N, Kc = it.transpose ? it.N : it.K;
  const int nslab = ((Kc + KS - 1) / KS);
  const long total = (long)((R + TN - 1) / TN) * nslab * 2 * TN;
  const long idx = ((long)blockIdx.x - it.first_block) * 256 + threadIdx.x;
  if (idx < total) emu_prep_weight_unit(it.W, it.ldw, R, Kc, it.transpose, nslab, idx, static_cast<u32x4*>(it.image));
}

// ---- main loop ("rotated", hand-interleaved, line-coalesced activation loads): the tile and epilogue described at the top of
// the file, products small terms first (x2 y0, x1 y1, x1 y0, x0 y2, x0 y1, x0 y0).  Against a plain double-buffered loop
// (stage slab s + 1, barrier, 48 MFMAs; retired, profiles/r04_kc2_dw2_vs_round3_forms.txt) the forward results are bit identical, but
//  * the six product groups of a slab are rotated by half a slab against the barrier: a phase = [x0 y2, x0 y1, x0 y0 of slab
//    s - 1 | x2 y0, x1 y1, x1 y0 of slab s], so the 24 MFMAs right behind the barrier take fragments that were read BEFORE it and
//    every fragment read of slab s is issued 4 ... 24 MFMAs ahead of its first use;
//  * the staging of slab s + 1 (16 f32 per thread -> three bf16 planes -> the other stage, plus the weight image pieces) is
//    cut into units of <= 5 VALU / one LDS or global instruction, and every unit is pinned behind ONE MFMA of the same wave:
//    on this part a wave's VALU work hides under its OWN MFMAs only (profiles/r03_mfma_valu_overlap.txt), and left alone hipcc
//    emits [convert + write everything | 48 MFMAs] - with one LDS array it even has to (every fragment read may alias the
//    staging writes that precede it in program order), which is why the two stages are two distinct __shared__ objects here;
//  * the activation tile is loaded with FOUR LANES PER ROW (lane = row l / 4 of a 16-row group, 16-byte quad l % 4 of the
//    slab's 64 bytes; four such items per thread): a wave instruction touches 16 cache lines instead of 64.  With thread =
//    row (the retired first form) every global_load_dwordx4 asks the vector memory pipe for 64 different lines, 16 bytes of each: the
//    ablations of round 4 (profiles/r04_kc2_ablation_loads.txt; their compile-time hooks last existed at commit 79e9e9c) showed
//    the loop running at 285 - 338 TF without staging and at 130 - 170 with the loads and LDS writes but WITHOUT any conversion
//    arithmetic - the address / tag path, not the VALU, was the limiter.  A quad converts to 8 bytes per plane (ds_write_b64);
//    rows of the second k-chunk are stored with bit 2 of the row flipped so that a 16-lane group's 4 rows x 2 chunks x 2 halves
//    cover all 32 banks once.
template <bool MASK, bool KTAIL>
__global__ __launch_bounds__(NT, 2) void emu_kc2_kernel(EmuArgs g) {
  __shared__ __attribute__((aligned(16))) u32x4 st0[STAGE_U4];
  __shared__ __attribute__((aligned(16))) u32x4 st1[STAGE_U4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int l31 = lane & 31, kh = lane >> 5;
  const int t = xcd_remap(blockIdx.x, g.tiles_m * g.tiles_n);
  const int tm = t / g.tiles_n, tn = t - tm * g.tiles_n;
  const int m0 = tm * TM, n0 = tn * TN;
  const int nslab = (g.K + KS - 1) / KS;
  const int last = nslab - 1;

  f32x16 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // staging roles, descriptors and LDS slots: gemm_emu.h (item i = row i * 64 + wave * 16 + lane / 4, quad lane % 4)
  const int rl = lane >> 2, qd = lane & 3, cq = qd >> 1;
  EMU_A_DESCRIPTORS(TM, m0)
  const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<u32x4*>(g.Bimg + (size_t)tn * nslab * B_U4), 0, nslab * B_U4 * 16, 0x00020000);
  EMU_A_SLOTS(TM)
  f32x2 rp[8], fu[8];                                            // the thread's 4 quads of the slab being staged, as pairs (+ unpacked planes)
  uint32_t t0[8], t1[8], t2[8];                                  // their three bf16 planes (two values per register)
  u32x4 rb[NB];
  uint32_t rm[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, mb = 0xfu;
  bool kin = true;
// ---- staging units.  LDGA(i, sl): the quad of item i in slab sl (gemm_emu.h); LDGB(q, sl): piece q of the slab's weight image
#define LDGA(i, sl) EMU_LDGA(i, sl)
#define LDGB(q, sl) rb[q] = __builtin_amdgcn_raw_buffer_load_b128(rsb, (tid + (q) * NT) * 16, min((sl), last) * (B_U4 * 16), 0)
// the conversion of pair p = 2 i + j (item i, half j of its quad) in four units (U1 .. U4) or two (CV1 = U1 + U2, CV2 = U3 + U4):
//   U1  sign bitmap (bit -> all-ones / zero word -> and; the 1 / keep factor is applied once, in the epilogue) and k tail;
//       first plane = bf16(v) (v_cvt_pk_bf16_f32), unpacked again    U2  first residual (one packed subtract)
//   U3  second plane, unpacked                                        U4  second residual, third plane
// UI(i, sl): per-item scalars of slab sl (gemm_emu.h)
#define UI(i, sl) EMU_UI(i, sl)
#define U1(p)                                                                                                          \
  do {                                                                                                                 \
    f32x2 v_ = rp[p];                                                                                                  \
    EMU_MASK_KTAIL(v_, p);                                                                                             \
    const uint32_t h_ = __builtin_bit_cast(uint32_t, __builtin_convertvector(v_, bf16x2));                             \
    t0[p] = h_; rp[p] = v_;                                                                                            \
    fu[p] = f32x2{__builtin_bit_cast(float, h_ << 16), __builtin_bit_cast(float, h_ & 0xffff0000u)};                   \
  } while (0)
#define U2(p) PK_SUB(rp[p], rp[p], fu[p])
#define U3(p)                                                                                                          \
  do {                                                                                                                 \
    const uint32_t h_ = __builtin_bit_cast(uint32_t, __builtin_convertvector(rp[p], bf16x2));                          \
    t1[p] = h_;                                                                                                        \
    fu[p] = f32x2{__builtin_bit_cast(float, h_ << 16), __builtin_bit_cast(float, h_ & 0xffff0000u)};                   \
  } while (0)
#define U4(p) do { f32x2 w_; PK_SUB(w_, rp[p], fu[p]); t2[p] = __builtin_bit_cast(uint32_t, __builtin_convertvector(w_, bf16x2)); } while (0)
// STA(st, i, tp, pl): the 8 bytes of plane pl (tp = t0 / t1 / t2) of item i -> the stage.  STB(st, q): weight image piece q.
#define STA(st, i, tp, pl) reinterpret_cast<u32x2*>(st)[wslot + (i) * 128 + (pl) * 4 * TM] = u32x2{tp[2 * (i)], tp[2 * (i) + 1]}
#define STB(st, q) (st)[A_U4 + tid + (q) * NT] = rb[q]
#define LDA(st, p, i) __builtin_bit_cast(bf16x8, (st)[aread + ((p) * 2 + kh) * TM + (i) * 32])
#define LDB(st, p, j) __builtin_bit_cast(bf16x8, (st)[A_U4 + wn * WN + l31 + ((p) * 2 + kh) * TN + (j) * 32])
// one MFMA + the unit that hides under it
#define M1(ax, bx, i, j, work) do { acc[i][j] = MFB(ax[i], bx[j], acc[i][j]); work; SB(); } while (0)
#define MM(ax, bx) _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < NJ; ++j) acc[i][j] = MFB(ax[i], bx[j], acc[i][j])
// phase s: on entry aX = x0 fragments of slab s - 1, b2 / b1 / bC = its weight fragments (planes 2, 1, 0), rp / rb / rm = slab
// s + 1 as loaded; cur = the stage that holds slab s, nxt = the stage that receives slab s + 1.  On exit aY, b2, b1, bN = slab s.
// The slot table (which unit hides under which MFMA) is generated: tools/gen/kc2_phase.py -> kc2_phase.inc.
#include "kc2_phase.inc"

  // the slab count is rounded up to an even number (a pad slab stages zeros for A: its products add exact zeros), so the phases
  // after the head come in pairs plus one and the two register assignments never have to merge
  const int nslab2 = (nslab + 1) & ~1;
  bf16x8 aP[4], aQ[4], bP[NJ], bQ[NJ], b1[NJ], b2[NJ];
  // prologue (left to the compiler): slab 0 -> st0, slab 1 -> registers; the first half of slab 0; slab 1 -> st1, slab 2 -> registers
#define STAGE_ALL(st, sl)                                                                                              \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                    \
      UI(i, sl);                                                                                                       \
      U1(2 * i); U2(2 * i); U3(2 * i); U4(2 * i); U1(2 * i + 1); U2(2 * i + 1); U3(2 * i + 1); U4(2 * i + 1);          \
      STA(st, i, t0, 0); STA(st, i, t1, 1); STA(st, i, t2, 2);                                                         \
    }                                                                                                                  \
    _Pragma("unroll") for (int q = 0; q < NB; ++q) STB(st, q);                                                         \
  } while (0)
#define LOAD_ALL(sl)                                                                                                   \
  do {                                                                                                                 \
    /* issue order pinned to a phase's: the vmcnt waits inside the loop are counted against BOTH histories that reach   */ \
    /* the loop head (left free, hipcc put item 0 second to last here and the odd phases waited vmcnt(1) at slot 2)    */ \
    SB(); LDGA(0, sl); SB();                                                                                           \
    _Pragma("unroll") for (int q = 0; q < NB; ++q) { LDGB(q, sl); SB(); }                                              \
    _Pragma("unroll") for (int i = 1; i < 4; ++i) { LDGA(i, sl); SB(); }                                               \
  } while (0)
  LOAD_ALL(0);
  STAGE_ALL(st0, 0);
  LOAD_ALL(1);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) { aQ[i] = LDA(st0, 2, i); aP[i] = LDA(st0, 1, i); }
#pragma unroll
  for (int j = 0; j < NJ; ++j) { bP[j] = LDB(st0, 0, j); b1[j] = LDB(st0, 1, j); b2[j] = LDB(st0, 2, j); }
  MM(aQ, bP);                                                  // x2 y0 of slab 0
#pragma unroll
  for (int i = 0; i < 4; ++i) aQ[i] = LDA(st0, 0, i);
  MM(aP, b1); MM(aP, bP);                                      // x1 y1, x1 y0
  STAGE_ALL(st1, 1);
  LOAD_ALL(2);
  SYNC();                                                      // aQ = x0 fragments of slab 0, bP / b1 / b2 its weight fragments
  for (int s = 1; s + 1 < nslab2; s += 2) {
    PHASE(st1, st0, s, aQ, aP, bP, bQ);
    SYNC();
    PHASE(st0, st1, s + 1, aP, aQ, bQ, bP);
    SYNC();
  }
  PHASE(st1, st0, nslab2 - 1, aQ, aP, bP, bQ);
  SB();
  MM(aP, b2); MM(aP, b1); MM(aP, bQ);
  __syncthreads();
#undef LDGA
#undef LDGB
#undef UI
#undef U1
#undef U2
#undef U3
#undef U4
#undef STA
#undef STB
#undef LDA
#undef LDB
#undef M1
#undef MM
#undef PHASE
#undef STAGE_ALL
#undef LOAD_ALL
  emu_epilogue<TM, TN, NJ>(g, acc, st0, m0, n0, wm, wn, wave, lane, l31, kh, MASK ? g.ascale : 1.f);
}

int emu_b3_prepare(const float* W, int ldw, int R, int Kc, int transpose, void* image, hipStream_t st) {
  const int nslab = cdiv(Kc, KS);
  const long total = (long)cdiv(R, TN) * nslab * 2 * TN;
  hipLaunchKernelGGL(emu_prep_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, W, ldw, R, Kc, transpose, nslab, total,
                     static_cast<u32x4*>(image));
  return check_launch("linear_emu_prepare");
}

int emu_b3_prepare_batch(const hoisdf_emu_prep_item* d_items, int n, long total_blocks, hipStream_t st) {
  hipLaunchKernelGGL(emu_prep_weight_batch_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, d_items, n);
  return check_launch("linear_emu_prepare_batch");
}

int emu_b3_launch(EmuArgs g, hipStream_t st) {
  g.tiles_m = cdiv(g.M, TM);
  g.tiles_n = cdiv(g.N, TN);
  const bool kt = g.K % KS != 0 || (cdiv(g.K, KS) & 1);      // a pad slab (odd slab count) stages zeros through the k-tail test
  static void (*const kernel[2][2])(EmuArgs) = {{emu_kc2_kernel<false, false>, emu_kc2_kernel<false, true>},      // [MASK][KTAIL]
                                                {emu_kc2_kernel<true, false>, emu_kc2_kernel<true, true>}};
  hipLaunchKernelGGL(kernel[g.abits != nullptr][kt], dim3((unsigned)(g.tiles_m * g.tiles_n)), dim3(NT), 0, st, g);
  return check_launch("linear_emu");
}

}  // namespace hoisdf
