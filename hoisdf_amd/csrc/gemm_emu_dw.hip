// grad-weight: dW[n][k] = sum_m dy_eff[m][n] x[m][k], db[n] = sum_m dy_eff[m][n].  The contraction runs over the ROWS of both
// operands, so each needs its planes transposed ([column][8 consecutive m]): a staging thread loads a 4-column x 8-row patch
// (8 float4, lanes along the columns: 1 KB contiguous per row), transposes it in registers and writes, per column, the three
// 16-byte pieces of that column's chunk - no transposed copy of an activation ever goes through HBM.
// Tile 256 (n) x 256 (k): one 4 x 8 patch per thread covers both operands of a 16-row slab (threads 0-127: dy, 128-255: x);
// 4 waves as 2 x 2, wave tile 128 x 128 = 4 x 4 MFMA blocks, 256 accumulators (AGPRs), one workgroup per CU; the rows are
// split over the workgroups (every slice of a tile on one XCD) into partial tiles + an ordered reduce: no atomics.
#include "gemm_emu.h"

namespace hoisdf {

namespace {
// a value the compiler cannot prove wave-uniform (it depends on tid < 128, which is uniform per wave) into scalar registers
__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
}  // namespace

// tile and row slice of a workgroup (all three kernels)
#define DW_TILE_SETUP(DTK_)                                                                                            \
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;                                                       \
  const int wm = wave >> 1, wn = wave & 1;                                                                             \
  const int l31 = lane & 31, kh = lane >> 5;                                                                           \
  const int ntile = g.tiles_n * g.tiles_k;                                                                             \
  const int bid = blockIdx.x;                                                                                          \
  const int split = (bid & 7) + 8 * (bid / (8 * ntile));      /* every slice of one tile on the same XCD (shared L2) */ \
  const int t = (bid >> 3) % ntile;                                                                                    \
  if (split >= g.splitk) return;                                                                                       \
  const int tn = t / g.tiles_k, tk = t - tn * g.tiles_k;                                                               \
  const int n0 = tn * DT, k0 = tk * DTK_;                                                                              \
  const int mbeg = split * g.m_per_split;                                                                              \
  const int mend = min(g.M, mbeg + g.m_per_split);                                                                     \
  const int nslab = (mend - mbeg + KS - 1) / KS;

// bias gradient partial of emu_dw2_kernel / emu_dw2h_kernel: the two chunk threads of a column group add up through LDS
#define DW2_STORE_COLSUM()                                                                                             \
  do {                                                                                                                 \
    if (HASDB && tk == 0) {                                                                                            \
      float* red = reinterpret_cast<float*>(lds);                                                                      \
      if (isA) *reinterpret_cast<f32x4*>(&red[c * DT + 4 * cg]) = csum * post;                                         \
      __syncthreads();                                                                                                 \
      if (tid < DT) {                                                                                                  \
        const int n = n0 + tid;                                                                                        \
        if (n < g.N) g.colsum[(size_t)split * g.colsum_split_stride + n] = red[tid] + red[DT + tid];                   \
      }                                                                                                                \
      __syncthreads();                                                                                                 \
    }                                                                                                                  \
  } while (0)
// transposing epilogue of a 256 x DTK_ tile (all three kernels): one row of 32 x 32 blocks (32 x DTK_ / 2) at a time through the wave's
// private LDS slice; VAL = what is stored for acc[i][j][r] (the 1 / keep of the sign bitmap, the f16x2 form's operand scales).  A macro:
// as a __forceinline__ function template it changed the register allocation of all ten kernels (profiles/gemm_emu_split_codegen.txt)
#define DW_EPILOGUE(DTK_, VAL)                                                                                         \
  do {                                                                                                                 \
    float* Cb = g.C + (size_t)split * g.c_split_stride;                                                                \
    const bool full = (n0 + DT <= g.N) && (k0 + (DTK_) <= g.K) && (g.K % 4 == 0);                                      \
    constexpr int WK_ = (DTK_) / 2, ES = WK_ + 4;                                                                      \
    constexpr int LPR = WK_ / 4, RPI = 64 / LPR;          /* lanes per row (one float4 each), rows per wave instruction */ \
    float* w = reinterpret_cast<float*>(lds) + wave * (32 * ES);                                                       \
    _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                    \
      _Pragma("unroll") for (int j = 0; j < (DTK_) / 64; ++j)                                                          \
        _Pragma("unroll") for (int r = 0; r < 16; ++r) w[((r & 3) + 8 * (r >> 2) + 4 * kh) * ES + j * 32 + l31] = (VAL); \
      _Pragma("unroll") for (int p = 0; p < 32 / RPI; ++p) {                                                           \
        const int rr = p * RPI + lane / LPR, cc = (lane % LPR) * 4;                                                    \
        const int row = n0 + wm * 128 + i * 32 + rr, col = k0 + wn * WK_ + cc;                                         \
        const float4 v = *reinterpret_cast<const float4*>(w + rr * ES + cc);                                           \
        if (full) {                                                                                                    \
          *reinterpret_cast<float4*>(Cb + (size_t)row * g.K + col) = v;                                                \
        } else if (row < g.N) {                                                                                        \
          float* cp = Cb + (size_t)row * g.K + col;                                                                    \
          if (col + 0 < g.K) cp[0] = v.x;                                                                              \
          if (col + 1 < g.K) cp[1] = v.y;                                                                              \
          if (col + 2 < g.K) cp[2] = v.z;                                                                              \
          if (col + 3 < g.K) cp[3] = v.w;                                                                              \
        }                                                                                                              \
      }                                                                                                                \
    }                                                                                                                  \
  } while (0)

// DTK = tile width along k: 128 (wave tile 128 x 64, two workgroups per CU: the conversion phase of one overlaps the MFMAs of the
// other; x patches on wave 2 only, wave 3 stages nothing) is the one instantiated, for K <= 128.  The body also holds the 256-wide
// tile (wave tile 128 x 128, one workgroup per CU), which emu_dw2_kernel / emu_dw2h_kernel replaced.
template <bool MASK, int DTK>
__global__ __launch_bounds__(NT, DTK == 256 ? 1 : 2) void emu_dw_kernel(DwArgs g) {
  constexpr int NJ = DTK / 64;                         // 32-column blocks per wave along k
  constexpr int WK = DTK / 2;                          // wave tile width along k
  constexpr int A_U4 = 3 * 2 * DT, STAGE = A_U4 + 3 * 2 * DTK;
  extern __shared__ __attribute__((aligned(16))) u32x4 lds[];
  DW_TILE_SETUP(DTK)
  const int last = nslab - 1;

  f32x16 acc[4][NJ];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // staging patch of this thread: operand (wave-uniform), column group cg (4 columns), chunk c (8 rows of the slab)
  const bool isA = tid < 128;
  const bool stager = DTK == 256 || tid < 192;          // (wave-uniform)
  const int cg = (isA || DTK == 256) ? (tid & 63) : (tid & 31), c = (isA || DTK == 256) ? ((tid >> 6) & 1) : ((tid >> 5) & 1);
  const int col0 = (isA ? n0 : k0) + 4 * cg;
  const int ncol = isA ? g.N : g.K;                      // multiples of 4 (checked by the host): a patch column group is all in or out
  const bool col_ok = stager && col0 < ncol;
  // addresses: a wave-uniform row base (scalar registers: operand pointer + slab row * leading dimension + e rows) plus ONE
  // per-thread byte offset that never changes (chunk rows + column group) - no vector address arithmetic in the slab loop
  const long ld = uni64(isA ? g.lddy : g.ldx);
  // (x addressed relative to dy: pointer arithmetic on a kernel argument keeps the global address space, an integer round trip
  // would turn the loads into flat ones)
  const char* opbase = reinterpret_cast<const char*>(g.dy) +
                       (long)uni64(isA ? 0ul : (uint64_t)(reinterpret_cast<const char*>(g.x) - reinterpret_cast<const char*>(g.dy)));
  const uint32_t voff = (uint32_t)(((long)c * 8 * ld + (col_ok ? col0 : 0)) * 4);
  const char* bitbase = reinterpret_cast<const char*>(g.bits);
  const uint32_t boff = (uint32_t)(((long)c * 8 * g.ldbits + ((col_ok ? col0 : 0) >> 5)) * 4);
  const float* src = (isA ? g.dy : g.x) + (col_ok ? col0 : 0);
  const uint32_t* bsrc = (MASK && isA) ? g.bits + ((col_ok ? col0 : 0) >> 5) : nullptr;
  const int bsh = col0 & 31;
  const bool do_colsum = isA && g.colsum != nullptr && tk == 0;
  float4 rv[8];
  uint32_t rm[8];
  float4 csum = make_float4(0.f, 0.f, 0.f, 0.f);
#define DW_LOAD(sl)                                                                                                   \
  do {                                                                                                                \
    const int ms_ = mbeg + (sl) * KS;                        /* (uniform) first row of the slab */                    \
    if (ms_ + KS <= g.M) {                                                                                            \
      const char* sb_ = opbase + (size_t)ms_ * ld * 4;                                                                \
      const char* mb2_ = bitbase + (size_t)ms_ * g.ldbits * 4;                                                        \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                 \
        rv[e] = *reinterpret_cast<const float4*>(sb_ + (size_t)e * ld * 4 + voff);                                    \
        if (MASK) rm[e] = isA ? *reinterpret_cast<const uint32_t*>(mb2_ + (size_t)e * g.ldbits * 4 + boff) : 0xffffffffu; \
      }                                                                                                               \
    } else {                                                 /* the slab that crosses the end of the operands */      \
      const int mb_ = ms_ + c * 8;                                                                                    \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                 \
        const int m_ = min(mb_ + e, g.M - 1);                                                                         \
        rv[e] = *reinterpret_cast<const float4*>(src + (size_t)m_ * ld);                                              \
        if (MASK) rm[e] = isA ? bsrc[(size_t)m_ * g.ldbits] : 0xffffffffu;                                            \
      }                                                                                                               \
    }                                                                                                                 \
  } while (0)
#define DW_STORE(st, sl)                                                                                              \
  do {                                                                                                                \
    const int mb_ = mbeg + (sl) * KS + c * 8;                                                                         \
    _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                   \
      float4 v_ = rv[e];                                                                                              \
      if (MASK && isA) {                                                                                              \
        const uint32_t nib_ = rm[e] >> bsh;                                                                           \
        v_.x = (nib_ & 1u) ? v_.x * g.ascale : 0.f;                                                                   \
        v_.y = (nib_ & 2u) ? v_.y * g.ascale : 0.f;                                                                   \
        v_.z = (nib_ & 4u) ? v_.z * g.ascale : 0.f;                                                                   \
        v_.w = (nib_ & 8u) ? v_.w * g.ascale : 0.f;                                                                   \
      }                                                                                                               \
      rv[e] = v_;                                                                                                     \
    }                                                                                                                 \
    if (!col_ok || mbeg + (sl) * KS + KS > mend) {           /* (rare) rows past the slice, columns past the operand */ \
      _Pragma("unroll") for (int e = 0; e < 8; ++e)                                                                   \
        if (mb_ + e >= mend || !col_ok) rv[e] = make_float4(0.f, 0.f, 0.f, 0.f);                                      \
    }                                                                                                                 \
    if (do_colsum) {                                                                                                  \
      _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                 \
        csum.x += rv[e].x; csum.y += rv[e].y; csum.z += rv[e].z; csum.w += rv[e].w;                                   \
      }                                                                                                               \
    }                                                                                                                 \
    const int rs_ = isA ? DT : DTK;                          /* rows per (plane, chunk) region of this operand */      \
    u32x4* dst_ = (st) + (isA ? 0 : A_U4) + c * rs_ + 4 * cg;                                                         \
    bf16x8 p0, p1, p2;                                                                                                \
    split3x8(make_float4(rv[0].x, rv[1].x, rv[2].x, rv[3].x), make_float4(rv[4].x, rv[5].x, rv[6].x, rv[7].x), p0, p1, p2); \
    dst_[0] = __builtin_bit_cast(u32x4, p0); dst_[2 * rs_] = __builtin_bit_cast(u32x4, p1); dst_[4 * rs_] = __builtin_bit_cast(u32x4, p2); \
    split3x8(make_float4(rv[0].y, rv[1].y, rv[2].y, rv[3].y), make_float4(rv[4].y, rv[5].y, rv[6].y, rv[7].y), p0, p1, p2); \
    dst_[1] = __builtin_bit_cast(u32x4, p0); dst_[2 * rs_ + 1] = __builtin_bit_cast(u32x4, p1); dst_[4 * rs_ + 1] = __builtin_bit_cast(u32x4, p2); \
    split3x8(make_float4(rv[0].z, rv[1].z, rv[2].z, rv[3].z), make_float4(rv[4].z, rv[5].z, rv[6].z, rv[7].z), p0, p1, p2); \
    dst_[2] = __builtin_bit_cast(u32x4, p0); dst_[2 * rs_ + 2] = __builtin_bit_cast(u32x4, p1); dst_[4 * rs_ + 2] = __builtin_bit_cast(u32x4, p2); \
    split3x8(make_float4(rv[0].w, rv[1].w, rv[2].w, rv[3].w), make_float4(rv[4].w, rv[5].w, rv[6].w, rv[7].w), p0, p1, p2); \
    dst_[3] = __builtin_bit_cast(u32x4, p0); dst_[2 * rs_ + 3] = __builtin_bit_cast(u32x4, p1); dst_[4 * rs_ + 3] = __builtin_bit_cast(u32x4, p2); \
  } while (0)

  if (nslab > 0 && stager) {
    DW_LOAD(0);
    DW_STORE(lds, 0);
    DW_LOAD(min(1, last));
  }
  __syncthreads();

  for (int s = 0; s < nslab; ++s) {
    const u32x4* st = lds + (s & 1) * STAGE;
    u32x4* nx = lds + ((s + 1) & 1) * STAGE;
    const u32x4* sa = st + wm * 128 + l31;
    const u32x4* sb = st + A_U4 + wn * WK + l31;
    bf16x8 b0[NJ], b1[NJ], b2[NJ], a[4];
#define RD_B(dst, p) _Pragma("unroll") for (int j = 0; j < NJ; ++j) dst[j] = __builtin_bit_cast(bf16x8, sb[((p) * 2 + kh) * DTK + j * 32])
#define RD_A(p) _Pragma("unroll") for (int i = 0; i < 4; ++i) a[i] = __builtin_bit_cast(bf16x8, sa[((p) * 2 + kh) * DT + i * 32])
#define MM1(bx) _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < NJ; ++j) acc[i][j] = MFB(a[i], bx[j], acc[i][j])
    // long phase first: 48 MFMAs queue up right behind the barrier, the conversion of the next slab follows them.  (Measured
    // on MI355X, tools/mb_emu.py: pinning only the global loads and letting hipcc spread the conversion over the MFMAs, or an
    // explicit sched_group_barrier pipeline of 1 MFMA + 6 VALU, are within 2 % of this form.)
    RD_B(b0, 0); RD_A(0); RD_B(b1, 1); RD_B(b2, 2);
    MM1(b2); MM1(b1); MM1(b0);                 // x0 y2, x0 y1, x0 y0
    __builtin_amdgcn_sched_barrier(0);
    RD_A(1);
    if (stager) {
      if (s + 1 < nslab) DW_STORE(nx, s + 1);
      DW_LOAD(min(s + 2, last));
    }
    __builtin_amdgcn_sched_barrier(0);
    MM1(b1); MM1(b0);                          // x1 y1, x1 y0
    RD_A(2);
    MM1(b0);                                   // x2 y0
    __syncthreads();
  }
#undef DW_LOAD
#undef DW_STORE
#undef RD_A
#undef RD_B
#undef MM1

  // bias gradient partial: the two chunk threads of a column group add up through LDS (all waves are past the last barrier)
  if (g.colsum != nullptr && tk == 0) {
    float* red = reinterpret_cast<float*>(lds);
    if (isA) *reinterpret_cast<float4*>(&red[c * DT + 4 * cg]) = csum;
    __syncthreads();
    if (tid < DT) {
      const int n = n0 + tid;
      if (n < g.N) g.colsum[(size_t)split * g.colsum_split_stride + n] = red[tid] + red[DT + tid];
    }
    __syncthreads();
  }

  DW_EPILOGUE(DTK, acc[i][j][r]);
}

// ---- text emu_dw2_kernel and emu_dw2h_kernel share (macros: each kernel sees the tokens it would see with the text in place).
// DW2_STAGING_SETUP(A_U4_): staging role, addresses and LDS units of a thread's patch (A_U4_ = 16-byte units of the dy half of a stage)
#define DW2_STAGING_SETUP(A_U4_)                                                                                       \
  /* staging role of the wave: waves 0 / 1 the dy patch of chunk 0 / 1 (rows 0-7 / 8-15 of the slab), waves 2 / 3 the x patch */ \
  const bool isA = wave < 2;                                                                                           \
  const int c = wave & 1, cg = lane;                                                                                   \
  const int col0 = (isA ? n0 : k0) + 4 * cg;                                                                           \
  const bool col_ok = col0 < (isA ? g.N : g.K);             /* N, K multiples of 4: a column group is all in or all out */ \
  const long ld = uni64(isA ? g.lddy : g.ldx);                                                                         \
  const char* opbase = reinterpret_cast<const char*>(g.dy) +                                                           \
                       (long)uni64(isA ? 0ul : (uint64_t)(reinterpret_cast<const char*>(g.x) - reinterpret_cast<const char*>(g.dy))); \
  /* row e of the patch: one per-lane offset register + e * (row stride), added at the load (a scalar operand of the add); a lane whose */ \
  /* columns lie past the operand starts 1 GB out of range and reads zeros */                                          \
  const int voff0 = col_ok ? (int)(((long)c * 8 * ld + col0) * 4) : 0x40000000;                                        \
  const int boff0 = (MASK && isA && col_ok) ? (int)(((long)c * 8 * g.ldbits + (col0 >> 5)) * 4) : 0x40000000;          \
  const int ldb4 = (int)(ld * 4), ldm4 = g.ldbits * 4;                                                                 \
  const uint32_t notA = isA ? 0u : 0xffffffffu;              /* x patches carry no bitmap */                           \
  const int bsh = col0 & 31;                                 /* the patch's four sign bits within its bitmap word */   \
  constexpr bool SWZ = true;                                                                                           \
  const int sw = SWZ ? (cg >> 1) & 3 : 0;                                                                              \
  const int wbase = (isA ? 0 : A_U4_) + c * DT + 4 * cg;       /* unit of the patch's first column in plane 0 (column j: + (j ^ sw)) */ \
  const int rsw = SWZ ? (l31 >> 3) & 3 : 0;                                                                            \
  const int aread = (wm * 128 + l31) ^ rsw, bread = A_U4_ + ((wn * 128 + l31) ^ rsw);                                  \
  f32x2 rvL[8], rvH[8];                                       /* the patch: columns 0-1 / 2-3 of its eight rows */     \
  uint32_t rm[8], mpk = 0xffffffffu;                          /* bitmap words of the slab in flight; the 8 x 4 sign bits of the patch being converted */
// DLDG(hf, e, sl): half hf (columns 2 hf, 2 hf + 1) of row e of the patch of slab sl through the slab's descriptor [first row of the
// slab, end of the slice);
// DLDM(e, sl): its bitmap word
#define DSLAB(sl)                                                                                                      \
    const int ms_ = mbeg + (sl) * KS;                                                                                  \
    const int left_ = max(mend - ms_, 0);                     /* (uniform) rows of the slice from this slab on */
#define DLDG(hf, e, sl)                                                                                                \
  do {                                                                                                                 \
    DSLAB(sl)                                                                                                          \
    const __amdgpu_buffer_rsrc_t r_ = __builtin_amdgcn_make_buffer_rsrc(                                               \
        const_cast<char*>(opbase + (size_t)ms_ * ld * 4), 0, (int)min((long)left_ * ld * 4, 0x3fffffffL), 0x00020000); \
    const f32x2 v_ = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r_, voff0 + (e) * ldb4 + (hf) * 8, 0, 0)); \
    if ((hf) == 0) rvL[e] = v_; else rvH[e] = v_;                                                                      \
  } while (0)
#define DLDM(e, sl)                                                                                                    \
  do {                                                                                                                 \
    if (MASK) {                                                                                                        \
      DSLAB(sl)                                                                                                        \
      const __amdgpu_buffer_rsrc_t b_ = __builtin_amdgcn_make_buffer_rsrc(                                             \
          const_cast<uint32_t*>(g.bits + (size_t)ms_ * g.ldbits), 0, (int)min((long)left_ * g.ldbits * 4, 0x3fffffffL), 0x00020000); \
      rm[e] = __builtin_amdgcn_raw_buffer_load_b32(b_, boff0 + (e) * ldm4, 0, 0);                                      \
    }                                                                                                                  \
  } while (0)
#define DLOAD_ALL(sl) _Pragma("unroll") for (int e = 0; e < 8; ++e) { DLDG(0, e, sl); DLDG(1, e, sl); }
#define DLOADM_ALL(sl) _Pragma("unroll") for (int e = 0; e < 8; ++e) DLDM(e, sl)

// ---- grad-weight, second form ("rotated", hand-interleaved; 256 x 256 tiles): same partial-tile plan, product order and
// epilogue as emu_dw_kernel (results are bit identical without a sign bitmap), with the main loop rebuilt the way
// emu_kc2_kernel's was - here it matters more, because this kernel runs ONE wave per SIMD (256 accumulators) and nothing else
// covers a wave's conversion phase:
//  * a phase = [x1 y1, x1 y0, x2 y0 of slab s - 1 | x0 y2, x0 y1, x0 y0 of slab s] between two barriers (96 MFMAs): the 48 MFMAs
//    behind the barrier run on fragments read before it, every fragment read is 12 ... 48 MFMAs ahead of its use;
//  * the staging of slab s + 1 (a 4-column x 8-row patch per thread: 16 row pairs x {first plane, residual, second plane,
//    residual + third plane}, 12 LDS writes) is pinned unit by unit behind the MFMAs of the same wave (tools/gen/dw2_phase.py);
//    the patch sits in two half sets (columns 0-1 / 2-3 of its rows, 8-byte loads): a half is requested again for slab s + 2
//    the moment its two columns of slab s + 1 are converted, >= 56 MFMAs ahead of its next use - no second patch set
//    (the arch-VGPR half of the register file holds the fragments, 96, and the staging state; the accumulators fill the AGPRs);
//  * loads are buffer loads through a per-slab descriptor [first row of the slab, end of the row slice): rows past the slice
//    and the pad slab read as zero without a single select, columns past the operand by an out-of-range offset;
//  * the LDS column of output index n is n ^ ((n >> 3) & 3): with the plain layout the 16-byte writes of a patch (four
//    adjacent columns per lane = a 64-byte lane stride) hit two of the 32 store banks groups 4-way; the fragment reads
//    (32 consecutive columns per half-wave) stay conflict-free under the swizzle;
//  * the 1 / keep factor of the sign bitmap is applied once to the finished tile / bias-gradient partial, the bitmap itself
//    as a bit-extended and.
namespace {
constexpr int DSTAGE = 3 * 2 * DT * 2;                   // 16-byte units per stage: three planes x two chunks x (256 dy + 256 x columns)
}
template <bool MASK, bool HASDB>
__global__ __launch_bounds__(NT, 1) void emu_dw2_kernel(DwArgs g) {
  constexpr int A_U4 = 3 * 2 * DT;
  __shared__ __attribute__((aligned(16))) u32x4 s0[DSTAGE];
  __shared__ __attribute__((aligned(16))) u32x4 s1[DSTAGE];
  DW_TILE_SETUP(DT)

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  DW2_STAGING_SETUP(A_U4)
  uint32_t t0[4], t1[4], t2[4];
  f32x2 rp_, fu_;
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};
// the conversion of rows 2 pr, 2 pr + 1 of column j of the patch: DU1 bitmap + first plane (column 0 first packs the two rows' four
// sign bits into mpk - nibble e = row e - which frees the word registers for the next slab's words), DU2 first residual, DU3 second
// plane, DU4 second residual + third plane
#define DU1(j, pr)                                                                                                     \
  do {                                                                                                                 \
    f32x2 v_ = (j) < 2 ? f32x2{rvL[2 * (pr)][(j) & 1], rvL[2 * (pr) + 1][(j) & 1]} : f32x2{rvH[2 * (pr)][(j) & 1], rvH[2 * (pr) + 1][(j) & 1]}; \
    if (MASK) {                                                                                                        \
      if ((j) == 0) {                                                                                                  \
        const uint32_t n0_ = ((rm[2 * (pr)] | notA) >> bsh) & 0xfu, n1_ = ((rm[2 * (pr) + 1] | notA) >> bsh) & 0xfu;   \
        mpk = ((pr) == 0 ? 0u : mpk) | (n0_ << (8 * (pr))) | (n1_ << (8 * (pr) + 4));                                  \
      }                                                                                                                \
      float xa_, xb_;     /* (asm: see emu_kc2_kernel's U1) */                                                         \
      asm("v_and_b32 %0, %1, %2" : "=v"(xa_) : "v"(__builtin_amdgcn_sbfe((int)mpk, 8 * (pr) + (j), 1)), "v"(v_.x));    \
      asm("v_and_b32 %0, %1, %2" : "=v"(xb_) : "v"(__builtin_amdgcn_sbfe((int)mpk, 8 * (pr) + 4 + (j), 1)), "v"(v_.y)); \
      v_ = f32x2{xa_, xb_};                                                                                            \
    }                                                                                                                  \
    if (HASDB) csum[j] += v_.x + v_.y;                                                                                 \
    const uint32_t h_ = __builtin_bit_cast(uint32_t, __builtin_convertvector(v_, bf16x2));                             \
    t0[pr] = h_; rp_ = v_;                                                                                             \
    fu_ = f32x2{__builtin_bit_cast(float, h_ << 16), __builtin_bit_cast(float, h_ & 0xffff0000u)};                     \
  } while (0)
#define DU2(j, pr) PK_SUB(rp_, rp_, fu_)
#define DU3(j, pr)                                                                                                     \
  do {                                                                                                                 \
    const uint32_t h_ = __builtin_bit_cast(uint32_t, __builtin_convertvector(rp_, bf16x2));                            \
    t1[pr] = h_;                                                                                                       \
    fu_ = f32x2{__builtin_bit_cast(float, h_ << 16), __builtin_bit_cast(float, h_ & 0xffff0000u)};                     \
  } while (0)
#define DU4(j, pr) do { f32x2 w_; PK_SUB(w_, rp_, fu_); t2[pr] = __builtin_bit_cast(uint32_t, __builtin_convertvector(w_, bf16x2)); } while (0)
#define DSTA(st, j, pl) (st)[wbase + ((j) ^ sw) + (pl) * 2 * DT] = ((pl) == 0 ? u32x4{t0[0], t0[1], t0[2], t0[3]} : (pl) == 1 ? u32x4{t1[0], t1[1], t1[2], t1[3]} : u32x4{t2[0], t2[1], t2[2], t2[3]})
#define DLA(st, p, i) __builtin_bit_cast(bf16x8, (st)[aread + ((p) * 2 + kh) * DT + (i) * 32])
#define DLB(st, p, j) __builtin_bit_cast(bf16x8, (st)[bread + ((p) * 2 + kh) * DT + (j) * 32])
#define M1(ax, bx, i, j, work) do { acc[i][j] = MFB(ax[i], bx[j], acc[i][j]); work; SB(); } while (0)
#define MM(ax, bx) _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[i][j] = MFB(ax[i], bx[j], acc[i][j])
#include "dw2_phase.inc"
#define DSTAGE_ALL(st)                                                                                                 \
  do {                                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                    \
      _Pragma("unroll") for (int pr = 0; pr < 4; ++pr) { DU1(j, pr); DU2(j, pr); DU3(j, pr); DU4(j, pr); }             \
      DSTA(st, j, 0); DSTA(st, j, 1); DSTA(st, j, 2);                                                                  \
    }                                                                                                                  \
  } while (0)

  // the slab count is rounded up to an even number (a pad slab reads zeros through its empty descriptor); phases after the head
  // come in pairs plus one.
  const int nslab2 = (max(nslab, 1) + 1) & ~1;
  bf16x8 aX[4], aY[4], aZ[4], bP[4], bQ[4], bR[4];
  DLOAD_ALL(0);
  DLOADM_ALL(0);
  DSTAGE_ALL(s0);
  DLOAD_ALL(1);
  DLOADM_ALL(1);
  __syncthreads();
  // head (left to the compiler): the first half of slab 0, slab 1 -> s1, slab 2 requested
#pragma unroll
  for (int i = 0; i < 4; ++i) { aZ[i] = DLA(s0, 0, i); aX[i] = DLA(s0, 1, i); aY[i] = DLA(s0, 2, i); }
#pragma unroll
  for (int j = 0; j < 4; ++j) { bQ[j] = DLB(s0, 0, j); bP[j] = DLB(s0, 1, j); bR[j] = DLB(s0, 2, j); }
  MM(aZ, bR); MM(aZ, bP); MM(aZ, bQ);                         // x0 y2, x0 y1, x0 y0 of slab 0; bP = y1, bQ = y0 stay for the next phase
  DSTAGE_ALL(s1);
  DLOAD_ALL(2);
  DLOADM_ALL(2);
  SYNC();
  for (int s = 1; s + 1 < nslab2; s += 2) {
    DPHASE(s1, s0, s, aX, aY, aZ, bP, bQ, bR);
    SYNC();
    DPHASE(s0, s1, s + 1, aX, aY, aZ, bR, bQ, bP);
    SYNC();
  }
  DPHASE(s1, s0, nslab2 - 1, aX, aY, aZ, bP, bQ, bR);
  SB();
  MM(aX, bR); MM(aX, bQ); MM(aY, bQ);                         // x1 y1, x1 y0, x2 y0 of the last slab
  __syncthreads();
#undef DU1
#undef DU2
#undef DU3
#undef DU4
#undef DSTA
#undef DLA
#undef DLB
#undef M1
#undef MM
#undef DPHASE
#undef DSTAGE_ALL
  const float post = MASK ? g.ascale : 1.f;
  u32x4* lds = s0;
  DW2_STORE_COLSUM();
  DW_EPILOGUE(DT, MASK ? acc[i][j][r] * post : acc[i][j][r]);
}

// ---- f16x2 form of the 256 x 256 grad-weight tile (see "f16x2 form" above): both f32 operands scaled by their own power of two and
// split into hi + lo f16 pieces in the staging registers, three MFMA products per slab (tools/gen/dw2h_phase.py -> dw2h_phase.inc),
// stage = two planes (32 KB), the bias gradient from the unscaled values, dW scaled back in the epilogue.  The largest magnitudes
// come as magnitude words (common.h) from whoever produced dy and x, or from emu_amax_launch.
template <bool MASK, bool HASDB>
__global__ __launch_bounds__(NT, 1) void emu_dw2h_kernel(DwArgs g) {
  constexpr int A_U4 = 2 * 2 * DT;                           // two planes x two chunks x 256 columns
  constexpr int STG = 2 * A_U4;                              // dy + x: 16-byte units per stage (32 KB)
  constexpr int EPI = (4 * 32 * (DT / 2 + 4) * 4 + 15) / 16; // the epilogue's four transposition slices
  __shared__ __attribute__((aligned(16))) u32x4 lds_all[2 * STG > EPI ? 2 * STG : EPI];
  __shared__ uint32_t red4[4];
  u32x4* const s0 = lds_all;
  u32x4* const s1 = lds_all + STG;
  DW_TILE_SETUP(DT)
  // operand scales from the row magnitudes (common.h) of THIS slice's rows (the contraction runs over them, so one scale per operand
  // and slice; the partial tile leaves unscaled): dy s_dy and x s_x in [2^13, 2^14) at the slice's largest element
  f16_saturate_on();
  uint32_t am_dy = 0u, am_x = 0u;
  for (int i = mbeg + (int)threadIdx.x; i < mend; i += NT) { am_dy = max(am_dy, g.dy_amax[i]); am_x = max(am_x, g.x_amax[i]); }
  am_dy = block_max_u32(am_dy, red4);
  __syncthreads();
  am_x = block_max_u32(am_x, red4);

  f32x16 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  DW2_STAGING_SETUP(A_U4)
  uint32_t t0[4], t1[4];
  const float sc = isA ? h2_scale(am_dy) : h2_scale(am_x);   // (wave-uniform)
  f32x2 rp_, fu_;
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};
// the conversion of rows 2 pr, 2 pr + 1 of column j of the patch: DU1 bitmap + first plane (column 0 first packs the two rows' four
// sign bits into mpk - nibble e = row e - which frees the word registers for the next slab's words), DU2 first residual, DU3 second
// plane, DU4 second residual + third plane
#define DU1(j, pr)                                                                                                     \
  do {                                                                                                                 \
    f32x2 v_ = (j) < 2 ? f32x2{rvL[2 * (pr)][(j) & 1], rvL[2 * (pr) + 1][(j) & 1]} : f32x2{rvH[2 * (pr)][(j) & 1], rvH[2 * (pr) + 1][(j) & 1]}; \
    if (MASK) {                                                                                                        \
      if ((j) == 0) {                                                                                                  \
        const uint32_t n0_ = ((rm[2 * (pr)] | notA) >> bsh) & 0xfu, n1_ = ((rm[2 * (pr) + 1] | notA) >> bsh) & 0xfu;   \
        mpk = ((pr) == 0 ? 0u : mpk) | (n0_ << (8 * (pr))) | (n1_ << (8 * (pr) + 4));                                  \
      }                                                                                                                \
      float xa_, xb_;     /* (asm: see emu_kc2_kernel's U1) */                                                         \
      asm("v_and_b32 %0, %1, %2" : "=v"(xa_) : "v"(__builtin_amdgcn_sbfe((int)mpk, 8 * (pr) + (j), 1)), "v"(v_.x));    \
      asm("v_and_b32 %0, %1, %2" : "=v"(xb_) : "v"(__builtin_amdgcn_sbfe((int)mpk, 8 * (pr) + 4 + (j), 1)), "v"(v_.y)); \
      v_ = f32x2{xa_, xb_};                                                                                            \
    }                                                                                                                  \
    if (HASDB) csum[j] += v_.x + v_.y;                                                                                 \
    v_ *= sc;                                                                                                          \
    const f16x2 h_ = __builtin_convertvector(v_, f16x2);      /* v_cvt_pk_f16_f32, round to nearest */                 \
    t0[pr] = __builtin_bit_cast(uint32_t, h_); rp_ = v_;                                                               \
    fu_ = __builtin_convertvector(h_, f32x2);                                                                          \
  } while (0)
#define DU2(j, pr) do { f32x2 w_; PK_SUB(w_, rp_, fu_); t1[pr] = __builtin_bit_cast(uint32_t, __builtin_convertvector(w_, f16x2)); } while (0)
#define DSTA(st, j, pl) (st)[wbase + ((j) ^ sw) + (pl) * 2 * DT] = ((pl) == 0 ? u32x4{t0[0], t0[1], t0[2], t0[3]} : u32x4{t1[0], t1[1], t1[2], t1[3]})
#define DLA(st, p, i) __builtin_bit_cast(f16x8, (st)[aread + ((p) * 2 + kh) * DT + (i) * 32])
#define DLB(st, p, j) __builtin_bit_cast(f16x8, (st)[bread + ((p) * 2 + kh) * DT + (j) * 32])
#define M1(ax, bx, i, j, work) do { acc[i][j] = MFH(ax[i], bx[j], acc[i][j]); work; SB(); } while (0)
#define MM(ax, bx) _Pragma("unroll") for (int i = 0; i < 4; ++i) _Pragma("unroll") for (int j = 0; j < 4; ++j) acc[i][j] = MFH(ax[i], bx[j], acc[i][j])
#include "dw2h_phase.inc"
#define DSTAGE_ALL(st)                                                                                                 \
  do {                                                                                                                 \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                    \
      _Pragma("unroll") for (int pr = 0; pr < 4; ++pr) { DU1(j, pr); DU2(j, pr); }                                     \
      DSTA(st, j, 0); DSTA(st, j, 1);                                                                                  \
    }                                                                                                                  \
  } while (0)

  // the slab count is rounded up to an even number (a pad slab reads zeros through its empty descriptor); phases after the head
  // come in pairs plus one.
  const int nslab2 = (max(nslab, 1) + 1) & ~1;
  f16x8 aH[4], aL[4], bP[4], bQ[4], bL[4];
  DLOAD_ALL(0);
  DLOADM_ALL(0);
  DSTAGE_ALL(s0);
  DLOAD_ALL(1);
  DLOADM_ALL(1);
  __syncthreads();
  // head (left to the compiler): the first half of slab 0, slab 1 -> s1, slab 2 requested
#pragma unroll
  for (int i = 0; i < 4; ++i) { aL[i] = DLA(s0, 1, i); aH[i] = DLA(s0, 0, i); }
#pragma unroll
  for (int j = 0; j < 4; ++j) { bP[j] = DLB(s0, 0, j); bL[j] = DLB(s0, 1, j); }
  MM(aL, bP); MM(aH, bL);                                     // lo hi, hi lo of slab 0; aH / bP = its hi pieces stay for the next phase
  DSTAGE_ALL(s1);
  DLOAD_ALL(2);
  DLOADM_ALL(2);
  SYNC();
  for (int s = 1; s + 1 < nslab2; s += 2) {
    DHPHASE(s1, s0, s, bP, bQ);
    SYNC();
    DHPHASE(s0, s1, s + 1, bQ, bP);
    SYNC();
  }
  DHPHASE(s1, s0, nslab2 - 1, bP, bQ);
  SB();
  MM(aH, bQ);                                                 // hi hi of the last slab
  __syncthreads();
#undef DU1
#undef DU2
#undef DSTA
#undef DLA
#undef DLB
#undef M1
#undef MM
#undef DHPHASE
#undef DSTAGE_ALL
  const float unscale = h2_inv_scale(am_dy) * h2_inv_scale(am_x);
  const float post = MASK ? g.ascale : 1.f;
  u32x4* lds = lds_all;
  DW2_STORE_COLSUM();
  DW_EPILOGUE(DT, acc[i][j][r] * (MASK ? post * unscale : unscale));
}

// out[i] = sum_s part[s * stride + i], deterministic: a block owns 256 consecutive floats (64 lanes x float4), its 16 waves sum
// the slices s = w, w + 16, ... in order (16 independent 1 KB streams per block keep the loads in flight) and the 16 partial sums
// are combined in wave order through LDS.  n must be a multiple of 4 (N * K and N are).
// Two reductions in one launch (dW and db of a grad-weight call): blocks [0, blocks0) serve (part, stride, out, n), the rest
// (part1, stride1, out1, n1).
__global__ __launch_bounds__(1024) void emu_reduce_partials_kernel(const float* __restrict__ part, long stride, int splits,
                                                                   float* __restrict__ out, long n, int blocks0,
                                                                   const float* __restrict__ part1, long stride1,
                                                                   float* __restrict__ out1, long n1) {
  __shared__ float4 red[16][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int blk = blockIdx.x;
  if (blk >= blocks0) { blk -= blocks0; part = part1; stride = stride1; out = out1; n = n1; }
  const long i = ((long)blk * 64 + lane) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n) {
    const float* p = part + i;
    int k = w;
    for (; k + 16 < splits; k += 32) {
      const float4 u = *reinterpret_cast<const float4*>(p + (size_t)k * stride);
      const float4 v = *reinterpret_cast<const float4*>(p + (size_t)(k + 16) * stride);
      s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (k < splits) {
      const float4 u = *reinterpret_cast<const float4*>(p + (size_t)k * stride);
      s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
    }
  }
  red[w][lane] = s;
  __syncthreads();
  if (w == 0 && i < n) {
    float4 t = red[0][lane];
#pragma unroll
    for (int j = 1; j < 16; ++j) {
      const float4 v = red[j][lane];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    *reinterpret_cast<float4*>(out + i) = t;
  }
}

// row slices for grad-weight: one workgroup per CU (256 slots), >= 8 slabs per slice
// k-tile width: 256 (one workgroup per CU: the rotated emu_dw2_kernel / emu_dw2h_kernel) unless K <= 128, where half of a 256-wide tile
// would be padding: emu_dw_kernel at its 128-wide tile, two workgroups per CU.
int dw_tile(int K) { return K <= 128 ? 128 : 256; }
void plan_dw(long M, int N, int K, int& splitk, int& mper) {
  const int dtk = dw_tile(K);
  const int ntile = cdiv(N, DT) * cdiv(K, dtk);
  const int slabs = cdiv(M, KS);
  const int slots = dtk == 256 ? 256 : 512;
  // slices of a tile go to the XCDs round-robin (split & 7): a whole number of slices per XCD that fits its share of the
  // slots in ONE round (768 x 256: 6 tiles x 85 slices put 66 workgroups on XCDs 0-3 with 64 slots - a second round for 2)
  const int per_xcd = slots / 8 / ntile;
  int want = per_xcd >= 1 ? per_xcd * 8 : (ntile >= slots ? 1 : slots / ntile);
  if (want > slabs / 8) want = slabs / 8 > 0 ? slabs / 8 : 1;
  mper = cdiv(slabs, want) * KS;
  splitk = cdiv(M, mper);
}

int emu_dw_launch(const DwArgs& g, bool h2, float* dW, float* db, float* workspace, hipStream_t st) {
  const int dtk = dw_tile(g.K);
  const unsigned lb = 2u * (3 * 2 * DT + 3 * 2 * 128) * 16u;      // emu_dw_kernel<.., 128>: two stages of dynamic LDS
  static bool attr_set = false;
  if (!attr_set) {
    auto raise = [&](const void* k) { return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb) == hipSuccess; };
    const bool ok = raise(reinterpret_cast<const void*>(emu_dw_kernel<false, 128>)) && raise(reinterpret_cast<const void*>(emu_dw_kernel<true, 128>));
    if (!ok) {
      set_error("linear_bwd_weight_emu: cannot raise the dynamic LDS limit");
      return HOISDF_ERR_LAUNCH;
    }
    attr_set = true;
  }
  const dim3 grid((unsigned)(g.tiles_n * g.tiles_k * 8 * cdiv(g.splitk, 8))), block(NT);
  const bool mask = g.bits != nullptr, hasdb = g.colsum != nullptr;
  static void (*const dw2h[2][2])(DwArgs) = {{emu_dw2h_kernel<false, false>, emu_dw2h_kernel<false, true>},      // [MASK][HASDB]
                                             {emu_dw2h_kernel<true, false>, emu_dw2h_kernel<true, true>}};
  static void (*const dw2[2][2])(DwArgs) = {{emu_dw2_kernel<false, false>, emu_dw2_kernel<false, true>},
                                            {emu_dw2_kernel<true, false>, emu_dw2_kernel<true, true>}};
  if (dtk == 256) hipLaunchKernelGGL((h2 ? dw2h : dw2)[mask][hasdb], grid, block, 0, st, g);
  else hipLaunchKernelGGL((mask ? emu_dw_kernel<true, 128> : emu_dw_kernel<false, 128>), grid, block, lb, st, g);
  if (int rc = check_launch("linear_bwd_weight_emu")) return rc;
  if (g.splitk > 1) {
    const long n = (long)g.N * g.K;
    const int b0 = (int)((n + 255) / 256), b1 = db ? (g.N + 255) / 256 : 0;
    hipLaunchKernelGGL(emu_reduce_partials_kernel, dim3((unsigned)(b0 + b1)), dim3(1024), 0, st, workspace, n, g.splitk, dW, n, b0,
                       workspace + (size_t)g.splitk * g.N * g.K, (long)g.N, db, (long)g.N);
    return check_launch("linear_bwd_weight_emu reduce");
  }
  return HOISDF_OK;
}

}  // namespace hoisdf
