// Shared declarations of the fp32-emulating linear kernels: gemm_emu_b3.hip (bf16x3 forward / grad-input), gemm_emu_h2.hip (f16x2
// forward / grad-input), gemm_emu_dw.hip (grad-weight, both forms), gemm_emu.hip (the C entries, the form switch, the magnitude passes);
// gemm_emu_small.hip takes its vector types from here.
#pragma once
#include "common.h"

namespace hoisdf {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
#define MFB(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)
#define MFH(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16((a), (b), (c), 0, 0, 0)

// bf16x3 forward / grad-input tile (gemm_emu_b3.hip)
constexpr int TM = 256, TN = 128, KS = 16, NT = 256;
constexpr int WN = TN / 2, NJ = WN / 32;
constexpr int A_U4 = 3 * 2 * TM, B_U4 = 3 * 2 * TN, STAGE_U4 = A_U4 + B_U4;
constexpr int NB = B_U4 / NT;
// f16x2 forward / grad-input tile (gemm_emu_h2.hip)
constexpr int HTM = 256, HTN = 256;
constexpr int HA_U4 = 2 * 2 * HTM, HB_U4 = 2 * 2 * HTN;      // 16-byte units of the activation stage / of one 256-row image block per slab
constexpr int H_TRAILER = 128;
constexpr int DT = 256;                                  // tile edge (both n and k)

// exact three-way split (native ext vectors only: arrays of HIP's uint4 / float4 structs end up in scratch)
#define SPLIT1(x, i)                             \
  do {                                           \
    const __bf16 a_ = (__bf16)(x);               \
    const float r1_ = (x) - (float)a_;           \
    const __bf16 b_ = (__bf16)r1_;               \
    const float r2_ = r1_ - (float)b_;           \
    p0[i] = a_; p1[i] = b_; p2[i] = (__bf16)r2_; \
  } while (0)
__device__ __forceinline__ void split3x8(const float4 u, const float4 w, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
  SPLIT1(u.x, 0); SPLIT1(u.y, 1); SPLIT1(u.z, 2); SPLIT1(u.w, 3);
  SPLIT1(w.x, 4); SPLIT1(w.y, 5); SPLIT1(w.z, 6); SPLIT1(w.w, 7);
}

struct EmuArgs {
  const float* A; long lda;                 // [M][lda] f32, k-contiguous
  const u32x4* Bimg;                        // slab image of the weight operand (rows = output columns)
  float* C; int ldc;
  const float* bias;
  const uint32_t* abits; int ldbits; float ascale;      // sign bitmap of A ([M][ceil(K / 32)]) and 1 / keep (grad-input)
  uint32_t* bits_out; int ldbits_out;
  int M, N, K;                              // output rows, output columns, contraction length
  int act; float drop_p, inv_keep; uint32_t thresh; uint64_t seed;
  int tiles_m, tiles_n, vecC, beta;
  QkvPlanes qkv;                            // .on: the output tile goes into attention planes instead of C (common.h)
  // f16x2 form: row magnitudes of A (common.h: one word per row, bits of max |A[row][:]| or an upper bound), the image's {scale, 1 / scale}
  const uint32_t* a_amax; const float* b_scale;
  uint32_t* amax_out;                       // row magnitudes of C (any form; zero on entry; null = not wanted)
  uint32_t* head_out; int head_L, head_nb;  // head magnitudes of C (common.h: word[(col / 64) * head_nb + row / head_L]; null = not wanted)
};

struct DwArgs {
  const float* dy; long lddy;
  const float* x; long ldx;
  const uint32_t* bits; int ldbits; float ascale;
  float* C; long c_split_stride;             // partial tiles [split][N][K] (or dW itself when splitk == 1)
  float* colsum; long colsum_split_stride;   // partial bias gradients [split][N] (or db), may be null
  int M, N, K;
  int splitk, m_per_split, tiles_n, tiles_k;
  const uint32_t* dy_amax; const uint32_t* x_amax;      // f16x2 form: row magnitudes (common.h) of dy and x, M words each
};

// (the power-of-two operand scale from the magnitude words and the 256-thread block maximum live in common.h: the attention kernels use them too)
__device__ __forceinline__ uint32_t h2_exp(uint32_t amax_bits) { return mag_exp(amax_bits); }
__device__ __forceinline__ float h2_scale(uint32_t amax_bits) { return mag_scale(amax_bits); }
__device__ __forceinline__ float h2_inv_scale(uint32_t amax_bits) { return mag_inv_scale(amax_bits); }
// the 128-byte trailer behind the last tile of an f16x2 weight image: 16 magnitude words, then {s, 1 / s} (gemm_emu_h2.hip)
__host__ __device__ __forceinline__ uint32_t* h2_trailer(void* image, int R, int Kc) {
  return reinterpret_cast<uint32_t*>(static_cast<char*>(image) + (size_t)((R + HTN - 1) / HTN) * ((Kc + KS - 1) / KS) * HB_U4 * 16);
}

// the batch weight-image builders of both forms: a block finds its item in the table by the items' first-block offsets (ascending);
// EMU_PREP_FIND declares `lo`, the item's index.  (A macro: as a device function it changed an instruction of both builders.)
#define EMU_PREP_FIND(items, n, lo)                                                                                    \
  int lo = 0, hi_ = (n) - 1;                                                                                           \
  while (lo < hi_) {                                                                                                   \
    const int mid_ = (lo + hi_ + 1) >> 1;                                                                              \
    if ((items)[mid_].first_block <= (long)blockIdx.x) lo = mid_; else hi_ = mid_ - 1;                                 \
  }

// ---- text the hand-pinned main loops share.  Macros, not functions: each kernel sees the tokens it would see with the text written
// in place, so its schedule does not depend on what the inliner makes of a call.  (SB() and PK_SUB: common.h.)
#define NOP_ ((void)0)
#define SYNC() do { SB(); __syncthreads(); SB(); } while (0)

// Activation staging of emu_kc2_kernel and emu_h2_kernel (tile TM_ rows; MASK, KTAIL, g, m0, wave, wm, lane, l31, kh, last from the kernel).
// Roles: item i (0..3) of a thread = row i * 64 + wave * 16 + lane / 4 of the tile (rl), quad qd = lane % 4 of the slab (k = 4 qd ..
// 4 qd + 3; chunk cq = qd / 2, half qd % 2 of the chunk's 16 bytes).  Rows past M read as zero (their products only reach rows that are
// never stored).
// EMU_A_DESCRIPTORS: buffer descriptors (wave-uniform) over the tile's row panel (first row arow0) and its sign-bitmap rows: the
// loads are buffer_load (32-bit per-lane offset in ONE register + scalar slab offset) - with flat addressing hipcc keeps a
// 64-bit address pair per item alive across the loop and spills
// (four descriptors each, one per item = 64-row quarter of the tile: the per-lane offset is the SAME register for all four,
// and rows past M read as zero through the quarter's record count - no clamping, no per-item offset registers)
#define EMU_A_DESCRIPTORS(TM_, arow0)                                                                                  \
  const int rows_in = min(TM_, g.M - m0);                                                                              \
  __amdgpu_buffer_rsrc_t rsa[4], rsm[4];                                                                               \
  _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                                      \
    const int rows_q = max(min(rows_in - i * 64, 64), 0);     /* valid rows of this quarter */                         \
    rsa[i] = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(g.A + ((size_t)(arow0) + i * 64) * g.lda), 0,        \
                                               rows_q > 0 ? (int)((((long)rows_q - 1) * g.lda + g.K) * 4) : 0, 0x00020000); \
    rsm[i] = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(MASK ? g.abits + ((size_t)m0 + i * 64) * g.ldbits : nullptr), 0, \
                                               MASK ? (int)((long)rows_q * g.ldbits * 4) : 0, 0x00020000);             \
  }
// EMU_A_SLOTS: per-lane load offsets; wslot = the 8-byte LDS slot of item 0, plane 0: unit (chunk cq, row ^ (cq << 2)), half qd & 1; item
// i adds 128 slots, plane p 2 * 2 * TM_.  ds_write_b64 is served in contiguous 16-lane groups over 32 banks (128 bytes): a group = 4 rows
// x 4 quads; flipping bit 2 of the row for the second chunk puts its 4 rows x 16 bytes into the other half of the bank row (PMC:
// SQ_LDS_BANK_CONFLICT back at the first form's level; with bit 3 flipped the two chunks collided, + 25 % LDS cycles).  aread: fragment
// rows follow the same row flip (chunk = kh).  kq: the quad is valid in slab sl iff sl * 16 < kq.
#define EMU_A_SLOTS(TM_)                                                                                               \
  const int aoff = (int)((((long)wave * 16 + rl) * g.lda + 4 * qd) * 4);                                               \
  const int moff = (int)(((long)wave * 16 + rl) * g.ldbits * 4);                                                       \
  const int wslot = 2 * (cq * TM_ + ((wave * 16 + rl) ^ (cq << 2))) + (qd & 1);                                        \
  const int aread = (wm * 128 + l31) ^ (kh << 2);                                                                      \
  const int kq = g.K - 4 * qd;
// EMU_LDGA(i, sl): the quad of item i in slab sl -> rp[2 i], rp[2 i + 1] (+ its sign-bitmap word)
#define EMU_LDGA(i, sl)                                                                                                \
  do {                                                                                                                 \
    const int k0_ = min((sl), last) * KS;                      /* (uniform) a pad slab re-reads the last one */        \
    const f32x4 v_ = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsa[i], aoff, k0_ * 4, 0));       \
    rp[2 * (i)] = f32x2{v_[0], v_[1]}; rp[2 * (i) + 1] = f32x2{v_[2], v_[3]};                                          \
    if (MASK) rm[i] = __builtin_amdgcn_raw_buffer_load_b32(rsm[i], moff, (k0_ >> 5) * 4, 0);                           \
  } while (0)
// EMU_UI(i, sl): per-item scalars of slab sl (the quad's four sign bits; is the quad inside K)
#define EMU_UI(i, sl) do { if (MASK) mb = rm[i] >> ((((sl) & 1) << 4) + 4 * qd); if (KTAIL) kin = (sl) * KS < kq; } while (0)
// EMU_MASK_KTAIL(v_, p): sign bitmap (the 1 / keep factor is applied once, in the epilogue) and k tail on pair p = 2 i + j (item i,
// half j of its quad)
#define EMU_MASK_KTAIL(v_, p)                                                                                          \
  do {                                                                                                                 \
    if (MASK) {           /* bit -> all-ones / zero word (v_bfe_i32) -> v_and: written as asm, hipcc (ROCm 7.2) turns the plain   */ \
      float xa_, xb_;     /* expression into compare + select, and MISCOMPILES the two-element form (the y lane reads x)        */ \
      asm("v_and_b32 %0, %1, %2" : "=v"(xa_) : "v"(__builtin_amdgcn_sbfe((int)mb, 2 * ((p) & 1), 1)), "v"(v_.x));       \
      asm("v_and_b32 %0, %1, %2" : "=v"(xb_) : "v"(__builtin_amdgcn_sbfe((int)mb, 2 * ((p) & 1) + 1, 1)), "v"(v_.y));   \
      v_ = f32x2{xa_, xb_};                                                                                            \
    }                                                                                                                  \
    if (KTAIL) { if (!kin) v_ = f32x2{0.f, 0.f}; }             /* K is a multiple of 4: a quad is all in or all out */ \
  } while (0)

// C-tile epilogue shared by all main-loop forms (tile TM_ x TN_, 2 x 2 waves, wave tile 128 x 32 NJ_): bias, ReLU, dropout, 1-bit
// sign map, accumulate-into, LDS-transposed 16-byte stores
template <int TM_, int TN_, int NJ_>
__device__ __forceinline__ void emu_epilogue(const EmuArgs& g, f32x16 (&acc)[4][NJ_], u32x4* lds, int m0, int n0, int wm, int wn, int wave,
                                             int lane, int l31, int kh, float post_scale, const float* row_post = nullptr) {
  constexpr int WN_ = TN_ / 2;
  static_assert(WN_ == NJ_ * 32, "wave tile");
  if (row_post) {                              // (f16x2) one factor per output ROW: the row's operand scale, the weight's, 1 / keep - from LDS
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const f32x4 ps = *reinterpret_cast<const f32x4*>(row_post + wm * 128 + i * 32 + 8 * q + 4 * kh);
#pragma unroll
        for (int j = 0; j < NJ_; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][4 * q + e] *= ps[e];
      }
  } else if (post_scale != 1.f) {                     // (grad-input, rotated form) 1 / keep of the forward's dropout, once per element; (f16x2) the operand scales
#pragma unroll
    for (int j = 0; j < NJ_; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][j][r] *= post_scale;
  }
  // ---- epilogue (C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)); all waves are
  // past the main loop's last barrier, the staging buffer is free
  const int rbase = m0 + wm * 128 + 4 * kh;
  const int cbase = n0 + wn * WN_ + l31;
#pragma unroll
  for (int j = 0; j < NJ_; ++j) {
    const int col = cbase + j * 32;
    const float bv = (g.bias != nullptr && col < g.N) ? g.bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[i][j][r] + bv;
        if (g.act == 1) v = fmaxf(v, 0.f);
        acc[i][j][r] = v;
      }
  }
  if (g.drop_p > 0.f) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = rbase + i * 32 + (r & 3) + 8 * (r >> 2);
        const uint32_t rk = drop_rowkey(g.seed, (uint32_t)row);
#pragma unroll
        for (int j = 0; j < NJ_; ++j) acc[i][j][r] *= drop_scale(rk, (uint32_t)(cbase + j * 32), g.thresh, g.inv_keep);
      }
  }
  if (g.head_out) {
    // head magnitudes (common.h): each 64-column group of the wave's 128-row sub-tile -> the word(s) of the sample(s) its rows belong to
    // (exact only when a sub-tile is one sample's: the host sets head_out when head_L % 128 == 0 and M % 128 == 0 and measures the stored
    // matrix otherwise - gemm_emu.hip heads_fold_exact(); a sub-tile of several samples would give each of them the maximum of all)
    const int row0 = m0 + wm * 128;
    if (row0 < g.M) {
      const int b0 = row0 / g.head_L, b1 = (min(row0 + 127, g.M - 1)) / g.head_L;
#pragma unroll
      for (int hh = 0; hh < NJ_ / 2; ++hh) {
        float m = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) m = fmaxf(m, __builtin_fabsf(acc[i][2 * hh + j][r]));
        uint32_t mb = group_max_u32<64>(__builtin_bit_cast(uint32_t, m));
        const int grp = (n0 + wn * WN_ + hh * 64) >> 6;
        if (lane == 0 && n0 + wn * WN_ + hh * 64 < g.N)
          for (int b = b0; b <= b1; ++b) atomicMax(g.head_out + (size_t)grp * g.head_nb + b, mb);
      }
    }
  }
  if (g.qkv.on) {
    // attention-plane output (common.h QkvPlanes): every 128 x 64 part of the wave's sub-tile is 128 consecutive tokens of one sample x
    // one head of one part; per 32-row block through the wave-private LDS slice: row planes as 8 lanes x 16 bytes per token and piece,
    // transposed value planes as one d per lane, 8 consecutive tokens (16 bytes) per store
    constexpr int ES = 64 + 4;
    float* w = reinterpret_cast<float*>(lds) + wave * (32 * ES);
    const int row0 = m0 + wm * 128, cw = n0 + wn * WN_;
    if (row0 + 128 > g.M || cw + WN_ > g.N) return;           // (never: the launcher takes whole wave tiles only)
    const int b = row0 / g.qkv.L, s0 = row0 - b * g.qkv.L;
#pragma unroll
    for (int hh = 0; hh < NJ_ / 2; ++hh) {
      const int colg = g.qkv.col0 + cw + hh * 64;
      const int part = colg / g.qkv.E, head = (colg - part * g.qkv.E) >> 6;
      const size_t bh = (size_t)b * g.qkv.H + head;
      const float sc = part == 0 ? g.qkv.qscale : 1.f;
      __bf16* const r0 = static_cast<__bf16*>(g.qkv.r[part][0]);
      __bf16* const r1 = static_cast<__bf16*>(g.qkv.r[part][1]);
      __bf16* const r2 = static_cast<__bf16*>(g.qkv.r[part][2]);
      const bool trn = part == 2 && g.qkv.vt[0] != nullptr;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) w[((r & 3) + 8 * (r >> 2) + 4 * kh) * ES + j * 32 + l31] = acc[i][2 * hh + j][r] * sc;
        if (r0) {
#pragma unroll
          for (int p = 0; p < 4; ++p) {
            const int rr = p * 8 + (lane >> 3), cc = (lane & 7) * 8;
            const float4 u = *reinterpret_cast<const float4*>(w + rr * ES + cc);
            const float4 v = *reinterpret_cast<const float4*>(w + rr * ES + cc + 4);
            bf16x8 p0, p1, p2;
            split3x8(u, v, p0, p1, p2);
            const size_t o = ((size_t)bh * g.qkv.Lp + s0 + i * 32 + rr) * 64 + cc;
            *reinterpret_cast<bf16x8*>(r0 + o) = p0;
            *reinterpret_cast<bf16x8*>(r1 + o) = p1;
            *reinterpret_cast<bf16x8*>(r2 + o) = p2;
          }
        }
        if (trn) {
          __bf16* const t0 = static_cast<__bf16*>(g.qkv.vt[0]);
          __bf16* const t1 = static_cast<__bf16*>(g.qkv.vt[1]);
          __bf16* const t2 = static_cast<__bf16*>(g.qkv.vt[2]);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float* c0 = w + (8 * q) * ES + lane;
            const float4 u = make_float4(c0[0], c0[ES], c0[2 * ES], c0[3 * ES]);
            const float4 v = make_float4(c0[4 * ES], c0[5 * ES], c0[6 * ES], c0[7 * ES]);
            bf16x8 p0, p1, p2;
            split3x8(u, v, p0, p1, p2);
            const size_t o = ((size_t)bh * 64 + lane) * g.qkv.Lp + s0 + i * 32 + 8 * q;
            *reinterpret_cast<bf16x8*>(t0 + o) = p0;
            *reinterpret_cast<bf16x8*>(t1 + o) = p1;
            *reinterpret_cast<bf16x8*>(t2 + o) = p2;
          }
        }
      }
    }
    return;
  }
  const bool full = (m0 + TM_ <= g.M) && (n0 + TN_ <= g.N);
  const bool stream_c = !g.beta && (long)g.M * g.N >= (16L << 20);
  if (full && g.vecC) {
    // one row of blocks (32 x WN_) per wave at a time through a wave-private LDS slice, read back row-wise: one
    // global_store_dwordx4 covers complete 256-byte row segments
    constexpr int ES = WN_ + 4, LPR = WN_ / 4, RPI = 64 / LPR;
    float* w = reinterpret_cast<float*>(lds) + wave * (32 * ES);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int j = 0; j < NJ_; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) w[((r & 3) + 8 * (r >> 2) + 4 * kh) * ES + j * 32 + l31] = acc[i][j][r];
      if (g.amax_out) {
        // row magnitudes of C (common.h): lane l folds the (l >> 5) half of row l & 31 of the 32-row block parked in its wave's LDS slice
        // (WN_ / 8 16-byte reads + as many v_max3 with |.| operands), the two halves meet through one exchange, lanes 0-31 publish
        // (the first form - 4 DPP steps per stored 16-byte piece - cost 700 issue slots per wave tile, this one ~120)
        const float* rp = w + l31 * ES + kh * (WN_ / 2);
        float m = 0.f;
#pragma unroll
        for (int q = 0; q < WN_ / 8; ++q) {
          const float4 t = *reinterpret_cast<const float4*>(rp + 4 * q);
          m = __builtin_fmaxf(__builtin_fmaxf(m, __builtin_fabsf(t.x)), __builtin_fmaxf(__builtin_fabsf(t.y), __builtin_fmaxf(__builtin_fabsf(t.z), __builtin_fabsf(t.w))));
        }
        uint32_t mb = __builtin_bit_cast(uint32_t, m);
        mb = max(mb, (uint32_t)__shfl_xor((int)mb, 32, 64));
        if (kh == 0) atomicMax(g.amax_out + (m0 + wm * 128 + i * 32 + l31), mb);
      }
#pragma unroll
      for (int p = 0; p < 32 / RPI; ++p) {
        const int rr = p * RPI + lane / LPR, cc = (lane % LPR) * 4;
        float4 v = *reinterpret_cast<const float4*>(w + rr * ES + cc);
        float4* cp = reinterpret_cast<float4*>(g.C + (size_t)(m0 + wm * 128 + i * 32 + rr) * g.ldc + n0 + wn * WN_ + cc);
        if (g.beta) {
          const float4 old = *cp;
          v.x += old.x; v.y += old.y; v.z += old.z; v.w += old.w;
        }
        // an output too large to stay in the L2s (>= 64 MB) is streamed past them: -0.12 ms per train step, two same-box pairs
        typedef float v4f_ __attribute__((ext_vector_type(4)));
#ifdef H2_ABL_NOSTORE                 /* (tools/ablate_h2.sh: how much of the kernel is the output's way to HBM?  never true at run time) */
        if (g.seed != 0x5eed5eed5eedull) continue;
#endif
        if (stream_c) __builtin_nontemporal_store(v4f_{v.x, v.y, v.z, v.w}, reinterpret_cast<v4f_*>(cp));
        else *cp = v;
      }
    }
  } else {
#pragma unroll
    for (int j = 0; j < NJ_; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rbase + i * 32 + (r & 3) + 8 * (r >> 2), col = cbase + j * 32;
          if (row < g.M && col < g.N) {
            float* cp = g.C + (size_t)row * g.ldc + col;
            *cp = g.beta ? *cp + acc[i][j][r] : acc[i][j][r];
          }
        }
    if (g.amax_out) {                         // (edge tiles / unaligned C: per row over the 32 lanes that hold its columns)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = rbase + i * 32 + (r & 3) + 8 * (r >> 2);
          uint32_t mb = 0u;
#pragma unroll
          for (int j = 0; j < NJ_; ++j) if (cbase + j * 32 < g.N) mb = max(mb, mag_bits(acc[i][j][r]));
          mb = group_max_u32<32>(mb);
          if (l31 == 0 && row < g.M) atomicMax(g.amax_out + row, mb);
        }
    }
  }
  if (g.bits_out) {
    // lanes 0-31 hold 32 consecutive columns of one row, lanes 32-63 of the row 4 below: one ballot is two mask words.
    // Each lane collects the words of "its" rows (lane and lane + 64 of the wave's 128-row sub-tile) and writes them once.
    uint32_t wd[2][NJ_];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int j = 0; j < NJ_; ++j) wd[hh][j] = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int rl = (i & 1) * 32 + (r & 3) + 8 * (r >> 2);      // row within a 64-row half, as held by lanes 0-31
#pragma unroll
        for (int j = 0; j < NJ_; ++j) {
          const unsigned long long q = __ballot(acc[i][j][r] > 0.f);
          if (lane == rl) wd[i >> 1][j] = (uint32_t)q;
          if (lane == rl + 4) wd[i >> 1][j] = (uint32_t)(q >> 32);
        }
      }
    const int wcol = (n0 + wn * WN_) >> 5;
    const int nvalid = g.N - (n0 + wn * WN_);
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int row = m0 + wm * 128 + hh * 64 + lane;
      if (row < g.M) {
#pragma unroll
        for (int j = 0; j < NJ_; ++j) {
          const int nv = nvalid - 32 * j;
          if (nv > 0) g.bits_out[(size_t)row * g.ldbits_out + wcol + j] = nv >= 32 ? wd[hh][j] : (wd[hh][j] & ((1u << nv) - 1u));
        }
      }
    }
  }
}

// ---- per-family launchers (each returns a HOISDF status).  gemm_emu_b3.hip: weight image(s) of the bf16x3 form (R image rows over
// a contraction of Kc), the forward / grad-input kernel for a filled EmuArgs (tiles_m / tiles_n are set there)
int emu_b3_prepare(const float* W, int ldw, int R, int Kc, int transpose, void* image, hipStream_t st);
int emu_b3_prepare_batch(const hoisdf_emu_prep_item* d_items, int n, long total_blocks, hipStream_t st);
int emu_b3_launch(EmuArgs g, hipStream_t st);
// gemm_emu_h2.hip: the same for the f16x2 form (g.a_amax is set by the caller; tile width, tiles and g.b_scale are set there)
int emu_h2_prepare(const float* W, int ldw, int N, int K, int transpose, void* image, hipStream_t st);
int emu_h2_prepare_batch(const hoisdf_emu_prep_item* d_items, int n, long total_blocks, hipStream_t st);
int emu_h2_launch(EmuArgs g, hipStream_t st);
// gemm_emu_dw.hip: k-tile width and row slices of a grad-weight problem; the kernel for a filled DwArgs (h2: the f16x2 form where the
// tile is 256 wide, g.dy_amax / g.x_amax set) + the ordered reduce of the partial tiles in `workspace` into dW / db
int dw_tile(int K);
void plan_dw(long M, int N, int K, int& splitk, int& mper);
int emu_dw_launch(const DwArgs& g, bool h2, float* dW, float* db, float* workspace, hipStream_t st);
}  // namespace hoisdf
