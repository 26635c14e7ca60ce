// fp32-EMULATED attention backward, f16x2 form: emu_attn_bwd4h_kernel = attention_emu_bwd4.inc (design, tiling, LDS layouts, shared
// units) with 76 instead of 120 MFMAs per query tile.  This file holds what only this form has:
//   * Q, K, V, dO: TWO f16 planes each (hi + lo of the values scaled by the power of two their magnitude words give;
//     emu_attn_convert_kernel<true>) - the planes the f16x2 forward keeps are the operands here;
//   * P = exp2(S / (sQ sK) - lse) is formed as 2^13 P (one fused multiply-add in front of the exponential) and split into two f16 pieces;
//   * dS = Pd dP - P delta is formed as dS sS with sS = sD sV 2^-23 - a scale that cannot overflow (|dP| <= 64 max|dO| max|V|, |delta|
//     likewise) but that a flat softmax undershoots by 20 binades - and therefore split into THREE f16 pieces (33 bits): the two
//     contractions that read it (dQ, dK) take five products per product, the other three (S, dP, dV) three;
//   * dK, dV leave scaled back; the dQ partials stay in accumulator units and emu_attn_dq_reduce_kernel applies 1 / (sK sS).
#include "attention_emu.h"

namespace hoisdf {
using namespace emu_attn;
namespace {
__device__ __forceinline__ uint32_t cvt2(f32x2 v) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2)); }     // v_cvt_pk_f16_f32
__device__ __forceinline__ f32x2 unpack2(uint32_t w) { return __builtin_convertvector(__builtin_bit_cast(f16x2, w), f32x2); }
}  // namespace
}  // namespace hoisdf

#define B4_NPL 2
#define B4_MFMA "v_mfma_f32_32x32x16_f16"
#define B4_KERNEL emu_attn_bwd4h_kernel
#define B4_LAUNCH attention_bwd4h_emu_launch
#define B4_WHO " (f16x2)"
#define B4_TAG "bwd4h"
#define B4_PHASE_INC "attn_bwd4h_phase.inc"
#define B4_ITER() BWD4H_ITER()
// ---- operand scales from the head magnitudes (common.h) of THIS (sample, head): sQ, sK, sV of the projected matrices, sD of dO's ----
#define B4_SCALES                                                                                                      \
  f16_saturate_on();                                                                                                   \
  const int hw_ = head * a.B + b;                                                                                      \
  const uint32_t aq_ = a.q_hm[hw_], ak_ = a.k_hm[hw_], av_ = a.v_hm[hw_], ad_ = a.d_hm[hw_];                           \
  const float iq = mag_inv_scale(aq_), ik = mag_inv_scale(ak_), iv = mag_inv_scale(av_), id = mag_inv_scale(ad_);      \
  const float cs = fmaxf(iq * ik, 0x1p-100f);                /* accumulated scores -> log2-domain scores */              \
  constexpr float PBIAS = 13.f;                              /* P is formed as 2^13 P */                                 \
  constexpr float K1 = 0x1p-36f;                             /* dS' = Pd' dP_acc 2^-36 - P' delta (sD sV 2^-36): dS sS with sS = sD sV 2^-23 */ \
  const float k2a = mag_scale(ad_) * 0x1p-18f, k2b = mag_scale(av_) * 0x1p-18f;      /* (two factors: sD sV alone can leave the f32 range) */ \
  const float dk_scale = (LN2 * 0x1p23f * id) * (iv * iq);   /* dK = dS'^T Q' ln 2 / (sS sQ) */                          \
  const float dv_scale = 0x1p-13f * id;                      /* dV = Pd'^T dO' / (2^13 sD) */                            \
  if (ktile == 0 && tid == 0 && a.dq_scale) a.dq_scale[bh] = (0.125f * 0x1p23f * id) * (ik * iv);      /* dQ = K'^T dS' / (8 sK sS), per (b, head) */
// (hy: the lane's half of the pair's sixteen hashes, see HA)
#define B4_FORM_STATE const bool kodd = (key & 1) != 0; bf16x8 ft[4][3]; uint32_t hy[8]; float dmine[8], dsend[8];
#define B4_HB_PAIR (kodd ? 16u * 0x85EBCA77U : 0u)           // (odd key: the pair's hashes of queries CR(8..15))
// Dropout decisions, one hash per KEY PAIR (common.h drop_hash: the low 16 bits decide the even key, the high ones the odd key): the two
// lanes of a key pair (lane, lane ^ 1) need the same sixteen hashes (one per query of the tile), so each computes EIGHT - the even lane
// those of queries CR(0..7), the odd lane those of CR(8..15): hb carries the 16-row offset -, decides them for itself and for its
// partner, and the partner's decisions travel through a DPP quad permute.  Units: HA / HB / HC over e = 4 q .. 4 q + 3 (q = 0, 1),
// HD puts the sixteen factors in their places.
#define HA(q_) do { if (DROP) { _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) { const int e_ = 4 * (q_) + i_; uint32_t x_ = hbn + (uint32_t)CRC(e_) * 0x85EBCA77U; x_ ^= x_ >> 15; hy[e_] = x_; PIN2(hy[e_]); } } } while (0)
#define HB(q_) do { if (DROP) { _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) { const int e_ = 4 * (q_) + i_; hy[e_] *= 0x2C1B3C6DU; PIN2(hy[e_]); } } } while (0)
#define HC(q_)                                                                                                         \
  do {                                                                                                                 \
    if (DROP) {                                                                                                        \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                               \
        const int e_ = 4 * (q_) + i_;                                                                                  \
        const uint32_t x_ = hy[e_] ^ (hy[e_] >> 12);                                                                   \
        dmine[e_] = (x_ << hsh) >= dthr ? a.inv_keep : 0.f;                                                            \
        dsend[e_] = (x_ << (hsh ^ 16)) >= dthr ? a.inv_keep : 0.f;                                                     \
        PIN2(dmine[e_]); PIN2(dsend[e_]);                                                                              \
      }                                                                                                                \
    }                                                                                                                  \
  } while (0)
#define HD(q_)                                                                                                         \
  do {                                                                                                                 \
    if (DROP) {                                                                                                        \
      _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                               \
        const int e_ = 4 * (q_) + i_;                                                                                  \
        const float got_ = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, dsend[e_]), 0xB1, 0xF, 0xF, true));   /* quad_perm [1, 0, 3, 2]: from lane ^ 1 */ \
        dsc[e_] = kodd ? got_ : dmine[e_];                                                                             \
        dsc[8 + e_] = kodd ? dmine[e_] : got_;                                                                         \
        PIN2(dsc[e_]); PIN2(dsc[8 + e_]);                                                                              \
      }                                                                                                                \
    }                                                                                                                  \
  } while (0)
#define B4_HASH_TILE0() do { HA(0); HA(1); HB(0); HB(1); HC(0); HC(1); HD(0); HD(1); } while (0)
#define LQ(g_) do { const f32x4 v_ = *reinterpret_cast<const f32x4*>(stats + st_cur + 8 * (g_) + 4 * h); lq[4 * (g_)] = PBIAS - v_.x; lq[4 * (g_) + 1] = PBIAS - v_.y; lq[4 * (g_) + 2] = PBIAS - v_.z; lq[4 * (g_) + 3] = PBIAS - v_.w; } while (0)     /* lq = 13 - lse: P is formed as 2^13 P */
#define DL(g_) do { const f32x4 v_ = *reinterpret_cast<const f32x4*>(stats + st_cur + 32 + 8 * (g_) + 4 * h); dl[4 * (g_)] = v_.x * k2a * k2b; dl[4 * (g_) + 1] = v_.y * k2a * k2b; dl[4 * (g_) + 2] = v_.z * k2a * k2b; dl[4 * (g_) + 3] = v_.w * k2a * k2b; } while (0)     /* delta in dS' units */
#define PA(q_)                                                                                                         \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                                 \
      const int m_ = 2 * (q_) + i_;                                                                                    \
      const float e0_ = __builtin_amdgcn_exp2f(__builtin_fmaf(s[2 * m_], cs, lq[2 * m_])), e1_ = __builtin_amdgcn_exp2f(__builtin_fmaf(s[2 * m_ + 1], cs, lq[2 * m_ + 1])); \
      pe[m_] = f32x2{e0_, e1_};                                                                                        \
      PIN2(pe[m_]);                                                                                                    \
    }                                                                                                                  \
  } while (0)
// (the second piece closes the split of Pd)
#define PD(q_)                                                                                                         \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                                 \
      const int m_ = 2 * (q_) + i_;                                                                                    \
      pwv[1][m_ >> 2][m_ & 3] = cvt2(xx[m_]);                                                                          \
      PIN2(pwv[1][m_ >> 2][m_ & 3]);                                                                                   \
    }                                                                                                                  \
  } while (0)
#define QA(q_)                                                                                                         \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                                 \
      const int m_ = 2 * (q_) + i_;                                                                                    \
      const f32x2 t_ = pe[m_] * f32x2{dl[2 * m_], dl[2 * m_ + 1]};                                                     \
      xx[m_] = pd[m_] * (f32x2{dp[2 * m_], dp[2 * m_ + 1]} * K1) - t_;                                                 \
      const uint32_t w_ = cvt2(xx[m_]);                                                                                \
      gwv[0][m_ >> 2][m_ & 3] = w_;                                                                                    \
      PIN2(gwv[0][m_ >> 2][m_ & 3]);                                                                                   \
    }                                                                                                                  \
  } while (0)
#include "attention_emu_bwd4.inc"
