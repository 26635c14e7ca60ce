// fp32-EMULATED attention backward, f16x2 form with TWO dS pieces: emu_attn_bwd4g_kernel = attention_emu_bwd4.inc (design, tiling, LDS
// layouts, shared units) with 60 instead of 76 MFMAs per query tile.  It is attention_emu_bwd4h.hip (read that first: the operand
// planes, 2^13 P, the dropout units) except for the scale of dS:
//   * dS = Pd dP - P delta is formed as dS sS with a power of two sS that follows the DATA of the (sample, head): from
//         |dS_ij| <= inv_keep ||dO_i||_2 ||v_j||_2 + |delta_i| <= inv_keep max_i ||dO_i||_2 8 max|V| + max_i |delta_i| =: Bd
//     (Cauchy-Schwarz on dP_ij = dO_i . v_j with d = 64, P <= 1, Pd <= inv_keep P) sS is the largest power of two with
//     sS Bd (1 + 2^-10) < 2^14.  max_i ||dO_i||_2 and max_i |delta_i| are the two bound words emu_attn_delta_bound_kernel leaves behind
//     dq_scale; max|V| is the head magnitude word.  The fixed scale of the three-piece unit (sD sV 2^-23: |dP| <= 64 max|dO| max|V|) sits
//     about six binades lower for flat softmaxes; here two f16 pieces (22 bits, like Q, K, V and dO) have the lower absolute floor;
//   * so dS has TWO pieces (B4_DSPL): dQ and dK take three products per product like S, dP and dV; the dS^T exchange tile has two planes;
//   * dK leaves scaled by 1 / (sS sQ), the dQ partials stay in accumulator units and emu_attn_dq_reduce_kernel applies 1 / (8 sK sS).
// f16_saturate_on() stays: were the bound ever missed, a piece clips at +-65504 (4 x head room) and never becomes Inf.
#include "attention_emu.h"

namespace hoisdf {
using namespace emu_attn;
namespace {
__device__ __forceinline__ uint32_t cvt2(f32x2 v) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, f16x2)); }     // v_cvt_pk_f16_f32
__device__ __forceinline__ f32x2 unpack2(uint32_t w) { return __builtin_convertvector(__builtin_bit_cast(f16x2, w), f32x2); }
}  // namespace
}  // namespace hoisdf

#define B4_NPL 2
#define B4_DSPL 2
#define B4_MFMA "v_mfma_f32_32x32x16_f16"
#define B4_KERNEL emu_attn_bwd4g_kernel
#define B4_LAUNCH attention_bwd4g_emu_launch
#define B4_WHO " (f16x2, two dS pieces)"
#define B4_TAG "bwd4g"
#define B4_PHASE_INC "attn_bwd4g_phase.inc"
#define B4_ITER() BWD4G_ITER()
// ---- operand scales from the head magnitudes (common.h) of THIS (sample, head): sQ, sK, sV of the projected matrices, sD of dO's; the
// dS scale from the bound words.  Everything below is a power of two made from exponent sums or a product of normalised factors:
//   n' = max||dO_i|| sD in [2^13, 2^17), v' = max|V| sV in [2^13, 2^14), d' = max|delta| sD sV <= 2^36 (two factors of 2^-18 on the way,
//   as for delta itself: sD sV alone can leave the f32 range), Bd' = Bd sD sV = inv_keep n' 8 v' + d' in [2^29, 2^38)
//   (floored at 2^29: all-zero / denormal dO, whose magnitude word clamps), e = the biased exponent of Bd' (1 + 2^-10): sS = sS' sD sV with
//   sS' = 2^(140 - e), i.e. sS Bd (1 + 2^-10) < 2^14 (the margin covers the rounding of the emulated dP, of the norm and of this sum)
#define B4_SCALES                                                                                                      \
  f16_saturate_on();                                                                                                   \
  const int hw_ = head * a.B + b;                                                                                      \
  const uint32_t aq_ = a.q_hm[hw_], ak_ = a.k_hm[hw_], av_ = a.v_hm[hw_], ad_ = a.d_hm[hw_];                           \
  const float iq = mag_inv_scale(aq_), ik = mag_inv_scale(ak_), iv = mag_inv_scale(av_), id = mag_inv_scale(ad_);      \
  const float cs = fmaxf(iq * ik, 0x1p-100f);                /* accumulated scores -> log2-domain scores */              \
  constexpr float PBIAS = 13.f;                              /* P is formed as 2^13 P */                                 \
  const float k2a = mag_scale(ad_) * 0x1p-18f, k2b = mag_scale(av_) * 0x1p-18f;                                        \
  const uint32_t* const bw_ = reinterpret_cast<const uint32_t*>(a.dq_scale + a.B * a.H) + 2 * bh;      /* the bound words of (b, head) */ \
  const float nd_ = __builtin_bit_cast(float, bw_[0]) * mag_scale(ad_), vm_ = __builtin_bit_cast(float, av_) * mag_scale(av_);     \
  const float dm_ = __builtin_bit_cast(float, bw_[1]) * k2a * k2b * 0x1p36f;                                           \
  const float bd_ = fminf(fmaxf((a.inv_keep * nd_ * 8.f * vm_ + dm_) * (1.f + 0x1p-10f), 0x1p29f), 0x1p60f);           \
  const uint32_t es_ = (__builtin_bit_cast(uint32_t, bd_) >> 23) & 0xffu;                                              \
  const float k1 = __builtin_bit_cast(float, (254u - es_) << 23);      /* sS' 2^-13: dS' = Pd' dP_acc k1 - P' delta (sD sV k1) */ \
  const float k2c = k2b * (k1 * 0x1p36f);                    /* (delta k2a) k2c = delta sD sV k1; exact as a denormal too (max|V| >= 2^121) */ \
  const float is_ = __builtin_bit_cast(float, (es_ - 13u) << 23);      /* 1 / sS' */                                    \
  const float dk_scale = (LN2 * is_ * id) * (iv * iq);       /* dK = dS'^T Q' ln 2 / (sS sQ) */                          \
  const float dv_scale = 0x1p-13f * id;                      /* dV = Pd'^T dO' / (2^13 sD) */                            \
  if (ktile == 0 && tid == 0 && a.dq_scale) a.dq_scale[bh] = (0.125f * is_ * id) * (ik * iv);      /* dQ = K'^T dS' / (8 sK sS), per (b, head) */
// (hy: the lane's half of the pair's sixteen hashes, see HA)
#define B4_FORM_STATE const bool kodd = (key & 1) != 0; bf16x8 ft[4][2]; uint32_t hy[8]; float dmine[8], dsend[8];
#define B4_HB_PAIR (kodd ? 16u * 0x85EBCA77U : 0u)           // (odd key: the pair's hashes of queries CR(8..15))
// Dropout decisions, one hash per KEY PAIR: the units of attention_emu_bwd4h.hip (the even lane of a key pair computes the hashes of
// queries CR(0..7), the odd lane those of CR(8..15), and each decides for itself and for its partner)
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
#define DL(g_) do { const f32x4 v_ = *reinterpret_cast<const f32x4*>(stats + st_cur + 32 + 8 * (g_) + 4 * h); dl[4 * (g_)] = v_.x * k2a * k2c; dl[4 * (g_) + 1] = v_.y * k2a * k2c; dl[4 * (g_) + 2] = v_.z * k2a * k2c; dl[4 * (g_) + 3] = v_.w * k2a * k2c; } while (0)     /* delta in dS' units */
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
      xx[m_] = pd[m_] * (f32x2{dp[2 * m_], dp[2 * m_ + 1]} * k1) - t_;                                                 \
      const uint32_t w_ = cvt2(xx[m_]);                                                                                \
      gwv[0][m_ >> 2][m_ & 3] = w_;                                                                                    \
      PIN2(gwv[0][m_ >> 2][m_ & 3]);                                                                                   \
    }                                                                                                                  \
  } while (0)
// (the second piece closes the split of dS; QB of the shared text leaves the remainder in xx)
#define QE(q_)                                                                                                         \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                                 \
      const int m_ = 2 * (q_) + i_;                                                                                    \
      gwv[1][m_ >> 2][m_ & 3] = cvt2(xx[m_]);                                                                          \
      PIN2(gwv[1][m_ >> 2][m_ & 3]);                                                                                   \
    }                                                                                                                  \
  } while (0)
#include "attention_emu_bwd4.inc"
