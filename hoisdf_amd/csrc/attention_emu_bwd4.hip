// fp32-EMULATED attention backward, bf16x3 form: emu_attn_bwd4_kernel = attention_emu_bwd4.inc (design, tiling, LDS layouts, shared
// units) with THREE bf16 planes per operand - exact splits of the f32 values, no scaling - and six products per product: 120 MFMAs per
// query tile.  This file holds what only this form has.
#include "attention_emu.h"

namespace hoisdf {
using namespace emu_attn;
namespace {
__device__ __forceinline__ uint32_t cvt2(f32x2 v) { return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2)); }
__device__ __forceinline__ f32x2 unpack2(uint32_t w) { return f32x2{__builtin_bit_cast(float, w << 16), __builtin_bit_cast(float, w & 0xffff0000u)}; }
}  // namespace
}  // namespace hoisdf

#define B4_NPL 3
#define B4_MFMA "v_mfma_f32_32x32x16_bf16"
#define B4_KERNEL emu_attn_bwd4_kernel
#define B4_LAUNCH attention_bwd4_emu_launch
#define B4_WHO ""
#define B4_TAG "bwd4"
#define B4_PHASE_INC "attn_bwd4_phase.inc"
#define B4_ITER() BWD4_ITER()
#define B4_SCALES constexpr float dk_scale = LN2, dv_scale = 1.f;      // no operand scales
#define B4_FORM_STATE bf16x8 fq0[4]; uint32_t hx[16];
#define B4_HB_PAIR 0u
// Dropout decisions: one hash per element (common.h drop_hash of the key PAIR; the lane's key takes its half through hsh)
#define HA(q_) do { if (DROP) { _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) { const int r_ = 4 * (q_) + i_; uint32_t x_ = hbn + (uint32_t)CRC(r_) * 0x85EBCA77U; x_ ^= x_ >> 15; hx[r_] = x_; PIN2(hx[r_]); } } } while (0)
#define HB(q_) do { if (DROP) { _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) { const int r_ = 4 * (q_) + i_; hx[r_] *= 0x2C1B3C6DU; PIN2(hx[r_]); } } } while (0)
#define HC(q_) do { if (DROP) { _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) { const int r_ = 4 * (q_) + i_; const uint32_t x_ = hx[r_] ^ (hx[r_] >> 12); dsc[r_] = (x_ << hsh) >= dthr ? a.inv_keep : 0.f; PIN2(dsc[r_]); } } } while (0)
#define B4_HASH_TILE0() do { HA(0); HA(1); HA(2); HA(3); HB(0); HB(1); HB(2); HB(3); HC(0); HC(1); HC(2); HC(3); } while (0)
#define LQ(g_) do { const f32x4 v_ = *reinterpret_cast<const f32x4*>(stats + st_cur + 8 * (g_) + 4 * h); lq[4 * (g_)] = v_.x; lq[4 * (g_) + 1] = v_.y; lq[4 * (g_) + 2] = v_.z; lq[4 * (g_) + 3] = v_.w; } while (0)
#define DL(g_) do { const f32x4 v_ = *reinterpret_cast<const f32x4*>(stats + st_cur + 32 + 8 * (g_) + 4 * h); dl[4 * (g_)] = v_.x; dl[4 * (g_) + 1] = v_.y; dl[4 * (g_) + 2] = v_.z; dl[4 * (g_) + 3] = v_.w; } while (0)
#define PA(q_)                                                                                                         \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                                 \
      const int m_ = 2 * (q_) + i_;                                                                                    \
      const float e0_ = __builtin_amdgcn_exp2f(s[2 * m_] - lq[2 * m_]), e1_ = __builtin_amdgcn_exp2f(s[2 * m_ + 1] - lq[2 * m_ + 1]); \
      pe[m_] = f32x2{e0_, e1_};                                                                                        \
      PIN2(pe[m_]);                                                                                                    \
    }                                                                                                                  \
  } while (0)
// (second and third piece of Pd)
#define PD(q_)                                                                                                         \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                                 \
      const int m_ = 2 * (q_) + i_;                                                                                    \
      const uint32_t w_ = cvt2(xx[m_]);                                                                                \
      pwv[1][m_ >> 2][m_ & 3] = w_;                                                                                    \
      ff[m_] = unpack2(w_);                                                                                            \
      PIN2(ff[m_]);                                                                                                    \
    }                                                                                                                  \
  } while (0)
#define PE(q_)                                                                                                         \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                                 \
      const int m_ = 2 * (q_) + i_;                                                                                    \
      pwv[2][m_ >> 2][m_ & 3] = cvt2(xx[m_] - ff[m_]);                                                                 \
      PIN2(pwv[2][m_ >> 2][m_ & 3]);                                                                                   \
    }                                                                                                                  \
  } while (0)
#define QA(q_)                                                                                                         \
  do {                                                                                                                 \
    _Pragma("unroll") for (int i_ = 0; i_ < 2; ++i_) {                                                                 \
      const int m_ = 2 * (q_) + i_;                                                                                    \
      const f32x2 t_ = pe[m_] * f32x2{dl[2 * m_], dl[2 * m_ + 1]};                                                     \
      xx[m_] = pd[m_] * f32x2{dp[2 * m_], dp[2 * m_ + 1]} - t_;                                                        \
      const uint32_t w_ = cvt2(xx[m_]);                                                                                \
      gwv[0][m_ >> 2][m_ & 3] = w_;                                                                                    \
      PIN2(gwv[0][m_ >> 2][m_ & 3]);                                                                                   \
    }                                                                                                                  \
  } while (0)
#include "attention_emu_bwd4.inc"
