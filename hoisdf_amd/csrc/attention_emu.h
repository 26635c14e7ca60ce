// Shared declarations of the fp32-emulating attention kernels (attention_emu.hip: conversion pre-pass, forward, the backward's delta and
// dQ reduce passes; attention_emu_bwd4.inc: the one-pass backward, compiled as attention_emu_bwd4.hip in the bf16x3 form and as
// attention_emu_bwd4h.hip in the f16x2 form).
#pragma once
#include "common.h"

namespace hoisdf {
namespace emu_attn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int D = 64;                                  // head width
constexpr float LN2 = 0.6931471805599453f;

struct EmuAttn {
  // planes (any may be null when a kernel does not use it): [p] = piece 0, 1, 2
  const __bf16 *q[3];              // Q rows (pre-scaled)
  const __bf16 *k[3];              // K rows
  const __bf16 *v[3], *vt[3];      // V rows (backward), V^T (forward)
  const __bf16 *d[3];              // dO rows
  const float* lse_in; const float* delta;
  float* out; float* lse; float* dq_part; float* dk; float* dv;
  int ldo, ldk, ldv;
  int B, H, Lq, Lk, Lqp, Lkp, kv_len;
  float drop_p, inv_keep;
  uint32_t thresh;
  uint64_t seed;
  // f16x2 form: head magnitudes (common.h) the planes of Q, K, V and dO were made with - ONE scale per (sample, head) and operand:
  // word of (b, head) at x_hm[head * B + b] (each pointer is positioned at its operand's first head inside its matrix' array)
  const uint32_t *q_hm, *k_hm, *v_hm, *d_hm;
  float* dq_scale;                 // f16x2 backward: one float per (b, head) the kernel leaves for the dQ reduce pass (0.125 / (sK sS))
  uint32_t* mag;                   // row magnitudes (common.h) of what the kernel writes: out (forward), [dq | dk | dv] rows (backward); null = none
};

__device__ __forceinline__ bool emu_block(int nx, int nbh, int& tile, int& bh) {
  const int L = blockIdx.x, slot = L >> 3;        // every tile of a (b, head) on one XCD, as in attention.hip
  bh = (slot / nx) * 8 + (L & 7);
  tile = slot % nx;
  return bh < nbh;
}

}  // namespace emu_attn

// attention_emu_bwd4.hip: launches emu_attn_bwd4_kernel over planes that are already converted (the argument block of
// hoisdf_attention_bwd_emu); returns a HOISDF status
int attention_bwd4_emu_launch(const emu_attn::EmuAttn& a, hipStream_t st);
// attention_emu_bwd4h.hip: the f16x2 form (two f16 planes per operand in a.q / a.k / a.v / a.d, per-(sample, head) scales from a.q_hm / k_hm / v_hm / d_hm)
int attention_bwd4h_emu_launch(const emu_attn::EmuAttn& a, hipStream_t st);
// attention_emu_bwd4g.hip: the f16x2 form with two dS pieces; behind a.dq_scale's B H floats it reads the 2 B H bound words of
// emu_attn_delta_bound_kernel (attention_emu.hip): [2 bh] = bits of max_q ||dO[q]||_2, [2 bh + 1] = bits of max_q |delta[q]|
int attention_bwd4g_emu_launch(const emu_attn::EmuAttn& a, hipStream_t st);
}  // namespace hoisdf
