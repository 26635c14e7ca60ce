// Image preparation (include/hoisdf.h, "image preparation"): camera frame -> model input on the device.
//   warp_kernel   nearest-neighbour affine gather of the u8 frame (float64 source coordinates, the left-hand flip folded in) into the
//                 u8 crop and / or the float model input, plus both heat-map masks (the NEAREST resize folded into the same map);
//   photo_kernel  7-tap separable Gaussian blur in LDS (64 x 16 tile, 3-pixel halo), then brightness / contrast / saturation / hue
//                 in registers in the per-sample order on integer levels, then / 255.  LSUM = true stops in front of the contrast
//                 and adds the tile's luma to the sample's u32 sum (integer atomics: any order gives the same bits).
// Memory-bound gathers: one HBM read and one write per pixel and pass, stores coalesced along the channel-interleaved row.  Sample
// descriptors travel as kernel arguments, IMG_CHUNK samples per launch, so an entry only enqueues.  No float atomics.
#include <math.h>

#include "common.h"

using namespace hoisdf;

extern "C" void hoisdf_internal_set_error(const char* msg) { set_error("%s", msg); }

namespace {

constexpr int IMG_CHUNK = 16;      // samples per launch (descriptors are kernel arguments: 16 x 88 bytes)
constexpr int WARP_THREADS = 256;  // output pixels per block

struct WarpSample {
  const uint8_t* frame;
  const uint8_t* mask[2];
  double t[6];
  int H, W, flip, packed;
};
struct WarpArgs { WarpSample s[IMG_CHUNK]; };

// source pixel of the output position (xc, yc) = pixel centre: floor in float64, products and sums rounded separately
__device__ __forceinline__ bool warp_source(const WarpSample& s, double xc, double yc, int& sx, int& sy) {
  const double fx = floor(__dadd_rn(__dadd_rn(__dmul_rn(s.t[0], xc), __dmul_rn(s.t[1], yc)), s.t[2]));
  const double fy = floor(__dadd_rn(__dadd_rn(__dmul_rn(s.t[3], xc), __dmul_rn(s.t[4], yc)), s.t[5]));
  const bool ok = fx >= 0.0 && fx < (double)s.W && fy >= 0.0 && fy < (double)s.H;      // false for NaN as well
  sx = ok ? (int)fx : 0;
  sy = ok ? (int)fy : 0;
  if (s.flip) sx = s.W - 1 - sx;
  return ok;
}

// grid (img_blocks + mask_blocks, samples of this launch).  Blocks below img_blocks own 256 consecutive crop pixels, the others 256
// consecutive heat-map pixels of the two masks ([mask][hm][hm] linearised).
__global__ __launch_bounds__(WARP_THREADS) void warp_kernel(const WarpArgs a, int b0, int res, int hm, int img_blocks, int nchw,
                                                            float* __restrict__ img, uint8_t* __restrict__ crop_u8,
                                                            float* __restrict__ hand_seg, float* __restrict__ obj_seg) {
  __shared__ uint8_t s_px[WARP_THREADS * 3];
  const WarpSample& s = a.s[blockIdx.y];
  const long b = b0 + blockIdx.y;
  const int tid = threadIdx.x;
  const int npix = res * res;
  if ((int)blockIdx.x < img_blocks) {
    const int p0 = blockIdx.x * WARP_THREADS, p = p0 + tid;
    uint8_t r = 0, g = 0, bl = 0;
    if (p < npix) {
      const int y = p / res, x = p - y * res;
      int sx, sy;
      if (warp_source(s, (double)x + 0.5, (double)y + 0.5, sx, sy)) {
        const uint8_t* q = s.frame + ((long)sy * s.W + sx) * 3;
        r = q[0]; g = q[1]; bl = q[2];
      }
      if (img && nchw) {
        float* o = img + b * 3 * npix + p;
        o[0] = __fdiv_rn((float)r, 255.f);
        o[npix] = __fdiv_rn((float)g, 255.f);
        o[2 * (long)npix] = __fdiv_rn((float)bl, 255.f);
      }
    }
    s_px[tid * 3] = r; s_px[tid * 3 + 1] = g; s_px[tid * 3 + 2] = bl;
    __syncthreads();
    const int n_el = min(WARP_THREADS, npix - p0) * 3;              // channel-interleaved elements this block owns
    const long e0 = (b * npix + p0) * 3;
    if (crop_u8)
      for (int e = tid; e < n_el; e += WARP_THREADS) crop_u8[e0 + e] = s_px[e];
    if (img && !nchw)
      for (int e = tid; e < n_el; e += WARP_THREADS) img[e0 + e] = __fdiv_rn((float)s_px[e], 255.f);
    return;
  }
  const int nm = hm * hm;
  const int p = ((int)blockIdx.x - img_blocks) * WARP_THREADS + tid;
  if (p >= 2 * nm) return;
  const int m = p >= nm, q = p - m * nm;
  const int i = q / hm, j = q - i * hm, step = res / hm;
  int sx, sy;
  float v = 0.f;
  const uint8_t* src = s.mask[m];
  if (warp_source(s, (double)(j * step + step / 2) + 0.5, (double)(i * step + step / 2) + 0.5, sx, sy)) {
    const long idx = (long)sy * s.W + sx;
    v = s.packed ? (float)((src[idx >> 3] >> (7 - (int)(idx & 7))) & 1) : (float)src[idx];
  }
  (m ? obj_seg : hand_seg)[b * nm + q] = v;
}

// ---- photometric chain -----------------------------------------------------------------------------------------------------
constexpr int TW = 64, TH = 16, HALO = 3, PH_THREADS = 256;
constexpr int IN_W = (TW + 2 * HALO) * 3, IN_H = TH + 2 * HALO;

struct PhotoSample {
  float w[4];          // blur weights at distance 0..3; w[0] = 0: no blur
  float factor[4];
  int order[4];
  int enabled, hue_shift;
};
struct PhotoArgs { PhotoSample s[IMG_CHUNK]; };

__device__ __forceinline__ int luma_level(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }
// trunc(clip(deg + f (x - deg), 0, 255)) in float32, each operation rounded on its own
__device__ __forceinline__ int blend_level(int x, float deg, float f) {
  const float v = __fadd_rn(deg, __fmul_rn(f, __fsub_rn((float)x, deg)));
  return (int)fminf(fmaxf(v, 0.f), 255.f);
}
__device__ __forceinline__ int round_half_up(float v) { return (int)floor((double)v + 0.5); }

// PIL's RGB -> HSV -> RGB with H moved by `shift` modulo 256 (image_oracle.rgb_to_hsv / hsv_to_rgb, equal to PIL on all 2^24 colours)
__device__ __forceinline__ void hue_rotate(int& r, int& g, int& b, int shift) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
  int uh = 0, us = 0;
  if (maxc != minc) {
    const float cr = (float)(maxc - minc);
    const float s = __fdiv_rn(cr, (float)maxc);
    const double rc = (double)__fdiv_rn((float)(maxc - r), cr), gc = (double)__fdiv_rn((float)(maxc - g), cr),
                 bc = (double)__fdiv_rn((float)(maxc - b), cr);
    double hd;
    if (r == maxc) hd = __dsub_rn(bc, gc);
    else if (g == maxc) hd = __dsub_rn(__dadd_rn(2.0, rc), bc);
    else hd = __dsub_rn(__dadd_rn(4.0, gc), rc);
    const float h0 = (float)hd;
    const float h1 = (float)fmod(__dadd_rn(__ddiv_rn((double)h0, 6.0), 1.0), 1.0);
    uh = min(max((int)__dmul_rn((double)h1, 255.0), 0), 255);
    us = min(max((int)__dmul_rn((double)s, 255.0), 0), 255);
  }
  const int h = (uh + shift) & 255, v = maxc;
  if (us == 0) { r = g = b = v; return; }
  const float fh = __fdiv_rn(__fmul_rn((float)h, 6.f), 255.f);
  const float fi = floorf(fh);
  const float f = __fsub_rn(fh, fi), fs = __fdiv_rn((float)us, 255.f), vv = (float)v;
  const int p = round_half_up(__fmul_rn(vv, __fsub_rn(1.f, fs)));
  const int q = round_half_up(__fmul_rn(vv, __fsub_rn(1.f, __fmul_rn(fs, f))));
  const int t = round_half_up(__fmul_rn(vv, __fsub_rn(1.f, __fmul_rn(fs, __fsub_rn(1.f, f)))));
  switch (((int)fi) % 6) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
  r = min(max(r, 0), 255); g = min(max(g, 0), 255); b = min(max(b, 0), 255);
}

// grid (tiles_x, tiles_y, samples of this launch); 256 threads own a 64 x 16 pixel tile, four pixels each
template <bool LSUM>
__global__ __launch_bounds__(PH_THREADS) void photo_kernel(const PhotoArgs a, int b0, int res, int nchw, const uint8_t* __restrict__ crop_u8,
                                                           uint32_t* __restrict__ lsum, float* __restrict__ img) {
  __shared__ uint8_t s_in[IN_H][IN_W];
  __shared__ float s_h[IN_H][TW * 3];
  __shared__ uint32_t s_red[PH_THREADS / 64];
  const PhotoSample& s = a.s[blockIdx.z];
  const long b = b0 + blockIdx.z;
  const int tid = threadIdx.x;
  const bool has_contrast = (s.enabled >> 1) & 1;
  if (LSUM && !has_contrast) return;                              // uniform per block
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const uint8_t* src = crop_u8 + b * res * res * 3;
  for (int e = tid; e < IN_H * IN_W; e += PH_THREADS) {
    const int ty = e / IN_W, bc = e - ty * IN_W, px = bc / 3, c = bc - px * 3;
    const int gy = min(max(y0 + ty - HALO, 0), res - 1), gx = min(max(x0 + px - HALO, 0), res - 1);      // edges replicated
    s_in[ty][bc] = src[((long)gy * res + gx) * 3 + c];
  }
  __syncthreads();
  const bool blur = s.w[0] != 0.f;
  if (blur) {
    for (int e = tid; e < IN_H * TW * 3; e += PH_THREADS) {
      const int ty = e / (TW * 3), bc = e - ty * (TW * 3);
      float acc = 0.f;
#pragma unroll
      for (int k = -HALO; k <= HALO; ++k) acc += s.w[k < 0 ? -k : k] * (float)s_in[ty][bc + (k + HALO) * 3];
      s_h[ty][bc] = acc;
    }
    __syncthreads();
  }
  uint32_t lacc = 0;
  float deg_c = 0.f;
  if (!LSUM && has_contrast) deg_c = (float)(int)((double)lsum[b] / (double)(res * res) + 0.5);
  for (int p = tid; p < TW * TH; p += PH_THREADS) {
    const int ty = p / TW, tx = p - ty * TW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= res || y >= res) continue;
    int lv[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (blur) {
        float acc = 0.f;
#pragma unroll
        for (int k = -HALO; k <= HALO; ++k) acc += s.w[k < 0 ? -k : k] * s_h[ty + HALO + k][tx * 3 + c];
        lv[c] = min(max((int)floorf(acc + 0.5f), 0), 255);
      } else {
        lv[c] = s_in[ty + HALO][(tx + HALO) * 3 + c];
      }
    }
    int r = lv[0], g = lv[1], bl = lv[2];
    bool stop = false;
    for (int i = 0; i < 4 && !stop; ++i) {
      const int op = s.order[i];
      if (!((s.enabled >> op) & 1)) continue;
      const float f = s.factor[op];
      if (op == 0) {
        r = blend_level(r, 0.f, f); g = blend_level(g, 0.f, f); bl = blend_level(bl, 0.f, f);
      } else if (op == 1) {
        if (LSUM) { lacc += (uint32_t)luma_level(r, g, bl); stop = true; }
        else { r = blend_level(r, deg_c, f); g = blend_level(g, deg_c, f); bl = blend_level(bl, deg_c, f); }
      } else if (op == 2) {
        const float L = (float)luma_level(r, g, bl);
        r = blend_level(r, L, f); g = blend_level(g, L, f); bl = blend_level(bl, L, f);
      } else {
        hue_rotate(r, g, bl, s.hue_shift);
      }
    }
    if (!LSUM) {
      const long npix = (long)res * res, pix = (long)y * res + x;
      if (nchw) {
        float* o = img + b * 3 * npix + pix;
        o[0] = __fdiv_rn((float)r, 255.f); o[npix] = __fdiv_rn((float)g, 255.f); o[2 * npix] = __fdiv_rn((float)bl, 255.f);
      } else {
        float* o = img + (b * npix + pix) * 3;
        o[0] = __fdiv_rn((float)r, 255.f); o[1] = __fdiv_rn((float)g, 255.f); o[2] = __fdiv_rn((float)bl, 255.f);
      }
    }
  }
  if (LSUM) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) lacc += (uint32_t)__shfl_xor((int)lacc, o, 64);
    if ((tid & 63) == 0) s_red[tid >> 6] = lacc;
    __syncthreads();
    if (tid == 0) atomicAdd(lsum + b, s_red[0] + s_red[1] + s_red[2] + s_red[3]);
  }
}

bool finite_d(double v) { return v == v && v - v == 0.0; }

int check_image_args(const char* what, const hoisdf_frame* frames, const hoisdf_crop* crops, int B, int res, int hm, const void* img,
                     const void* hand_seg, const void* obj_seg) {
  HOISDF_REQUIRE(B >= 0, HOISDF_ERR_INVALID, "%s: B=%d", what, B);
  HOISDF_REQUIRE(res > 0 && hm > 0, HOISDF_ERR_INVALID, "%s: res=%d hm=%d (both > 0)", what, res, hm);
  HOISDF_REQUIRE(res % hm == 0, HOISDF_ERR_INVALID, "%s: res=%d is no multiple of hm=%d", what, res, hm);
  HOISDF_REQUIRE(res <= 16384, HOISDF_ERR_INVALID, "%s: res=%d (at most 16384)", what, res);
  HOISDF_REQUIRE(frames && crops && img && hand_seg && obj_seg, HOISDF_ERR_INVALID, "%s: null pointer", what);
  for (int b = 0; b < B; ++b) {
    const hoisdf_frame& f = frames[b];
    HOISDF_REQUIRE(f.frame && f.hand_mask && f.obj_mask, HOISDF_ERR_INVALID, "%s: sample %d: null frame or mask pointer", what, b);
    HOISDF_REQUIRE(f.H > 0 && f.W > 0 && (long)f.H * f.W <= (1L << 30), HOISDF_ERR_INVALID, "%s: sample %d: frame %d x %d", what, b, f.H, f.W);
    const double* t = crops[b].inverse;
    bool fin = true;
    for (int i = 0; i < 6; ++i) fin = fin && finite_d(t[i]);
    const double det = t[0] * t[4] - t[1] * t[3];
    HOISDF_REQUIRE(fin && finite_d(det) && det != 0.0, HOISDF_ERR_INVALID, "%s: sample %d: the affine is not invertible", what, b);
  }
  return HOISDF_OK;
}

int launch_warp(const hoisdf_frame* frames, const hoisdf_crop* crops, int B, int res, int hm, int nchw, float* img, uint8_t* crop_u8,
                float* hand_seg, float* obj_seg, hipStream_t st) {
  const int img_blocks = cdiv((long)res * res, WARP_THREADS), mask_blocks = cdiv(2L * hm * hm, WARP_THREADS);
  for (int b0 = 0; b0 < B; b0 += IMG_CHUNK) {
    const int nb = B - b0 < IMG_CHUNK ? B - b0 : IMG_CHUNK;
    WarpArgs a = {};
    for (int i = 0; i < nb; ++i) {
      const hoisdf_frame& f = frames[b0 + i];
      WarpSample& s = a.s[i];
      s.frame = f.frame; s.mask[0] = f.hand_mask; s.mask[1] = f.obj_mask;
      for (int k = 0; k < 6; ++k) s.t[k] = crops[b0 + i].inverse[k];
      s.H = f.H; s.W = f.W; s.flip = crops[b0 + i].flip != 0; s.packed = f.mask_packed != 0;
    }
    hipLaunchKernelGGL(warp_kernel, dim3(img_blocks + mask_blocks, nb), dim3(WARP_THREADS), 0, st, a, b0, res, hm, img_blocks, nchw, img,
                       crop_u8, hand_seg, obj_seg);
  }
  return check_launch("image warp");
}

}  // namespace

extern "C" int hoisdf_image_crop(const hoisdf_frame* frames, const hoisdf_crop* crops, int B, int res, int hm, int nchw, float* img,
                                 uint8_t* crop_u8, float* hand_seg, float* obj_seg, void* stream) {
  const int rc = check_image_args("image_crop", frames, crops, B, res, hm, img, hand_seg, obj_seg);
  if (rc != HOISDF_OK) return rc;
  if (B == 0) return HOISDF_OK;
  return launch_warp(frames, crops, B, res, hm, nchw, img, crop_u8, hand_seg, obj_seg, as_stream(stream));
}

extern "C" int hoisdf_image_augment(const hoisdf_frame* frames, const hoisdf_crop* crops, const hoisdf_photo* photo, int B, int res, int hm,
                                    int nchw, float* img, uint8_t* crop_u8, uint32_t* lsum, float* hand_seg, float* obj_seg, void* stream) {
  int rc = check_image_args("image_augment", frames, crops, B, res, hm, img, hand_seg, obj_seg);
  if (rc != HOISDF_OK) return rc;
  HOISDF_REQUIRE(photo && crop_u8 && lsum, HOISDF_ERR_INVALID, "image_augment: null pointer");
  bool any_contrast = false;
  for (int b = 0; b < B; ++b) {
    const hoisdf_photo& p = photo[b];
    HOISDF_REQUIRE((p.enabled & ~15) == 0, HOISDF_ERR_INVALID, "image_augment: sample %d: enabled=%d (bits 0 .. 3)", b, p.enabled);
    int seen = 0;
    for (int i = 0; i < 4; ++i)
      if (p.order[i] >= 0 && p.order[i] < 4) seen |= 1 << p.order[i];
    HOISDF_REQUIRE(seen == 15, HOISDF_ERR_INVALID, "image_augment: sample %d: order (%d, %d, %d, %d) is no permutation of 0 .. 3", b,
                   p.order[0], p.order[1], p.order[2], p.order[3]);
    HOISDF_REQUIRE(finite_d(p.blur_sigma) && p.blur_sigma >= 0.f, HOISDF_ERR_INVALID, "image_augment: sample %d: blur_sigma=%g", b,
                   (double)p.blur_sigma);
    for (int i = 0; i < 4; ++i)
      HOISDF_REQUIRE(!((p.enabled >> i) & 1) || (finite_d(p.factor[i]) && (i == 3 || p.factor[i] >= 0.f)), HOISDF_ERR_INVALID,
                     "image_augment: sample %d: factor[%d]=%g", b, i, (double)p.factor[i]);
    any_contrast = any_contrast || ((p.enabled >> 1) & 1);
  }
  if (B == 0) return HOISDF_OK;
  hipStream_t st = as_stream(stream);
  rc = launch_warp(frames, crops, B, res, hm, 0, nullptr, crop_u8, hand_seg, obj_seg, st);
  if (rc != HOISDF_OK) return rc;
  hipError_t e = hipMemsetAsync(lsum, 0, sizeof(uint32_t) * B, st);
  HOISDF_REQUIRE(e == hipSuccess, HOISDF_ERR_LAUNCH, "image_augment: %s", hipGetErrorString(e));
  const dim3 tiles(cdiv(res, TW), cdiv(res, TH));
  for (int pass = any_contrast ? 0 : 1; pass < 2; ++pass)
    for (int b0 = 0; b0 < B; b0 += IMG_CHUNK) {
      const int nb = B - b0 < IMG_CHUNK ? B - b0 : IMG_CHUNK;
      PhotoArgs a = {};
      for (int i = 0; i < nb; ++i) {
        const hoisdf_photo& p = photo[b0 + i];
        PhotoSample& s = a.s[i];
        if (p.blur_sigma >= 0.05f) {      // image_oracle.blur_weights: float64, normalised over the 7 taps, rounded to float32
          double w[4], sum = 0.0;
          for (int k = 0; k < 4; ++k) w[k] = exp(-(double)(k * k) / (2.0 * (double)p.blur_sigma * (double)p.blur_sigma));
          sum = w[0] + 2.0 * (w[1] + w[2] + w[3]);
          for (int k = 0; k < 4; ++k) s.w[k] = (float)(w[k] / sum);
        }
        for (int k = 0; k < 4; ++k) { s.factor[k] = p.factor[k]; s.order[k] = p.order[k]; }
        s.enabled = p.enabled;
        s.hue_shift = ((p.enabled >> 3) & 1) ? ((int)((double)p.factor[3] * 255.0) & 255) : 0;      // uint8(hue_factor * 255), modulo 256
      }
      if (pass == 0)
        hipLaunchKernelGGL(photo_kernel<true>, dim3(tiles.x, tiles.y, nb), dim3(PH_THREADS), 0, st, a, b0, res, nchw, crop_u8, lsum, img);
      else
        hipLaunchKernelGGL(photo_kernel<false>, dim3(tiles.x, tiles.y, nb), dim3(PH_THREADS), 0, st, a, b0, res, nchw, crop_u8, lsum, img);
    }
  return check_launch("image photometric chain");
}
