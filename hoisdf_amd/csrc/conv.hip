// NHWC implicit-GEMM convolution, forward, exact f32 on the gfx950 f32 MFMA pipe (v_mfma_f32_32x32x2_f32: bit-for-bit an fmaf
// chain, so no operand scales - image maps carry no magnitude words and folded BatchNorm scales spread a weight's channels over
// decades).  The tile structure, the k-major LDS orientation and the XCD remap are gemm.hip's; the A operand is not a matrix:
//   output row  m = (b, oy, ox)            contraction index k = (ky, kx, ci)
//   A[m][k] = x[b][oy s - p + ky][ox s - p + kx][ci]  (0 outside the map),  x dense channels-last with a row stride ldx >= C_in
//   B[k][n] = the weight packed once to [ky][kx][ci][co] (row stride ldw = C_out rounded up to 4, zero filled)
// so every thread keeps the (b, oy, ox) of the tile rows it stages and resolves (ky, kx, ci) once per k-tile: with C_in % 4 == 0
// four consecutive k are four consecutive channels of one tap (one 16-byte load, or zeros for a tap in the padding); the stem
// (C_in = 3, K = 147) takes the element-wise form of the same code.
// ConvTranspose2d(4, 2, 1) runs as its four output-parity classes (blockIdx.y): output pixel (2 qy + py, 2 qx + px) reads the
// 2 x 2 input taps iy = qy - (1 - py) + ty, ix = qx - (1 - px) + tx with the weight taps ky = 3 - py - 2 ty, kx = 3 - px - 2 tx,
// i.e. a 2 x 2 convolution (K = 4 C_in) whose rows are written to every second output pixel.
// Epilogue: y[pixel][c_off + co] = act(acc + bias[co] (+ residual[pixel][co])), row stride ldy >= c_off + C_out: two producers write
// channel slices of one map instead of a concatenation.  Problems with a handful of output tiles (the deep layers at B = 1: M = 64,
// K up to 8192) cut K over blockIdx.z; every slice parks its partial tile in the caller's workspace and a second kernel adds the
// slices in slice order and applies the epilogue: no float atomics, two runs give the same bits.
// Also here: maxpool 3 x 3 s2 p1 on NHWC, and the fold (eval-mode BatchNorm into weight + bias) / pack kernels.
#include "common.h"

namespace hoisdf {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int CBK = 16, CNT = 256;

struct ConvArgs {
  const float* x;
  const float* w;
  const float* bias;
  const float* res;
  float* y;          // c_off already applied
  float* part;       // split-K partial tiles [class][slice][M][N]
  int B, H, W, Cin;
  int OH, OW;        // the row grid (of one parity class for the transposed form)
  int KH, KW, stride, pad_y, pad_x;
  int M, N, K;
  int ldx, ldw, ldr, ldy;
  int act;
  int ncls;          // 1, or the 4 parity classes of the transposed form
  int YH, YW;        // the output map (transposed: 2 OH x 2 OW)
  int splitk, k_per_split;
  int tiles_m, tiles_n;
  int vecA;
};

__device__ __forceinline__ float conv_act(float v, int act) {
  if (act == 1) return fmaxf(v, 0.f);
  if (act == 2) return 1.f / (1.f + expf(-v));
  return v;
}
// output pixel index of row `row` (class cls)
__device__ __forceinline__ long conv_out_pixel(const ConvArgs& g, int row, int cls) {
  if (g.ncls == 1) return row;
  const int hw = g.OH * g.OW;
  const int b = row / hw, rem = row - b * hw;
  const int qy = rem / g.OW, qx = rem - qy * g.OW;
  return ((long)b * g.YH + 2 * qy + (cls >> 1)) * g.YW + 2 * qx + (cls & 1);
}
__device__ __forceinline__ void conv_finish(const ConvArgs& g, float v, long pix, int col) {
  if (g.bias) v += g.bias[col];
  if (g.res) v += g.res[(size_t)pix * g.ldr + col];
  g.y[(size_t)pix * g.ldy + col] = conv_act(v, g.act);
}

// tile = (64 WM) x (64 WN), 4 waves as 2 x 2, each wave WM x WN MFMA tiles of 32 x 32
template <int WM, int WN>
__global__ __launch_bounds__(CNT) void conv_igemm_kernel(ConvArgs g) {
  constexpr int BMt = 64 * WM, BNt = 64 * WN;
  constexpr int SA = BMt + 1;          // transposing ds_write_b32, stride = 1 mod 32
  constexpr int SB = BNt + 4;          // ds_write_b128, 16-byte aligned rows
  constexpr int B_LPR = BNt / 4;       // lanes per k-row of the weight tile
  constexpr int B_RPP = CNT / B_LPR;   // k-rows per pass
  static_assert(B_RPP * WN == CBK, "weight tile staging");
  __shared__ __attribute__((aligned(16))) float lds[CBK * SA + CBK * SB];
  float* As = lds;
  float* Bs = lds + CBK * SA;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int cls = blockIdx.y, split = blockIdx.z;
  const int t = xcd_remap(blockIdx.x, g.tiles_m * g.tiles_n);
  const int tm = t / g.tiles_n, tn = t - tm * g.tiles_n;
  const int m0 = tm * BMt, n0 = tn * BNt;
  const int kbeg = split * g.k_per_split;
  const int kend = min(g.K, kbeg + g.k_per_split);
  const int nk = (kend - kbeg + CBK - 1) / CBK;

  int pad_y = g.pad_y, pad_x = g.pad_x;
  const float* __restrict__ wp = g.w;
  if (g.ncls > 1) {
    pad_y = 1 - (cls >> 1);
    pad_x = 1 - (cls & 1);
    wp += (size_t)cls * g.K * g.ldw;
  }

  // the tile rows this thread stages: (b, oy, ox) -> first input pixel of the window
  int iy0[WM], ix0[WM], pix0[WM];
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int r = m0 + (tid >> 2) + 64 * i;
    if (r < g.M) {
      const int hw = g.OH * g.OW;
      const int b = r / hw, rem = r - b * hw;
      const int oy = rem / g.OW, ox = rem - oy * g.OW;
      iy0[i] = oy * g.stride - pad_y;
      ix0[i] = ox * g.stride - pad_x;
      pix0[i] = b * g.H * g.W;
    } else {
      iy0[i] = -(1 << 20);      // every tap lands outside the map: zeros
      ix0[i] = 0;
      pix0[i] = 0;
    }
  }

  float4 ra[WM], rb[WN];
  auto load_a = [&](int k0) {
    const int kq = k0 + (tid & 3) * 4;
    if (g.vecA) {
      // C_in % 4 == 0: k .. k + 3 are four channels of one tap
      int ky = 0, kx = 0, ci = 0;
      const bool kin = kq < kend;
      if (kin) {
        const int tap = kq / g.Cin;
        ci = kq - tap * g.Cin;
        ky = tap / g.KW;
        kx = tap - ky * g.KW;
      }
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const int iy = iy0[i] + ky, ix = ix0[i] + kx;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (kin && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
          v = *reinterpret_cast<const float4*>(g.x + (size_t)(pix0[i] + iy * g.W + ix) * g.ldx + ci);
        ra[i] = v;
      }
    } else {
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = kq + j;
          float v = 0.f;
          if (k < kend) {
            const int tap = k / g.Cin, ci = k - tap * g.Cin;
            const int ky = tap / g.KW, kx = tap - ky * g.KW;
            const int iy = iy0[i] + ky, ix = ix0[i] + kx;
            if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) v = g.x[(size_t)(pix0[i] + iy * g.W + ix) * g.ldx + ci];
          }
          e[j] = v;
        }
        ra[i] = make_float4(e[0], e[1], e[2], e[3]);
      }
    }
  };
  auto load_b = [&](int k0) {
#pragma unroll
    for (int i = 0; i < WN; ++i) {
      const int k = k0 + tid / B_LPR + B_RPP * i;
      const int n = n0 + (tid % B_LPR) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < kend && n < g.ldw) v = *reinterpret_cast<const float4*>(wp + (size_t)k * g.ldw + n);      // ldw % 4 == 0, zero filled
      rb[i] = v;
    }
  };
  auto store_ab = [&]() {
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int r = (tid >> 2) + 64 * i, k = (tid & 3) * 4;
      As[(k + 0) * SA + r] = ra[i].x;
      As[(k + 1) * SA + r] = ra[i].y;
      As[(k + 2) * SA + r] = ra[i].z;
      As[(k + 3) * SA + r] = ra[i].w;
    }
#pragma unroll
    for (int i = 0; i < WN; ++i) {
      const int k = tid / B_LPR + B_RPP * i, n = (tid % B_LPR) * 4;
      *reinterpret_cast<float4*>(&Bs[k * SB + n]) = rb[i];
    }
  };

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    load_a(kbeg);
    load_b(kbeg);
    store_ab();
  }
  __syncthreads();
  const int arow = wm * 32 * WM + (lane & 31);
  const int brow = wn * 32 * WN + (lane & 31);
  const int khalf = lane >> 5;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {
      load_a(kbeg + (kt + 1) * CBK);
      load_b(kbeg + (kt + 1) * CBK);
    }
#pragma unroll
    for (int kk = 0; kk < CBK; kk += 2) {
      float a[WM], b[WN];
#pragma unroll
      for (int i = 0; i < WM; ++i) a[i] = As[(kk + khalf) * SA + arow + 32 * i];
#pragma unroll
      for (int j = 0; j < WN; ++j) b[j] = Bs[(kk + khalf) * SB + brow + 32 * j];
#pragma unroll
      for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();      // every wave is done reading this stage
    if (kt + 1 < nk) {
      store_ab();
      __syncthreads();
    }
  }

  // C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int rbase = m0 + wm * 32 * WM + 4 * khalf;
  const int cbase = n0 + wn * 32 * WN + (lane & 31);
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = rbase + i * 32 + (r & 3) + 8 * (r >> 2);
      if (row >= g.M) continue;
      if (g.splitk > 1) {
        float* p = g.part + ((size_t)(cls * g.splitk + split) * g.M + row) * g.N;
#pragma unroll
        for (int j = 0; j < WN; ++j) {
          const int col = cbase + j * 32;
          if (col < g.N) p[col] = acc[i][j][r];
        }
      } else {
        const long pix = conv_out_pixel(g, row, cls);
#pragma unroll
        for (int j = 0; j < WN; ++j) {
          const int col = cbase + j * 32;
          if (col < g.N) conv_finish(g, acc[i][j][r], pix, col);
        }
      }
    }
}

// the slices of one output element, added in slice order, then the epilogue
__global__ __launch_bounds__(256) void conv_splitk_reduce_kernel(ConvArgs g) {
  const long total = (long)g.ncls * g.M * g.N;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const long mn = (long)g.M * g.N;
  const int cls = (int)(idx / mn);
  const long e = idx - (long)cls * mn;
  const int row = (int)(e / g.N), col = (int)(e - (long)row * g.N);
  const float* p = g.part + (size_t)cls * g.splitk * mn + e;
  float s = p[0];
  for (int k = 1; k < g.splitk; ++k) s += p[(size_t)k * mn];
  conv_finish(g, s, conv_out_pixel(g, row, cls), col);
}

// 3 x 3 s2 p1 maximum over the taps inside the map (the padding takes no part: a negative maximum survives)
__global__ __launch_bounds__(256) void maxpool3x3s2_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int B, int H,
                                                           int W, int C, int OH, int OW) {
  const long total = (long)B * OH * OW * C;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long pix = idx / C;
  const int ox = (int)(pix % OW);
  const int oy = (int)((pix / OW) % OH);
  const int b = (int)(pix / ((long)OW * OH));
  float m = -INFINITY;
  for (int ky = 0; ky < 3; ++ky) {
    const int iy = 2 * oy - 1 + ky;
    if (iy < 0 || iy >= H) continue;
    for (int kx = 0; kx < 3; ++kx) {
      const int ix = 2 * ox - 1 + kx;
      if (ix < 0 || ix >= W) continue;
      m = fmaxf(m, x[((size_t)((long)b * H + iy) * W + ix) * ldx + c]);
    }
  }
  y[(size_t)pix * ldy + c] = m;
}

// fold + pack: s = gamma / sqrt(var + eps) in f64, rounded once; w' = w s; b' = (b_conv - mean) s + beta.
// plain:      w [co][ci][KH][KW]  -> packed[((ky KW + kx) C_in + ci) ldw + co]
// transposed: w [ci][co][4][4]    -> packed[cls][((ty 2 + tx) C_in + ci) ldw + co], ky = 3 - py - 2 ty, kx = 3 - px - 2 tx
// columns C_out .. ldw - 1 are zero.  One thread per packed element (+ ldw threads for the bias).
__global__ __launch_bounds__(256) void conv_pack_kernel(const float* __restrict__ w, const float* __restrict__ cb, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ mean,
                                                        const float* __restrict__ var, float eps, int Cout, int Cin, int KH, int KW,
                                                        int transposed, int ldw, float* __restrict__ packed, float* __restrict__ bias_out) {
  const long nw = (long)KH * KW * Cin * ldw;
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= nw + ldw) return;
  const int co = (int)(idx % ldw);
  float s = 1.f;
  if (gamma && co < Cout) s = (float)((double)gamma[co] / sqrt((double)var[co] + (double)eps));
  if (idx >= nw) {
    float b = 0.f;
    if (co < Cout) {
      b = cb ? cb[co] : 0.f;
      if (gamma) b = (b - mean[co]) * s + beta[co];
    }
    bias_out[co] = b;
    return;
  }
  float v = 0.f;
  if (co < Cout) {
    const long k = idx / ldw;
    if (!transposed) {
      const int ci = (int)(k % Cin);
      const int tap = (int)(k / Cin);
      const int ky = tap / KW, kx = tap - ky * KW;
      v = w[(((size_t)co * Cin + ci) * KH + ky) * KW + kx];
    } else {
      const long kc = 4L * Cin;
      const int cls = (int)(k / kc);
      const int kk = (int)(k - cls * kc);
      const int tap = kk / Cin, ci = kk - tap * Cin;
      const int ty = tap >> 1, tx = tap & 1;
      const int ky = 3 - (cls >> 1) - 2 * ty, kx = 3 - (cls & 1) - 2 * tx;
      v = w[(((size_t)ci * Cout + co) * 4 + ky) * 4 + kx];
    }
    v *= s;
  }
  packed[idx] = v;
}

static int aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

ConvPlan conv_plan(long M, int N, int K, int ncls) {
  ConvPlan p;
  const long t128 = (long)cdiv(M, 128) * cdiv(N, 128) * ncls;
  p.tile = (M >= 128 && N >= 128 && t128 >= 256) ? 128 : 64;
  const long tiles = p.tile == 128 ? t128 : (long)cdiv(M, 64) * cdiv(N, 64) * ncls;
  const int ksteps = cdiv(K, CBK);
  int s = 1;
  // a handful of output tiles on 256 CUs: cut K over more workgroups (>= 4 k-steps each)
  if (tiles <= 64) {
    s = (int)(256 / tiles);
    if (s > ksteps / 4) s = ksteps / 4;
    if (s < 2) s = 1;
  }
  p.k_per_split = cdiv(ksteps, s) * CBK;
  p.splitk = cdiv(K, p.k_per_split);
  p.workspace_bytes = p.splitk > 1 ? (long)sizeof(float) * ncls * p.splitk * M * N : 0;
  return p;
}

int conv_launch(const ConvProblem& c, const float* x, int ldx, const float* w_packed, const float* bias, const float* residual, int ldr,
                float* y, int ldy, int c_off, void* workspace, long workspace_bytes, hipStream_t st) {
  ConvArgs g{};
  g.x = x; g.w = w_packed; g.bias = bias; g.res = residual; g.y = y + c_off;
  g.B = c.B; g.H = c.H; g.W = c.W; g.Cin = c.C_in;
  g.ldx = ldx; g.ldw = (c.C_out + 3) & ~3; g.ldr = ldr; g.ldy = ldy; g.act = c.act;
  g.N = c.C_out;
  if (c.transposed) {
    g.OH = c.H; g.OW = c.W; g.KH = 2; g.KW = 2; g.stride = 1; g.ncls = 4; g.YH = 2 * c.H; g.YW = 2 * c.W;
  } else {
    g.OH = (c.H + 2 * c.pad - c.KH) / c.stride + 1;
    g.OW = (c.W + 2 * c.pad - c.KW) / c.stride + 1;
    g.KH = c.KH; g.KW = c.KW; g.stride = c.stride; g.pad_y = g.pad_x = c.pad; g.ncls = 1; g.YH = g.OH; g.YW = g.OW;
  }
  g.K = g.KH * g.KW * c.C_in;
  const long M = (long)c.B * g.OH * g.OW;
  g.M = (int)M;
  const ConvPlan p = conv_plan(M, g.N, g.K, g.ncls);
  HOISDF_REQUIRE(p.workspace_bytes == 0 || (workspace && workspace_bytes >= p.workspace_bytes), HOISDF_ERR_WORKSPACE,
                 "conv: workspace of %ld bytes, need %ld", workspace_bytes, p.workspace_bytes);
  g.splitk = p.splitk; g.k_per_split = p.k_per_split;
  g.part = reinterpret_cast<float*>(workspace);
  g.vecA = (c.C_in % 4 == 0) && (ldx % 4 == 0) && aligned16(x);
  g.tiles_m = cdiv(M, p.tile); g.tiles_n = cdiv(g.N, p.tile);
  const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)g.ncls, (unsigned)g.splitk);
  if (p.tile == 128) hipLaunchKernelGGL((conv_igemm_kernel<2, 2>), grid, dim3(CNT), 0, st, g);
  else hipLaunchKernelGGL((conv_igemm_kernel<1, 1>), grid, dim3(CNT), 0, st, g);
  if (int rc = check_launch("conv_igemm")) return rc;
  if (g.splitk > 1) {
    const long total = (long)g.ncls * M * g.N;
    hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, g);
    return check_launch("conv_splitk_reduce");
  }
  return HOISDF_OK;
}

int conv_pack_launch(const float* w, const float* conv_bias, const float* gamma, const float* beta, const float* mean, const float* var,
                     float eps, int C_out, int C_in, int KH, int KW, int transposed, float* packed, float* bias_out, hipStream_t st) {
  const int ldw = (C_out + 3) & ~3;
  const long n = (long)KH * KW * C_in * ldw + ldw;
  hipLaunchKernelGGL(conv_pack_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, w, conv_bias, gamma, beta, mean, var, eps, C_out, C_in,
                     KH, KW, transposed, ldw, packed, bias_out);
  return check_launch("conv_pack");
}

int maxpool_launch(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C, hipStream_t st) {
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const long total = (long)B * OH * OW * C;
  hipLaunchKernelGGL(maxpool3x3s2_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, st, x, ldx, y, ldy, B, H, W, C, OH, OW);
  return check_launch("maxpool3x3s2");
}

static int conv_check_sizes(const char* who, int B, int H, int W, int C_in, int C_out, int KH, int KW, int stride, int pad, int act) {
  HOISDF_REQUIRE(B > 0 && H > 0 && W > 0 && C_in > 0 && C_out > 0 && KH > 0 && KW > 0 && stride > 0 && pad >= 0 && pad < KH && pad < KW,
                 HOISDF_ERR_INVALID, "%s: bad sizes B=%d H=%d W=%d C_in=%d C_out=%d kernel=%dx%d stride=%d pad=%d", who, B, H, W, C_in, C_out,
                 KH, KW, stride, pad);
  HOISDF_REQUIRE(H + 2 * pad >= KH && W + 2 * pad >= KW, HOISDF_ERR_INVALID, "%s: a %dx%d kernel does not fit the %dx%d map", who, KH, KW, H, W);
  HOISDF_REQUIRE(act >= 0 && act <= 2, HOISDF_ERR_INVALID, "%s: act=%d (0 none, 1 ReLU, 2 sigmoid)", who, act);
  HOISDF_REQUIRE((long)B * H * W < (1L << 31) / 4 && (long)KH * KW * C_in < (1L << 24), HOISDF_ERR_INVALID, "%s: problem too large", who);
  return HOISDF_OK;
}

}  // namespace hoisdf

using namespace hoisdf;

extern "C" long hoisdf_conv_packed_floats(int C_out, int C_in, int KH, int KW) {
  if (C_out <= 0 || C_in <= 0 || KH <= 0 || KW <= 0) {
    set_error("conv_packed_floats: bad sizes C_out=%d C_in=%d kernel=%dx%d", C_out, C_in, KH, KW);
    return -1;
  }
  return (long)KH * KW * C_in * ((C_out + 3) & ~3);
}

extern "C" int hoisdf_conv_pack_weight(const float* w, const float* conv_bias, const float* gamma, const float* beta, const float* mean,
                                       const float* var, float eps, int C_out, int C_in, int KH, int KW, int transposed, float* packed,
                                       float* bias_out, void* stream) {
  HOISDF_REQUIRE(w && packed && bias_out, HOISDF_ERR_INVALID, "conv_pack_weight: null pointer");
  HOISDF_REQUIRE(C_out > 0 && C_in > 0 && KH > 0 && KW > 0, HOISDF_ERR_INVALID, "conv_pack_weight: bad sizes");
  HOISDF_REQUIRE(!transposed || (KH == 4 && KW == 4), HOISDF_ERR_INVALID, "conv_pack_weight: the transposed form is ConvTranspose2d(4, 2, 1)");
  HOISDF_REQUIRE(!gamma || (beta && mean && var && eps > 0.f), HOISDF_ERR_INVALID,
                 "conv_pack_weight: a BatchNorm fold needs gamma, beta, mean, var and eps > 0");
  HOISDF_REQUIRE(aligned16(packed), HOISDF_ERR_INVALID, "conv_pack_weight: packed must be 16-byte aligned");
  return conv_pack_launch(w, conv_bias, gamma, beta, mean, var, eps, C_out, C_in, KH, KW, transposed, packed, bias_out, as_stream(stream));
}

extern "C" int hoisdf_conv_plan(long M, int C_out, int K, int classes, int* tile, int* splitk) {
  HOISDF_REQUIRE(M > 0 && C_out > 0 && K > 0 && (classes == 1 || classes == 4) && M < (1L << 31), HOISDF_ERR_INVALID,
                 "conv_plan: bad sizes M=%ld C_out=%d K=%d classes=%d", M, C_out, K, classes);
  const ConvPlan p = conv_plan(M, C_out, K, classes);
  if (tile) *tile = p.tile;
  if (splitk) *splitk = p.splitk;
  return HOISDF_OK;
}

extern "C" long hoisdf_conv_workspace_bytes(long M, int C_out, int K, int classes) {
  if (!(M > 0 && C_out > 0 && K > 0 && (classes == 1 || classes == 4) && M < (1L << 31))) {
    set_error("conv_workspace_bytes: bad sizes M=%ld C_out=%d K=%d classes=%d", M, C_out, K, classes);
    return -1;
  }
  return conv_plan(M, C_out, K, classes).workspace_bytes;
}

extern "C" int hoisdf_conv2d_fwd(const float* x, int ldx, const float* w_packed, const float* bias, const float* residual, int ldr, float* y,
                                 int ldy, int c_off, int B, int H, int W, int C_in, int C_out, int KH, int KW, int stride, int pad, int act,
                                 void* workspace, long workspace_bytes, void* stream) {
  HOISDF_REQUIRE(x && w_packed && y, HOISDF_ERR_INVALID, "conv2d_fwd: null pointer");
  if (int rc = conv_check_sizes("conv2d_fwd", B, H, W, C_in, C_out, KH, KW, stride, pad, act)) return rc;
  HOISDF_REQUIRE(ldx >= C_in && c_off >= 0 && ldy >= c_off + C_out && (!residual || ldr >= C_out), HOISDF_ERR_INVALID,
                 "conv2d_fwd: bad strides ldx=%d ldy=%d c_off=%d ldr=%d for C_in=%d C_out=%d", ldx, ldy, c_off, ldr, C_in, C_out);
  HOISDF_REQUIRE(aligned16(w_packed), HOISDF_ERR_INVALID, "conv2d_fwd: w_packed must be 16-byte aligned");
  ConvProblem c{B, H, W, C_in, C_out, KH, KW, stride, pad, act, 0};
  return conv_launch(c, x, ldx, w_packed, bias, residual, ldr, y, ldy, c_off, workspace, workspace_bytes, as_stream(stream));
}

extern "C" int hoisdf_conv_transpose2d_fwd(const float* x, int ldx, const float* w_packed, const float* bias, float* y, int ldy, int c_off, int B,
                                           int H, int W, int C_in, int C_out, int act, void* workspace, long workspace_bytes, void* stream) {
  HOISDF_REQUIRE(x && w_packed && y, HOISDF_ERR_INVALID, "conv_transpose2d_fwd: null pointer");
  HOISDF_REQUIRE(B > 0 && H > 0 && W > 0 && C_in > 0 && C_out > 0, HOISDF_ERR_INVALID,
                 "conv_transpose2d_fwd: bad sizes B=%d H=%d W=%d C_in=%d C_out=%d", B, H, W, C_in, C_out);
  HOISDF_REQUIRE(act >= 0 && act <= 2, HOISDF_ERR_INVALID, "conv_transpose2d_fwd: act=%d (0 none, 1 ReLU, 2 sigmoid)", act);
  HOISDF_REQUIRE((long)B * H * W < (1L << 31) / 16 && C_in < (1 << 22), HOISDF_ERR_INVALID, "conv_transpose2d_fwd: problem too large");
  HOISDF_REQUIRE(ldx >= C_in && c_off >= 0 && ldy >= c_off + C_out, HOISDF_ERR_INVALID,
                 "conv_transpose2d_fwd: bad strides ldx=%d ldy=%d c_off=%d for C_in=%d C_out=%d", ldx, ldy, c_off, C_in, C_out);
  HOISDF_REQUIRE(aligned16(w_packed), HOISDF_ERR_INVALID, "conv_transpose2d_fwd: w_packed must be 16-byte aligned");
  ConvProblem c{B, H, W, C_in, C_out, 4, 4, 2, 1, act, 1};
  return conv_launch(c, x, ldx, w_packed, bias, nullptr, 0, y, ldy, c_off, workspace, workspace_bytes, as_stream(stream));
}

extern "C" int hoisdf_maxpool2d_fwd(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C, void* stream) {
  HOISDF_REQUIRE(x && y, HOISDF_ERR_INVALID, "maxpool2d_fwd: null pointer");
  HOISDF_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0 && ldx >= C && ldy >= C && (long)B * H * W < (1L << 31) / 4, HOISDF_ERR_INVALID,
                 "maxpool2d_fwd: bad sizes B=%d H=%d W=%d C=%d ldx=%d ldy=%d", B, H, W, C, ldx, ldy);
  return maxpool_launch(x, ldx, y, ldy, B, H, W, C, as_stream(stream));
}
