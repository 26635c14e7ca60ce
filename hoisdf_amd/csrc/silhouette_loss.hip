// Silhouette LOSS (include/hoisdf.h "silhouette loss"): what holds a predicted mesh to a mask without a differentiable rasteriser - the
// distance transform of the target mask, read at the projected vertices (they are pulled into the silhouette), and the nearest
// projected vertex of every mask pixel (the silhouette is pulled under the mesh).  Integers and fp64, no float atomics.
//   edt_columns_kernel     pass 1 of hoisdf_mask_edt: one thread per column sweeps down and up and leaves, per pixel, the set row of
//                          its column nearest to it (the upper one on a tie, -1: the column has none) in d2_out.
//   edt_rows_kernel        pass 2: a workgroup owns one row.  Per column x' the row's g^2 = (y - y')^2 and the packed (y', x') sit in
//                          LDS; thread x takes the smallest key (g^2 + (x - x')^2, y', x') over x', every lane reading the same x' (a
//                          broadcast), and overwrites its own pixel of d2_out: nobody else reads that row.
//   sil_project_kernel     per vertex u, v in fp64 and its bilinear cell (-1: invalid) into the workspace.
//   sil_nearest_kernel     one workgroup per sample and tile of 256 pixels; the sample's (u, v) pairs pass through LDS in chunks of
//                          SIL_CHUNK, all lanes reading the same vertex; a wave without a set pixel skips the scan.
//   sil_reduce_kernel      one block per sample: both sums and both denominators in fp64, interact_loss.hip's order.
//   sil_bwd_kernel         one lane per vertex (a block is ONE wave of 64 vertices): its own inside term, then the pixel records in
//                          ascending pixel index, staged through LDS in tiles of 64 (lane j makes the record of pixel t0 + j), all
//                          lanes reading the same record; a tile without a record is skipped.  The sums live in (u, v); the chain
//                          rule to x, y, z and ONE rounding to fp32 end the lane's work.
#include "common.h"

namespace hoisdf {

constexpr int EDT_NONE = HOISDF_EDT_NONE, EDT_MAX = HOISDF_EDT_MAX_SIZE;
constexpr int SIL_TILE = HOISDF_SIL_LOSS_TILE, SIL_CHUNK = 1024;   // vertices per LDS chunk of the nearest scan: 16 KiB
static_assert(SIL_TILE == 64, "a tile is what one wave stages: one record per lane");
static_assert(EDT_NONE == (1 << 15) * (1 << 15) && EDT_MAX <= 1024, "a column without a set pixel is 2^15 away; y', x' pack into 10 bits");

__device__ __forceinline__ bool mask_set(const float* __restrict__ m, const float* __restrict__ m_or, size_t i) {
  return m[i] > 0.5f || (m_or && m_or[i] > 0.5f);
}

// ---- hoisdf_mask_edt ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void edt_columns_kernel(const float* __restrict__ mask, const float* __restrict__ mask_or, int w, int h,
                                                         int32_t* __restrict__ row_out) {
  const int x = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
  if (x >= w) return;
  const size_t base = (size_t)b * w * h + x;
  int last = -1;
  for (int y = 0; y < h; ++y) {                          // down: the nearest set row at or above y
    if (mask_set(mask, mask_or, base + (size_t)y * w)) last = y;
    row_out[base + (size_t)y * w] = last;
  }
  int next = -1;
  for (int y = h - 1; y >= 0; --y) {                     // up: the nearest set row at or below y; the upper one wins a tie
    const size_t o = base + (size_t)y * w;
    const int up = row_out[o];
    if (up == y) next = y;
    row_out[o] = up < 0 ? next : (next < 0 || y - up <= next - y) ? up : next;
  }
}

__global__ __launch_bounds__(EDT_MAX) void edt_rows_kernel(int w, int h, int32_t* __restrict__ d2, int32_t* __restrict__ nearest) {
  __shared__ int s_g2[EDT_MAX];                          // (y - y')^2 of column x', EDT_NONE: the column has no set pixel
  __shared__ int s_at[EDT_MAX];                          // y' << 10 | x'
  const int x = threadIdx.x, y = blockIdx.x, b = blockIdx.y;
  const size_t o = ((size_t)b * h + y) * w + x;
  if (x < w) {
    const int r = d2[o];
    s_g2[x] = r < 0 ? EDT_NONE : (y - r) * (y - r);
    s_at[x] = (max(r, 0) << 10) | x;
  }
  __syncthreads();
  if (x >= w) return;
  unsigned long long best = ((unsigned long long)EDT_NONE << 20) | 0xFFFFFull;
  for (int c = 0; c < w; ++c) {                          // every lane reads the same c
    const int g2 = s_g2[c];
    if (g2 >= EDT_NONE) continue;                        // (the same for every lane)
    const int dx = x - c;
    const unsigned long long key = ((unsigned long long)(g2 + dx * dx) << 20) | (unsigned)s_at[c];
    best = min(best, key);
  }
  const int d = (int)(best >> 20);
  d2[o] = d;
  if (nearest) nearest[o] = d >= EDT_NONE ? -1 : (int)((best >> 10) & 1023) * w + (int)(best & 1023);
}

// ---- the loss ----------------------------------------------------------------------------------------------------------------------
struct SilWorkspace {
  double *u, *v;                 // [B][V]
  int32_t* cell;                 // [B][V]: y0 w + x0 of the bilinear read, -1: an invalid vertex
  int32_t* nearest;              // [B][h w]: the nearest valid vertex of a set pixel of cover, -1: unset, or no valid vertex
  double* den;                   // [B][2]: the sum of the weights of the rows that count, the number of pixels with a nearest vertex
};
// ONE layout for the size query, the forward and the backward (tests read u, v, cell and nearest through it: the header states it)
static SilWorkspace sil_workspace(Bump& w, long B, long V, long npix) {
  SilWorkspace s;
  s.u = (double*)w.take(B * V * 8);
  s.v = (double*)w.take(B * V * 8);
  s.cell = w.ints(B * V);
  s.nearest = w.ints(B * npix);
  s.den = (double*)w.take(B * 16);
  return s;
}

struct SilArgs {
  const float* verts; const int32_t* n_verts; int V; const float* K;
  const int32_t* d2; const float* cover; int w, h; float near;
  const float* weight; long weight_stride;
  SilWorkspace s;
  float *inside, *cover_out;                 // forward
  const float *g_inside, *g_cover; float* d_verts;   // backward
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.4028234664e38f; }
__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; }
__device__ __forceinline__ int live_verts(const SilArgs& a, int b) { return a.n_verts ? min(max(a.n_verts[b], 0), a.V) : a.V; }
__device__ __forceinline__ double sil_weight(const SilArgs& a, int b, int i) {
  return a.weight ? (double)a.weight[(size_t)b * a.weight_stride + i] : 1.;
}

__global__ __launch_bounds__(256) void sil_project_kernel(const SilArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= a.V) return;
  const size_t o = (size_t)b * a.V + i;
  const float* p = a.verts + o * 3;
  const float* K = a.K + (size_t)b * 6;
  double u = 0., v = 0.;
  int cell = -1;
  if (i < live_verts(a, b) && finite_f(p[0]) && finite_f(p[1]) && finite_f(p[2]) && !(p[2] < a.near)) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    u = (((double)K[0] * x + (double)K[1] * y) + (double)K[2] * z) / z;
    v = (((double)K[3] * x + (double)K[4] * y) + (double)K[5] * z) / z;
    if (finite_d(u) && finite_d(v)) {                    // (a K that is not finite makes no vertex valid)
      const double uc = fmin(fmax(u, 0.), (double)(a.w - 1)), vc = fmin(fmax(v, 0.), (double)(a.h - 1));
      cell = min((int)floor(vc), max(a.h - 2, 0)) * a.w + min((int)floor(uc), max(a.w - 2, 0));
    }
  }
  a.s.u[o] = u; a.s.v[o] = v; a.s.cell[o] = cell;
}

__global__ __launch_bounds__(256) void sil_nearest_kernel(const SilArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_u[SIL_CHUNK], s_v[SIL_CHUNK];
  const int tid = threadIdx.x, p = blockIdx.x * 256 + tid, b = blockIdx.y, npix = a.w * a.h;
  const bool set = p < npix && a.cover[(size_t)b * npix + p] > 0.5f;
  const bool scan = __ballot(set) != 0ull;               // per wave
  const double px = (double)(p % a.w), py = (double)(p / a.w);
  double best = __builtin_huge_val();
  int who = -1;
  for (int v0 = 0; v0 < a.V; v0 += SIL_CHUNK) {
    const int cnt = min(SIL_CHUNK, a.V - v0);
    __syncthreads();
    for (int j = tid; j < cnt; j += 256) {
      const size_t o = (size_t)b * a.V + v0 + j;
      const bool ok = a.s.cell[o] >= 0;                  // an invalid vertex is infinitely far: never nearer than anything
      s_u[j] = ok ? a.s.u[o] : __builtin_huge_val();
      s_v[j] = ok ? a.s.v[o] : __builtin_huge_val();
    }
    __syncthreads();
    if (!scan) continue;
    for (int j = 0; j < cnt; ++j) {                      // ascending vertex index; every lane reads the same vertex
      const double du = px - s_u[j], dv = py - s_v[j];
      const double dd = du * du + dv * dv;
      if (dd < best) { best = dd; who = v0 + j; }        // strict: the lowest index keeps an exact tie
    }
  }
  if (p < npix) a.s.nearest[(size_t)b * npix + p] = set ? who : -1;
}

// What vertex i of sample b adds to the inside term: val + out, and its derivative by (u, v).  false: invalid, or a corner of the
// allowed map that says "no set pixel" - the term is 0 with zero gradient.
__device__ __forceinline__ bool inside_term(const SilArgs& a, int b, int i, double* term, double* tu, double* tv) {
#pragma clang fp contract(off)
  const size_t o = (size_t)b * a.V + i;
  const int cell = a.s.cell[o];
  if (cell < 0) return false;
  const int x0 = cell % a.w, y0 = cell / a.w, x1 = min(x0 + 1, a.w - 1), y1 = min(y0 + 1, a.h - 1);
  const int32_t* m = a.d2 + (size_t)b * a.w * a.h;
  const int c00 = m[y0 * a.w + x0], c10 = m[y0 * a.w + x1], c01 = m[y1 * a.w + x0], c11 = m[y1 * a.w + x1];
  if (c00 >= EDT_NONE || c10 >= EDT_NONE || c01 >= EDT_NONE || c11 >= EDT_NONE) return false;
  const double u = a.s.u[o], v = a.s.v[o];
  const double uc = fmin(fmax(u, 0.), (double)(a.w - 1)), vc = fmin(fmax(v, 0.), (double)(a.h - 1));
  const double fx = a.w > 1 ? uc - (double)x0 : 0., fy = a.h > 1 ? vc - (double)y0 : 0.;
  const double d00 = sqrt((double)c00), d10 = sqrt((double)c10), d01 = sqrt((double)c01), d11 = sqrt((double)c11);
  const double val = ((1. - fx) * (1. - fy) * d00 + fx * (1. - fy) * d10) + ((1. - fx) * fy * d01 + fx * fy * d11);
  const double ou = u - uc, ov = v - vc;
  const double out = sqrt(ou * ou + ov * ov);
  *term = val + out;
  double gu = 0., gv = 0.;                               // the bilinear derivative: zero along an axis that was clamped
  if (ou == 0. && a.w > 1) gu = (1. - fy) * (d10 - d00) + fy * (d11 - d01);
  if (ov == 0. && a.h > 1) gv = (1. - fx) * (d01 - d00) + fx * (d11 - d10);
  if (out > 0.) { gu = gu + ou / out; gv = gv + ov / out; }
  *tu = gu; *tv = gv;
  return true;
}

__global__ __launch_bounds__(256) void sil_reduce_kernel(const SilArgs a) {
#pragma clang fp contract(off)
  __shared__ double s[4][256];
  const int b = blockIdx.x, tid = threadIdx.x, npix = a.w * a.h;
  double acc[4] = {0., 0., 0., 0.};                      // inside, cover, and their denominators
  const int n = live_verts(a, b);
  for (int i = tid; i < n; i += 256) {                   // (a row from n on is invalid: it adds nothing)
    const double wt = sil_weight(a, b, i);
    acc[2] = acc[2] + wt;
    double term, tu, tv;
    if (inside_term(a, b, i, &term, &tu, &tv)) acc[0] = acc[0] + wt * term;
  }
  for (int p = tid; p < npix; p += 256) {
    const int i = a.s.nearest[(size_t)b * npix + p];
    if (i < 0) continue;
    const double du = (double)(p % a.w) - a.s.u[(size_t)b * a.V + i], dv = (double)(p / a.w) - a.s.v[(size_t)b * a.V + i];
    acc[1] = acc[1] + sqrt(du * du + dv * dv);
    acc[3] = acc[3] + 1.;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k][tid] = acc[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                    // a fixed tree: s[t] += s[t + o]
    if (tid < o)
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k][tid] = s[k][tid] + s[k][tid + o];
    __syncthreads();
  }
  if (tid != 0) return;
  a.inside[b] = s[2][0] > 0. ? (float)(s[0][0] / s[2][0]) : 0.f;
  a.cover_out[b] = s[3][0] > 0. ? (float)(s[1][0] / s[3][0]) : 0.f;
  a.s.den[(size_t)b * 2] = s[2][0];
  a.s.den[(size_t)b * 2 + 1] = s[3][0];
}

__global__ __launch_bounds__(SIL_TILE) void sil_bwd_kernel(const SilArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_gu[SIL_TILE], s_gv[SIL_TILE];
  __shared__ int s_i[SIL_TILE];
  const int b = blockIdx.y, lane = threadIdx.x, me = blockIdx.x * SIL_TILE + lane, npix = a.w * a.h;
  const size_t o = (size_t)b * a.V + min(me, a.V - 1);
  const bool valid = me < a.V && a.s.cell[o] >= 0;
  const double den = a.s.den[(size_t)b * 2], n_pix = a.s.den[(size_t)b * 2 + 1];
  double acc_u = 0., acc_v = 0.;
  if (valid && a.g_inside && den > 0.) {                 // its own term first
    double term, tu, tv;
    if (inside_term(a, b, me, &term, &tu, &tv)) {
      const double coef = (double)a.g_inside[b] * sil_weight(a, b, me) / den;
      acc_u = coef * tu; acc_v = coef * tv;
    }
  }
  if (a.g_cover && n_pix > 0.) {
    const double c = (double)a.g_cover[b] / n_pix;
    for (int t0 = 0; t0 < npix; t0 += SIL_TILE) {
      const int p = t0 + lane;
      int i = p < npix ? a.s.nearest[(size_t)b * npix + p] : -1;
      double gu = 0., gv = 0.;
      if (i >= 0) {
        const double du = a.s.u[(size_t)b * a.V + i] - (double)(p % a.w), dv = a.s.v[(size_t)b * a.V + i] - (double)(p / a.w);
        const double dd = du * du + dv * dv;
        if (dd > 0.) { const double sq = sqrt(dd); gu = c * du / sq; gv = c * dv / sq; }
        else i = -1;                                     // the pixel sits on its vertex: no direction, nothing to add
      }
      if (__ballot(i >= 0) == 0ull) continue;            // a tile without a record (the block is one wave: the same for every lane)
      __syncthreads();
      s_i[lane] = i; s_gu[lane] = gu; s_gv[lane] = gv;
      __syncthreads();
      const int cnt = min(SIL_TILE, npix - t0);
      for (int j = 0; j < cnt; ++j)                      // ascending pixel index; every lane reads the same record
        if (s_i[j] == me) { acc_u = acc_u + s_gu[j]; acc_v = acc_v + s_gv[j]; }
    }
  }
  if (me >= a.V) return;
  float* d = a.d_verts + o * 3;
  if (!valid) { d[0] = d[1] = d[2] = 0.f; return; }
  const float* K = a.K + (size_t)b * 6;
  const double z = (double)a.verts[o * 3 + 2], u = a.s.u[o], v = a.s.v[o];
  d[0] = (float)(acc_u * ((double)K[0] / z) + acc_v * ((double)K[3] / z));
  d[1] = (float)(acc_u * ((double)K[1] / z) + acc_v * ((double)K[4] / z));
  d[2] = (float)(acc_u * (((double)K[2] - u) / z) + acc_v * (((double)K[5] - v) / z));
}

static bool sil_shape_ok(const char* what, int B, int V, int w, int h) {
  if (B < 0 || B > 65535) { set_error("%s: B=%d (0 .. 65535)", what, B); return false; }
  if (V < 1) { set_error("%s: V=%d (>= 1)", what, V); return false; }
  if (w < 1 || w > EDT_MAX || h < 1 || h > EDT_MAX) { set_error("%s: w=%d h=%d (1 .. %d)", what, w, h, EDT_MAX); return false; }
  return true;
}

// every check the two entries share, before any launch, and the workspace laid out into a->s; > 0: B = 0, nothing to do
static int sil_check(const char* what, SilArgs* a, int B, const void* workspace, long workspace_bytes) {
  if (!sil_shape_ok(what, B, a->V, a->w, a->h)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(a->near > 0.f && a->near <= 3.4028234664e38f, HOISDF_ERR_INVALID, "%s: near=%g (finite, > 0)", what, (double)a->near);
  HOISDF_REQUIRE(a->weight_stride == 0 || a->weight_stride == a->V, HOISDF_ERR_INVALID, "%s: weight_stride=%ld (0 or V)", what,
                 a->weight_stride);
  if (B == 0) return 1;
  HOISDF_REQUIRE(a->verts, HOISDF_ERR_INVALID, "%s: null pointer (verts)", what);
  HOISDF_REQUIRE(a->K, HOISDF_ERR_INVALID, "%s: null pointer (K)", what);
  HOISDF_REQUIRE(a->d2, HOISDF_ERR_INVALID, "%s: null pointer (allow_d2)", what);
  HOISDF_REQUIRE(a->cover, HOISDF_ERR_INVALID, "%s: null pointer (cover)", what);
  HOISDF_REQUIRE(workspace, HOISDF_ERR_INVALID, "%s: null pointer (workspace)", what);
  Bump bump(const_cast<void*>(workspace), workspace_bytes);
  a->s = sil_workspace(bump, B, a->V, (long)a->w * a->h);
  HOISDF_REQUIRE(workspace_bytes >= bump.bytes(), HOISDF_ERR_INVALID, "%s: workspace of %ld bytes, %ld needed", what, workspace_bytes,
                 bump.bytes());
  return 0;
}

}  // namespace hoisdf

using namespace hoisdf;

extern "C" int hoisdf_mask_edt(const float* mask, const float* mask_or, int B, int w, int h, int32_t* d2_out, int32_t* nearest_out,
                               void* stream) {
  HOISDF_REQUIRE(B >= 0 && B <= 65535, HOISDF_ERR_INVALID, "mask_edt: B=%d (0 .. 65535)", B);
  HOISDF_REQUIRE(w >= 1 && w <= EDT_MAX && h >= 1 && h <= EDT_MAX, HOISDF_ERR_INVALID, "mask_edt: w=%d h=%d (1 .. %d)", w, h, EDT_MAX);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(mask, HOISDF_ERR_INVALID, "mask_edt: null pointer (mask)");
  HOISDF_REQUIRE(d2_out, HOISDF_ERR_INVALID, "mask_edt: null pointer (d2_out)");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(edt_columns_kernel, dim3(cdiv(w, 64), B), dim3(64), 0, st, mask, mask_or, w, h, d2_out);
  hipLaunchKernelGGL(edt_rows_kernel, dim3(h, B), dim3(cdiv(w, 64) * 64), 0, st, w, h, d2_out, nearest_out);
  return check_launch("mask_edt");
}

extern "C" long hoisdf_silhouette_loss_workspace_bytes(int B, int V, int w, int h) {
  if (!sil_shape_ok("silhouette_loss_workspace_bytes", B, V, w, h)) return -1;
  Bump bump(nullptr, 0);
  sil_workspace(bump, B, V, (long)w * h);
  return bump.bytes();
}

extern "C" int hoisdf_silhouette_loss_fwd(const float* verts, const int32_t* n_verts, int V, const float* K, int B,
                                          const int32_t* allow_d2, const float* cover, int w, int h, float near, const float* weight,
                                          long weight_stride, float* inside, float* cover_out, void* workspace, long workspace_bytes,
                                          void* stream) {
  SilArgs a = {verts, n_verts, V, K, allow_d2, cover, w, h, near, weight, weight_stride, {}, inside, cover_out, nullptr, nullptr, nullptr};
  const int rc = sil_check("silhouette_loss_fwd", &a, B, workspace, workspace_bytes);
  if (rc != 0) return rc > 0 ? HOISDF_OK : rc;
  HOISDF_REQUIRE(inside && cover_out, HOISDF_ERR_INVALID, "silhouette_loss_fwd: null pointer (inside, cover_out)");
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(sil_project_kernel, dim3(cdiv(V, 256), B), dim3(256), 0, st, a);
  hipLaunchKernelGGL(sil_nearest_kernel, dim3(cdiv((long)w * h, 256), B), dim3(256), 0, st, a);
  hipLaunchKernelGGL(sil_reduce_kernel, dim3(B), dim3(256), 0, st, a);
  return check_launch("silhouette_loss_fwd");
}

extern "C" int hoisdf_silhouette_loss_bwd(const float* verts, const int32_t* n_verts, int V, const float* K, int B,
                                          const int32_t* allow_d2, const float* cover, int w, int h, float near, const float* weight,
                                          long weight_stride, const float* g_inside, const float* g_cover, float* d_verts,
                                          const void* workspace, long workspace_bytes, void* stream) {
  SilArgs a = {verts, n_verts, V, K, allow_d2, cover, w, h, near, weight, weight_stride, {}, nullptr, nullptr, g_inside, g_cover, d_verts};
  const int rc = sil_check("silhouette_loss_bwd", &a, B, workspace, workspace_bytes);
  if (rc != 0) return rc > 0 ? HOISDF_OK : rc;
  HOISDF_REQUIRE(d_verts, HOISDF_ERR_INVALID, "silhouette_loss_bwd: null pointer (d_verts)");
  hipLaunchKernelGGL(sil_bwd_kernel, dim3(cdiv(V, SIL_TILE), B), dim3(SIL_TILE), 0, as_stream(stream), a);
  return check_launch("silhouette_loss_bwd");
}
