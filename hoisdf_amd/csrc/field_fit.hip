// Rigid pose refinement against a sampled signed-distance field (include/hoisdf.h "field fit"): the predicted points move, as a
// rigid body, onto the zero level set of the field the network predicts - a damped Gauss-Newton fit per sample, fp64 on the f32
// inputs, by the rules of hoisdf_amd/field_fit_oracle.py.  The rules themselves (per-point term, solve, accept, stop) are
// field_fit_rules.h, which a host program compiles too; this file is the summation order and the launches.
//   ff_init_kernel    pivot and extent, the sums of the start pose, lane 0: the state and the first plan
//   ff_round_kernel   x iters: the sums at the trial pose, lane 0: accept / reject and the next plan
//   ff_finish_kernel  the posed points and the f32 outputs, each rounded once from fp64
// One workgroup of 256 lanes per sample; the state of a sample (FFState) lives in the workspace between the launches.  The
// iteration over steps is the HOST's: a fixed sequence of iters + 2 launches, nothing synchronises.  A sample that has stopped
// costs a launch slot and one scalar load per remaining round: every lane reads the status word, makes it scalar and returns before
// any barrier.  NO KERNEL HERE HAS A BARRIER INSIDE A LOOP (tests/test_field_fit_codegen.py reads the assembly): the loops - the point
// stride, lane 0's lambda loop, the Cholesky loops - are barrier-free, every __syncthreads() stands in straight-line code that all
// 256 lanes reach, and lane 0's serial work of a launch is ONE block after the last barrier.  A one-launch form with the step loop
// in the kernel once had its barrier threaded into a loop that 63 lanes of wave 0 ran while lane 0 waited outside it.
// Reduction order = the oracle's: lane l takes points l, l + 256, ... ascending; xor tree over 32, 16, 8, 4, 2, 1 within a wave;
// the four wave results through LDS; ((w0 + w1) + w2) + w3.
#include "common.h"

#pragma clang fp contract(off)            // the Makefile builds with -ffp-contract=on: here every product and sum rounds on its own
#define FF_FN __device__ __forceinline__
#include "field_fit_rules.h"

namespace hoisdf {

constexpr int FF_T = 256;                 // lanes per workgroup: the summation order of the rules
constexpr int FF_OUT = 2 * FF_TERMS;      // normal_out: the 28 sums, then their 28 magnitude sums

struct FFArgs {
  const float* values; long ld;           // [B][ld], ld >= n^3
  const float* grid;                      // [B][8]
  const float* points; int V;             // [B][V][3]
  const int32_t* n_points;                // [B] or null = V
  const float* pivot;                     // [B][3] or null = the mean
  FFParams p;
  FFState* state;                         // [B]
  float *rot, *trans, *points_out;
  double* cost; int32_t* info;
  double *normal_out, *pose64_out;        // optional
};

__device__ __forceinline__ int ff_count(const FFArgs& a, int b) {
  const int nv = a.n_points ? a.n_points[b] : a.V;
  return nv < 0 ? 0 : (nv > a.V ? a.V : nv);
}

__device__ __forceinline__ double ff_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}

// this lane's part of the sums of pose (R, t) about c over the sample's nv points (no barrier in here)
template <bool ABS>
__device__ __forceinline__ void ff_lane_sums(const FFArgs& a, int b, int nv, const double* R, const double* t, const double* c,
                                             double* acc, double* acc_abs, int* used) {
  const float* val = a.values + (size_t)b * a.ld;
  const float* grid = a.grid + (size_t)b * 8;
  const float* pts = a.points + (size_t)b * a.V * 3;
#pragma unroll
  for (int k = 0; k < FF_TERMS; ++k) { acc[k] = 0.0; if (ABS) acc_abs[k] = 0.0; }
  *used = 0;
  for (int i = threadIdx.x; i < nv; i += FF_T) {
    const double p[3] = {(double)pts[(size_t)i * 3], (double)pts[(size_t)i * 3 + 1], (double)pts[(size_t)i * 3 + 2]};
    double term[FF_TERMS];
    if (!ff_point_terms(val, grid, a.p.n, R, t, c, p, a.p.huber, term)) continue;
    *used += 1;
#pragma unroll
    for (int k = 0; k < FF_TERMS; ++k) { acc[k] = acc[k] + term[k]; if (ABS) acc_abs[k] = acc_abs[k] + fabs(term[k]); }
  }
}

// xor tree within the wave, lane 0 of each wave -> its row of LDS.  The caller's __syncthreads() follows.
template <int N>
__device__ __forceinline__ void ff_wave_rows(const double* acc, double (*red)[N], int col0, int n) {
#pragma unroll
  for (int k = 0; k < n; ++k) {
    const double v = ff_wave_sum(acc[k]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][col0 + k] = v;
  }
}

__global__ __launch_bounds__(FF_T) void ff_init_kernel(const FFArgs a) {
  __shared__ double s_c[4][3];
  __shared__ double s_red[4][FF_OUT];
  __shared__ double s_ext[4];
  __shared__ int s_used[4];
  const int b = blockIdx.x, tid = threadIdx.x, nv = ff_count(a, b);
  const float* pts = a.points + (size_t)b * a.V * 3;
  // the pivot: the given one, or the mean in the order of the sums
  double m[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < nv; i += FF_T) {
#pragma unroll
    for (int k = 0; k < 3; ++k) m[k] = m[k] + (double)pts[(size_t)i * 3 + k];
  }
  ff_wave_rows<3>(m, s_c, 0, 3);
  __syncthreads();
  // (branch-free: without a pivot the three loads read the sample's grid row, which is always there, and the select drops them)
  const float* given = a.pivot ? a.pivot + (size_t)b * 3 : a.grid + (size_t)b * 8;
  double c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double mean = (((s_c[0][k] + s_c[1][k]) + s_c[2][k]) + s_c[3][k]) / (double)(nv > 1 ? nv : 1);
    const double g = (double)given[k];
    c[k] = a.pivot ? g : mean;
  }
  // the extent (a NaN counts as 0) and the sums of the start pose
  double ext = 0.0;
  for (int i = tid; i < nv; i += FF_T) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double q = fabs((double)pts[(size_t)i * 3 + k] - c[k]);
      ext = q > ext ? q : ext;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { const double y = __shfl_xor(ext, o, 64); ext = y > ext ? y : ext; }
  const double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  double acc[FF_TERMS], acc_abs[FF_TERMS];
  int used;
  ff_lane_sums<true>(a, b, nv, R, t, c, acc, acc_abs, &used);
  ff_wave_rows<FF_OUT>(acc, s_red, 0, FF_TERMS);
  ff_wave_rows<FF_OUT>(acc_abs, s_red, FF_TERMS, FF_TERMS);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o, 64);
  if ((tid & 63) == 0) { s_used[tid >> 6] = used; s_ext[tid >> 6] = ext; }
  __syncthreads();
  if (tid != 0) return;
  // lane 0: everything serial, in one block
  FFState* s = a.state + b;
  double sums[FF_TERMS];
#pragma unroll
  for (int k = 0; k < FF_TERMS; ++k) sums[k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
  const int n0 = s_used[0] + s_used[1] + s_used[2] + s_used[3];
  double e = s_ext[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) e = s_ext[w] > e ? s_ext[w] : e;
#pragma unroll
  for (int k = 0; k < 3; ++k) s->c[k] = c[k];
  s->extent = e;
  ff_start(s, &a.p, sums, n0);
  if (a.normal_out) {
    double* o = a.normal_out + (size_t)b * FF_OUT;
    const double div = (double)(n0 > 1 ? n0 : 1);
#pragma unroll
    for (int k = 0; k < FF_TERMS; ++k) {
      const double sa = ((s_red[0][FF_TERMS + k] + s_red[1][FF_TERMS + k]) + s_red[2][FF_TERMS + k]) + s_red[3][FF_TERMS + k];
      o[k] = n0 ? sums[k] : 0.0;
      o[FF_TERMS + k] = n0 ? sa / div : 0.0;
    }
  }
}

__global__ __launch_bounds__(FF_T) void ff_round_kernel(const FFArgs a) {
  __shared__ double s_red[4][FF_TERMS];
  __shared__ int s_used[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  FFState* s = a.state + b;
  // the same word for every lane of the workgroup, and nobody writes it before the barrier below: a stopped sample leaves whole
  if (__builtin_amdgcn_readfirstlane(s->status) != FF_ACTIVE) return;
  const int nv = ff_count(a, b);
  double R[9], t[3], c[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = s->R1[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { t[k] = s->t1[k]; c[k] = s->c[k]; }
  double acc[FF_TERMS];
  int used;
  ff_lane_sums<false>(a, b, nv, R, t, c, acc, nullptr, &used);
  ff_wave_rows<FF_TERMS>(acc, s_red, 0, FF_TERMS);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) used += __shfl_xor(used, o, 64);
  if ((tid & 63) == 0) s_used[tid >> 6] = used;
  __syncthreads();
  if (tid != 0) return;
  double sums[FF_TERMS];
#pragma unroll
  for (int k = 0; k < FF_TERMS; ++k) sums[k] = ((s_red[0][k] + s_red[1][k]) + s_red[2][k]) + s_red[3][k];
  ff_decide(s, &a.p, sums, s_used[0] + s_used[1] + s_used[2] + s_used[3]);
}

__global__ __launch_bounds__(FF_T) void ff_finish_kernel(const FFArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nv = ff_count(a, b);
  const FFState* s = a.state + b;
  double R[9], t[3], c[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = s->R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) { t[k] = s->t[k]; c[k] = s->c[k]; }
  if (a.points_out) {
    const float* pts = a.points + (size_t)b * a.V * 3;
    float* out = a.points_out + (size_t)b * a.V * 3;
    for (int i = tid; i < nv; i += FF_T) {
      const double p[3] = {(double)pts[(size_t)i * 3], (double)pts[(size_t)i * 3 + 1], (double)pts[(size_t)i * 3 + 2]};
      double rq[3], x[3];
      ff_pose(R, t, c, p, rq, x);
#pragma unroll
      for (int k = 0; k < 3; ++k) out[(size_t)i * 3 + k] = (float)x[k];
    }
  }
  if (tid != 0) return;
  const bool empty = s->status == FF_EMPTY;
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    a.rot[(size_t)b * 9 + k] = (float)R[k];
    if (a.pose64_out) a.pose64_out[(size_t)b * 12 + k] = R[k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    a.trans[(size_t)b * 3 + k] = (float)t[k];
    if (a.pose64_out) a.pose64_out[(size_t)b * 12 + 9 + k] = t[k];
  }
  a.cost[(size_t)b * 2] = empty ? 0.0 : s->cost0;
  a.cost[(size_t)b * 2 + 1] = empty ? 0.0 : s->sums[27];
  a.info[(size_t)b * 4] = s->n0;
  a.info[(size_t)b * 4 + 1] = s->n_used;
  a.info[(size_t)b * 4 + 2] = s->tried;
  a.info[(size_t)b * 4 + 3] = s->accepted;
}

static bool ff_batch_ok(const char* what, int B) {
  if (B < 0 || B > 65535) {
    set_error("%s: B=%d (0 .. 65535)", what, B);
    return false;
  }
  return true;
}

}  // namespace hoisdf

using namespace hoisdf;

extern "C" long hoisdf_field_fit_workspace_bytes(int B) {
  if (!ff_batch_ok("field_fit_workspace_bytes", B)) return -1;
  Bump w(nullptr, 0);
  w.take((long)B * (long)sizeof(FFState));
  return w.bytes();
}

extern "C" int hoisdf_field_fit_launch_count(int iters) {
  if (iters < 0 || iters > HOISDF_FIELD_FIT_MAX_ITERS) {
    set_error("field_fit_launch_count: iters=%d (0 .. %d)", iters, HOISDF_FIELD_FIT_MAX_ITERS);
    return -1;
  }
  return iters + 2;
}

extern "C" int hoisdf_field_fit(const float* values, long ld, const float* grid, int n, const float* points, int V,
                                const int32_t* n_points, const float* pivot, int B, int iters, float huber, float lambda0,
                                float step_tol, int min_used_percent, float* rot, float* trans, float* points_out, double* cost,
                                int32_t* info, double* normal_out, double* pose64_out, void* workspace, long workspace_bytes,
                                void* stream) {
  if (!ff_batch_ok("field_fit", B)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(n >= 2 && n <= HOISDF_ISO_MAX_GRID, HOISDF_ERR_INVALID, "field_fit: n=%d (2 .. %d)", n, HOISDF_ISO_MAX_GRID);
  HOISDF_REQUIRE(iters >= 0 && iters <= HOISDF_FIELD_FIT_MAX_ITERS, HOISDF_ERR_INVALID, "field_fit: iters=%d (0 .. %d)", iters,
                 HOISDF_FIELD_FIT_MAX_ITERS);
  HOISDF_REQUIRE(ld >= (long)n * n * n, HOISDF_ERR_INVALID, "field_fit: ld=%ld (>= n^3 = %ld)", ld, (long)n * n * n);
  HOISDF_REQUIRE(V >= 0 && V <= (1 << 24), HOISDF_ERR_INVALID, "field_fit: V=%d (0 .. 2^24)", V);
  HOISDF_REQUIRE(huber > 0.f, HOISDF_ERR_INVALID, "field_fit: huber=%g (> 0)", (double)huber);
  HOISDF_REQUIRE(lambda0 >= 0.f && step_tol >= 0.f, HOISDF_ERR_INVALID, "field_fit: lambda0=%g step_tol=%g (>= 0)", (double)lambda0,
                 (double)step_tol);
  HOISDF_REQUIRE(min_used_percent >= 0 && min_used_percent <= 100, HOISDF_ERR_INVALID, "field_fit: min_used_percent=%d (0 .. 100)",
                 min_used_percent);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(values && grid && (V == 0 || points), HOISDF_ERR_INVALID, "field_fit: null pointer (values, grid, points)");
  HOISDF_REQUIRE(rot && trans && cost && info && (V == 0 || points_out), HOISDF_ERR_INVALID,
                 "field_fit: null pointer (rot, trans, points_out, cost, info)");
  HOISDF_REQUIRE(workspace, HOISDF_ERR_INVALID, "field_fit: null pointer (workspace)");
  HOISDF_REQUIRE(((uintptr_t)workspace & 7) == 0, HOISDF_ERR_INVALID, "field_fit: workspace %p is not aligned to 8 bytes", workspace);
  Bump w(workspace, workspace_bytes);
  FFState* state = (FFState*)w.take((long)B * (long)sizeof(FFState));
  HOISDF_REQUIRE(workspace_bytes >= w.bytes(), HOISDF_ERR_INVALID, "field_fit: workspace of %ld bytes, %ld needed", workspace_bytes, w.bytes());
  FFArgs a;
  a.values = values; a.ld = ld; a.grid = grid;
  a.points = points; a.V = V; a.n_points = n_points; a.pivot = pivot;
  a.p.n = n; a.p.iters = iters; a.p.min_used_percent = min_used_percent;
  a.p.huber = (double)huber; a.p.lambda0 = (double)lambda0; a.p.step_tol = (double)step_tol;
  a.state = state;
  a.rot = rot; a.trans = trans; a.points_out = points_out; a.cost = cost; a.info = info;
  a.normal_out = normal_out; a.pose64_out = pose64_out;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(ff_init_kernel, dim3(B), dim3(FF_T), 0, st, a);
  for (int r = 0; r < iters; ++r) hipLaunchKernelGGL(ff_round_kernel, dim3(B), dim3(FF_T), 0, st, a);
  hipLaunchKernelGGL(ff_finish_kernel, dim3(B), dim3(FF_T), 0, st, a);
  return check_launch("field_fit");
}
