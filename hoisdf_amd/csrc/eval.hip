// Evaluation metrics of the reference's test driver (main/test.py:65-261 over common/metrics.py:62-232 and common/eval_util.py:11-136)
// as HIP kernels behind the hoisdf_eval_* entries: a C host turns predictions into the numbers of results.txt without PyTorch.
//
//   align_kernel        one workgroup per sample: similarity (Procrustes) alignment of n points in fp64 - centroids, H = (A-ca)^T (B-cb)/n
//                       and varP from the fp32 inputs, a one-sided Jacobi SVD of the 3x3 H in ONE thread, the reference's reflection rule
//                       (det(V U^T) < 0: last singular value and last row of V^T negated) - then the aligned points as fp32, the per-point
//                       distances before and after, and their per-sample means (MJE / PA-MJE for 21 joints; 778 vertices for the mesh).
//   nn_kernel           the nearest-neighbour pass.  Grid = (query chunk of 256, direction / cloud pair, sample).  A thread keeps one query
//                       point in registers, the other cloud streams through LDS in SoA tiles of 256 (every lane reads the same address:
//                       broadcast, no bank conflict), the minimum is kept SQUARED (dx^2 + dy^2 + dz^2 directly - no |a|^2 + |b|^2 - 2ab)
//                       and the root taken once.  The object form transforms the template on the fly (no transformed copy in memory).
//   object_finish / mesh_finish   one workgroup per sample reduce the per-query distances in a fixed order: ADD-S, MCE, OCE, MME; integer
//                       counts below each threshold -> F-scores.
//   accum_feed / accum_finish     EvalUtil.feed / get_measures for fully visible meshes: fp64 sum per vertex (one thread owns a vertex
//                       and walks the samples of a call in order) and u32 counts per (threshold, vertex).
// No float atomics anywhere; every floating-point sum has one fixed order (xor-shuffle tree in a wave, then the waves in order), so two
// calls give the same bits and a set of samples fed in pieces gives the bits of one feed.
#include "common.h"

namespace hoisdf {
namespace {

constexpr int ENT = 256, ENW = ENT / 64;     // threads / waves of every workgroup here; also the query chunk and the LDS tile of the pass
constexpr int EVAL_MAX_THRESH = 16;          // F-score thresholds of one call
constexpr float FAR = 1e18f;                 // padding of a partial tile: (q - FAR)^2 is finite and never the minimum

// ---- fixed-order workgroup reductions; red: ENW * N shared values; the result is in every thread ------------------------------------
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double* red) {
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[n] += __shfl_xor(v[n], o, 64);
  __syncthreads();                                            // red may still be read from an earlier reduction
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int n = 0; n < N; ++n) red[(threadIdx.x >> 6) * N + n] = v[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = ((red[n] + red[N + n]) + red[2 * N + n]) + red[3 * N + n];
}
template <int N>
__device__ __forceinline__ void block_max(float (&v)[N], float* red) {
#pragma unroll
  for (int n = 0; n < N; ++n)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[n] = fmaxf(v[n], __shfl_xor(v[n], o, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int n = 0; n < N; ++n) red[(threadIdx.x >> 6) * N + n] = v[n];
  __syncthreads();
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = fmaxf(fmaxf(red[n], red[N + n]), fmaxf(red[2 * N + n], red[3 * N + n]));
}
static_assert(ENW == 4, "the reductions above sum four waves");

__device__ __forceinline__ float dist3(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrtf(dx * dx + dy * dy + dz * dz);
}

// ---- object pose ---------------------------------------------------------------------------------------------------------------------
struct ObjArgs {
  const float* rot; const float* trans; int P;        // [B][P][3] per-point predictions (axis-angle, translation)
  const float* rot_gt; const float* trans_gt;         // [B][3]
  const float* templates; int T, V;                   // [T][V][3]
  const int32_t* ids; int B;                          // [B]; outside [0, T): the sample is not evaluated
  float *adds, *mce, *oce, *mme; int32_t* used;       // [B] each
  float* nn;                                          // workspace [B][V]: pred vertex -> nearest target vertex
};
struct Pose { float Rp[9], tp[3], Rg[9], tg[3], oce; };

// metrics.batch_rodrigues (the quaternion form of manopth's rodrigues_layer, |aa + 1e-8|), in fp64
__device__ void rodrigues(const double* aa, float* R) {
  const double ex = aa[0] + 1e-8, ey = aa[1] + 1e-8, ez = aa[2] + 1e-8;
  const double ang = sqrt(ex * ex + ey * ey + ez * ez), h = 0.5 * ang, sh = sin(h) / ang;
  double w = cos(h), x = sh * aa[0], y = sh * aa[1], z = sh * aa[2];
  const double qn = 1.0 / sqrt(w * w + x * x + y * y + z * z);
  w *= qn; x *= qn; y *= qn; z *= qn;
  R[0] = (float)(w * w + x * x - y * y - z * z); R[1] = (float)(2 * x * y - 2 * w * z); R[2] = (float)(2 * w * y + 2 * x * z);
  R[3] = (float)(2 * w * z + 2 * x * y); R[4] = (float)(w * w - x * x + y * y - z * z); R[5] = (float)(2 * y * z - 2 * w * x);
  R[6] = (float)(2 * x * z - 2 * w * y); R[7] = (float)(2 * w * x + 2 * y * z); R[8] = (float)(w * w - x * x - y * y + z * z);
}
// mean over the P per-point predictions (fp64, fixed order) -> both poses of sample b, the same bits in every workgroup that asks
__device__ void object_pose(const ObjArgs& a, int b, double* red, Pose* out) {
  double s[6] = {0, 0, 0, 0, 0, 0};
  const float* r = a.rot + (long)b * a.P * 3;
  const float* t = a.trans + (long)b * a.P * 3;
  for (int p = threadIdx.x; p < a.P; p += ENT)
#pragma unroll
    for (int c = 0; c < 3; ++c) { s[c] += (double)r[p * 3 + c]; s[3 + c] += (double)t[p * 3 + c]; }
  block_sum<6>(s, red);
  if (threadIdx.x == 0) {
    double g[3], o = 0;
#pragma unroll
    for (int c = 0; c < 6; ++c) s[c] /= (double)a.P;
    rodrigues(s, out->Rp);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      g[c] = (double)a.rot_gt[b * 3 + c];
      out->tp[c] = (float)s[3 + c];
      out->tg[c] = a.trans_gt[b * 3 + c];
      const double d = s[3 + c] - (double)a.trans_gt[b * 3 + c];
      o += d * d;
    }
    rodrigues(g, out->Rg);
    out->oce = (float)sqrt(o);
  }
  __syncthreads();
}
__device__ __forceinline__ void xform(const float* R, const float* t, const float* v, float& x, float& y, float& z) {
  x = fmaf(R[2], v[2], fmaf(R[1], v[1], R[0] * v[0])) + t[0];
  y = fmaf(R[5], v[2], fmaf(R[4], v[1], R[3] * v[0])) + t[1];
  z = fmaf(R[8], v[2], fmaf(R[7], v[1], R[6] * v[0])) + t[2];
}

// ---- nearest neighbours --------------------------------------------------------------------------------------------------------------
struct MeshArgs {
  const float* pred; const float* gt; const float* aligned;    // [B][V][3] each
  int V, B;
  const double* thresholds; int n_thresh;
  float *fscore, *fscore_aligned;                              // [B][n_thresh]
  float* nn;                                                   // workspace [4][B][V]: gt->pred, pred->gt, gt->aligned, aligned->gt
};

template <bool OBJ, typename A>
__global__ __launch_bounds__(ENT) void nn_kernel(const A a) {
  __shared__ __attribute__((aligned(16))) float tile[3][ENT];
  __shared__ double red[ENW * 6];
  __shared__ Pose pose;
  const int b = blockIdx.z, combo = blockIdx.y, tid = threadIdx.x, V = a.V;
  const int i = blockIdx.x * ENT + tid;
  const float *qsrc, *ssrc;
  if constexpr (OBJ) {
    const int id = a.ids[b];
    if (id < 0 || id >= a.T) return;                           // the whole workgroup: not evaluated
    object_pose(a, b, red, &pose);
    qsrc = ssrc = a.templates + (long)id * V * 3;
  } else {
    const float* other = combo < 2 ? a.pred : a.aligned;
    qsrc = ((combo & 1) ? other : a.gt) + (long)b * V * 3;
    ssrc = ((combo & 1) ? a.gt : other) + (long)b * V * 3;
  }
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (i < V) {
    if constexpr (OBJ) xform(pose.Rp, pose.tp, qsrc + (long)i * 3, qx, qy, qz);
    else { qx = qsrc[(long)i * 3]; qy = qsrc[(long)i * 3 + 1]; qz = qsrc[(long)i * 3 + 2]; }
  }
  float best = INFINITY;
  for (int j0 = 0; j0 < V; j0 += ENT) {
    __syncthreads();                                           // the previous tile has been read
    const int j = j0 + tid;
    float x = FAR, y = FAR, z = FAR;
    if (j < V) {
      if constexpr (OBJ) xform(pose.Rg, pose.tg, ssrc + (long)j * 3, x, y, z);
      else { x = ssrc[(long)j * 3]; y = ssrc[(long)j * 3 + 1]; z = ssrc[(long)j * 3 + 2]; }
    }
    tile[0][tid] = x; tile[1][tid] = y; tile[2][tid] = z;
    __syncthreads();
    const int n = min(ENT, (V - j0 + 3) & ~3);                 // whole float4 groups; the tail of a group is FAR
    for (int k = 0; k < n; k += 4) {
      const float4 X = *reinterpret_cast<const float4*>(&tile[0][k]);
      const float4 Y = *reinterpret_cast<const float4*>(&tile[1][k]);
      const float4 Z = *reinterpret_cast<const float4*>(&tile[2][k]);
#define HOISDF_NN_STEP(c) { const float dx = qx - X.c, dy = qy - Y.c, dz = qz - Z.c; best = fminf(best, fmaf(dz, dz, fmaf(dy, dy, dx * dx))); }
      HOISDF_NN_STEP(x) HOISDF_NN_STEP(y) HOISDF_NN_STEP(z) HOISDF_NN_STEP(w)
#undef HOISDF_NN_STEP
    }
  }
  if (i < V) a.nn[((long)combo * a.B + b) * V + i] = sqrtf(best);
}

// ---- object metrics of one sample ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ENT) void object_finish_kernel(const ObjArgs a) {
  __shared__ double red[ENW * 6];
  __shared__ float redf[ENW * 12];
  __shared__ Pose pose;
  const int b = blockIdx.x, tid = threadIdx.x, V = a.V;
  const int id = a.ids[b];
  if (id < 0 || id >= a.T) {
    if (tid == 0) { a.adds[b] = 0.f; a.mce[b] = 0.f; a.oce[b] = 0.f; a.mme[b] = 0.f; a.used[b] = 0; }
    return;
  }
  object_pose(a, b, red, &pose);
  const float* tpl = a.templates + (long)id * V * 3;
  const float* nn = a.nn + (long)b * V;
  double s[2] = {0, 0};                                       // ADD-S, MME
  float m[12];                                                // max of (-pred, +pred, -target, +target) per axis
#pragma unroll
  for (int c = 0; c < 12; ++c) m[c] = -INFINITY;
  for (int i = tid; i < V; i += ENT) {
    float p[3], g[3];
    xform(pose.Rp, pose.tp, tpl + (long)i * 3, p[0], p[1], p[2]);
    xform(pose.Rg, pose.tg, tpl + (long)i * 3, g[0], g[1], g[2]);
    s[0] += (double)nn[i];
    s[1] += (double)dist3(g[0], g[1], g[2], p[0], p[1], p[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      m[c] = fmaxf(m[c], -p[c]); m[3 + c] = fmaxf(m[3 + c], p[c]);
      m[6 + c] = fmaxf(m[6 + c], -g[c]); m[9 + c] = fmaxf(m[9 + c], g[c]);
    }
  }
  block_sum<2>(s, red);
  block_max<12>(m, redf);
  if (tid == 0) {
    // common/metrics.py:70-72: corner k takes min (0) or max (1) per axis
    const int cx[8] = {0, 1, 0, 0, 1, 0, 1, 1}, cy[8] = {0, 0, 1, 0, 1, 1, 0, 1}, cz[8] = {0, 0, 0, 1, 0, 1, 1, 1};
    double mce = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float px = cx[k] ? m[3] : -m[0], py = cy[k] ? m[4] : -m[1], pz = cz[k] ? m[5] : -m[2];
      const float gx = cx[k] ? m[9] : -m[6], gy = cy[k] ? m[10] : -m[7], gz = cz[k] ? m[11] : -m[8];
      mce += (double)dist3(px, py, pz, gx, gy, gz);
    }
    a.adds[b] = (float)(s[0] / (double)V);
    a.mme[b] = (float)(s[1] / (double)V);
    a.mce[b] = (float)(mce / 8.0);
    a.oce[b] = pose.oce;
    a.used[b] = 1;
  }
}

// ---- F-scores of one sample ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ENT) void mesh_finish_kernel(const MeshArgs a) {
  __shared__ int cnt[EVAL_MAX_THRESH][4];
  const int b = blockIdx.x, tid = threadIdx.x, V = a.V;
  if (tid < EVAL_MAX_THRESH * 4) (&cnt[0][0])[tid] = 0;
  __syncthreads();
  for (int combo = 0; combo < 4; ++combo) {
    const float* nn = a.nn + ((long)combo * a.B + b) * V;
    for (int t = 0; t < a.n_thresh; ++t) {
      const double th = a.thresholds[t];
      int c = 0;
      for (int i = tid; i < V; i += ENT) c += ((double)nn[i] < th) ? 1 : 0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
      if ((tid & 63) == 0) atomicAdd(&cnt[t][combo], c);       // integers: any order, same sum
    }
  }
  __syncthreads();
  if (tid < a.n_thresh) {
    // eval_util.py:117-136: precision = share of gt points with a pred point nearer than th, recall = the other way round
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double pr = (double)cnt[tid][2 * k] / (double)V, rc = (double)cnt[tid][2 * k + 1] / (double)V;
      const float f = pr + rc > 0 ? (float)(2.0 * pr * rc / (pr + rc)) : 0.f;
      (k ? a.fscore_aligned : a.fscore)[(long)b * a.n_thresh + tid] = f;
    }
  }
}

// ---- Procrustes ----------------------------------------------------------------------------------------------------------------------
// One-sided (Hestenes) Jacobi: H J1 J2 ... = U diag(s), V = J1 J2 ...; columns sorted by descending s.  All 3x3 row-major.
__device__ void svd3(const double* H, double* U, double* s, double* V) {
  double A[9];
  for (int k = 0; k < 9; ++k) { A[k] = H[k]; V[k] = (k % 4 == 0) ? 1.0 : 0.0; }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int pq = 0; pq < 3; ++pq) {
      const int p = pq == 2 ? 1 : 0, q = pq == 0 ? 1 : 2;
      double al = 0, be = 0, ga = 0;
      for (int r = 0; r < 3; ++r) { al += A[r * 3 + p] * A[r * 3 + p]; be += A[r * 3 + q] * A[r * 3 + q]; ga += A[r * 3 + p] * A[r * 3 + q]; }
      if (ga == 0.0 || fabs(ga) <= 1e-15 * sqrt(al * be)) continue;      // orthogonal to a few fp64 roundings: 4 to 6 sweeps
      rotated = true;
      const double zeta = (be - al) / (2.0 * ga);
      const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
      for (int r = 0; r < 3; ++r) {
        const double ap = A[r * 3 + p], aq = A[r * 3 + q], vp = V[r * 3 + p], vq = V[r * 3 + q];
        A[r * 3 + p] = c * ap - sn * aq; A[r * 3 + q] = sn * ap + c * aq;
        V[r * 3 + p] = c * vp - sn * vq; V[r * 3 + q] = sn * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  for (int k = 0; k < 3; ++k) s[k] = sqrt(A[k] * A[k] + A[3 + k] * A[3 + k] + A[6 + k] * A[6 + k]);
  for (int pass = 0; pass < 3; ++pass) {                      // descending: compare-swap (0,1) (1,2) (0,1)
    const int p = pass == 1 ? 1 : 0, q = p + 1;
    if (s[p] < s[q]) {
      double tmp = s[p]; s[p] = s[q]; s[q] = tmp;
      for (int r = 0; r < 3; ++r) {
        tmp = A[r * 3 + p]; A[r * 3 + p] = A[r * 3 + q]; A[r * 3 + q] = tmp;
        tmp = V[r * 3 + p]; V[r * 3 + p] = V[r * 3 + q]; V[r * 3 + q] = tmp;
      }
    }
  }
  const double tiny = 1e-14 * s[0];
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) U[r * 3 + k] = s[k] > tiny ? A[r * 3 + k] / s[k] : 0.0;
  // rank-deficient H (degenerate input: all points on a line / in a plane): complete U to a proper frame
  if (!(s[0] > 0.0)) { for (int k = 0; k < 9; ++k) U[k] = (k % 4 == 0) ? 1.0 : 0.0; return; }
  if (!(s[1] > tiny)) {
    const int ax = fabs(U[0]) <= fabs(U[3]) ? (fabs(U[0]) <= fabs(U[6]) ? 0 : 2) : (fabs(U[3]) <= fabs(U[6]) ? 1 : 2);
    double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
    double w[3] = {U[3] * e[2] - U[6] * e[1], U[6] * e[0] - U[0] * e[2], U[0] * e[1] - U[3] * e[0]};
    const double n = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    U[1] = w[0] / n; U[4] = w[1] / n; U[7] = w[2] / n;
  }
  if (!(s[2] > tiny)) {
    U[2] = U[3] * U[7] - U[6] * U[4]; U[5] = U[6] * U[1] - U[0] * U[7]; U[8] = U[0] * U[4] - U[3] * U[1];
  }
}

struct AlignArgs {
  const float* A; const float* Bp; int n, B;         // [B][n][3] each: A is aligned onto Bp
  float* aligned;                                    // [B][n][3] or null
  float *dist_raw, *dist_al;                         // [B][n] or null
  float *mean_raw, *mean_al;                         // [B] or null
  double* transform;                                 // [B][13] = c, R row-major, t; or null
};

__global__ __launch_bounds__(ENT) void align_kernel(const AlignArgs a) {
  __shared__ double red[ENW * 10];
  __shared__ double xf[13];
  const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
  const float* A = a.A + (long)b * n * 3;
  const float* Bp = a.Bp + (long)b * n * 3;
  double c6[6] = {0, 0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += ENT)
#pragma unroll
    for (int c = 0; c < 3; ++c) { c6[c] += (double)A[i * 3 + c]; c6[3 + c] += (double)Bp[i * 3 + c]; }
  block_sum<6>(c6, red);
#pragma unroll
  for (int c = 0; c < 6; ++c) c6[c] /= (double)n;
  double h[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = tid; i < n; i += ENT) {
    double da[3], db[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) { da[c] = (double)A[i * 3 + c] - c6[c]; db[c] = (double)Bp[i * 3 + c] - c6[3 + c]; }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) h[r * 3 + c] += da[r] * db[c];
      h[9] += da[r] * da[r];
    }
  }
  block_sum<10>(h, red);
  if (tid == 0) {
    double H[9], U[9], s[3], V[9], R[9];
    for (int k = 0; k < 9; ++k) H[k] = h[k] / (double)n;
    const double varP = h[9] / (double)n;
    svd3(H, U, s, V);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[i * 3 + j] = V[i * 3] * U[j * 3] + V[i * 3 + 1] * U[j * 3 + 1] + V[i * 3 + 2] * U[j * 3 + 2];
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    if (det < 0) {                                             // common/metrics.py:195-198
      s[2] = -s[2];
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = V[i * 3] * U[j * 3] + V[i * 3 + 1] * U[j * 3 + 1] - V[i * 3 + 2] * U[j * 3 + 2];
    }
    const double c = varP > 0 ? ((s[0] + s[1]) + s[2]) / varP : 0.0;      // all points of A equal: no scale to fit
    xf[0] = c;
    for (int k = 0; k < 9; ++k) xf[1 + k] = R[k];
    for (int r = 0; r < 3; ++r) xf[10 + r] = c6[3 + r] - c * (R[r * 3] * c6[0] + R[r * 3 + 1] * c6[1] + R[r * 3 + 2] * c6[2]);
    if (a.transform)
      for (int k = 0; k < 13; ++k) a.transform[(long)b * 13 + k] = xf[k];
  }
  __syncthreads();
  const double c = xf[0];
  double acc[2] = {0, 0};
  for (int i = tid; i < n; i += ENT) {
    const double x = (double)A[i * 3], y = (double)A[i * 3 + 1], z = (double)A[i * 3 + 2];
    float al[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) al[r] = (float)(c * (xf[1 + r * 3] * x + xf[2 + r * 3] * y + xf[3 + r * 3] * z) + xf[10 + r]);
    const float d0 = dist3(A[i * 3], A[i * 3 + 1], A[i * 3 + 2], Bp[i * 3], Bp[i * 3 + 1], Bp[i * 3 + 2]);
    const float d1 = dist3(al[0], al[1], al[2], Bp[i * 3], Bp[i * 3 + 1], Bp[i * 3 + 2]);
    if (a.aligned) {
#pragma unroll
      for (int r = 0; r < 3; ++r) a.aligned[((long)b * n + i) * 3 + r] = al[r];
    }
    if (a.dist_raw) a.dist_raw[(long)b * n + i] = d0;
    if (a.dist_al) a.dist_al[(long)b * n + i] = d1;
    acc[0] += (double)d0; acc[1] += (double)d1;
  }
  block_sum<2>(acc, red);
  if (tid == 0) {
    if (a.mean_raw) a.mean_raw[b] = (float)(acc[0] / (double)n);
    if (a.mean_al) a.mean_al[b] = (float)(acc[1] / (double)n);
  }
}

// ---- mesh-error accumulator ----------------------------------------------------------------------------------------------------------
// state: u64 samples fed (16 bytes with padding) | double sum[V] | u32 count[steps][V]
constexpr long ACC_HDR = 16;
__host__ __device__ inline long accum_bytes(long V, long steps) { return ACC_HDR + 8 * V + ((4 * steps * V + 7) & ~7L); }
__device__ __forceinline__ double* accum_sums(void* st) { return reinterpret_cast<double*>(reinterpret_cast<char*>(st) + ACC_HDR); }
__device__ __forceinline__ uint32_t* accum_counts(void* st, int V) { return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(st) + ACC_HDR + 8L * V); }

// grid (vertex chunk of 64, threshold): thread (v, t) owns count[t][v]; the threads of t = 0 own sum[v] and walk the samples in order
__global__ __launch_bounds__(64) void accum_feed_kernel(void* state, const float* dist, int B, int V, const double* thresholds) {
  const int v = blockIdx.x * 64 + threadIdx.x, t = blockIdx.y;
  if (v == 0 && t == 0) *reinterpret_cast<unsigned long long*>(state) += (unsigned long long)B;
  if (v >= V) return;
  const double th = thresholds[t];
  uint32_t* cnt = accum_counts(state, V) + (long)t * V + v;
  uint32_t c = *cnt;
  for (int s = 0; s < B; ++s) c += ((double)dist[(long)s * V + v] <= th) ? 1u : 0u;
  *cnt = c;
  if (t == 0) {
    double* sum = accum_sums(state) + v;
    double acc = *sum;
    for (int s = 0; s < B; ++s) acc += (double)dist[(long)s * V + v];
    *sum = acc;
  }
}

// out[0] = mean EPE, out[1] = AUC, out[2 .. 2 + steps) = the PCK curve (EvalUtil.get_measures, :62-103, every keypoint fully visible)
__global__ __launch_bounds__(ENT) void accum_finish_kernel(void* state, int V, const double* thresholds, int steps, double* out) {
  __shared__ double red[ENW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const double n = (double)*reinterpret_cast<const unsigned long long*>(state);
  const double* sum = accum_sums(state);
  const uint32_t* cnt = accum_counts(state, V);
  double e[1] = {0};
  for (int v = tid; v < V; v += ENT) e[0] += sum[v] / n;
  block_sum<1>(e, red);
  if (tid == 0) out[0] = e[0] / (double)V;
  for (int t = w; t < steps; t += ENW) {                       // a wave per threshold: an integer total, any order
    unsigned long long c = 0;
    for (int v = lane; v < V; v += 64) c += cnt[(long)t * V + v];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) out[2 + t] = (double)c / (n * (double)V);
  }
  __syncthreads();
  if (tid == 0) {                                              // trapezoid over the thresholds, normalised by the trapezoid of ones
    double area = 0;
    for (int t = 0; t + 1 < steps; ++t) area += (thresholds[t + 1] - thresholds[t]) * (out[2 + t + 1] + out[2 + t]) * 0.5;
    out[1] = area / (thresholds[steps - 1] - thresholds[0]);
  }
}

int launch_align(const AlignArgs& a, const char* what, void* stream) {
  hipLaunchKernelGGL(align_kernel, dim3((unsigned)a.B), dim3(ENT), 0, as_stream(stream), a);
  return check_launch(what);
}

}  // namespace
}  // namespace hoisdf

using namespace hoisdf;

extern "C" long hoisdf_eval_workspace_bytes(int B, int V) {
  if (B < 0 || V <= 0) { set_error("eval_workspace_bytes: B=%d V=%d", B, V); return -1; }
  return 7L * sizeof(float) * (long)(B > 0 ? B : 1) * V;      // eval_mesh: four distance arrays + the aligned mesh; eval_object: one array
}

extern "C" long hoisdf_eval_accum_state_bytes(int V, int steps) {
  if (V <= 0 || steps < 2 || steps > 65535) { set_error("eval_accum_state_bytes: V=%d steps=%d (2 .. 65535)", V, steps); return -1; }
  return accum_bytes(V, steps);
}

extern "C" int hoisdf_eval_object(const float* obj_rot, const float* obj_trans, int P, const float* obj_rot_gt, const float* obj_trans_gt,
                                  const float* templates, int T, int V, const int32_t* obj_ids, int B, float* adds, float* mce, float* oce,
                                  float* mme, int32_t* used, void* workspace, long workspace_bytes, void* stream) {
  HOISDF_REQUIRE(B >= 0, HOISDF_ERR_INVALID, "eval_object: B=%d", B);
  HOISDF_REQUIRE(P > 0, HOISDF_ERR_INVALID, "eval_object: P=%d (per-point predictions of a sample)", P);
  HOISDF_REQUIRE(T > 0, HOISDF_ERR_INVALID, "eval_object: T=%d (templates)", T);
  HOISDF_REQUIRE(V > 0, HOISDF_ERR_INVALID, "eval_object: V=%d (vertices of a template)", V);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(obj_rot && obj_trans && obj_rot_gt && obj_trans_gt && templates && obj_ids && adds && mce && oce && mme && used && workspace,
                 HOISDF_ERR_INVALID, "eval_object: null pointer");
  HOISDF_REQUIRE(workspace_bytes >= (long)sizeof(float) * B * V, HOISDF_ERR_WORKSPACE,
                 "eval_object: workspace_bytes=%ld, %ld needed (hoisdf_eval_workspace_bytes)", workspace_bytes, (long)sizeof(float) * B * V);
  ObjArgs a{obj_rot, obj_trans, P, obj_rot_gt, obj_trans_gt, templates, T, V, obj_ids, B, adds, mce, oce, mme, used,
            reinterpret_cast<float*>(workspace)};
  hipLaunchKernelGGL((nn_kernel<true, ObjArgs>), dim3((unsigned)cdiv(V, ENT), 1, (unsigned)B), dim3(ENT), 0, as_stream(stream), a);
  if (int rc = check_launch("eval_object (nearest neighbours)")) return rc;
  hipLaunchKernelGGL(object_finish_kernel, dim3((unsigned)B), dim3(ENT), 0, as_stream(stream), a);
  return check_launch("eval_object");
}

extern "C" int hoisdf_eval_hand_joints(const float* pred, const float* gt, int B, int J, float* mje, float* pamje, float* aligned_out,
                                       double* transform_out, float* dist_out, float* dist_aligned_out, void* stream) {
  HOISDF_REQUIRE(B >= 0, HOISDF_ERR_INVALID, "eval_hand_joints: B=%d", B);
  HOISDF_REQUIRE(J > 0, HOISDF_ERR_INVALID, "eval_hand_joints: J=%d (points of a sample)", J);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(pred && gt && mje && pamje, HOISDF_ERR_INVALID, "eval_hand_joints: null pointer");
  AlignArgs a{pred, gt, J, B, aligned_out, dist_out, dist_aligned_out, mje, pamje, transform_out};
  return launch_align(a, "eval_hand_joints", stream);
}

extern "C" int hoisdf_eval_mesh(const float* pred, const float* gt, int B, int V, const double* thresholds, int n_thresh, float* dist_raw,
                                float* dist_aligned, float* fscore, float* fscore_aligned, float* aligned_out, void* workspace,
                                long workspace_bytes, void* stream) {
  HOISDF_REQUIRE(B >= 0, HOISDF_ERR_INVALID, "eval_mesh: B=%d", B);
  HOISDF_REQUIRE(V > 0, HOISDF_ERR_INVALID, "eval_mesh: V=%d (vertices of a mesh)", V);
  HOISDF_REQUIRE(n_thresh >= 1 && n_thresh <= EVAL_MAX_THRESH, HOISDF_ERR_INVALID, "eval_mesh: n_thresh=%d (1 .. %d F-score thresholds)",
                 n_thresh, EVAL_MAX_THRESH);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(pred && gt && thresholds && dist_raw && dist_aligned && fscore && fscore_aligned && workspace, HOISDF_ERR_INVALID,
                 "eval_mesh: null pointer");
  const long nn_bytes = 4L * sizeof(float) * B * V, al_bytes = aligned_out ? 0 : 3L * sizeof(float) * B * V;
  HOISDF_REQUIRE(workspace_bytes >= nn_bytes + al_bytes, HOISDF_ERR_WORKSPACE,
                 "eval_mesh: workspace_bytes=%ld, %ld needed (hoisdf_eval_workspace_bytes)", workspace_bytes, nn_bytes + al_bytes);
  float* nn = reinterpret_cast<float*>(workspace);
  float* aligned = aligned_out ? aligned_out : nn + 4L * B * V;
  AlignArgs al{pred, gt, V, B, aligned, dist_raw, dist_aligned, nullptr, nullptr, nullptr};
  if (int rc = launch_align(al, "eval_mesh (alignment)", stream)) return rc;
  MeshArgs a{pred, gt, aligned, V, B, thresholds, n_thresh, fscore, fscore_aligned, nn};
  hipLaunchKernelGGL((nn_kernel<false, MeshArgs>), dim3((unsigned)cdiv(V, ENT), 4, (unsigned)B), dim3(ENT), 0, as_stream(stream), a);
  if (int rc = check_launch("eval_mesh (nearest neighbours)")) return rc;
  hipLaunchKernelGGL(mesh_finish_kernel, dim3((unsigned)B), dim3(ENT), 0, as_stream(stream), a);
  return check_launch("eval_mesh");
}

extern "C" int hoisdf_eval_accum_init(void* state, int V, int steps, void* stream) {
  HOISDF_REQUIRE(V > 0, HOISDF_ERR_INVALID, "eval_accum_init: V=%d", V);
  HOISDF_REQUIRE(steps >= 2 && steps <= 65535, HOISDF_ERR_INVALID, "eval_accum_init: steps=%d (2 .. 65535; the AUC needs two thresholds)", steps);
  HOISDF_REQUIRE(state, HOISDF_ERR_INVALID, "eval_accum_init: null pointer");
  const hipError_t e = hipMemsetAsync(state, 0, (size_t)accum_bytes(V, steps), as_stream(stream));
  HOISDF_REQUIRE(e == hipSuccess, HOISDF_ERR_LAUNCH, "eval_accum_init: %s", hipGetErrorString(e));
  return HOISDF_OK;
}

extern "C" int hoisdf_eval_accum_feed(void* state, const float* dist, int B, int V, const double* thresholds, int steps, void* stream) {
  HOISDF_REQUIRE(B >= 0, HOISDF_ERR_INVALID, "eval_accum_feed: B=%d", B);
  HOISDF_REQUIRE(V > 0, HOISDF_ERR_INVALID, "eval_accum_feed: V=%d", V);
  HOISDF_REQUIRE(steps >= 2 && steps <= 65535, HOISDF_ERR_INVALID, "eval_accum_feed: steps=%d (2 .. 65535)", steps);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(state && dist && thresholds, HOISDF_ERR_INVALID, "eval_accum_feed: null pointer");
  hipLaunchKernelGGL(accum_feed_kernel, dim3((unsigned)cdiv(V, 64), (unsigned)steps), dim3(64), 0, as_stream(stream), state, dist, B, V, thresholds);
  return check_launch("eval_accum_feed");
}

extern "C" int hoisdf_eval_accum_finish(const void* state, int V, const double* thresholds, int steps, double* out, void* stream) {
  HOISDF_REQUIRE(V > 0, HOISDF_ERR_INVALID, "eval_accum_finish: V=%d", V);
  HOISDF_REQUIRE(steps >= 2 && steps <= 65535, HOISDF_ERR_INVALID, "eval_accum_finish: steps=%d (2 .. 65535)", steps);
  HOISDF_REQUIRE(state && thresholds && out, HOISDF_ERR_INVALID, "eval_accum_finish: null pointer");
  hipLaunchKernelGGL(accum_finish_kernel, dim3(1), dim3(ENT), 0, as_stream(stream), const_cast<void*>(state), V, thresholds, steps, out);
  return check_launch("eval_accum_finish");
}
