// Whole-model inference behind one C entry (include/hoisdf.h "whole-model inference"): the eval forward of everything after the image
// encoder (main/model.py:424-662 on the sdf_infer branch; hoisdf_amd/model.py Model.hot_path(..., "eval")) as a host-side chain of
// this library's coarse entries - hoisdf_sdf_infer, hoisdf_project_gather_fwd, hoisdf_sdf_query_fwd, hoisdf_tokens_fwd,
// hoisdf_token_build_fwd, hoisdf_encoder_layer_fwd, hoisdf_decoder_layer_fwd, hoisdf_mano_head_fwd - over ONE
// prepared blob (weights + everything derived from them alone) and ONE caller workspace.  The coarse entries make the kernel choices
// (emulated / small / exact-f32 GEMM by row count, fused in-projection planes, f16x2 attention) from the same arguments Python hands
// them, so either host runs the same kernels on the same shape; the hidden layers of the head MLPs go through chain.h's lin_fwd, the
// dispatch of ops.py's _gemm_fwd.  New device code, where the Python path leans on ATen or spends a GEMM launch on a ragged tail:
//   pose_recentre_kernel   (cam - other centre) * other scale of a gathered point set (+ cam - own centre for the vote stage);
//   pose_head_tail_kernel  the last layer of up to two head MLPs (N <= 96 columns: 3 / 3 / 6 / 10 / 60 / 20) on selected rows of
//                          the last decoder / encoder layer's hidden activations: f32 FMA over K in ascending order;
//   pose_vote_part / _merge the eval form of the joint vote (no loss reductions), the points of a sample cut into segments;
//   pose_prep_misc_kernel  (prepare) both sigmoid_beta floored at 2e-3 and the MANO target mask.
// No float atomics anywhere in the path: two calls on the same inputs give the same bits, with or without a side stream.
#include <unordered_map>

#include "chain.h"

using namespace hoisdf;

namespace {
constexpr int MAXL = HOISDF_POSE_MAX_LAYERS;
constexpr int J_HAND = 20, MANO_Q = 17, SHAPE_IDX = 16, N_BETAS = 10, N_VERTS = 778;
constexpr float LN_EPS = 1e-5f, BETA_FLOOR = 2e-3f;

// ---------------------------------------------------------------- device code ----------------------------------------------------------------
// cross[i] = (cam[i] - c_other[b][i % 3]) * s_other, rel[i] = cam[i] - c_own[b][i % 3] over the flat [n_rows * 3] array, four floats
// (16 bytes) a thread; b = row / P
__device__ __forceinline__ void recentre_one(long i, float v, int P, const float* __restrict__ c_other, float s_other,
                                             const float* __restrict__ c_own, float& cross, float& rel) {
  const long row = i / 3;
  const int d = (int)(i - row * 3);
  const long b = row / P;
  cross = (v - c_other[b * 3 + d]) * s_other;
  rel = c_own ? v - c_own[b * 3 + d] : 0.f;
}
__global__ __launch_bounds__(256) void pose_recentre_kernel(const float* __restrict__ cam, long total, int P, const float* __restrict__ c_other,
                                                            float s_other, const float* __restrict__ c_own, float* __restrict__ cross,
                                                            float* __restrict__ rel) {
  const long n4 = total >> 2;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n4; t += (long)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(cam)[t];
    float4 c, r;
    recentre_one(4 * t + 0, v.x, P, c_other, s_other, c_own, c.x, r.x);
    recentre_one(4 * t + 1, v.y, P, c_other, s_other, c_own, c.y, r.y);
    recentre_one(4 * t + 2, v.z, P, c_other, s_other, c_own, c.z, r.z);
    recentre_one(4 * t + 3, v.w, P, c_other, s_other, c_own, c.w, r.w);
    reinterpret_cast<float4*>(cross)[t] = c;
    if (rel) reinterpret_cast<float4*>(rel)[t] = r;
  }
  if (blockIdx.x == 0 && threadIdx.x < (total & 3)) {          // (n_rows * 3 need not be a multiple of four)
    const long i = (n4 << 2) + threadIdx.x;
    float c, r;
    recentre_one(i, cam[i], P, c_other, s_other, c_own, c, r);
    cross[i] = c;
    if (rel) rel[i] = r;
  }
}

// The last layer of up to two head MLPs in one launch (blockIdx.y = job).  Output row R of a job reads hidden row
// (R / take) * group + first + R % take: `take` consecutive rows out of every `group` (the 16 pose queries / the shape query of
// each sample's 17 decoder rows; take == group: every row).  y[R][n] = b[n] + sum_k x[row][k] W[n][k], k ascending, f32 FMA.
struct HeadJob { const float* x; const float* W; const float* b; float* y; long rows; int N, ldy, take, group, first; };
struct HeadJobs { HeadJob j[2]; };
typedef float vec4 __attribute__((ext_vector_type(4)));      // staging registers
constexpr int HT_KC = 64, HT_LD = HT_KC + 4, HT_NMAX = 96;   // K chunk, padded LDS row (conflict-free 16-byte reads), widest head
// RPT rows per thread: a block of 256 threads covers 64 * RPT output rows.  NJ columns per thread: wave w owns columns w, w + 4, ...,
// w + 4 (NJ - 1), a compile-time count (a per-column test inside the contraction cost more than the contraction: 24 predicated
// branches per K step) - columns >= N are computed on a copy of the last weight row and never stored.  The K chunks are
// software-pipelined: chunk c + 1 travels from HBM into registers while chunk c is contracted out of the LDS (the kernel is a chain
// of K / 64 dependent steps per block - at B = 1 a handful of blocks - so its time is the latency of that chain).
template <int RPT, int NJ>
__global__ __launch_bounds__(256) void pose_head_tail_kernel(HeadJobs jobs, int K) {
  const HeadJob jb = jobs.j[blockIdx.y];
  constexpr int ROWS = 64 * RPT, C4 = HT_KC / 4, XV = ROWS * C4 / 256, WROWS = 4 * NJ, WV = (WROWS * C4 + 255) / 256;
  const int rows = (int)jb.rows, row0 = blockIdx.x * ROWS;
  if (row0 >= rows) return;
  __shared__ __attribute__((aligned(16))) float xs[ROWS * HT_LD];
  __shared__ __attribute__((aligned(16))) float ws[WROWS * HT_LD];
  const int tid = threadIdx.x, lane = tid & 63, cg = tid >> 6;
  // what this thread stages per chunk: XV 16-byte pieces of the hidden rows (16 consecutive threads read 256 contiguous bytes of a
  // row), WV of the weight rows.  Rows / columns outside the job are clamped to its last one: always a valid address, and what lands
  // in the LDS for them is never stored to the output
  const float* xp[XV]; const float* wp[WV];
#pragma unroll
  for (int i = 0; i < XV; ++i) {
    const int idx = tid + i * 256, R = min(row0 + idx / C4, rows - 1);
    xp[i] = jb.x + (long)((R / jb.take) * jb.group + jb.first + R % jb.take) * K + 4 * (idx % C4);
  }
#pragma unroll
  for (int i = 0; i < WV; ++i) {
    const int idx = min(tid + i * 256, WROWS * C4 - 1), n = min(idx / C4, jb.N - 1);
    wp[i] = jb.W + (long)n * K + 4 * (idx % C4);
  }
  vec4 xr[XV], wr[WV];
#pragma unroll
  for (int i = 0; i < XV; ++i) xr[i] = *reinterpret_cast<const vec4*>(xp[i]);
#pragma unroll
  for (int i = 0; i < WV; ++i) wr[i] = *reinterpret_cast<const vec4*>(wp[i]);
  float acc[RPT][NJ];
#pragma unroll
  for (int r = 0; r < RPT; ++r)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[r][j] = 0.f;
  for (int k0 = 0; k0 < K; k0 += HT_KC) {
#pragma unroll
    for (int i = 0; i < XV; ++i) { const int idx = tid + i * 256; *reinterpret_cast<vec4*>(xs + (idx / C4) * HT_LD + 4 * (idx % C4)) = xr[i]; }
#pragma unroll
    for (int i = 0; i < WV; ++i) {
      const int idx = tid + i * 256;
      if (idx < WROWS * C4) *reinterpret_cast<vec4*>(ws + (idx / C4) * HT_LD + 4 * (idx % C4)) = wr[i];
    }
    __syncthreads();
    if (k0 + HT_KC < K) {                                        // the next chunk, in flight under the contraction below
#pragma unroll
      for (int i = 0; i < XV; ++i) xr[i] = *reinterpret_cast<const vec4*>(xp[i] + k0 + HT_KC);
#pragma unroll
      for (int i = 0; i < WV; ++i) wr[i] = *reinterpret_cast<const vec4*>(wp[i] + k0 + HT_KC);
    }
#pragma unroll 2
    for (int k = 0; k < HT_KC; k += 4) {
      float4 xv[RPT];
#pragma unroll
      for (int r = 0; r < RPT; ++r) xv[r] = *reinterpret_cast<const float4*>(xs + (lane + 64 * r) * HT_LD + k);
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float4 wv = *reinterpret_cast<const float4*>(ws + (cg + 4 * j) * HT_LD + k);   // one address per wave: a broadcast
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
          acc[r][j] = fmaf(xv[r].x, wv.x, acc[r][j]);
          acc[r][j] = fmaf(xv[r].y, wv.y, acc[r][j]);
          acc[r][j] = fmaf(xv[r].z, wv.z, acc[r][j]);
          acc[r][j] = fmaf(xv[r].w, wv.w, acc[r][j]);
        }
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < RPT; ++r) {
    const long R = row0 + lane + 64 * r;
    if (R >= rows) continue;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int n = cg + 4 * j;
      if (n < jb.N) jb.y[R * jb.ldy + n] = acc[r][j] + (jb.b ? jb.b[n] : 0.f);
    }
  }
}
template <int NJ>
void head_tail_launch(const HeadJobs& js, int n_jobs, long rows, int K, hipStream_t st) {
  // one row per thread while that still gives fewer blocks than two per CU (B = 1), two rows per thread (half the weight reads) beyond
  if (rows <= 64L * 512) hipLaunchKernelGGL((pose_head_tail_kernel<1, NJ>), dim3((unsigned)cdiv(rows, 64), n_jobs), dim3(256), 0, st, js, K);
  else hipLaunchKernelGGL((pose_head_tail_kernel<2, NJ>), dim3((unsigned)cdiv(rows, 128), n_jobs), dim3(256), 0, st, js, K);
}

// The eval form of the joint vote (common/nets/loss.py:31-56 without its losses): joints[b][j] = sum_p softmax_p(cls[b][:, j])[p] *
// (pts[b][p] + off[b][p][j]).  The points of a sample are cut into segments, one block each (a single block per sample walks 3072
// points in 146 us at B = 1); a block reduces its segment against the segment's own maxima, the merge combines the segments in
// segment order: order-fixed, no atomics.  part[b][seg][5][J] = (m, s, a0, a1, a2).
__global__ __launch_bounds__(256) void pose_vote_part_kernel(const float* __restrict__ off, const float* __restrict__ cls,
                                                             const float* __restrict__ pts, float* __restrict__ part, int P, int J, int chunk) {
  __shared__ float red[4][256];
  __shared__ float smax[64];
  const int b = blockIdx.y, seg = blockIdx.x, nseg = gridDim.x;
  const int p0 = seg * chunk, p1 = min(P, p0 + chunk);
  const float* c = cls + (size_t)b * P * J;
  const float* o = off + (size_t)b * P * J * 3;
  const float* pp = pts + (size_t)b * P * 3;
  const int tid = threadIdx.x;
  const int per = 256 / J;
  const int j = tid % J, pl = tid / J;
  const bool active = pl < per;
  float m = -INFINITY;
  if (active)
    for (int p = p0 + pl; p < p1; p += per) m = fmaxf(m, c[(size_t)p * J + j]);
  red[0][tid] = m;
  __syncthreads();
  if (tid < J) {
    float mm = -INFINITY;
    for (int k = 0; k < per; ++k) mm = fmaxf(mm, red[0][k * J + tid]);
    smax[tid] = mm;
  }
  __syncthreads();
  float s = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
  if (active) {
    const float M = smax[j];
    for (int p = p0 + pl; p < p1; p += per) {
      const float e = expf(c[(size_t)p * J + j] - M);
      const float* oo = o + ((size_t)p * J + j) * 3;
      s += e;
      a0 += e * (pp[p * 3 + 0] + oo[0]);
      a1 += e * (pp[p * 3 + 1] + oo[1]);
      a2 += e * (pp[p * 3 + 2] + oo[2]);
    }
  }
  red[0][tid] = s; red[1][tid] = a0; red[2][tid] = a1; red[3][tid] = a2;
  __syncthreads();
  if (tid < J) {
    float S = 0.f, A0 = 0.f, A1 = 0.f, A2 = 0.f;
    for (int k = 0; k < per; ++k) {
      S += red[0][k * J + tid]; A0 += red[1][k * J + tid]; A1 += red[2][k * J + tid]; A2 += red[3][k * J + tid];
    }
    float* out = part + ((size_t)b * nseg + seg) * 5 * J;
    out[tid] = smax[tid]; out[J + tid] = S; out[2 * J + tid] = A0; out[3 * J + tid] = A1; out[4 * J + tid] = A2;
  }
}
__global__ __launch_bounds__(64) void pose_vote_merge_kernel(const float* __restrict__ part, int nseg, float* __restrict__ joints, int J) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid >= J) return;
  const float* in = part + (size_t)b * nseg * 5 * J;
  float M = -INFINITY;
  for (int g = 0; g < nseg; ++g) M = fmaxf(M, in[(size_t)g * 5 * J + tid]);
  float S = 0.f, A0 = 0.f, A1 = 0.f, A2 = 0.f;
  for (int g = 0; g < nseg; ++g) {
    const float* q = in + (size_t)g * 5 * J;
    const float w = expf(q[tid] - M);
    S += q[J + tid] * w; A0 += q[2 * J + tid] * w; A1 += q[3 * J + tid] * w; A2 += q[4 * J + tid] * w;
  }
  float* jo = joints + ((size_t)b * J + tid) * 3;
  jo[0] = A0 / S; jo[1] = A1 / S; jo[2] = A2 / S;
}
constexpr int VOTE_CHUNK = 128;
inline int vote_segments(int B, int P) { const int want = cdiv(P, VOTE_CHUNK), cap = 1024 / B > 1 ? 1024 / B : 1; return want < cap ? want : cap; }
int vote_only(const float* off, const float* cls, const float* pts, float* joints, float* part, int B, int P, int J, hipStream_t st) {
  const int nseg = vote_segments(B, P);
  hipLaunchKernelGGL(pose_vote_part_kernel, dim3(nseg, B), dim3(256), 0, st, off, cls, pts, part, P, J, cdiv(P, nseg));
  hipLaunchKernelGGL(pose_vote_merge_kernel, dim3(B), dim3(64), 0, st, part, nseg, joints, J);
  return check_launch("pose vote");
}
int head_tail(const HeadJob* jobs, int n_jobs, int K, hipStream_t st) {
  HeadJobs js{};
  long rows = 0;
  int nmax = 0;
  for (int i = 0; i < n_jobs; ++i) {
    js.j[i] = jobs[i];
    if (jobs[i].rows > rows) rows = jobs[i].rows;
    if (jobs[i].N > nmax) nmax = jobs[i].N;
    if (jobs[i].N < 1 || jobs[i].N > HT_NMAX || K % HT_KC || !al16(jobs[i].x) || !al16(jobs[i].W) || jobs[i].rows >= (1L << 31) - 128) {
      set_error("pose_infer: head of %d columns over K=%d does not fit the fused head kernel", jobs[i].N, K);
      return HOISDF_ERR_INVALID;
    }
  }
  if (rows == 0) return HOISDF_OK;
  const int nj = (nmax + 3) / 4;                  // columns per thread: the model's heads are 3 | 6, 10 | 20, 60 wide
  if (nj <= 1) head_tail_launch<1>(js, n_jobs, rows, K, st);
  else if (nj <= 3) head_tail_launch<3>(js, n_jobs, rows, K, st);
  else if (nj <= 15) head_tail_launch<15>(js, n_jobs, rows, K, st);
  else head_tail_launch<HT_NMAX / 4>(js, n_jobs, rows, K, st);
  return check_launch("pose head tail");
}

// prepare: beta_out[0 / 1] = max(beta, 2e-3) (main/model.py:123-126) and the MANO target mask (common/utils/misc.py:11-31; 1 = masked)
__global__ void pose_prep_misc_kernel(const float* __restrict__ hand_beta, const float* __restrict__ obj_beta, float* __restrict__ beta_out,
                                      uint8_t* __restrict__ mask, int Q) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) { beta_out[0] = fmaxf(hand_beta[0], BETA_FLOOR); beta_out[1] = fmaxf(obj_beta[0], BETA_FLOOR); }
  if (i >= Q * Q) return;
  const int r = i / Q, c = i % Q;
  bool open = Q == 1 || (r == 0 && c == 0) || (r == SHAPE_IDX && c == SHAPE_IDX);
  if (r >= 1 && r < SHAPE_IDX && c >= 1 && c < SHAPE_IDX && (r - 1) / 3 == (c - 1) / 3) open = true;      // the three joints of a finger
  mask[i] = open ? 0 : 1;
}

// ---------------------------------------------------------------- geometry ----------------------------------------------------------------
struct PGeo { int B, nh, no, S, E, F, H, C, Lh, Lo, Ld, Q; bool ik, iks /* ik_solve */; long Mh, Mo; };
int pose_geometry(const hoisdf_pose_desc* d, PGeo& g) {
  HOISDF_REQUIRE(d, HOISDF_ERR_INVALID, "pose: null descriptor");
  HOISDF_REQUIRE(d->B > 0 && d->num_samp_hand > 0 && d->num_samp_obj > 0 && d->bins_n > 0 && d->img_h > 0 && d->img_w > 0, HOISDF_ERR_INVALID,
                 "pose: bad sizes B=%d num_samp_hand=%d num_samp_obj=%d bins_n=%d image %dx%d", d->B, d->num_samp_hand, d->num_samp_obj, d->bins_n,
                 d->img_h, d->img_w);
  HOISDF_REQUIRE(d->hand_sdf_scale > 0.f && d->obj_sdf_scale > 0.f && d->clamping_distance > 0.f, HOISDF_ERR_INVALID,
                 "pose: the SDF scales and the clamping distance must be positive");
  HOISDF_REQUIRE(d->hidden_dim == 256, HOISDF_ERR_INVALID,
                 "pose: hidden_dim=%d; the SDF decoders and the token layout are built for the released width 256", d->hidden_dim);
  HOISDF_REQUIRE(d->nheads > 0 && d->nheads * 64 == d->hidden_dim, HOISDF_ERR_INVALID,
                 "pose: nheads=%d; the attention kernels hold heads of 64 (hidden_dim / 64 = %d heads)", d->nheads, d->hidden_dim / 64);
  HOISDF_REQUIRE(d->dim_feedforward > 0 && d->dim_feedforward % 4 == 0, HOISDF_ERR_INVALID, "pose: dim_feedforward=%d", d->dim_feedforward);
  HOISDF_REQUIRE(d->enc_layers >= 2 && d->enc_layers <= MAXL && d->dec_layers >= 1 && d->dec_layers <= MAXL, HOISDF_ERR_INVALID,
                 "pose: enc_layers=%d (2..%d; the object stack has enc_layers / 2), dec_layers=%d (1..%d)", d->enc_layers, MAXL, d->dec_layers, MAXL);
  HOISDF_REQUIRE(d->C > 0 && d->C % 4 == 0, HOISDF_ERR_INVALID, "pose: C=%d pyramid channels (a multiple of 4)", d->C);
  HOISDF_REQUIRE(!d->pre_norm, HOISDF_ERR_INVALID, "pose: pre_norm is not implemented by the coarse layer entries (post-norm only)");
  HOISDF_REQUIRE(d->attention == 0 || d->attention == 2, HOISDF_ERR_INVALID, "pose: attention must be 0 (exact f32) or 2 (emulated fp32)");
  g.B = d->B; g.nh = d->num_samp_hand; g.no = d->num_samp_obj; g.S = g.nh + g.no; g.E = d->hidden_dim; g.F = d->dim_feedforward; g.H = d->nheads;
  HOISDF_REQUIRE(!d->ik_solve || d->use_inverse_kinematics, HOISDF_ERR_INVALID, "pose: ik_solve needs use_inverse_kinematics");
  g.C = d->C; g.Lh = d->enc_layers; g.Lo = d->enc_layers / 2; g.Ld = d->dec_layers; g.ik = d->use_inverse_kinematics != 0;
  g.iks = g.ik && d->ik_solve != 0;
  g.Q = g.ik ? 1 : MANO_Q;
  g.Mh = (long)g.B * g.nh; g.Mo = (long)g.B * g.no;
  HOISDF_REQUIRE((long)g.B * g.S < (1L << 28), HOISDF_ERR_INVALID, "pose: %ld token rows", (long)g.B * g.S);
  return HOISDF_OK;
}

// ---------------------------------------------------------------- the prepared blob ----------------------------------------------------------------
// Its layout is a pure function of the descriptor: prepare and infer run the same carving code (with a null base it only measures).
struct Prep {
  hoisdf_sdf_weights sdf[2];           // 0 = hand field, 1 = object field (linear_sdfin shared)
  float* wn_tmp;                       // [512][512]: linh2 folded, before the re-lay into [512][516]
  hoisdf_mlp tin, pose, shape, vote, cls, rot, trans;
  float* betas;                        // [2] floored
  hoisdf_encoder_layer_weights he[MAXL], oe[MAXL];
  hoisdf_decoder_layer_weights hd[MAXL];
  float* qembed; float* tgt0; uint8_t* mask;
  float *mano_image, *mano_tmpl, *mano_jreg, *mano_w, *mano_mean;
};
struct Placer {
  Bump b; hipStream_t st; bool copy; int rc = HOISDF_OK;
  Placer(void* base, long cap, hipStream_t s, bool cp) : b(base, cap), st(s), copy(cp) {}
  // n floats of the blob; when preparing, filled from src (a null src is the caller's missing weight)
  float* put(long n, const float* src, const char* name) {
    float* p = b.floats(n);
    if (!copy || rc != HOISDF_OK) return p;
    if (!src) { set_error("pose_prepare: null weight %s", name); rc = HOISDF_ERR_INVALID; return p; }
    if (!p) { rc = HOISDF_ERR_WORKSPACE; return p; }
    if (hipMemcpyAsync(p, src, sizeof(float) * n, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("pose_prepare: copying %s failed: %s", name, hipGetErrorString(hipGetLastError()));
      rc = HOISDF_ERR_LAUNCH;
    }
    return p;
  }
  float* raw(long n) { return b.floats(n); }
  // the weight image of W [N][K] (dense) in the process's form
  const void* image(const float* W, int N, int K, int ldw = 0) {
    void* img = b.take(hoisdf_linear_emu_image_bytes(N, K));
    if (!copy || rc != HOISDF_OK) return img;
    if (!img) { rc = HOISDF_ERR_WORKSPACE; return img; }
    rc = hoisdf_linear_emu_prepare(W, ldw ? ldw : K, N, K, 0, img, st);
    return img;
  }
};
bool mlp_shape(const hoisdf_mlp& m, int n_layers, const int* dims, int act_last) {
  if (m.n_layers != n_layers || (m.act_last != 0) != (act_last != 0)) return false;
  for (int i = 0; i <= n_layers; ++i) if (m.dims[i] != dims[i]) return false;
  return true;
}
// an MLP's weights (+ the images of every layer whose contraction the emulated GEMM takes: K % 4 == 0)
void place_mlp(Placer& P, hoisdf_mlp& out, const hoisdf_mlp* src, int n_layers, const int* dims, int act_last, const char* name, bool last_image) {
  out = hoisdf_mlp{};
  out.n_layers = n_layers; out.act_last = act_last;
  for (int i = 0; i <= n_layers; ++i) out.dims[i] = dims[i];
  if (P.copy && P.rc == HOISDF_OK && !mlp_shape(*src, n_layers, dims, act_last)) {
    set_error("pose_prepare: %s does not have the layer sizes of the reference model", name);
    P.rc = HOISDF_ERR_INVALID;
  }
  for (int i = 0; i < n_layers; ++i) {
    out.w[i] = P.put((long)dims[i + 1] * dims[i], src ? src->w[i] : nullptr, name);
    out.b[i] = P.put(dims[i + 1], src ? src->b[i] : nullptr, name);
    if ((i < n_layers - 1 || last_image) && dims[i] % 4 == 0) out.img[i] = P.image(out.w[i], dims[i + 1], dims[i]);
  }
}
void place_sdf(Placer& P, const PGeo& g, hoisdf_sdf_weights& w, const hoisdf_sdf_weights* shared, const hoisdf_mlp* sdfin,
               const hoisdf_sdf_decoder_params* dec, float* tmp, const char* name) {
  const int C = g.C;
  w = hoisdf_sdf_weights{};
  w.C = C;
  if (shared) {
    w.sdfin_w0 = shared->sdfin_w0; w.sdfin_b0 = shared->sdfin_b0; w.sdfin_w1 = shared->sdfin_w1; w.sdfin_b1 = shared->sdfin_b1;
    w.emu_img[0] = shared->emu_img[0]; w.emu_img[1] = shared->emu_img[1];
  } else {
    w.sdfin_w0 = P.put(512L * C, sdfin ? sdfin->w[0] : nullptr, "linear_sdfin"); w.sdfin_b0 = P.put(512, sdfin ? sdfin->b[0] : nullptr, "linear_sdfin");
    w.sdfin_w1 = P.put(256L * 512, sdfin ? sdfin->w[1] : nullptr, "linear_sdfin"); w.sdfin_b1 = P.put(256, sdfin ? sdfin->b[1] : nullptr, "linear_sdfin");
    w.emu_img[0] = P.image(w.sdfin_w0, 512, C); w.emu_img[1] = P.image(w.sdfin_w1, 256, 512);
  }
  // the weight-norm folds in the layouts of hoisdf_sdf_weights: row 223 of dec_w1 / dec_b1 and the pad columns of dec_w2 stay zero
  float* W0 = P.raw(512L * 289); float* w1 = P.raw(224L * 512); float* b1 = P.raw(224); float* w2 = P.raw(512L * 516); float* W3 = P.raw(512L * 512);
  w.dec_w0 = W0; w.dec_ld0 = 289; w.dec_w1 = w1; w.dec_b1 = b1; w.dec_w2 = w2; w.dec_w3 = W3;
  w.dec_b0 = P.put(512, dec ? dec->bias[0] : nullptr, name);
  w.dec_b2 = P.put(512, dec ? dec->bias[2] : nullptr, name);
  w.dec_b3 = P.put(512, dec ? dec->bias[3] : nullptr, name);
  w.dec_w4 = P.put(512, dec ? dec->linh4_weight : nullptr, name);
  w.dec_b4 = P.put(1, dec ? dec->linh4_bias : nullptr, name);
  if (P.copy && P.rc == HOISDF_OK) {
    bool all = dec->bias[1] != nullptr;
    for (int i = 0; i < 4; ++i) all = all && dec->weight_v[i] && dec->weight_g[i];
    if (!all) { set_error("pose_prepare: null weight %s", name); P.rc = HOISDF_ERR_INVALID; return; }
    if (!W0 || !w1 || !b1 || !w2 || !W3 || !tmp) { P.rc = HOISDF_ERR_WORKSPACE; return; }
    hipStream_t st = P.st;
    bool ok = hipMemsetAsync(w1, 0, sizeof(float) * 224 * 512, st) == hipSuccess && hipMemsetAsync(b1, 0, sizeof(float) * 224, st) == hipSuccess &&
              hipMemsetAsync(w2, 0, sizeof(float) * 512 * 516, st) == hipSuccess;
    if (ok) P.rc = hoisdf_weightnorm_fwd(dec->weight_v[0], dec->weight_g[0], W0, 289, nullptr, 512, 289, st);
    if (ok && !P.rc) P.rc = hoisdf_weightnorm_fwd(dec->weight_v[1], dec->weight_g[1], w1, 512, nullptr, 223, 512, st);
    if (ok && !P.rc) P.rc = hoisdf_weightnorm_fwd(dec->weight_v[2], dec->weight_g[2], tmp, 512, nullptr, 512, 512, st);
    if (ok && !P.rc) P.rc = hoisdf_weightnorm_fwd(dec->weight_v[3], dec->weight_g[3], W3, 512, nullptr, 512, 512, st);
    if (P.rc) return;
    // dec_w2 [512][516]: columns 0..222 = W2[:, 0:223] (h1), 223 = 0, 224..512 = W2[:, 223:512] (x0), 513..515 = 0
    ok = ok && hipMemcpy2DAsync(w2, 516 * sizeof(float), tmp, 512 * sizeof(float), 223 * sizeof(float), 512, hipMemcpyDeviceToDevice, st) == hipSuccess &&
         hipMemcpy2DAsync(w2 + 224, 516 * sizeof(float), tmp + 223, 512 * sizeof(float), 289 * sizeof(float), 512, hipMemcpyDeviceToDevice, st) == hipSuccess &&
         hipMemcpyAsync(b1, dec->bias[1], sizeof(float) * 223, hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (!ok) { set_error("pose_prepare: laying out %s failed: %s", name, hipGetErrorString(hipGetLastError())); P.rc = HOISDF_ERR_LAUNCH; return; }
  }
  // the images of the four decoder matrices, with the arguments hoisdf_amd/ops.py SdfQueryWeights builds them from
  w.emu_img[2] = P.image(W0, 512, 289); w.emu_img[3] = P.image(w1, 224, 512); w.emu_img[4] = P.image(w2, 512, 516); w.emu_img[5] = P.image(W3, 512, 512);
}
void place_encoder(Placer& P, const PGeo& g, hoisdf_encoder_layer_weights& w, const hoisdf_encoder_layer_weights* s, bool last, const char* name) {
  const long E = g.E, F = g.F;
  w = hoisdf_encoder_layer_weights{};
  w.w_in = P.put(3 * E * E, s ? s->w_in : nullptr, name); w.b_in = P.put(3 * E, s ? s->b_in : nullptr, name);
  w.w_out = P.put(E * E, s ? s->w_out : nullptr, name); w.b_out = P.put(E, s ? s->b_out : nullptr, name);
  w.g1 = P.put(E, s ? s->g1 : nullptr, name); w.be1 = P.put(E, s ? s->be1 : nullptr, name);
  w.w1 = P.put(F * E, s ? s->w1 : nullptr, name); w.b1 = P.put(F, s ? s->b1 : nullptr, name);
  w.w2 = P.put(E * F, s ? s->w2 : nullptr, name); w.b2 = P.put(E, s ? s->b2 : nullptr, name);
  w.g2 = P.put(E, s ? s->g2 : nullptr, name); w.be2 = P.put(E, s ? s->be2 : nullptr, name);
  if (last) {             // inter_norm: only the last layer's is read (main/model.py:587-593 slices [-1] of the stack)
    w.g3 = P.put(E, s ? s->g3 : nullptr, name); w.be3 = P.put(E, s ? s->be3 : nullptr, name);
    w.img_in_q = P.image(w.w_in, (int)E, (int)E); w.img_in_kv = P.image(w.w_in + E * E, 2 * (int)E, (int)E);   // its queries are the kept rows only
  } else {
    w.img_in = P.image(w.w_in, 3 * (int)E, (int)E);
  }
  w.img_out = P.image(w.w_out, (int)E, (int)E); w.img_1 = P.image(w.w1, (int)F, (int)E); w.img_2 = P.image(w.w2, (int)E, (int)F);
}
void place_decoder(Placer& P, const PGeo& g, hoisdf_decoder_layer_weights& w, const hoisdf_decoder_layer_weights* s, bool last, const char* name) {
  const long E = g.E, F = g.F;
  w = hoisdf_decoder_layer_weights{};
  w.sa_w_in = P.put(3 * E * E, s ? s->sa_w_in : nullptr, name); w.sa_b_in = P.put(3 * E, s ? s->sa_b_in : nullptr, name);
  w.sa_w_out = P.put(E * E, s ? s->sa_w_out : nullptr, name); w.sa_b_out = P.put(E, s ? s->sa_b_out : nullptr, name);
  w.ca_w_in = P.put(3 * E * E, s ? s->ca_w_in : nullptr, name); w.ca_b_in = P.put(3 * E, s ? s->ca_b_in : nullptr, name);
  w.ca_w_out = P.put(E * E, s ? s->ca_w_out : nullptr, name); w.ca_b_out = P.put(E, s ? s->ca_b_out : nullptr, name);
  w.w1 = P.put(F * E, s ? s->w1 : nullptr, name); w.b1 = P.put(F, s ? s->b1 : nullptr, name);
  w.w2 = P.put(E * F, s ? s->w2 : nullptr, name); w.b2 = P.put(E, s ? s->b2 : nullptr, name);
  w.g1 = P.put(E, s ? s->g1 : nullptr, name); w.be1 = P.put(E, s ? s->be1 : nullptr, name);
  w.g2 = P.put(E, s ? s->g2 : nullptr, name); w.be2 = P.put(E, s ? s->be2 : nullptr, name);
  w.g3 = P.put(E, s ? s->g3 : nullptr, name); w.be3 = P.put(E, s ? s->be3 : nullptr, name);
  if (last) { w.g4 = P.put(E, s ? s->g4 : nullptr, name); w.be4 = P.put(E, s ? s->be4 : nullptr, name); }   // decoder.norm of the last layer's output only
  w.img_ca_kv = P.image(w.ca_w_in + E * E, 2 * (int)E, (int)E);
}
// carves (and, with src, fills) the whole blob
int place_all(Placer& P, const PGeo& g, const hoisdf_pose_weights* src, Prep& p) {
  const int E = g.E, C = g.C;
  p.wn_tmp = P.raw(512L * 512);
  place_sdf(P, g, p.sdf[0], nullptr, src ? &src->linear_sdfin : nullptr, src ? &src->hand_sdf_decoder : nullptr, p.wn_tmp, "hand_sdf_decoder");
  place_sdf(P, g, p.sdf[1], &p.sdf[0], nullptr, src ? &src->obj_sdf_decoder : nullptr, p.wn_tmp, "obj_sdf_decoder");
  if (P.copy && P.rc == HOISDF_OK) {
    const int ds[3] = {C, 512, 256};
    if (!mlp_shape(src->linear_sdfin, 2, ds, 1)) { set_error("pose_prepare: linear_sdfin must be C -> 512 -> 256 with ReLU after both"); P.rc = HOISDF_ERR_INVALID; }
  }
  const int dt[5] = {C, 1024, 512, 256, E - 33};
  place_mlp(P, p.tin, src ? &src->linear_transformerin : nullptr, 4, dt, 1, "linear_transformerin", true);
  const int d6[4] = {E, E, E, 6}, d10[4] = {E, E, E, N_BETAS}, dv[5] = {E, E, E, E, 3 * J_HAND}, dc[4] = {E, E, E, J_HAND}, d3[4] = {E, E, E, 3};
  if (!g.ik) place_mlp(P, p.pose, src ? &src->linear_pose : nullptr, 3, d6, 0, "linear_pose", false);
  place_mlp(P, p.shape, src ? &src->linear_shape : nullptr, 3, d10, 0, "linear_shape", false);
  place_mlp(P, p.vote, src ? &src->linear_handvote : nullptr, 4, dv, 0, "linear_handvote", false);
  place_mlp(P, p.cls, src ? &src->linear_handcls : nullptr, 3, dc, 0, "linear_handcls", false);
  place_mlp(P, p.rot, src ? &src->linear_obj_rot : nullptr, 3, d3, 0, "linear_obj_rot", false);
  place_mlp(P, p.trans, src ? &src->linear_obj_rel_trans : nullptr, 3, d3, 0, "linear_obj_rel_trans", false);
  for (int i = 0; i < g.Lh; ++i) place_encoder(P, g, p.he[i], src ? &src->hand_encoder[i] : nullptr, i == g.Lh - 1, "hand_transformer.encoder");
  for (int i = 0; i < g.Lo; ++i) place_encoder(P, g, p.oe[i], src ? &src->obj_encoder[i] : nullptr, i == g.Lo - 1, "obj_transformer.encoder");
  for (int i = 0; i < g.Ld; ++i) place_decoder(P, g, p.hd[i], src ? &src->hand_decoder[i] : nullptr, i == g.Ld - 1, "hand_transformer.decoder");
  p.qembed = P.put((long)g.Q * E, src ? src->mano_query_embed : nullptr, "mano_query_embed.weight");
  p.betas = P.raw(2);
  p.tgt0 = P.raw((long)g.B * g.Q * E);
  p.mask = static_cast<uint8_t*>(P.b.take((long)g.Q * g.Q));
  p.mano_image = p.mano_tmpl = p.mano_jreg = p.mano_w = p.mano_mean = nullptr;
  if (!g.ik || g.iks) {                // the MANO head's tables, or the same tables for the IK solve (last in the blob either way)
    p.mano_image = P.raw(hoisdf_mano_dirs_image_floats());
    p.mano_tmpl = P.put(N_VERTS * 3, src ? src->mano_v_template : nullptr, "mano v_template");
    p.mano_jreg = P.put(16 * N_VERTS, src ? src->mano_j_regressor : nullptr, "mano J_regressor");
    p.mano_w = P.put(N_VERTS * 16, src ? src->mano_weights : nullptr, "mano weights");
    if (!g.ik) p.mano_mean = P.put(45, src ? src->mano_hands_mean : nullptr, "mano hands_mean");   // (the IK solve takes the mean as zero)
  }
  if (!P.copy || P.rc != HOISDF_OK) return P.rc;
  if (!src->hand_sigmoid_beta || !src->obj_sigmoid_beta) { set_error("pose_prepare: null weight sigmoid_beta"); return HOISDF_ERR_INVALID; }
  if (P.b.overflow || !p.betas || !p.tgt0 || !p.mask) return HOISDF_ERR_WORKSPACE;
  if (hipMemsetAsync(p.tgt0, 0, sizeof(float) * g.B * g.Q * E, P.st) != hipSuccess) { set_error("pose_prepare: memset failed"); return HOISDF_ERR_LAUNCH; }
  hipLaunchKernelGGL(pose_prep_misc_kernel, dim3(cdiv(g.Q * g.Q, 64)), dim3(64), 0, P.st, src->hand_sigmoid_beta, src->obj_sigmoid_beta, p.betas, p.mask, g.Q);
  if (int rc = check_launch("pose_prepare misc")) return rc;
  if (!g.ik || g.iks) {
    if (!src->mano_shapedirs || !src->mano_posedirs) { set_error("pose_prepare: null MANO asset"); return HOISDF_ERR_INVALID; }
    if (int rc = hoisdf_mano_prepare(src->mano_shapedirs, src->mano_posedirs, p.mano_w, p.mano_image, P.st)) return rc;
  }
  return HOISDF_OK;
}

// ---------------------------------------------------------------- the frame workspace ----------------------------------------------------------------
struct Frame {
  float *hand_pts, *hand_sdf, *hand_pe, *obj_pts, *obj_sdf, *obj_pe;
  float *hand_feat, *hand_cam, *hand_rel, *hand_o_pts, *hand_o_sdf, *hand_o_raw, *hand_o_pe, *hand_fea;
  float *obj_feat, *obj_cam, *obj_h_pts, *obj_h_sdf, *obj_h_raw, *obj_h_pe, *obj_fea;
  float *hand_tok, *obj_tok, *hx[2], *ox[2], *memory, *hand_enc, *obj_enc, *dt[2], *hs;
  float *hid_h[4], *hid_o[4], *hid_m[4];      // hidden activations of the head chains: [vote a, vote b, cls a, cls b] on the hand rows, ...
  float *off, *cls, *stats /* the vote's segment partials */, *pose6d, *shape, *rot;
  void *scr_h, *scr_o, *sav_h, *sav_o; long scr_h_bytes, scr_o_bytes, sav_h_bytes, sav_o_bytes;
};
hoisdf_encoder_layer_desc enc_desc(const PGeo& g, int attention, int keep, bool last) {
  hoisdf_encoder_layer_desc d{};
  d.B = g.B; d.S = g.S; d.E = g.E; d.F = g.F; d.H = g.H;
  d.n_query = last ? keep : g.S; d.n_inter = keep;
  d.eps = LN_EPS; d.drop_p = 0.f; d.attention = attention; d.attention_bwd_emulated = 0; d.training = 0; d.x_mag = nullptr;
  return d;
}
hoisdf_decoder_layer_desc dec_desc(const PGeo& g) {
  hoisdf_decoder_layer_desc d{};
  d.B = g.B; d.Q = g.Q; d.S = g.nh; d.E = g.E; d.F = g.F; d.H = g.H; d.kv_len = g.nh; d.eps = LN_EPS; d.drop_p = 0.f; d.training = 0;
  return d;
}
inline long lmax(long a, long b) { return a > b ? a : b; }
// hidden layers of a head MLP through the library's linear dispatch (dry: only reserves what lin_fwd may need).  In the f16x2 form
// the row magnitudes travel from each layer's epilogue to the next contraction as in heads.hip's mlp_forward: x is measured once
// (*x_mag: in = the words another chain over the same x left, out = the words this chain used), nothing else is re-read.
const float* head_hidden(Ctx& c, const hoisdf_mlp& m, const float* x, long M, float* a, float* b, const uint32_t** x_mag = nullptr) {
  const int hidden = m.n_layers - 1;
  uint32_t* mg = nullptr;
  if (c.emu && emu_form_h2() && M >= EMU_MIN_ROWS) {
    mg = static_cast<uint32_t*>(c.ws->take((long)hidden * M * 4));
    if (c.dry || !c.ok()) mg = nullptr;
    else if (!mg) { c.rc = HOISDF_ERR_WORKSPACE; return nullptr; }
    else if (hipMemsetAsync(mg, 0, (size_t)hidden * M * 4, c.st) != hipSuccess) { c.rc = HOISDF_ERR_LAUNCH; return nullptr; }
  }
  const uint32_t* in_mag = mg && x_mag ? *x_mag : nullptr;
  if (mg && !in_mag && emu_rows(c, M, x, m.dims[0], m.dims[0])) {
    if ((c.rc = emu_mag_measure(x, m.dims[0], M, m.dims[0], mg, c.st)) != HOISDF_OK) return nullptr;
    in_mag = mg;
    if (x_mag) *x_mag = mg;
  }
  const float* in = x;
  for (int i = 0; i < hidden; ++i) {
    float* out = (i & 1) ? b : a;
    // (the tiled emulated form is the one that writes the words: the test lin_fwd makes; the last hidden layer feeds the FMA kernel)
    uint32_t* out_mag = mg && i + 1 < hidden && emu_rows(c, M, in, m.dims[i], m.dims[i]) ? mg + (long)(i + 1) * M : nullptr;
    lin_fwd(c, in, m.dims[i], m.w[i], m.dims[i], m.img[i], m.b[i], out, m.dims[i + 1], M, m.dims[i + 1], m.dims[i], 1, 0.f, 0, nullptr, 0, in_mag, out_mag);
    in = out; in_mag = out_mag;
  }
  return in;
}
int carve_frame(const hoisdf_pose_desc* d, const PGeo& g, const Prep& p, long n_hand, long n_obj, Bump& b, Frame& f) {
  const long Mh = g.Mh, Mo = g.Mo, E = g.E, C = g.C, BS = (long)g.B * g.S;
  f.hand_pts = b.floats(Mh * 3); f.hand_sdf = b.floats(Mh); f.hand_pe = b.floats(Mh * 30);
  f.obj_pts = b.floats(Mo * 3); f.obj_sdf = b.floats(Mo); f.obj_pe = b.floats(Mo * 30);
  f.hand_feat = b.floats(Mh * C); f.hand_cam = b.floats(Mh * 3); f.hand_rel = b.floats(Mh * 3); f.hand_o_pts = b.floats(Mh * 3);
  f.hand_o_sdf = b.floats(Mh); f.hand_o_raw = b.floats(Mh); f.hand_o_pe = b.floats(Mh * 30); f.hand_fea = b.floats(Mh * (E - 33));
  f.obj_feat = b.floats(Mo * C); f.obj_cam = b.floats(Mo * 3); f.obj_h_pts = b.floats(Mo * 3);
  f.obj_h_sdf = b.floats(Mo); f.obj_h_raw = b.floats(Mo); f.obj_h_pe = b.floats(Mo * 30); f.obj_fea = b.floats(Mo * (E - 33));
  f.hand_tok = b.floats(BS * E); f.obj_tok = b.floats(BS * E);
  for (int i = 0; i < 2; ++i) { f.hx[i] = b.floats(BS * E); f.ox[i] = b.floats(BS * E); f.dt[i] = b.floats((long)g.B * g.Q * E); }
  f.memory = b.floats(Mh * E); f.hand_enc = b.floats(Mh * E); f.obj_enc = b.floats(Mo * E); f.hs = b.floats((long)g.B * g.Q * E);
  for (int i = 0; i < 4; ++i) { f.hid_h[i] = b.floats(Mh * E); f.hid_o[i] = b.floats(Mo * E); f.hid_m[i] = b.floats((long)g.B * g.Q * E); }
  f.off = b.floats(Mh * 3 * J_HAND); f.cls = b.floats(Mh * J_HAND); f.stats = b.floats((long)g.B * vote_segments(g.B, g.nh) * 5 * J_HAND);
  f.pose6d = b.floats((long)g.B * 16 * 6); f.shape = b.floats((long)g.B * N_BETAS); f.rot = b.floats((long)g.B * 16 * 9);
  // scratch of the coarse entries: one region per stream, reused by the calls that follow each other on it
  const hoisdf_encoder_layer_desc eh0 = enc_desc(g, d->attention, g.nh, false), eh1 = enc_desc(g, d->attention, g.nh, true);
  const hoisdf_encoder_layer_desc eo0 = enc_desc(g, d->attention, g.no, false), eo1 = enc_desc(g, d->attention, g.no, true);
  const hoisdf_decoder_layer_desc dd = dec_desc(g);
  long sh = lmax(hoisdf_sdf_infer_workspace(n_hand, g.B, g.C), hoisdf_sdf_infer_workspace(n_obj, g.B, g.C));
  sh = lmax(sh, hoisdf_sdf_query_workspace(Mh, g.C, 0));
  sh = lmax(sh, hoisdf_tokens_workspace_bytes(&p.tin, Mh, 0));
  sh = lmax(sh, lmax(hoisdf_encoder_layer_workspace_bytes(&eh0, 0), hoisdf_encoder_layer_workspace_bytes(&eh1, 0)));
  sh = lmax(sh, hoisdf_decoder_layer_workspace_bytes(&dd, 0));
  long so = lmax(hoisdf_sdf_query_workspace(Mo, g.C, 0), hoisdf_tokens_workspace_bytes(&p.tin, Mo, 0));
  so = lmax(so, lmax(hoisdf_encoder_layer_workspace_bytes(&eo0, 0), hoisdf_encoder_layer_workspace_bytes(&eo1, 0)));
  {   // the head chains' own needs (an image lin_fwd would build when the blob carries none: never, but the size query stays honest)
    Bump m1(nullptr, 0), m2(nullptr, 0);
    Ctx c1{nullptr, nullptr, &m1, true, gemm_emu_mode()}, c2{nullptr, nullptr, &m2, true, gemm_emu_mode()};
    const uint32_t* xm = nullptr;
    head_hidden(c1, p.vote, nullptr, Mh, nullptr, nullptr, &xm); head_hidden(c1, p.cls, nullptr, Mh, nullptr, nullptr, &xm);
    head_hidden(c2, p.rot, nullptr, Mo, nullptr, nullptr, &xm); head_hidden(c2, p.trans, nullptr, Mo, nullptr, nullptr, &xm);
    head_hidden(c2, p.shape, nullptr, (long)g.B * g.Q, nullptr, nullptr);
    if (!g.ik) head_hidden(c2, p.pose, nullptr, (long)g.B * g.Q, nullptr, nullptr);
    sh = lmax(sh, m1.off + 256); so = lmax(so, m2.off + 256);
  }
  f.scr_h_bytes = sh; f.scr_o_bytes = so;
  f.sav_h_bytes = hoisdf_tokens_saved_bytes(&p.tin, Mh, 0); f.sav_o_bytes = hoisdf_tokens_saved_bytes(&p.tin, Mo, 0);
  f.scr_h = b.take(sh); f.scr_o = b.take(so); f.sav_h = b.take(f.sav_h_bytes); f.sav_o = b.take(f.sav_o_bytes);
  return HOISDF_OK;
}
int counts_total(const PGeo& g, const int32_t* counts_host, long& n_hand, long& n_obj, bool check) {
  n_hand = n_obj = 0;
  for (int b = 0; b < g.B; ++b) {
    const int ch = counts_host[b], co = counts_host[g.B + b];
    HOISDF_REQUIRE(ch >= 0 && co >= 0, HOISDF_ERR_INVALID, "pose: negative survivor count for sample %d", b);
    if (check) {
      HOISDF_REQUIRE(ch >= g.nh, HOISDF_ERR_TOO_FEW, "sdf_infer(hand): sample %d has only %d lattice points inside its bbox, fewer than num_points=%d", b, ch, g.nh);
      HOISDF_REQUIRE(co >= g.no, HOISDF_ERR_TOO_FEW, "sdf_infer(obj): sample %d has only %d lattice points inside its bbox, fewer than num_points=%d", b, co, g.no);
    }
    n_hand += ch; n_obj += co;
  }
  return HOISDF_OK;
}

// two events per device and host thread: fork and join of the side stream (recorded and waited for again on every call)
hipEvent_t* stream_events() {
  thread_local std::unordered_map<int, hipEvent_t*> pool;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  auto it = pool.find(dev);
  if (it != pool.end()) return it->second;
  hipEvent_t* ev = new hipEvent_t[2];
  for (int i = 0; i < 2; ++i)
    if (hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) { delete[] ev; return nullptr; }
  pool[dev] = ev;
  return ev;
}
// `to` waits for everything queued on `from` so far
int order_after(hipStream_t from, hipStream_t to, hipEvent_t ev) {
  if (from == to) return HOISDF_OK;
  if (hipEventRecord(ev, from) != hipSuccess || hipStreamWaitEvent(to, ev, 0) != hipSuccess) {
    set_error("pose_infer: ordering the two streams failed: %s", hipGetErrorString(hipGetLastError()));
    return HOISDF_ERR_LAUNCH;
  }
  return HOISDF_OK;
}
int recentre(const float* cam, long rows, int P, const float* c_other, float s_other, const float* c_own, float* cross, float* rel, hipStream_t st) {
  const long total = rows * 3;
  long blocks = cdiv(lmax(total >> 2, 1), 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(pose_recentre_kernel, dim3((unsigned)blocks), dim3(256), 0, st, cam, total, P, c_other, s_other, c_own, cross, rel);
  return check_launch("pose recentre");
}
}  // namespace

extern "C" long hoisdf_pose_prepared_bytes(const hoisdf_pose_desc* desc) {
  PGeo g;
  if (pose_geometry(desc, g)) return -1;
  Placer P(nullptr, 0, nullptr, false);
  Prep p;
  place_all(P, g, nullptr, p);
  return P.b.off + 256;
}

extern "C" int hoisdf_pose_prepare(const hoisdf_pose_desc* desc, const hoisdf_pose_weights* weights, void* prepared, long prepared_bytes,
                                   void* stream) {
  PGeo g;
  if (int rc = pose_geometry(desc, g)) return rc;
  HOISDF_REQUIRE(weights && prepared, HOISDF_ERR_INVALID, "pose_prepare: null pointer");
  HOISDF_REQUIRE((reinterpret_cast<uintptr_t>(prepared) & 255) == 0, HOISDF_ERR_INVALID, "pose_prepare: the blob must be 256-byte aligned");
  const long need = hoisdf_pose_prepared_bytes(desc);
  HOISDF_REQUIRE(prepared_bytes >= need, HOISDF_ERR_WORKSPACE, "pose_prepare: blob of %ld bytes, need %ld", prepared_bytes, need);
  Placer P(prepared, prepared_bytes, as_stream(stream), true);
  Prep p;
  const int rc = place_all(P, g, weights, p);
  if (rc == HOISDF_ERR_WORKSPACE) set_error("pose_prepare: blob of %ld bytes too small", prepared_bytes);
  return rc;
}

extern "C" int hoisdf_pose_infer_begin(const hoisdf_pose_desc* desc, const float* center_hand, const float* center_obj, const float* cam_intr,
                                       const float* bbox_hand, const float* bbox_obj, int32_t* counts_device, int32_t* counts_host,
                                       void* stream) {
  PGeo g;
  if (int rc = pose_geometry(desc, g)) return rc;
  HOISDF_REQUIRE(center_hand && center_obj && cam_intr && bbox_hand && bbox_obj && counts_device && counts_host, HOISDF_ERR_INVALID,
                 "pose_infer_begin: null pointer");
  if (int rc = hoisdf_sdf_infer_count_begin(center_hand, cam_intr, bbox_hand, desc->hand_sdf_scale, desc->bins_n, g.B, counts_device, counts_host, stream))
    return rc;
  return hoisdf_sdf_infer_count_begin(center_obj, cam_intr, bbox_obj, desc->obj_sdf_scale, desc->bins_n, g.B, counts_device + g.B, counts_host + g.B,
                                      stream);
}

extern "C" long hoisdf_pose_infer_workspace(const hoisdf_pose_desc* desc, const int32_t* counts_host) {
  PGeo g;
  if (pose_geometry(desc, g)) return -1;
  if (!counts_host) { set_error("pose_infer_workspace: null counts"); return -1; }
  long n_hand, n_obj;
  if (counts_total(g, counts_host, n_hand, n_obj, false)) return -1;
  Placer P(nullptr, 0, nullptr, false);
  Prep p;
  place_all(P, g, nullptr, p);
  Bump b(nullptr, 0);
  Frame f;
  carve_frame(desc, g, p, n_hand, n_obj, b, f);
  return b.off + 256;
}

extern "C" int hoisdf_pose_infer(const hoisdf_pose_desc* desc, const void* prepared, const hoisdf_pyramid* pyr, const float* center_hand,
                                 const float* center_obj, const float* cam_intr, const float* bbox_hand, const float* bbox_obj,
                                 const int32_t* counts_device, const int32_t* counts_host, const hoisdf_pose_outputs* out, void* workspace,
                                 long workspace_bytes, void* side_stream, void* stream) {
  PGeo g;
  if (int rc = pose_geometry(desc, g)) return rc;
  HOISDF_REQUIRE(prepared && pyr && center_hand && center_obj && cam_intr && bbox_hand && bbox_obj && counts_device && counts_host && workspace,
                 HOISDF_ERR_INVALID, "pose_infer: null pointer");
  HOISDF_REQUIRE(out && out->hand_joints_out && out->obj_rot_out && out->obj_trans_out &&
                     (g.ik ? out->mano_shape_out != nullptr : (out->mano_mesh_out && out->mano_joints_out)),
                 HOISDF_ERR_INVALID, "pose_infer: null output (%s)", g.ik ? "hand_joints / obj_rot / obj_trans / mano_shape" : "hand_joints / obj_rot / obj_trans / mano_mesh / mano_joints");
  HOISDF_REQUIRE(!g.iks || (out->mano_mesh_out && out->mano_joints_out && out->mano_pose_out), HOISDF_ERR_INVALID,
                 "pose_infer: null output (ik_solve needs mano_mesh_out / mano_joints_out / mano_pose_out)");
  HOISDF_REQUIRE(((reinterpret_cast<uintptr_t>(prepared) | reinterpret_cast<uintptr_t>(workspace)) & 255) == 0, HOISDF_ERR_INVALID,
                 "pose_infer: the prepared blob and the workspace must be 256-byte aligned");
  long pc = 0;
  for (int l = 0; l < pyr->n_levels && l < HOISDF_MAX_LEVELS; ++l) pc += pyr->C[l];
  HOISDF_REQUIRE(pyr->B == g.B && pc == g.C, HOISDF_ERR_INVALID, "pose_infer: pyramid of %d samples x %ld channels, descriptor says %d x %d", pyr->B, pc, g.B, g.C);
  long n_hand, n_obj;
  if (int rc = counts_total(g, counts_host, n_hand, n_obj, true)) return rc;
  const long need = hoisdf_pose_infer_workspace(desc, counts_host);
  HOISDF_REQUIRE(workspace_bytes >= need, HOISDF_ERR_INVALID, "pose_infer: workspace of %ld bytes, need %ld", workspace_bytes, need);

  Placer P(const_cast<void*>(prepared), 1L << 62, nullptr, false);
  Prep p;
  place_all(P, g, nullptr, p);
  Bump wb(workspace, workspace_bytes);
  Frame f;
  carve_frame(desc, g, p, n_hand, n_obj, wb, f);
  if (wb.overflow) { set_error("pose_infer: workspace too small"); return HOISDF_ERR_INVALID; }

  hipStream_t sh = as_stream(stream), so = side_stream ? as_stream(side_stream) : sh;
  void* vh = stream; void* vo = side_stream ? side_stream : stream;
  hipEvent_t* ev = nullptr;
  if (so != sh) {
    ev = stream_events();
    HOISDF_REQUIRE(ev, HOISDF_ERR_LAUNCH, "pose_infer: creating the stream events failed");
  }
  const int B = g.B, nh = g.nh, no = g.no, S = g.S, E = g.E, C = g.C, Fd = E - 33, ih = desc->img_h, iw = desc->img_w;
  const float hs_ = desc->hand_sdf_scale, os_ = desc->obj_sdf_scale, clamp = desc->clamping_distance;
  const float* hbeta = p.betas; const float* obeta = p.betas + 1;
  float* hand_pts = out->hand_points_out ? out->hand_points_out : f.hand_pts;
  float* obj_pts = out->obj_points_out ? out->obj_points_out : f.obj_pts;
  float* hand_sdf = out->hand_sdf_out ? out->hand_sdf_out : f.hand_sdf;
  float* obj_sdf = out->obj_sdf_out ? out->obj_sdf_out : f.obj_sdf;
  int rc;
#define STEP(call) do { rc = (call); if (rc) return rc; } while (0)

  // ---- the query points of both fields (main/model.py:462-481), on the main stream
  STEP(hoisdf_sdf_infer(pyr, center_hand, cam_intr, bbox_hand, hs_, desc->bins_n, B, counts_device, counts_host, nh, ih, iw, &p.sdf[0], clamp, 0.f, 0,
                        hand_pts, hand_sdf, f.hand_pe, f.scr_h, f.scr_h_bytes, vh));
  STEP(hoisdf_sdf_infer(pyr, center_obj, cam_intr, bbox_obj, os_, desc->bins_n, B, counts_device + B, counts_host + B, no, ih, iw, &p.sdf[1], clamp, 0.f,
                        0, obj_pts, obj_sdf, f.obj_pe, f.scr_h, f.scr_h_bytes, vh));
  if (so != sh) STEP(order_after(sh, so, ev[0]));
  // ---- object points (side stream): ONE gather feeds the token MLP and the evaluation of the same camera points in the hand field
  STEP(hoisdf_project_gather_fwd(pyr, obj_pts, nullptr, g.Mo, no, center_obj, cam_intr, os_, ih, iw, f.obj_feat, C, f.obj_cam, nullptr, vo));
  STEP(recentre(f.obj_cam, g.Mo, no, center_hand, hs_, nullptr, f.obj_h_pts, nullptr, so));                             // :495-518
  STEP(hoisdf_sdf_query_fwd(nullptr, f.obj_h_pts, nullptr, g.Mo, no, center_hand, cam_intr, hs_, ih, iw, f.obj_feat, nullptr, &p.sdf[0], clamp, 0.f, 0,
                            f.obj_h_sdf, f.obj_h_raw, f.obj_h_pe, nullptr, f.scr_o, f.scr_o_bytes, vo));
  STEP(hoisdf_tokens_fwd(nullptr, nullptr, center_obj, nullptr, 1.f, 0, 0, f.obj_feat, f.obj_cam, &p.tin, f.obj_pe, obj_sdf, obeta, f.obj_tok, f.obj_fea,
                         nullptr, B, no, S, 0, E, f.sav_o, f.sav_o_bytes, f.scr_o, f.scr_o_bytes, vo));
  // ---- hand points (main stream)
  STEP(hoisdf_project_gather_fwd(pyr, hand_pts, nullptr, g.Mh, nh, center_hand, cam_intr, hs_, ih, iw, f.hand_feat, C, f.hand_cam, nullptr, vh));
  STEP(recentre(f.hand_cam, g.Mh, nh, center_obj, os_, center_hand, f.hand_o_pts, f.hand_rel, sh));
  STEP(hoisdf_sdf_query_fwd(nullptr, f.hand_o_pts, nullptr, g.Mh, nh, center_obj, cam_intr, os_, ih, iw, f.hand_feat, nullptr, &p.sdf[1], clamp, 0.f, 0,
                            f.hand_o_sdf, f.hand_o_raw, f.hand_o_pe, nullptr, f.scr_h, f.scr_h_bytes, vh));
  if (so != sh) STEP(order_after(so, sh, ev[1]));
  // ---- token rows: own points first, then the cross-field rows with the OTHER centre (:498,:508 as the reference has them)
  STEP(hoisdf_tokens_fwd(nullptr, nullptr, center_hand, nullptr, 1.f, 0, 0, f.hand_feat, f.hand_cam, &p.tin, f.hand_pe, hand_sdf, hbeta, f.hand_tok,
                         f.hand_fea, nullptr, B, nh, S, 0, E, f.sav_h, f.sav_h_bytes, f.scr_h, f.scr_h_bytes, vh));
  STEP(hoisdf_token_build_fwd(f.obj_cam, center_hand, f.obj_h_pe, f.obj_fea, Fd, f.obj_h_sdf, hbeta, f.hand_tok, B, no, S, nh, E, vh));
  STEP(hoisdf_token_build_fwd(f.hand_cam, center_obj, f.hand_o_pe, f.hand_fea, Fd, f.hand_o_sdf, obeta, f.obj_tok, B, nh, S, no, E, vh));
  if (so != sh) STEP(order_after(sh, so, ev[0]));
  // ---- object encoder stack + its two heads (side stream); only the last layer's kept rows are normalised and read
  {
    const float* x = f.obj_tok;
    for (int i = 0; i < g.Lo; ++i) {
      const bool last = i == g.Lo - 1;
      const hoisdf_encoder_layer_desc ed = enc_desc(g, desc->attention, no, last);
      STEP(hoisdf_encoder_layer_fwd(x, &p.oe[i], &ed, f.ox[i & 1], last ? f.obj_enc : nullptr, nullptr, 0, f.scr_o, f.scr_o_bytes, vo));
      x = f.ox[i & 1];
    }
    Bump scr(f.scr_o, f.scr_o_bytes);
    Ctx c{so, vo, &scr, false, gemm_emu_mode()};
    const uint32_t* xm = nullptr;                  // obj_enc's row magnitudes: measured by the first chain, reused by the second
    const float* hr = head_hidden(c, p.rot, f.obj_enc, g.Mo, f.hid_o[0], f.hid_o[1], &xm);
    const float* ht = head_hidden(c, p.trans, f.obj_enc, g.Mo, f.hid_o[2], f.hid_o[3], &xm);
    if (!c.ok()) return c.rc;
    const HeadJob jobs[2] = {{hr, p.rot.w[2], p.rot.b[2], out->obj_rot_out, g.Mo, 3, 3, 1, 1, 0},
                             {ht, p.trans.w[2], p.trans.b[2], out->obj_trans_out, g.Mo, 3, 3, 1, 1, 0}};
    STEP(head_tail(jobs, 2, E, so));
  }
  // ---- hand encoder stack, decoder stack (main stream)
  {
    const float* x = f.hand_tok;
    for (int i = 0; i < g.Lh; ++i) {
      const bool last = i == g.Lh - 1;
      const hoisdf_encoder_layer_desc ed = enc_desc(g, desc->attention, nh, last);
      STEP(hoisdf_encoder_layer_fwd(x, &p.he[i], &ed, last ? f.memory : f.hx[i & 1], last ? f.hand_enc : nullptr, nullptr, 0, f.scr_h, f.scr_h_bytes, vh));
      x = f.hx[i & 1];
    }
    const hoisdf_decoder_layer_desc dd = dec_desc(g);
    const float* t = p.tgt0;
    for (int i = 0; i < g.Ld; ++i) {
      const bool last = i == g.Ld - 1;
      STEP(hoisdf_decoder_layer_fwd(t, f.memory, p.qembed, p.mask, &p.hd[i], &dd, f.dt[i & 1], last ? f.hs : nullptr, nullptr, 0, f.scr_h, f.scr_h_bytes, vh));
      t = f.dt[i & 1];
    }
  }
  if (so != sh) STEP(order_after(sh, so, ev[1]));
  // ---- MANO parameter heads + the MANO layer (side stream, under the vote heads of the main stream)
  {
    const long Mq = (long)B * g.Q;
    Bump scr(f.scr_o, f.scr_o_bytes);
    Ctx c{so, vo, &scr, false, gemm_emu_mode()};
    const float* hshape = head_hidden(c, p.shape, f.hs, Mq, f.hid_m[0], f.hid_m[1]);
    if (g.ik) {                                                                                                     // :595-597
      if (!c.ok()) return c.rc;
      const HeadJob job = {hshape, p.shape.w[2], p.shape.b[2], out->mano_shape_out, B, N_BETAS, N_BETAS, 1, 1, 0};
      STEP(head_tail(&job, 1, E, so));
    } else {                                                                                                        // :599-620
      const float* hpose = head_hidden(c, p.pose, f.hs, Mq, f.hid_m[2], f.hid_m[3]);
      if (!c.ok()) return c.rc;
      const HeadJob jobs[2] = {{hpose, p.pose.w[2], p.pose.b[2], f.pose6d, (long)B * 16, 6, 6, SHAPE_IDX, MANO_Q, 0},
                               {hshape, p.shape.w[2], p.shape.b[2], f.shape, B, N_BETAS, N_BETAS, 1, MANO_Q, SHAPE_IDX}};
      STEP(head_tail(jobs, 2, E, so));
      STEP(hoisdf_mano_head_fwd(f.pose6d, 96, 0, f.shape, N_BETAS, B, p.mano_image, p.mano_tmpl, p.mano_jreg, p.mano_w, p.mano_mean, nullptr, nullptr,
                                nullptr, nullptr, 0, 0, out->mano_mesh_out, out->mano_joints_out, f.rot, nullptr, vo));
    }
  }
  // ---- hand vote heads + vote aggregation (main stream): joints only, no loss reductions
  {
    Bump scr(f.scr_h, f.scr_h_bytes);
    Ctx c{sh, vh, &scr, false, gemm_emu_mode()};
    const uint32_t* xm = nullptr;
    const float* hv = head_hidden(c, p.vote, f.hand_enc, g.Mh, f.hid_h[0], f.hid_h[1], &xm);
    const float* hc = head_hidden(c, p.cls, f.hand_enc, g.Mh, f.hid_h[2], f.hid_h[3], &xm);
    if (!c.ok()) return c.rc;
    const HeadJob jobs[2] = {{hv, p.vote.w[3], p.vote.b[3], f.off, g.Mh, 3 * J_HAND, 3 * J_HAND, 1, 1, 0},
                             {hc, p.cls.w[2], p.cls.b[2], f.cls, g.Mh, J_HAND, J_HAND, 1, 1, 0}};
    STEP(head_tail(jobs, 2, E, sh));
    STEP(vote_only(f.off, f.cls, f.hand_rel, out->hand_joints_out, f.stats, B, nh, J_HAND, sh));
  }
  if (so != sh) STEP(order_after(so, sh, ev[0]));
  // ---- the IK variant's post-process (main/test.py:139-160): one launch behind the join, on the 20 voted joints and the shape
  if (g.iks)
    STEP(hoisdf_ik_mano_fwd(out->hand_joints_out, J_HAND, out->mano_shape_out, N_BETAS, B, p.mano_image, p.mano_tmpl, p.mano_jreg, p.mano_w,
                            out->mano_pose_out, out->mano_mesh_out, out->mano_joints_out, out->ik_valid_out, vh));
#undef STEP
  return HOISDF_OK;
}
