// Hand-object interaction LOSS (include/hoisdf.h "interaction loss"): the quantities of interact.hip in a form a model can be trained
// against - ObMan's repulsion of vertices that lie inside the other mesh and its saturating attraction of contact zones onto the
// surface - with the derivative towards BOTH vertex arrays.  From the pieces of mesh_sdf.hip: both meshes prepared by
// mesh_prepare_kernel, every vertex of one against the other by mesh_sdf_kernel, which leaves the winning face and the barycentric
// weights of the closest point: all the backward needs.
//   interact_loss_reduce_kernel  one block per sample: the three weighted sums and their three denominators, in fp64, thread t
//                                taking vertices t, t + 256, ... in ascending order and the 256 partial sums meeting in a fixed
//                                tree; rounded to fp32 once.  The denominators stay in the workspace for the backward.
//   interact_loss_bwd_kernel     one launch per destination mesh, one lane per destination vertex (a block is ONE wave of 64
//                                vertices), no atomics.  The derivative of sdf = s |p - c|, c = sum_k beta_k x_k the closest point on
//                                the winning face, s = -1 / +1 held piecewise constant, is the envelope rule d sdf / d p = s n,
//                                d sdf / d x_k = -beta_k s n with n = (p - c) / |p - c|, in the face, edge and corner regions alike.
//                                A vertex u therefore receives (1) its own term as a query point and (2) for every query point of
//                                the OTHER mesh whose winning face names u as corner k, -beta_k times that point's term.  (2) is a
//                                scan: the wave stages the other mesh's query records through LDS in tiles of 64 (lane j makes the
//                                record of query t0 + j from what the forward kept) and every lane walks the tile in ascending
//                                order, all lanes reading the same record (a broadcast: conflict-free), keeping what names its own
//                                vertex.  Sums in fp64, own term first, then ascending query index and corner 0, 1, 2 within a
//                                record: two calls give the same bits and a batch is its samples.
// Cost: Vdst x Nquery compares per sample (778 x 1000: under a million), records recomputed once per block of 64 destinations; the
// two mesh_sdf_kernel passes of the forward are where the time goes (profiles/interaction_loss_microbench.txt).
#include "mesh.h"

namespace hoisdf {

constexpr int IL_TILE = HOISDF_INTERACT_LOSS_TILE;
static_assert(IL_TILE == 64, "a tile is what one wave stages: one record per lane");

// the vertices of one mesh as query points against the prepared OTHER mesh, what the forward kept of them and how they are weighted
struct LossQueries {
  const float* pts; int N;                              // [B][N][3]
  const int32_t* n_count;                               // [B] or null: queries from n_count[b] on are padding and take no part
  const int32_t* own_n_faces; int own_max_faces;        // the face count of the mesh the points belong to: 0 = no mesh, no query
  const float4* tris; const float* box; int max_faces;  // the other mesh, prepared
  float* sdf; int32_t* face; float* bary;               // [B][N], [B][N], [B][N][3]: written by the forward's mesh_sdf_kernel
  const float* w_rep; long s_rep;                       // [N] per sample (stride 0: shared) or null = ones
  const float* w_att; long s_att; int has_att;          // the attraction term exists for the hand's vertices only
  const float* g_rep; const float* g_att;               // upstream gradients [B] or null (backward)
  int den_rep, den_att;                                 // the columns of den[b][4] that hold the two denominators
};

__device__ __forceinline__ int live_queries(const LossQueries& q, int b) {
  if (sample_faces(q.own_n_faces, b, q.own_max_faces) == 0) return 0;
  return q.n_count ? min(max(q.n_count[b], 0), q.N) : q.N;
}
__device__ __forceinline__ float weight_of(const float* w, long stride, int b, int i) { return w ? w[(size_t)b * stride + i] : 1.f; }

struct LossReduceArgs {
  LossQueries ho, oh;                    // hand vertices against the object, object vertices against the hand
  float alpha;
  float *rep_hand, *att, *rep_obj;       // [B]
  double* den;                           // [B][4]: sum of rep_w_hand, of att_w_hand, of rep_w_obj (over the vertices that count), 0
};

__global__ __launch_bounds__(256) void interact_loss_reduce_kernel(const LossReduceArgs a) {
  __shared__ double s[6][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  double acc[6] = {0., 0., 0., 0., 0., 0.};              // rep_hand, att, rep_obj and their denominators
  const double alpha = (double)a.alpha;
  {
    const LossQueries& q = a.ho;
    const int n = live_queries(q, b);
    for (int v = tid; v < n; v += 256) {
      const double wr = (double)weight_of(q.w_rep, q.s_rep, b, v), wa = (double)weight_of(q.w_att, q.s_att, b, v);
      acc[3] += wr;
      acc[4] += wa;
      const size_t o = (size_t)b * q.N + v;
      if (q.face[o] < 0) continue;                       // no usable face: 3e38 away, adds nothing
      const double sd = (double)q.sdf[o];
      acc[0] += wr * fmax(0., -sd);
      acc[1] += wa * (alpha * tanh(fmax(0., sd) / alpha));
    }
  }
  {
    const LossQueries& q = a.oh;
    const int n = live_queries(q, b);
    for (int v = tid; v < n; v += 256) {
      const double wr = (double)weight_of(q.w_rep, q.s_rep, b, v);
      acc[5] += wr;
      const size_t o = (size_t)b * q.N + v;
      if (q.face[o] < 0) continue;
      acc[2] += wr * fmax(0., -(double)q.sdf[o]);
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k][tid] = acc[k];
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {                    // a fixed tree: s[t] += s[t + o]
    if (tid < o)
#pragma unroll
      for (int k = 0; k < 6; ++k) s[k][tid] += s[k][tid + o];
    __syncthreads();
  }
  if (tid != 0) return;
  float* out[3] = {a.rep_hand, a.att, a.rep_obj};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double den = s[3 + k][0];
    out[k][b] = den > 0. ? (float)(s[k][0] / den) : 0.f;
    a.den[(size_t)b * 4 + k] = den;
  }
  a.den[(size_t)b * 4 + 3] = 0.;
}

// What query point i of sample b passes on: g = coef s n (its own gradient) and the winning face's corners with their weights (each
// corner k receives -beta_k g).  i0 < 0: nothing - padding, no usable face, d = 0, or a term whose derivative is zero.
struct LossRecord { float g[3]; float beta[3]; int idx[3]; };

__device__ __forceinline__ LossRecord query_record(const LossQueries& q, const double* __restrict__ den, float alpha, int b, int i) {
  LossRecord r;
  r.g[0] = r.g[1] = r.g[2] = 0.f;
  r.beta[0] = r.beta[1] = r.beta[2] = 0.f;
  r.idx[0] = r.idx[1] = r.idx[2] = -1;
  if (i >= live_queries(q, b)) return r;
  const size_t o = (size_t)b * q.N + i;
  const int f = q.face[o];
  if (f < 0 || f >= q.max_faces) return r;
  const float sd = q.sdf[o];
  // coef = d(term)/d(sdf) x weight / denominator x upstream, in fp64
  double coef = 0.;
  if (q.g_rep && sd < 0.f) {
    const double d = den[(size_t)b * 4 + q.den_rep];
    if (d > 0.) coef -= (double)q.g_rep[b] * (double)weight_of(q.w_rep, q.s_rep, b, i) / d;
  }
  if (q.has_att && q.g_att && sd > 0.f) {
    const double d = den[(size_t)b * 4 + q.den_att];
    const double th = tanh((double)sd / (double)alpha);
    if (d > 0.) coef += (double)q.g_att[b] * (double)weight_of(q.w_att, q.s_att, b, i) / d * (1. - th * th);
  }
  if (coef == 0.) return r;
  // n = (p - c) / |p - c| in the mesh's own frame (centred on its box, as the forward measured), c from the kept weights
  const float* bx = q.box + (size_t)b * 8;
  const float* pt = q.pts + o * 3;
  const f3 p = {pt[0] - bx[0], pt[1] - bx[1], pt[2] - bx[2]};
  const float4* t = q.tris + ((size_t)b * q.max_faces + f) * 3;
  const float4 A = t[0], Bq = t[1], Cq = t[2];
  const f3 va = xyz(A), ab = sub(xyz(Bq), va), ac = sub(xyz(Cq), va), ap = sub(p, va);
  const float v = q.bary[o * 3 + 1], w = q.bary[o * 3 + 2];
  const f3 d = {ap.x - v * ab.x - w * ac.x, ap.y - v * ab.y - w * ac.y, ap.z - v * ab.z - w * ac.z};
  const float dd = dot(d, d);
  if (!(dd > 0.f)) return r;                             // on the surface: no direction, no gradient
  const float cs = (float)(sd < 0.f ? -coef : coef) / sqrtf(dd);
  r.g[0] = cs * d.x; r.g[1] = cs * d.y; r.g[2] = cs * d.z;
  r.beta[0] = q.bary[o * 3]; r.beta[1] = v; r.beta[2] = w;
  r.idx[0] = __float_as_int(A.w); r.idx[1] = __float_as_int(Bq.w); r.idx[2] = __float_as_int(Cq.w);
  return r;
}

struct LossBwdArgs {
  LossQueries own;                       // the destination mesh's vertices as query points
  LossQueries other;                     // the other mesh's vertices: their winning faces name destination vertices
  const double* den;
  float alpha;
  float* d_out;                          // [B][own.N][3]: every row written
};

__global__ __launch_bounds__(IL_TILE) void interact_loss_bwd_kernel(const LossBwdArgs a) {
  __shared__ float s_g[IL_TILE][3], s_b[IL_TILE][3];
  __shared__ int s_i[IL_TILE][3];
  const int b = blockIdx.y, lane = threadIdx.x, u = blockIdx.x * IL_TILE + lane;
  double acc[3] = {0., 0., 0.};
  if (u < a.own.N) {
    const LossRecord r = query_record(a.own, a.den, a.alpha, b, u);
    if (r.idx[0] >= 0) { acc[0] = (double)r.g[0]; acc[1] = (double)r.g[1]; acc[2] = (double)r.g[2]; }
  }
  const int nq = live_queries(a.other, b);
  for (int t0 = 0; t0 < nq; t0 += IL_TILE) {
    const int cnt = min(IL_TILE, nq - t0);
    __syncthreads();
    {
      const LossRecord r = query_record(a.other, a.den, a.alpha, b, t0 + lane);      // past the last query: an empty record
#pragma unroll
      for (int k = 0; k < 3; ++k) { s_g[lane][k] = r.g[k]; s_b[lane][k] = r.beta[k]; s_i[lane][k] = r.idx[k]; }
    }
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {                      // ascending query index; every lane reads the same record
      if (s_i[j][0] < 0) continue;                       // (the same for every lane)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        if (s_i[j][k] == u) {
          const double bk = (double)s_b[j][k];
          acc[0] -= bk * (double)s_g[j][0];
          acc[1] -= bk * (double)s_g[j][1];
          acc[2] -= bk * (double)s_g[j][2];
        }
    }
  }
  if (u >= a.own.N) return;
  float* o = a.d_out + ((size_t)b * a.own.N + u) * 3;
  o[0] = (float)acc[0]; o[1] = (float)acc[1]; o[2] = (float)acc[2];
}

// ---- workspace: both prepared meshes, then per direction sdf / face / bary, then the denominators -----------------------------------
// The forward writes it and the backward reads it: one layout function for both and for the size query.
struct LossWorkspace { MeshPair m; VertexSdf ho, oh; double* den; };

static VertexSdf vertex_sdf(Bump& w, long B, long V) {
  VertexSdf v;
  v.sdf = w.floats(B * V);
  v.face = w.ints(B * V);
  v.bary = w.floats(B * V * 3);
  return v;
}
static LossWorkspace loss_workspace(Bump& w, long B, long Vh, long Fh, long Vo, long Fo) {
  LossWorkspace s;
  s.m = mesh_pair(w, B, Fh, Fo);
  s.ho = vertex_sdf(w, B, Vh);
  s.oh = vertex_sdf(w, B, Vo);
  s.den = (double*)w.take(B * 32);
  return s;
}

struct LossWeights { const float *rep_w_hand, *att_w_hand, *rep_w_obj; long s_rep_hand, s_att_hand, s_rep_obj; };

// every check the two entries share, before any launch, and the workspace laid out into *s; > 0: B = 0, nothing to do
static int loss_check(const char* what, const hoisdf_mesh* hand, const hoisdf_mesh* obj, int B, const LossWeights& w, float alpha,
                      const void* workspace, long workspace_bytes, LossWorkspace* s) {
  if (!mesh_desc_ok(what, "hand", hand, B) || !mesh_desc_ok(what, "obj", obj, B)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(alpha > 0.f && alpha <= 3.0e38f, HOISDF_ERR_INVALID, "%s: alpha=%g (> 0, finite)", what, (double)alpha);
  HOISDF_REQUIRE(w.s_rep_hand == 0 || w.s_rep_hand == hand->V, HOISDF_ERR_INVALID, "%s: rep_w_hand_stride=%ld (0 or hand V)", what, w.s_rep_hand);
  HOISDF_REQUIRE(w.s_att_hand == 0 || w.s_att_hand == hand->V, HOISDF_ERR_INVALID, "%s: att_w_hand_stride=%ld (0 or hand V)", what, w.s_att_hand);
  HOISDF_REQUIRE(w.s_rep_obj == 0 || w.s_rep_obj == obj->V, HOISDF_ERR_INVALID, "%s: rep_w_obj_stride=%ld (0 or obj V)", what, w.s_rep_obj);
  if (B == 0) return 1;
  if (!mesh_data_ok(what, "hand", hand) || !mesh_data_ok(what, "obj", obj)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(workspace, HOISDF_ERR_INVALID, "%s: null pointer (workspace)", what);
  Bump bump(const_cast<void*>(workspace), workspace_bytes);
  *s = loss_workspace(bump, B, hand->V, hand->max_faces, obj->V, obj->max_faces);
  HOISDF_REQUIRE(workspace_bytes >= bump.bytes(), HOISDF_ERR_INVALID, "%s: workspace of %ld bytes, %ld needed", what, workspace_bytes,
                 bump.bytes());
  return 0;
}

static void loss_queries(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* obj_n_verts, const LossWeights& w,
                         const LossWorkspace& s, const float* g_rep_hand, const float* g_att, const float* g_rep_obj, LossQueries* ho,
                         LossQueries* oh) {
  *ho = {hand->verts, hand->V, nullptr, hand->n_faces, hand->max_faces, s.m.obj.tris, s.m.obj.box, obj->max_faces, s.ho.sdf, s.ho.face, s.ho.bary, w.rep_w_hand, w.s_rep_hand,
         w.att_w_hand, w.s_att_hand, 1, g_rep_hand, g_att, 0, 1};
  *oh = {obj->verts, obj->V, obj_n_verts, obj->n_faces, obj->max_faces, s.m.hand.tris, s.m.hand.box, hand->max_faces, s.oh.sdf, s.oh.face, s.oh.bary, w.rep_w_obj, w.s_rep_obj,
         nullptr, 0, 0, g_rep_obj, nullptr, 2, 2};
}

}  // namespace hoisdf

using namespace hoisdf;


extern "C" long hoisdf_interaction_loss_workspace_bytes(int B, int hand_V, int hand_max_faces, int obj_V, int obj_max_faces) {
  if (!mesh_shape_ok("interaction_loss_workspace_bytes (hand)", B, hand_V, hand_max_faces) ||
      !mesh_shape_ok("interaction_loss_workspace_bytes (obj)", B, obj_V, obj_max_faces))
    return -1;
  Bump w(nullptr, 0);
  loss_workspace(w, B, hand_V, hand_max_faces, obj_V, obj_max_faces);
  return w.bytes();
}

extern "C" int hoisdf_interaction_loss_fwd(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* obj_n_verts, int B,
                                           const float* rep_w_hand, long rep_w_hand_stride, const float* att_w_hand,
                                           long att_w_hand_stride, const float* rep_w_obj, long rep_w_obj_stride, float alpha,
                                           float* rep_hand, float* att, float* rep_obj, void* workspace, long workspace_bytes,
                                           void* stream) {
  const LossWeights w = {rep_w_hand, att_w_hand, rep_w_obj, rep_w_hand_stride, att_w_hand_stride, rep_w_obj_stride};
  LossWorkspace s;
  const int rc = loss_check("interaction_loss_fwd", hand, obj, B, w, alpha, workspace, workspace_bytes, &s);
  if (rc != 0) return rc > 0 ? HOISDF_OK : rc;
  HOISDF_REQUIRE(rep_hand && att && rep_obj, HOISDF_ERR_INVALID, "interaction_loss_fwd: null pointer (rep_hand, att, rep_obj)");
  hipStream_t st = as_stream(stream);
  launch_both_ways(*hand, *obj, B, s.m, s.ho, s.oh, st);
  LossReduceArgs ra;
  loss_queries(hand, obj, obj_n_verts, w, s, nullptr, nullptr, nullptr, &ra.ho, &ra.oh);
  ra.alpha = alpha;
  ra.rep_hand = rep_hand; ra.att = att; ra.rep_obj = rep_obj;
  ra.den = s.den;
  hipLaunchKernelGGL(interact_loss_reduce_kernel, dim3(B), dim3(256), 0, st, ra);
  return check_launch("interaction_loss_fwd");
}

extern "C" int hoisdf_interaction_loss_bwd(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* obj_n_verts, int B,
                                           const float* rep_w_hand, long rep_w_hand_stride, const float* att_w_hand,
                                           long att_w_hand_stride, const float* rep_w_obj, long rep_w_obj_stride, float alpha,
                                           const float* g_rep_hand, const float* g_att, const float* g_rep_obj, float* d_hand_verts,
                                           float* d_obj_verts, const void* workspace, long workspace_bytes, void* stream) {
  const LossWeights w = {rep_w_hand, att_w_hand, rep_w_obj, rep_w_hand_stride, att_w_hand_stride, rep_w_obj_stride};
  LossWorkspace s;
  const int rc = loss_check("interaction_loss_bwd", hand, obj, B, w, alpha, workspace, workspace_bytes, &s);
  if (rc != 0) return rc > 0 ? HOISDF_OK : rc;
  HOISDF_REQUIRE(d_hand_verts && d_obj_verts, HOISDF_ERR_INVALID, "interaction_loss_bwd: null pointer (d_hand_verts, d_obj_verts)");
  hipStream_t st = as_stream(stream);
  LossQueries ho, oh;
  loss_queries(hand, obj, obj_n_verts, w, s, g_rep_hand, g_att, g_rep_obj, &ho, &oh);
  const LossBwdArgs to_hand = {ho, oh, s.den, alpha, d_hand_verts}, to_obj = {oh, ho, s.den, alpha, d_obj_verts};
  hipLaunchKernelGGL(interact_loss_bwd_kernel, dim3(cdiv(hand->V, IL_TILE), B), dim3(IL_TILE), 0, st, to_hand);
  hipLaunchKernelGGL(interact_loss_bwd_kernel, dim3(cdiv(obj->V, IL_TILE), B), dim3(IL_TILE), 0, st, to_obj);
  return check_launch("interaction_loss_bwd");
}
