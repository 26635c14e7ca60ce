// SDF supervision from meshes: the rows [x y z sdf_hand sdf_obj label] that tool/pre_process_sdf.py:140-148 repacks from an
// offline CPU mesh-to-SDF pass, computed on the device from the two meshes of the step (include/hoisdf.h "mesh SDF").
//   mesh_prepare_kernel  one block per sample: bounding box of the vertices -> centre; every face gathered, re-centred, its normal
//                        and area taken; the inclusive area prefix sum (fixed order: two calls give the same bits)
//   mesh_sample_kernel   counter-based query points: area-weighted face + uniform barycentrics + Gaussian noise, or uniform in the
//                        padded box; the kind of point i is a function of i alone
//   mesh_sdf_kernel      brute force point x triangle: exact closest point (Ericson, Real-Time Collision Detection 5.1.5) and the
//                        triangle's solid angle (Van Oosterom & Strackee 1983); sign from the winding number
// Why brute force: F <= HOISDF_MESH_MAX_FACES and a few thousand points per sample are ~1e7 pairs per sample of ~150 VALU
// instructions each, all of them independent; a hierarchy would add divergence and a build per step for nothing.
// Shape of the hot kernel: a block is 64 points (one per lane) x 4 waves; the block's 256 threads stage the sample's triangles
// through LDS in tiles of MESH_TILE faces x 48 bytes, and wave s takes faces s, s + 4, ... of every tile for the block's 64 points.
// All 64 lanes of a wave read the same three float4 of the same triangle: identical addresses broadcast, so the reads are
// conflict-free whatever the banking, and three ds_read_b128 per ~150 VALU instructions leave the LDS idle.  Splitting the FACES
// over the waves and not the points is what fills the machine: 32 x 3200 points are only 1600 waves for 1024 SIMDs, and the
// per-pair work is one long dependent chain (dots -> region -> reciprocal -> distance; dots -> square roots -> polynomial), so
// one or two waves per SIMD leave it waiting on its own latencies.  Measured at the training shape (profiles/mesh_sdf_microbench.txt):
// one thread per point over all faces, library atan2f / sqrtf and divergent region branches 3.74 ms; this form 1.69 ms.
// The four partial answers of a point meet in LDS and wave 0 combines them in wave order: strictly nearer wins, the LOWER face
// index on an exact tie - so the nearest face is the lowest index among equals whatever the tile and wave order - and the angle
// sums are added in one fixed order.
// The vector helpers, atan2_poly, MeshSdfArgs, the workspace layout and the declarations of the descriptor check and the launches
// that the other mesh files run as well are in mesh.h.
#include "mesh.h"

namespace hoisdf {

// ---- a. triangle preparation -----------------------------------------------------------------------------------------------------
// tris [B][max_faces][3] float4: (a, b, c) - centre, .w = the bits of the three vertex indices; a.w = -1 marks a skipped face.
// box [B][8]: centre xyz, total area, half extent xyz, 0.
__global__ __launch_bounds__(256) void mesh_prepare_kernel(const float* __restrict__ verts, int V, const int32_t* __restrict__ faces,
                                                           long face_stride, const int32_t* __restrict__ n_faces, int max_faces,
                                                           float4* __restrict__ tris, float* __restrict__ area,
                                                           float* __restrict__ cdf, float* __restrict__ box) {
  __shared__ float s_red[6][4];
  __shared__ float s_part[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* v = verts + (size_t)b * V * 3;
  float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
  for (int i = tid; i < V; i += 256)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float x = v[(size_t)i * 3 + k];
      lo[k] = fminf(lo[k], x);
      hi[k] = fmaxf(hi[k], x);
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float m = -wave_max(-lo[k]), M = wave_max(hi[k]);
    if ((tid & 63) == 0) { s_red[k][tid >> 6] = m; s_red[3 + k][tid >> 6] = M; }
  }
  __syncthreads();
  float ctr[3], half[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float m = fminf(fminf(s_red[k][0], s_red[k][1]), fminf(s_red[k][2], s_red[k][3]));
    const float M = fmaxf(fmaxf(s_red[3 + k][0], s_red[3 + k][1]), fmaxf(s_red[3 + k][2], s_red[3 + k][3]));
    ctr[k] = 0.5f * (m + M);
    half[k] = 0.5f * (M - m);
  }
  const f3 c0 = {ctr[0], ctr[1], ctr[2]};
  const int nf = sample_faces(n_faces, b, max_faces);
  const int32_t* fb = faces + (size_t)b * face_stride;
  float4* tb = tris + (size_t)b * max_faces * 3;
  float* ab = area + (size_t)b * max_faces;
  float* cb = cdf + (size_t)b * max_faces;
  // thread t owns faces [t per, (t + 1) per): its areas are summed in index order, the 256 partial sums scanned in thread order
  const int per = (nf + 255) / 256;
  const int f0 = min(tid * per, nf), f1 = min(f0 + per, nf);
  float run = 0.f;
  for (int f = f0; f < f1; ++f) {
    const int i0 = fb[(size_t)f * 3], i1 = fb[(size_t)f * 3 + 1], i2 = fb[(size_t)f * 3 + 2];
    float4 A = {0.f, 0.f, 0.f, __int_as_float(-1)}, Bq = {0.f, 0.f, 0.f, 0.f}, Cq = {0.f, 0.f, 0.f, 0.f};
    float ar = 0.f;
    if ((unsigned)i0 < (unsigned)V && (unsigned)i1 < (unsigned)V && (unsigned)i2 < (unsigned)V) {   // an index outside the mesh: skipped, never read
      const f3 pa = sub({v[(size_t)i0 * 3], v[(size_t)i0 * 3 + 1], v[(size_t)i0 * 3 + 2]}, c0);
      const f3 pb = sub({v[(size_t)i1 * 3], v[(size_t)i1 * 3 + 1], v[(size_t)i1 * 3 + 2]}, c0);
      const f3 pc = sub({v[(size_t)i2 * 3], v[(size_t)i2 * 3 + 1], v[(size_t)i2 * 3 + 2]}, c0);
      const f3 n = cross_unfused(sub(pb, pa), sub(pc, pa));
      const bool skip = n.x == 0.f && n.y == 0.f && n.z == 0.f;
      ar = skip ? 0.f : 0.5f * sqrtf(dot(n, n));
      A = {pa.x, pa.y, pa.z, __int_as_float(skip ? -1 : i0)};
      Bq = {pb.x, pb.y, pb.z, __int_as_float(i1)};
      Cq = {pc.x, pc.y, pc.z, __int_as_float(i2)};
    }
    tb[(size_t)f * 3] = A;
    tb[(size_t)f * 3 + 1] = Bq;
    tb[(size_t)f * 3 + 2] = Cq;
    ab[f] = ar;
    run += ar;
    cb[f] = run;                                       // the thread's own running sum; its offset is added below
  }
  s_part[tid] = run;
  __syncthreads();
  if (tid == 0) {
    float acc = 0.f;
    for (int t = 0; t < 256; ++t) { const float x = s_part[t]; s_part[t] = acc; acc += x; }
    float* bx = box + (size_t)b * 8;
    bx[0] = ctr[0]; bx[1] = ctr[1]; bx[2] = ctr[2]; bx[3] = acc;
    bx[4] = half[0]; bx[5] = half[1]; bx[6] = half[2]; bx[7] = 0.f;
  }
  __syncthreads();
  const float off = s_part[tid];
  for (int f = f0; f < f1; ++f) cb[f] += off;
}

// ---- b. point sampler ------------------------------------------------------------------------------------------------------------
// draw c (0..7) of point i of sample b: one hash of (seed, b, 8 i + c), the construction of sample.hip
__device__ __forceinline__ uint32_t draw24(uint32_t sk, uint32_t i, uint32_t c) { return mix32(((i * 8u + c) * 0x85EBCA77U) ^ sk) >> 8; }
__device__ __forceinline__ float u01(uint32_t h24) { return (float)h24 * (1.0f / 16777216.0f); }                  // [0, 1)
__device__ __forceinline__ float u01_open(uint32_t h24) { return ((float)h24 + 0.5f) * (1.0f / 16777216.0f); }    // (0, 1)

// kind of point i: 2 = uniform in the padded box (the last of every `uniform_every` points; never when uniform_every <= 0),
// else 0 = sigma1 (even position in its group), 1 = sigma2 (odd position)
__device__ __forceinline__ int point_kind(int i, int uniform_every) {
  const int k = uniform_every > 0 ? i % uniform_every : i;
  return (uniform_every > 0 && k == uniform_every - 1) ? 2 : (k & 1);
}

__global__ __launch_bounds__(256) void mesh_sample_kernel(const float4* __restrict__ tris, const float* __restrict__ cdf,
                                                          const float* __restrict__ box, const int32_t* __restrict__ n_faces,
                                                          int max_faces, int N, float sigma1, float sigma2, int uniform_every,
                                                          float pad, uint64_t seed, float* __restrict__ points, long pstride,
                                                          int ldp, int32_t* __restrict__ face_out) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const float* bx = box + (size_t)b * 8;
  const int nf = sample_faces(n_faces, b, max_faces);
  const float total = bx[3];
  const uint32_t sk = drop_rowkey(seed, (uint32_t)b);
  int kind = point_kind(i, uniform_every);
  if (!(total > 0.f)) kind = 2;                        // no face has an area: every point is a box point
  float px, py, pz;
  int face = -1;
  if (kind == 2) {
    px = (2.f * u01(draw24(sk, i, 0)) - 1.f) * (bx[4] + pad);
    py = (2.f * u01(draw24(sk, i, 1)) - 1.f) * (bx[5] + pad);
    pz = (2.f * u01(draw24(sk, i, 2)) - 1.f) * (bx[6] + pad);
  } else {
    const float* cb = cdf + (size_t)b * max_faces;
    const float target = u01(draw24(sk, i, 0)) * total;
    int lo = 0, hi = nf;                               // first face with cdf > target: a face of area 0 never is
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cb[mid] > target) hi = mid; else lo = mid + 1;
    }
    if (lo >= nf) {                                    // target rounded up to the total: the face at which the sum reaches it
      lo = 0; hi = nf - 1;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cb[mid] >= total) hi = mid; else lo = mid + 1;
      }
    }
    face = lo;
    const float4* t = tris + ((size_t)b * max_faces + face) * 3;
    const float4 A = t[0], Bq = t[1], Cq = t[2];
    const float s = sqrtf(u01(draw24(sk, i, 1))), u2 = u01(draw24(sk, i, 2));
    const float wa = 1.f - s, wb = s * (1.f - u2), wc = s * u2;
    const float sg = kind == 0 ? sigma1 : sigma2;
    // Box-Muller on two pairs of draws: three of the four normals
    const float r0 = sqrtf(-2.f * __logf(u01_open(draw24(sk, i, 3)))), a0 = 6.2831853071795865f * u01(draw24(sk, i, 4));
    const float r1 = sqrtf(-2.f * __logf(u01_open(draw24(sk, i, 5)))), a1 = 6.2831853071795865f * u01(draw24(sk, i, 6));
    px = wa * A.x + wb * Bq.x + wc * Cq.x + sg * r0 * __cosf(a0);
    py = wa * A.y + wb * Bq.y + wc * Cq.y + sg * r0 * __sinf(a0);
    pz = wa * A.z + wb * Bq.z + wc * Cq.z + sg * r1 * __cosf(a1);
  }
  float* o = points + (size_t)b * pstride + (size_t)i * ldp;       // pstride: floats between the sets of two samples
  o[0] = px + bx[0];
  o[1] = py + bx[1];
  o[2] = pz + bx[2];
  if (face_out) face_out[(size_t)b * N + i] = face;
}

// ---- c. signed distance ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mesh_sdf_kernel(const MeshSdfArgs a) {
  __shared__ float4 s_tri[MESH_TILE * 3];
  __shared__ float s_best[256], s_v[256], s_w[256], s_om[256];
  __shared__ int s_face[256];
  const int b = blockIdx.y, tid = threadIdx.x, slice = tid >> 6, i = blockIdx.x * MESH_PTS + (tid & 63);
  const bool live = i < a.N;
  const float* bx = a.box + (size_t)b * 8;
  f3 p = {0.f, 0.f, 0.f};
  if (live) {
    const float* q = a.points + ((size_t)b * a.N + i) * a.ldp;
    p = {q[0] - bx[0], q[1] - bx[1], q[2] - bx[2]};
  }
  const int nf = sample_faces(a.n_faces, b, a.max_faces);
  const float4* tb = a.tris + (size_t)b * a.max_faces * 3;
  float best = 3.0e38f, bv = 0.f, bw = 0.f, omega = 0.f;
  int bf = -1;
  for (int t0 = 0; t0 < nf; t0 += MESH_TILE) {
    const int cnt = min(MESH_TILE, nf - t0);
    __syncthreads();
    for (int k = tid; k < cnt * 3; k += 256) s_tri[k] = tb[(size_t)t0 * 3 + k];
    __syncthreads();
    for (int j = slice; j < cnt; j += MESH_SLICES) {   // this wave's faces, in ascending order
      const float4 A = s_tri[j * 3], Bq = s_tri[j * 3 + 1], Cq = s_tri[j * 3 + 2];
      if (__float_as_int(A.w) < 0) continue;           // a skipped face (the same for every lane): neither distance nor sign
      const f3 va = xyz(A), vb = xyz(Bq), vc = xyz(Cq);
      const f3 ab = sub(vb, va), ac = sub(vc, va);
      const f3 ap = sub(p, va), bp = sub(p, vb), cp = sub(p, vc);
      // closest point of the triangle, as barycentrics (1 - v - w, v, w) = (., nv, nw) / den.  Regions in the order corner a, b, c,
      // edge ab, ac, bc, face: the later assignment overrides, so the chain runs backwards; selects, no divergent branch
      const float d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp);
      const float ec = d1 * d4 - d3 * d2, eb = d5 * d2 - d1 * d6, ea = d3 * d6 - d5 * d4, e3 = d4 - d3, e4 = d5 - d6;
      float nv = eb, nw = ec, den = ea + eb + ec;
      if (ea <= 0.f && e3 >= 0.f && e4 >= 0.f) { nv = e4; nw = e3; den = e3 + e4; }
      if (eb <= 0.f && d2 >= 0.f && d6 <= 0.f) { nv = 0.f; nw = d2; den = d2 - d6; }
      if (ec <= 0.f && d1 >= 0.f && d3 <= 0.f) { nv = d1; nw = 0.f; den = d1 - d3; }
      if (d6 >= 0.f && d5 <= d6) { nv = 0.f; nw = 1.f; den = 1.f; }
      if (d3 >= 0.f && d4 <= d3) { nv = 1.f; nw = 0.f; den = 1.f; }
      if (d1 <= 0.f && d2 <= 0.f) { nv = 0.f; nw = 0.f; den = 1.f; }
      const float inv = __builtin_amdgcn_rcpf(den);    // 1 ulp: 1e-7 of an edge, 1e-9 m
      const float v = nv * inv, w = nw * inv;
      const f3 r = {ap.x - v * ab.x - w * ac.x, ap.y - v * ab.y - w * ac.y, ap.z - v * ab.z - w * ac.z};
      const float dd = dot(r, r);
      if (dd < best) { best = dd; bf = t0 + j; bv = v; bw = w; }      // strict: the lowest face index of this wave's wins a tie
      // solid angle of (a, b, c) - p:  2 atan2(det, |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|);  (a, b, c) - p = -(ap, bp, cp)
      const float la = __builtin_amdgcn_sqrtf(dot(ap, ap)), lb = __builtin_amdgcn_sqrtf(dot(bp, bp)), lc = __builtin_amdgcn_sqrtf(dot(cp, cp));
      const float det = ap.x * (bp.y * cp.z - bp.z * cp.y) + ap.y * (bp.z * cp.x - bp.x * cp.z) + ap.z * (bp.x * cp.y - bp.y * cp.x);
      const float den_w = la * lb * lc + dot(ap, bp) * lc + dot(bp, cp) * la + dot(cp, ap) * lb;
      omega += atan2_poly(-det, den_w);
    }
  }
  // the four waves' answers for a point, combined by wave 0 in wave order: the nearest face, the LOWEST index on an exact tie
  // (a wave's faces interleave with the others'), and the angle sums in one fixed order
  s_best[tid] = best; s_face[tid] = bf; s_v[tid] = bv; s_w[tid] = bw; s_om[tid] = omega;
  __syncthreads();
  if (slice != 0 || !live) return;
#pragma unroll
  for (int s = 1; s < MESH_SLICES; ++s) {
    const int k = tid + 64 * s;
    const float dd = s_best[k];
    const int f = s_face[k];
    if (dd < best || (dd == best && f >= 0 && f < bf)) { best = dd; bf = f; bv = s_v[k]; bw = s_w[k]; }
    omega += s_om[k];
  }
  const size_t o = (size_t)b * a.N + i;
  const float wind = omega * (2.f / 12.566370614359172f);
  const float dist = bf < 0 ? 3.0e38f : sqrtf(best);   // a mesh without a usable face: +huge, outside
  const float sdf = wind > 0.5f ? -dist : dist;
  a.sdf[o * a.ld] = sdf;
  if (a.face_out) a.face_out[o] = bf;
  const float wa = 1.f - bv - bw;
  if (a.bary_out) { a.bary_out[o * 3] = wa; a.bary_out[o * 3 + 1] = bv; a.bary_out[o * 3 + 2] = bw; }
  if (a.winding_out) a.winding_out[o] = wind;
  if (a.label_out || a.label_f) {
    int lab = -1;
    if (bf >= 0 && a.vert_label) {
      int k = 0;                                       // the corner with the largest weight; the earlier corner on a tie
      float m = wa;
      if (bv > m) { m = bv; k = 1; }
      if (bw > m) { k = 2; }
      const int corner = __float_as_int(tb[(size_t)bf * 3 + k].w);
      lab = a.vert_label[(size_t)b * a.label_stride + corner];
    }
    if (a.label_out) a.label_out[o] = lab;
    if (a.label_f) a.label_f[o * a.ld] = (i < a.n_label && fabsf(sdf) <= a.clamp) ? (float)lab : -1.f;
  }
}

// ---- launches --------------------------------------------------------------------------------------------------------------------
bool mesh_shape_ok(const char* what, int B, int V, int max_faces) {
  if (B < 0 || B > 65535 || V < 0 || max_faces < 0 || max_faces > HOISDF_MESH_MAX_FACES) {
    set_error("%s: B=%d (0 .. 65535) V=%d max_faces=%d (0 .. %d)", what, B, V, max_faces, HOISDF_MESH_MAX_FACES);
    return false;
  }
  return true;
}

bool mesh_desc_ok(const char* what, const char* name, const hoisdf_mesh* m, int B, bool may_be_absent) {
  if (!m) {
    if (!may_be_absent) set_error("%s: null pointer (%s)", what, name);
    return may_be_absent;
  }
  char label[96];
  snprintf(label, sizeof label, "%s (%s)", what, name);
  if (!mesh_shape_ok(label, B, m->V, m->max_faces)) return false;
  if (m->face_batch_stride != 0 && m->face_batch_stride < 3L * m->max_faces) {
    set_error("%s: %s face_batch_stride=%ld (0 or >= 3 max_faces)", what, name, m->face_batch_stride);
    return false;
  }
  return true;
}
bool mesh_data_ok(const char* what, const char* name, const hoisdf_mesh* m) {
  if (m && !(m->V > 0 && m->verts && (m->max_faces == 0 || m->faces))) {
    set_error("%s: null pointer (%s verts, faces) or a mesh without vertices", what, name);
    return false;
  }
  return true;
}

void launch_prepare(const hoisdf_mesh& mesh, int B, const MeshBuffers& m, hipStream_t st) {
  hipLaunchKernelGGL(mesh_prepare_kernel, dim3(B), dim3(256), 0, st, mesh.verts, mesh.V, mesh.faces, mesh.face_batch_stride, mesh.n_faces,
                     mesh.max_faces, m.tris, m.area, m.cdf, m.box);
}
void launch_sample(const MeshBuffers& m, const int32_t* n_faces, int max_faces, int B, int N, float s1, float s2, int every,
                          float pad, uint64_t seed, float* points, long pstride, int ldp, int32_t* face_out, hipStream_t st) {
  hipLaunchKernelGGL(mesh_sample_kernel, dim3(cdiv(N, 256), B), dim3(256), 0, st, m.tris, m.cdf, m.box, n_faces, max_faces, N, s1, s2,
                     every, pad, seed, points, pstride, ldp, face_out);
}
void launch_sdf(const MeshSdfArgs& a, int B, hipStream_t st) {
  hipLaunchKernelGGL(mesh_sdf_kernel, dim3(cdiv(a.N, MESH_PTS), B), dim3(256), 0, st, a);
}
void launch_both_ways(const hoisdf_mesh& hand, const hoisdf_mesh& obj, int B, const MeshPair& m, const VertexSdf& hand_to_obj,
                      const VertexSdf& obj_to_hand, hipStream_t st) {
  launch_prepare(hand, B, m.hand, st);
  launch_prepare(obj, B, m.obj, st);
  MeshSdfArgs ho = sdf_args(hand.verts, 3, hand.V, m.obj, obj.n_faces, obj.max_faces, hand_to_obj.sdf, 1);
  ho.face_out = hand_to_obj.face; ho.bary_out = hand_to_obj.bary;
  launch_sdf(ho, B, st);
  MeshSdfArgs oh = sdf_args(obj.verts, 3, obj.V, m.hand, hand.n_faces, hand.max_faces, obj_to_hand.sdf, 1);
  oh.face_out = obj_to_hand.face; oh.bary_out = obj_to_hand.bary;
  launch_sdf(oh, B, st);
}

}  // namespace hoisdf

using namespace hoisdf;

extern "C" int hoisdf_mesh_prepare(const float* verts, int B, int V, const int32_t* faces, long face_batch_stride,
                                   const int32_t* n_faces, int max_faces, float* tris, float* area, float* cdf, float* box,
                                   void* stream) {
  if (!mesh_shape_ok("mesh_prepare", B, V, max_faces)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(face_batch_stride == 0 || face_batch_stride >= 3L * max_faces, HOISDF_ERR_INVALID,
                 "mesh_prepare: face_batch_stride=%ld (0 or >= 3 max_faces)", face_batch_stride);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(box && (V == 0 || verts), HOISDF_ERR_INVALID, "mesh_prepare: null pointer (verts, box)");
  HOISDF_REQUIRE(max_faces == 0 || (V > 0 && faces && tris && area && cdf), HOISDF_ERR_INVALID,
                 "mesh_prepare: null pointer (faces, tris, area, cdf) or faces without vertices");
  launch_prepare({verts, faces, n_faces, face_batch_stride, V, max_faces}, B, {(float4*)tris, area, cdf, box}, as_stream(stream));
  return check_launch("mesh_prepare");
}

extern "C" int hoisdf_mesh_sample_points(const float* tris, const float* cdf, const float* box, const int32_t* n_faces, int max_faces,
                                         int B, int N, float sigma1, float sigma2, int uniform_every, float pad, uint64_t seed,
                                         float* points, int ldp, int32_t* face_out, void* stream) {
  if (!mesh_shape_ok("mesh_sample_points", B, 0, max_faces)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(N >= 0 && N <= (1 << 28) && ldp >= 3, HOISDF_ERR_INVALID, "mesh_sample_points: N=%d (0 .. 2^28) ldp=%d (>= 3)", N, ldp);
  HOISDF_REQUIRE(sigma1 >= 0.f && sigma2 >= 0.f && pad >= 0.f, HOISDF_ERR_INVALID, "mesh_sample_points: sigma1=%g sigma2=%g pad=%g (>= 0)",
                 (double)sigma1, (double)sigma2, (double)pad);
  if (B == 0 || N == 0) return HOISDF_OK;
  HOISDF_REQUIRE(box && points && (max_faces == 0 || (tris && cdf)), HOISDF_ERR_INVALID, "mesh_sample_points: null pointer");
  launch_sample({(float4*)tris, nullptr, (float*)cdf, (float*)box}, n_faces, max_faces, B, N, sigma1, sigma2, uniform_every, pad, seed,
                points, (long)N * ldp, ldp, face_out, as_stream(stream));
  return check_launch("mesh_sample_points");
}

extern "C" int hoisdf_mesh_sdf(const float* points, int ldp, int B, int N, const float* tris, const float* box, const int32_t* n_faces,
                               int max_faces, const int32_t* vert_label, long label_batch_stride, float* sdf, int ld,
                               int32_t* face_out, float* bary_out, float* winding_out, int32_t* label_out, void* stream) {
  if (!mesh_shape_ok("mesh_sdf", B, 0, max_faces)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(N >= 0 && ldp >= 3 && ld >= 1 && label_batch_stride >= 0, HOISDF_ERR_INVALID,
                 "mesh_sdf: N=%d ldp=%d (>= 3) ld=%d (>= 1) label_batch_stride=%ld", N, ldp, ld, label_batch_stride);
  if (B == 0 || N == 0) return HOISDF_OK;
  HOISDF_REQUIRE(points && box && sdf && (max_faces == 0 || tris), HOISDF_ERR_INVALID, "mesh_sdf: null pointer");
  HOISDF_REQUIRE(!label_out || vert_label, HOISDF_ERR_INVALID, "mesh_sdf: null pointer (label_out without vert_label)");
  MeshSdfArgs a = sdf_args(points, ldp, N, {(float4*)tris, nullptr, nullptr, (float*)box}, n_faces, max_faces, sdf, ld);
  a.face_out = face_out; a.bary_out = bary_out; a.winding_out = winding_out;
  a.vert_label = vert_label; a.label_stride = label_batch_stride; a.label_out = label_out;
  launch_sdf(a, B, as_stream(stream));
  return check_launch("mesh_sdf");
}

extern "C" long hoisdf_mesh_sdf_rows_workspace_bytes(int B, int hand_max_faces, int obj_max_faces) {
  if (!mesh_shape_ok("mesh_sdf_rows_workspace_bytes", B, 0, hand_max_faces) ||
      !mesh_shape_ok("mesh_sdf_rows_workspace_bytes", B, 0, obj_max_faces))
    return -1;
  Bump w(nullptr, 0);
  mesh_pair(w, B, hand_max_faces, obj_max_faces);
  return w.bytes();
}

extern "C" int hoisdf_mesh_sdf_rows(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* hand_vert_label, int B, int n_hand,
                                    int n_obj, float sigma1, float sigma2, int uniform_every, float pad, float clamp, uint64_t seed,
                                    float* rows, int ld, void* workspace, long workspace_bytes, void* stream) {
  if (!mesh_desc_ok("mesh_sdf_rows", "hand", hand, B) || !mesh_desc_ok("mesh_sdf_rows", "obj", obj, B)) return HOISDF_ERR_INVALID;
  const long n = (long)n_hand + n_obj;
  HOISDF_REQUIRE(n_hand >= 0 && n_obj >= 0 && n <= (1 << 28) && ld >= 6, HOISDF_ERR_INVALID,
                 "mesh_sdf_rows: n_hand=%d n_obj=%d (>= 0, sum <= 2^28) ld=%d (>= 6)", n_hand, n_obj, ld);
  HOISDF_REQUIRE(sigma1 >= 0.f && sigma2 >= 0.f && pad >= 0.f && clamp >= 0.f, HOISDF_ERR_INVALID,
                 "mesh_sdf_rows: sigma1=%g sigma2=%g pad=%g clamp=%g (>= 0)", (double)sigma1, (double)sigma2, (double)pad, (double)clamp);
  if (B == 0 || n == 0) return HOISDF_OK;
  if (!mesh_data_ok("mesh_sdf_rows", "hand", hand) || !mesh_data_ok("mesh_sdf_rows", "obj", obj)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(rows && workspace && hand_vert_label, HOISDF_ERR_INVALID, "mesh_sdf_rows: null pointer (rows, workspace, hand_vert_label)");
  Bump w(workspace, workspace_bytes);
  const MeshPair m = mesh_pair(w, B, hand->max_faces, obj->max_faces);
  HOISDF_REQUIRE(workspace_bytes >= w.bytes(), HOISDF_ERR_INVALID, "mesh_sdf_rows: workspace of %ld bytes, %ld needed", workspace_bytes, w.bytes());
  hipStream_t st = as_stream(stream);
  launch_prepare(*hand, B, m.hand, st);
  launch_prepare(*obj, B, m.obj, st);
  // the row block of sample b: n_hand points drawn at the hand, then n_obj drawn at the object, the points written straight into
  // columns 0-2; two seeds, so that the two sets do not share their draws
  const long rs = n * ld;
  if (n_hand) launch_sample(m.hand, hand->n_faces, hand->max_faces, B, n_hand, sigma1, sigma2, uniform_every, pad, seed * 2, rows, rs, ld, nullptr, st);
  if (n_obj) launch_sample(m.obj, obj->n_faces, obj->max_faces, B, n_obj, sigma1, sigma2, uniform_every, pad, seed * 2 + 1,
                           rows + (size_t)n_hand * ld, rs, ld, nullptr, st);
  // every row against both meshes: sdf_hand -> column 3 with the label -> column 5, sdf_obj -> column 4
  MeshSdfArgs a = sdf_args(rows, ld, (int)n, m.hand, hand->n_faces, hand->max_faces, rows + 3, ld);
  a.vert_label = hand_vert_label; a.label_f = rows + 5; a.clamp = clamp; a.n_label = n_hand;
  launch_sdf(a, B, st);
  launch_sdf(sdf_args(rows, ld, (int)n, m.obj, obj->n_faces, obj->max_faces, rows + 4, ld), B, st);
  return check_launch("mesh_sdf_rows");
}
