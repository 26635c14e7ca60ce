// Hand-object interaction metrics (include/hoisdf.h "interaction"): is the predicted hand physically compatible with the predicted
// object?  Penetration depth, contact and intersection volume of the two posed meshes of every sample (ObMan's three numbers), from
// the pieces of mesh_sdf.hip: both meshes prepared by mesh_prepare_kernel, every vertex of one against the other by mesh_sdf_kernel.
//   interact_voxel_kernel   the hot path.  The overlap of the two bounding boxes is cut into <= 64^3 cells; one lane per cell centre,
//                           generated from the cell's index (no point array goes through HBM), and only the solid-angle half of
//                           mesh_sdf_kernel's pair loop: no closest point is needed to say inside or outside.  Same block shape as
//                           mesh_sdf_kernel - 64 centres (one per lane) x 4 waves, wave s taking faces s, s + 4, ... of every LDS tile
//                           of MESH_TILE faces, all lanes reading the same triangle (a broadcast: conflict-free), the four partial
//                           sums of a centre added by wave 0 in wave order - so a centre's winding number has one fixed summation
//                           order.  The object comes first: a block none of whose centres is inside the object skips the hand.
//                           Each block leaves its inside count in its own slot: integers, no atomics, nothing to zero.
//   interact_reduce_kernel  one block per sample, after the voxel pass: the maxima, the minimum and the counts over the two vertex
//                           distance arrays, the sum of the sample's block counts, the volume and the grid description.  Maxima,
//                           minima and integer sums do not depend on the order they are taken in: two calls give the same bits.
// The kernel is VALU-bound (three square roots, a reciprocal and the degree-17 polynomial per centre x face); it needs 42 VGPRs and
// 7 KiB of LDS, so the registers allow 8 waves per SIMD.  Samples differ in their cell counts and the host does not know them: the
// launch covers 64^3 cells per sample and a block past its sample's count leaves at once.
#include "mesh.h"

namespace hoisdf {

constexpr int IG = HOISDF_INTERACT_MAX_GRID;
constexpr int IG_CELLS = IG * IG * IG, IG_BLOCKS = IG_CELLS / MESH_PTS;
static_assert(IG <= 255, "grid_out packs the three cell counts into bytes");

// The grid of a sample from the two box[8] of mesh_prepare_kernel (centre xyz, area, half extent xyz, 0), in fp32 and in THIS order
// (interaction_oracle.grid repeats it, so both evaluate the same centres); no product is fused into a sum.  Per axis:
//   lo = max(c_h - h_h, c_o - h_o);  hi = min(c_h + h_h, c_o + h_o);  extent = hi - lo
//   n = min(ceil(extent / voxel), 64), at least 1;  cell = extent / n;  any extent <= 0: no cell at all
struct InteractGrid { float lo[3], cell[3]; int n[3]; int total; };
__device__ __forceinline__ InteractGrid interact_grid(const float* bh, const float* bo, float voxel) {
#pragma clang fp contract(off)
  InteractGrid g;
  bool empty = false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float lo = fmaxf(bh[k] - bh[4 + k], bo[k] - bo[4 + k]), hi = fminf(bh[k] + bh[4 + k], bo[k] + bo[4 + k]);
    const float ext = hi - lo;
    int n = 0;
    if (ext > 0.f) n = max(1, (int)fminf(ceilf(ext / voxel), (float)IG));
    empty |= n == 0;
    g.lo[k] = lo;
    g.n[k] = n;
    g.cell[k] = n > 0 ? ext / (float)n : 0.f;
  }
  if (empty) {
    g.n[0] = g.n[1] = g.n[2] = 0;
    g.cell[0] = g.cell[1] = g.cell[2] = 0.f;
  }
  g.total = g.n[0] * g.n[1] * g.n[2];
  return g;
}

// the winding number of the block's 64 centres (p = centre - the mesh's own centre) against one prepared mesh; the value is
// complete in wave 0.  Pair loop, skipped-face rule and summation order are mesh_sdf_kernel's.
__device__ __forceinline__ float winding_pass(const float4* __restrict__ tb, int nf, f3 p, float4* s_tri, float* s_om) {
  const int tid = threadIdx.x, slice = tid >> 6;
  float omega = 0.f;
  for (int t0 = 0; t0 < nf; t0 += MESH_TILE) {
    const int cnt = min(MESH_TILE, nf - t0);
    __syncthreads();
    for (int k = tid; k < cnt * 3; k += 256) s_tri[k] = tb[(size_t)t0 * 3 + k];
    __syncthreads();
    for (int j = slice; j < cnt; j += MESH_SLICES) {   // this wave's faces, in ascending order
      const float4 A = s_tri[j * 3], Bq = s_tri[j * 3 + 1], Cq = s_tri[j * 3 + 2];
      if (__float_as_int(A.w) < 0) continue;           // a skipped face (the same for every lane)
      const f3 ap = sub(p, xyz(A)), bp = sub(p, xyz(Bq)), cp = sub(p, xyz(Cq));
      const float la = __builtin_amdgcn_sqrtf(dot(ap, ap)), lb = __builtin_amdgcn_sqrtf(dot(bp, bp)), lc = __builtin_amdgcn_sqrtf(dot(cp, cp));
      const float det = ap.x * (bp.y * cp.z - bp.z * cp.y) + ap.y * (bp.z * cp.x - bp.x * cp.z) + ap.z * (bp.x * cp.y - bp.y * cp.x);
      const float den_w = la * lb * lc + dot(ap, bp) * lc + dot(bp, cp) * la + dot(cp, ap) * lb;
      omega += atan2_poly(-det, den_w);
    }
  }
  s_om[tid] = omega;
  __syncthreads();
  if (slice != 0) return 0.f;
#pragma unroll
  for (int s = 1; s < MESH_SLICES; ++s) omega += s_om[tid + 64 * s];
  return omega * (2.f / 12.566370614359172f);
}

struct InteractVoxelArgs {
  const float4* tris_h; const float* box_h; const int32_t* nf_h; int maxf_h;
  const float4* tris_o; const float* box_o; const int32_t* nf_o; int maxf_o;
  float voxel;
  int32_t* partial;                      // [B][IG_BLOCKS]: cells of the block inside both meshes; slots from ceil(total / 64) on
                                         // are not written
  uint8_t* inside_out;                   // [B][IG_CELLS] or null
};

__global__ __launch_bounds__(256) void interact_voxel_kernel(const InteractVoxelArgs a) {
  __shared__ float4 s_tri[MESH_TILE * 3];
  __shared__ float s_om[256];
  const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * MESH_PTS + (tid & 63);
  const float* bh = a.box_h + (size_t)b * 8;
  const float* bo = a.box_o + (size_t)b * 8;
  const InteractGrid g = interact_grid(bh, bo, a.voxel);
  if (blockIdx.x * MESH_PTS >= g.total) return;        // the whole block: before any barrier
  const bool live = i < g.total;
  f3 c = {0.f, 0.f, 0.f};
  if (live) {
#pragma clang fp contract(off)
    const int ix = i % g.n[0], iy = (i / g.n[0]) % g.n[1], iz = i / (g.n[0] * g.n[1]);
    c = {g.lo[0] + ((float)ix + 0.5f) * g.cell[0], g.lo[1] + ((float)iy + 0.5f) * g.cell[1], g.lo[2] + ((float)iz + 0.5f) * g.cell[2]};
  }
  const f3 po = {c.x - bo[0], c.y - bo[1], c.z - bo[2]};
  const float wo = winding_pass(a.tris_o + (size_t)b * a.maxf_o * 3, sample_faces(a.nf_o, b, a.maxf_o), po, s_tri, s_om);
  const bool in_obj = live && tid < 64 && wo > 0.5f;
  uint8_t* mask = a.inside_out ? a.inside_out + (size_t)b * IG_CELLS : nullptr;
  if (!__syncthreads_or(in_obj)) {                     // no centre of this block is inside the object: the hand cannot matter
    if (tid == 0) a.partial[(size_t)b * IG_BLOCKS + blockIdx.x] = 0;
    if (mask && live && tid < 64) mask[i] = 0;
    return;
  }
  const f3 ph = {c.x - bh[0], c.y - bh[1], c.z - bh[2]};
  const float wh = winding_pass(a.tris_h + (size_t)b * a.maxf_h * 3, sample_faces(a.nf_h, b, a.maxf_h), ph, s_tri, s_om);
  if (tid >= 64) return;
  const bool inside = in_obj && wh > 0.5f;
  const int cnt = __popcll(__ballot(inside));
  if (tid == 0) a.partial[(size_t)b * IG_BLOCKS + blockIdx.x] = cnt;
  if (mask && live) mask[i] = inside ? 1 : 0;
}

struct InteractReduceArgs {
  const float* sdf_ho; int Vh;           // [B][Vh] hand vertices against the object
  const float* sdf_oh; int Vo;           // [B][Vo] object vertices against the hand
  const int32_t* obj_n_verts;            // [B] or null
  const float* box_h; const float* box_o;
  float voxel, contact_dist;
  const int32_t* partial;
  float *pen_hand, *pen_obj, *min_dist, *volume, *grid_out;
  int32_t *contact_verts, *in_contact, *inside_count;
};

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void interact_reduce_kernel(const InteractReduceArgs a) {
  __shared__ float s_f[3][4];
  __shared__ int s_i[2][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const InteractGrid g = interact_grid(a.box_h + (size_t)b * 8, a.box_o + (size_t)b * 8, a.voxel);
  float ph = 0.f, po = 0.f, md = 3.0e38f;
  int nc = 0, cells = 0;
  const float* sh = a.sdf_ho + (size_t)b * a.Vh;
  for (int v = tid; v < a.Vh; v += 256) {
    const float s = sh[v];
    ph = fmaxf(ph, -s);
    md = fminf(md, fabsf(s));
    nc += s <= a.contact_dist ? 1 : 0;
  }
  const int nvo = a.obj_n_verts ? min(max(a.obj_n_verts[b], 0), a.Vo) : a.Vo;
  const float* so = a.sdf_oh + (size_t)b * a.Vo;
  for (int v = tid; v < nvo; v += 256) po = fmaxf(po, -so[v]);
  const int32_t* part = a.partial + (size_t)b * IG_BLOCKS;
  for (int k = tid; k < (g.total + MESH_PTS - 1) / MESH_PTS; k += 256) cells += part[k];
  ph = wave_max(ph); po = wave_max(po); md = -wave_max(-md);
  nc = wave_sum_i(nc); cells = wave_sum_i(cells);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    s_f[0][w] = ph; s_f[1][w] = po; s_f[2][w] = md; s_i[0][w] = nc; s_i[1][w] = cells;
  }
  __syncthreads();
  if (tid != 0) return;
  ph = fmaxf(fmaxf(s_f[0][0], s_f[0][1]), fmaxf(s_f[0][2], s_f[0][3]));
  po = fmaxf(fmaxf(s_f[1][0], s_f[1][1]), fmaxf(s_f[1][2], s_f[1][3]));
  md = fminf(fminf(s_f[2][0], s_f[2][1]), fminf(s_f[2][2], s_f[2][3]));
  nc = s_i[0][0] + s_i[0][1] + s_i[0][2] + s_i[0][3];
  cells = s_i[1][0] + s_i[1][1] + s_i[1][2] + s_i[1][3];
  a.pen_hand[b] = ph;
  a.pen_obj[b] = po;
  a.min_dist[b] = md;
  a.contact_verts[b] = nc;
  a.in_contact[b] = (nc > 0 || po > 0.f) ? 1 : 0;
  a.inside_count[b] = cells;
  {
#pragma clang fp contract(off)
    a.volume[b] = (float)cells * g.cell[0] * g.cell[1] * g.cell[2];      // ((count cell_x) cell_y) cell_z, nothing fused
  }
  if (a.grid_out) {
    float* o = a.grid_out + (size_t)b * 8;
    o[0] = g.lo[0]; o[1] = g.lo[1]; o[2] = g.lo[2];
    o[3] = g.cell[0]; o[4] = g.cell[1]; o[5] = g.cell[2];
    o[6] = __int_as_float(g.n[0] | g.n[1] << 8 | g.n[2] << 16);
    o[7] = 0.f;
  }
}

// ---- workspace: both prepared meshes, the two vertex distance arrays, the voxel pass's block counts ------------------------------------
struct InteractWorkspace { MeshPair m; float *sdf_ho, *sdf_oh; int32_t* partial; };

static InteractWorkspace interact_workspace(Bump& w, long B, long Vh, long Fh, long Vo, long Fo) {
  InteractWorkspace s;
  s.m = mesh_pair(w, B, Fh, Fo);
  s.sdf_ho = w.floats(B * Vh);
  s.sdf_oh = w.floats(B * Vo);
  s.partial = w.ints(B * IG_BLOCKS);
  return s;
}

}  // namespace hoisdf

using namespace hoisdf;

extern "C" long hoisdf_eval_interaction_workspace_bytes(int B, int hand_V, int hand_max_faces, int obj_V, int obj_max_faces) {
  if (!mesh_shape_ok("eval_interaction_workspace_bytes (hand)", B, hand_V, hand_max_faces) ||
      !mesh_shape_ok("eval_interaction_workspace_bytes (obj)", B, obj_V, obj_max_faces))
    return -1;
  Bump w(nullptr, 0);
  interact_workspace(w, B, hand_V, hand_max_faces, obj_V, obj_max_faces);
  return w.bytes();
}

extern "C" int hoisdf_eval_interaction(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const int32_t* obj_n_verts, int B,
                                       float contact_dist, float voxel, float* pen_hand, float* pen_obj, float* min_dist,
                                       int32_t* contact_verts, int32_t* in_contact, float* volume, int32_t* inside_count,
                                       uint8_t* inside_out, float* grid_out, void* workspace, long workspace_bytes, void* stream) {
  if (!mesh_desc_ok("eval_interaction", "hand", hand, B) || !mesh_desc_ok("eval_interaction", "obj", obj, B)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(contact_dist >= 0.f && contact_dist <= 3.0e38f, HOISDF_ERR_INVALID, "eval_interaction: contact_dist=%g (>= 0, finite)",
                 (double)contact_dist);
  HOISDF_REQUIRE(voxel > 0.f && voxel <= 3.0e38f, HOISDF_ERR_INVALID, "eval_interaction: voxel=%g (> 0, finite)", (double)voxel);
  if (B == 0) return HOISDF_OK;
  if (!mesh_data_ok("eval_interaction", "hand", hand) || !mesh_data_ok("eval_interaction", "obj", obj)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(pen_hand && pen_obj && min_dist && contact_verts && in_contact && volume && inside_count, HOISDF_ERR_INVALID,
                 "eval_interaction: null pointer (pen_hand, pen_obj, min_dist, contact_verts, in_contact, volume, inside_count)");
  HOISDF_REQUIRE(workspace, HOISDF_ERR_INVALID, "eval_interaction: null pointer (workspace)");
  Bump w(workspace, workspace_bytes);
  const InteractWorkspace s = interact_workspace(w, B, hand->V, hand->max_faces, obj->V, obj->max_faces);
  HOISDF_REQUIRE(workspace_bytes >= w.bytes(), HOISDF_ERR_INVALID, "eval_interaction: workspace of %ld bytes, %ld needed", workspace_bytes,
                 w.bytes());
  hipStream_t st = as_stream(stream);
  launch_both_ways(*hand, *obj, B, s.m, {s.sdf_ho, nullptr, nullptr}, {s.sdf_oh, nullptr, nullptr}, st);
  InteractVoxelArgs va = {s.m.hand.tris, s.m.hand.box, hand->n_faces, hand->max_faces, s.m.obj.tris, s.m.obj.box, obj->n_faces,
                          obj->max_faces, voxel, s.partial, inside_out};
  hipLaunchKernelGGL(interact_voxel_kernel, dim3(IG_BLOCKS, B), dim3(256), 0, st, va);
  InteractReduceArgs ra = {s.sdf_ho, hand->V, s.sdf_oh, obj->V, obj_n_verts, s.m.hand.box, s.m.obj.box, voxel, contact_dist, s.partial,
                           pen_hand, pen_obj, min_dist, volume, grid_out, contact_verts, in_contact, inside_count};
  hipLaunchKernelGGL(interact_reduce_kernel, dim3(B), dim3(256), 0, st, ra);
  return check_launch("eval_interaction");
}

