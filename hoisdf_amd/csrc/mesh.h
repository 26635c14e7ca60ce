// What the mesh entries (mesh_sdf.hip, interact.hip, interact_loss.hip, isosurf.hip, raster.hip) share: the small vector helpers,
// the skipped-face rule's unfused cross product, the polynomial atan2 of the solid angle, the argument block of mesh_sdf_kernel,
// the layout of the prepared-mesh buffers inside a workspace, the check of a hoisdf_mesh descriptor and the launches of the kernels
// several files run (defined in mesh_sdf.hip, where the kernels are).
#pragma once
#include "common.h"

namespace hoisdf {

constexpr int MESH_TILE = 128;            // faces per LDS tile: 6 KiB, 384 float4 = 1.5 loads per thread of a 256-thread block
static_assert(HOISDF_MESH_TILE == MESH_TILE, "the header states the tile the tests aim at");
constexpr int MESH_PTS = 64, MESH_SLICES = 4;          // a block: 64 points (one per lane) x 4 waves, each wave a quarter of the faces

struct f3 { float x, y, z; };
__device__ __forceinline__ f3 sub(f3 a, f3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ f3 xyz(const float4& v) { return {v.x, v.y, v.z}; }

// u x v with every product rounded on its own: u x u and 0 x v are then EXACTLY zero (a fused multiply-add would leave the
// rounding error of one product behind), which is what the skipped-face rule tests
__device__ __forceinline__ f3 cross_unfused(f3 u, f3 v) {
#pragma clang fp contract(off)
  f3 n;
  n.x = u.y * v.z - u.z * v.y;
  n.y = u.z * v.x - u.x * v.z;
  n.z = u.x * v.y - u.y * v.x;
  return n;
}

__device__ __forceinline__ int sample_faces(const int32_t* n_faces, int b, int max_faces) {
  const int n = n_faces ? n_faces[b] : max_faces;
  return n < 0 ? 0 : (n > max_faces ? max_faces : n);
}

struct MeshSdfArgs {
  const float* points; int ldp;          // [B][N] rows of ldp floats, xyz first
  const float4* tris; const float* box; const int32_t* n_faces; int max_faces;
  int N;
  float* sdf; int ld;                    // sdf of point (b, i) -> sdf[(b N + i) ld]  (the caller folds the column into the pointer)
  int32_t* face_out;                     // [B][N] or null
  float* bary_out;                       // [B][N][3] or null
  float* winding_out;                    // [B][N] or null
  const int32_t* vert_label; long label_stride;   // [V] per sample (stride 0: shared) or null
  int32_t* label_out;                    // [B][N] or null
  float* label_f; float clamp; int n_label;       // rows form: label as a float at label_f[(b N + i) ld]: the vertex label where
                                                  // i < n_label and |sdf| <= clamp, else -1; null: not wanted
};

// atan2(y, x) to 1.1e-7 rad: one hardware reciprocal and a degree-17 odd polynomial on [0, 1] (the library routine costs about three
// times as much, and the sign rule compares a sum of <= 4096 of these, each at most pi, with 0.5 of 2 pi); 0 for y = x = 0
__device__ __forceinline__ float atan2_poly(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y), mx = fmaxf(ax, ay), mn = fminf(ax, ay);
  const float t = mx > 0.f ? mn * __builtin_amdgcn_rcpf(mx) : 0.f, s = t * t;
  float r = 0.00282363896f;
  r = r * s - 0.0159569028f;
  r = r * s + 0.0425049886f;
  r = r * s - 0.0748900920f;
  r = r * s + 0.106347933f;
  r = r * s - 0.142027363f;
  r = r * s + 0.199926957f;
  r = r * s - 0.333331018f;
  r = r * s * t + t;
  if (ay > ax) r = 1.57079637f - r;
  if (x < 0.f) r = 3.14159274f - r;
  return copysignf(r, y);
}

// ---- the prepared mesh of a batch inside a workspace, and the launches (mesh_sdf.hip) --------------------------------------------
// Every workspace of the family has ONE layout function over a Bump (common.h): measuring (null base) it is the size query, over
// the caller's buffer it makes the pointers of the call.
struct MeshBuffers { float4* tris; float* area; float* cdf; float* box; };
static inline MeshBuffers mesh_buffers(Bump& w, long B, long max_faces) {
  MeshBuffers m;
  m.tris = (float4*)w.take(B * max_faces * 48);
  m.area = w.floats(B * max_faces);
  m.cdf = w.floats(B * max_faces);
  m.box = w.floats(B * 8);
  return m;
}
// the hand's, then the object's: all of hoisdf_mesh_sdf_rows' workspace and the head of the two interaction workspaces
struct MeshPair { MeshBuffers hand, obj; };
static inline MeshPair mesh_pair(Bump& w, long B, long hand_max_faces, long obj_max_faces) {
  MeshPair p;
  p.hand = mesh_buffers(w, B, hand_max_faces);
  p.obj = mesh_buffers(w, B, obj_max_faces);
  return p;
}

bool mesh_shape_ok(const char* what, int B, int V, int max_faces);
// The rules of a hoisdf_mesh descriptor, in two steps because B == 0 returns HOISDF_OK between them.  `what` names the entry,
// `name` the mesh (hand, obj, gt); a null descriptor passes both only where the entry allows an absent mesh.
//   mesh_desc_ok  before B == 0: the descriptor is there, the shape limits (mesh_shape_ok), face_batch_stride 0 or >= 3 max_faces
//   mesh_data_ok  after it: V > 0, verts, and faces where max_faces > 0
bool mesh_desc_ok(const char* what, const char* name, const hoisdf_mesh* m, int B, bool may_be_absent = false);
bool mesh_data_ok(const char* what, const char* name, const hoisdf_mesh* m);

void launch_prepare(const hoisdf_mesh& mesh, int B, const MeshBuffers& m, hipStream_t st);
// the plain case: N points per sample against a prepared mesh, the distance alone; whoever wants the winning face, the weights or
// the labels sets those fields afterwards
static inline MeshSdfArgs sdf_args(const float* points, int ldp, int N, const MeshBuffers& m, const int32_t* n_faces, int max_faces,
                                   float* sdf, int ld) {
  MeshSdfArgs a = {};
  a.points = points; a.ldp = ldp; a.N = N;
  a.tris = m.tris; a.box = m.box; a.n_faces = n_faces; a.max_faces = max_faces;
  a.sdf = sdf; a.ld = ld;
  return a;
}
void launch_sdf(const MeshSdfArgs& a, int B, hipStream_t st);
// Both meshes prepared, then every hand vertex against the object and every object vertex (padding rows too) against the hand:
// 4 launches, in this order.  Where a direction leaves its [B][V] distances and, if wanted, winning faces and [B][V][3] weights.
struct VertexSdf { float* sdf; int32_t* face; float* bary; };
void launch_both_ways(const hoisdf_mesh& hand, const hoisdf_mesh& obj, int B, const MeshPair& m, const VertexSdf& hand_to_obj,
                      const VertexSdf& obj_to_hand, hipStream_t st);
// N points per sample into points[b pstride + i ldp + 0..2] (hoisdf_mesh_sample_points; isosurf.hip draws its surface points with it)
void launch_sample(const MeshBuffers& m, const int32_t* n_faces, int max_faces, int B, int N, float s1, float s2, int every, float pad,
                   uint64_t seed, float* points, long pstride, int ldp, int32_t* face_out, hipStream_t st);

}  // namespace hoisdf
