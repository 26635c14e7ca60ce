// Surface from a sampled field (include/hoisdf.h "iso-surface"): dense grid of field values -> indexed triangle mesh, and the
// Chamfer distance of such a mesh's vertices to a ground-truth mesh.  Marching tetrahedra on the Kuhn subdivision: every cell is six
// tetrahedra around its 000 -> 111 diagonal, all their edges are of the form p -> p + d with d one of seven directions, so the
// low node of an edge owns its vertex and a vertex id is "vertices of the nodes before p" + "active edges of p before this one".
//   iso_points_kernel   node positions as rows for hoisdf_sdf_query_fwd
//   iso_refine_kernel   one block per sample: integer min / max of the inside nodes' indices -> the refined grid
//   iso_count_kernel    one node per thread: its 7-bit edge mask and the triangle count of the cell it is the 000 corner of, from
//                       the cell's 8 values (the node's own and its 7 edge partners: the same 8 loads serve both); per block the two
//                       totals go to the block's own slot
//   iso_scan_kernel     one block per sample: exclusive scan of the <= 8192 block totals (thread t owns a contiguous run, the 256
//                       run sums are scanned in LDS), the sample's two needed counts
//   iso_vertex_kernel   the counts again (cheaper than storing them: 8 cached loads against 8 bytes per node each way), an in-block
//                       exclusive scan + the block's offset -> the node's first vertex id; node word = id << 7 | mask; the vertices
//   iso_face_kernel     the same for the faces; the three vertex ids of a triangle come from the node words of the cell's corners
// Everything that decides a slot is an integer prefix sum over a fixed element order: no atomics, no dependence on scheduling, two
// calls give the same bits.  All kernels are bound by their loads (ix runs fastest: a wave reads 64 consecutive values per corner
// row, the +y / +z rows come from L2) and by launch latency at the sizes of the model (64^3 nodes x 22 samples = 23 MB of values).
//   surf_nn_kernel      gt -> pred half of the Chamfer distance: a thread keeps one surface point, the sample's predicted vertices
//                       stream through LDS in tiles of 256 (all lanes read the same address: broadcast), per-sample vertex count
//   surf_reduce_kernel  one block per sample: both means in fp64, one fixed order
#include "mesh.h"

namespace hoisdf {

constexpr int ISO_T = 256;                                    // threads of every block here = nodes per block
static_assert(7L * HOISDF_ISO_MAX_GRID * HOISDF_ISO_MAX_GRID * HOISDF_ISO_MAX_GRID < (1L << 24), "a node word keeps the vertex id in 24 bits");

// the six tetrahedra: corner c of tetrahedron k as the bits dx | dy << 1 | dz << 2 (000, e_a, e_a + e_b, 111 for the k-th
// permutation (a, b, c) of the axes in lexicographic order); an odd permutation mirrors the tetrahedron
__constant__ uint8_t TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ uint8_t TET_ODD[6] = {0, 1, 1, 0, 0, 1};
// edge e of a tetrahedron joins corners TET_EDGE[e][0] < TET_EDGE[e][1]
__constant__ uint8_t TET_EDGE[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
// direction bits -> the owner's edge number (100, 010, 001, 110, 101, 011, 111 are edges 0..6)
__constant__ uint8_t EDGE_OF_DIR[8] = {0, 0, 1, 3, 2, 4, 5, 6};
// case (bit k = corner k inside) -> up to two triangles as tetrahedron edges, wound counter-clockwise seen from outside in an EVEN
// tetrahedron.  Two inside corners i < j, outside k < l: the quad ik, il, jl, jk cut along ik - jl.
__constant__ uint8_t CASE_TRI[16][2][3] = {
    {{0, 0, 0}, {0, 0, 0}}, {{0, 1, 2}, {0, 0, 0}}, {{0, 4, 3}, {0, 0, 0}}, {{1, 2, 4}, {1, 4, 3}},
    {{1, 3, 5}, {0, 0, 0}}, {{0, 5, 2}, {0, 3, 5}}, {{0, 4, 5}, {0, 5, 1}}, {{2, 4, 5}, {0, 0, 0}},
    {{2, 5, 4}, {0, 0, 0}}, {{0, 1, 5}, {0, 5, 4}}, {{0, 5, 3}, {0, 2, 5}}, {{1, 5, 3}, {0, 0, 0}},
    {{1, 3, 4}, {1, 4, 2}}, {{0, 3, 4}, {0, 0, 0}}, {{0, 2, 1}, {0, 0, 0}}, {{0, 0, 0}, {0, 0, 0}}};

__device__ __forceinline__ int case_tris(int c) { return (0x0112122112212110ULL >> (4 * c)) & 3; }   // 0, 1 or 2 triangles

// lo + i cell: product, then sum
__device__ __forceinline__ float node_coord(float lo, int i, float cell) {
#pragma clang fp contract(off)
  const float s = (float)i * cell;
  return lo + s;
}

// ---- what one node sees: its own value and those of its 7 edge partners (= the 8 corners of the cell it is the 000 corner of) -----
struct NodeView {
  int ix, iy, iz;
  float v[8];          // by direction bits; a partner outside the grid: NaN
  int inside;          // bit c: corner c exists, is finite and v < iso
  int finite;          // bit c: corner c exists and is finite
  int mask;            // bit e: owned edge e is active
  int ntri;            // triangles of the cell (0 where the node is on an upper border or a corner is not finite)
};

__device__ __forceinline__ NodeView node_view(const float* __restrict__ val, int ld, int n, int i, float iso) {
  NodeView w;
  w.ix = i % n;
  w.iy = (i / n) % n;
  w.iz = i / (n * n);
  w.inside = w.finite = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int dx = c & 1, dy = (c >> 1) & 1, dz = c >> 2;
    const bool ex = w.ix + dx < n && w.iy + dy < n && w.iz + dz < n;
    const float x = ex ? val[(size_t)(i + dx + n * (dy + n * dz)) * ld] : __int_as_float(0x7fc00000);
    w.v[c] = x;
    const bool fin = fabsf(x) <= 3.4028234664e38f;            // false for NaN and the infinities
    w.finite |= (fin ? 1 : 0) << c;
    w.inside |= ((fin && x < iso) ? 1 : 0) << c;
  }
  w.mask = 0;
  const int in0 = w.inside & 1;
#pragma unroll
  for (int c = 1; c < 8; ++c) {
    const bool act = (w.finite & 1) && (w.finite >> c & 1) && ((w.inside >> c & 1) != in0);
    w.mask |= (act ? 1 : 0) << EDGE_OF_DIR[c];
  }
  w.ntri = 0;
  if (w.finite == 0xff) {
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      int cs = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) cs |= (w.inside >> TET_CORNER[k][c] & 1) << c;
      w.ntri += case_tris(cs);
    }
  }
  return w;
}

// exclusive prefix sum of one int per thread over the block's 256 threads, in thread order; s4: four shared ints
__device__ __forceinline__ int block_exclusive_scan(int x, int* s4, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  __syncthreads();                                            // s4 may still be read from an earlier scan
  if (lane == 63) s4[wv] = inc;
  __syncthreads();
  int off = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) off += k < wv ? s4[k] : 0;
  if (total) *total = s4[0] + s4[1] + s4[2] + s4[3];
  return off + inc - x;
}

// ---- a. node positions --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ISO_T) void iso_points_kernel(const float* __restrict__ grid, int n, float* __restrict__ points,
                                                          int32_t* __restrict__ sample_idx) {
  const int b = blockIdx.y, i = blockIdx.x * ISO_T + threadIdx.x, N = n * n * n;
  if (i >= N) return;
  const float* g = grid + (size_t)b * 8;
  const int ix = i % n, iy = (i / n) % n, iz = i / (n * n);
  float* o = points + ((size_t)b * N + i) * 3;
  o[0] = node_coord(g[0], ix, g[3]);
  o[1] = node_coord(g[1], iy, g[4]);
  o[2] = node_coord(g[2], iz, g[5]);
  if (sample_idx) sample_idx[(size_t)b * N + i] = b;
}

// ---- b. coarse to fine ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ISO_T) void iso_refine_kernel(const float* __restrict__ values, int ld, const float* __restrict__ grid_in,
                                                          int n, float iso, int pad, int n_out, float* __restrict__ grid_out) {
  __shared__ int s_lo[3][4], s_hi[3][4];
  const int b = blockIdx.x, tid = threadIdx.x, N = n * n * n;
  const float* val = values + (size_t)b * N * ld;
  int lo[3] = {n, n, n}, hi[3] = {-1, -1, -1};
  for (int i = tid; i < N; i += ISO_T) {
    if (!(val[(size_t)i * ld] < iso)) continue;
    const int c[3] = {i % n, (i / n) % n, i / (n * n)};
#pragma unroll
    for (int k = 0; k < 3; ++k) { lo[k] = min(lo[k], c[k]); hi[k] = max(hi[k], c[k]); }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo[k] = min(lo[k], __shfl_xor(lo[k], o, 64)); hi[k] = max(hi[k], __shfl_xor(hi[k], o, 64)); }
    if ((tid & 63) == 0) { s_lo[k][tid >> 6] = lo[k]; s_hi[k][tid >> 6] = hi[k]; }
  }
  __syncthreads();
  if (tid >= 3) return;
  const int k = tid;
  int i0 = min(min(s_lo[k][0], s_lo[k][1]), min(s_lo[k][2], s_lo[k][3]));
  int i1 = max(max(s_hi[k][0], s_hi[k][1]), max(s_hi[k][2], s_hi[k][3]));
  if (i1 < 0) { i0 = 0; i1 = n - 1; }                         // no inside node: the whole coarse grid
  else { i0 = max(i0 - pad, 0); i1 = min(i1 + pad, n - 1); }
  const float* g = grid_in + (size_t)b * 8;
  float* o = grid_out + (size_t)b * 8;
  const float a = node_coord(g[k], i0, g[3 + k]), e = node_coord(g[k], i1, g[3 + k]);
  o[k] = a;
  o[3 + k] = (e - a) / (float)(n_out - 1);
  if (k < 2) o[6 + k] = 0.f;
}

// ---- c. extraction ----------------------------------------------------------------------------------------------------------------------
struct IsoArgs {
  const float* values; int ld;
  const float* grid; int n; float iso;
  int32_t *blk_v, *blk_f; int nblk;        // [B][nblk] block totals, then (in place) exclusive block offsets
  uint32_t* word;                          // [B][n^3]: first vertex id << 7 | edge mask
  float out_scale; const float* out_shift; // shift null: vertices stay in the grid's frame
  float* verts; int max_verts;
  int32_t* faces; int max_faces;
  int32_t *n_verts, *n_faces;
};

__global__ __launch_bounds__(ISO_T) void iso_count_kernel(const IsoArgs a) {
  __shared__ int s_v[4], s_f[4];
  const int b = blockIdx.y, i = blockIdx.x * ISO_T + threadIdx.x, N = a.n * a.n * a.n;
  int nv = 0, nf = 0;
  if (i < N) {
    const NodeView w = node_view(a.values + (size_t)b * N * a.ld, a.ld, a.n, i, a.iso);
    nv = __popc(w.mask);
    nf = w.ntri;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { nv += __shfl_xor(nv, o, 64); nf += __shfl_xor(nf, o, 64); }
  if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = nv; s_f[threadIdx.x >> 6] = nf; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.blk_v[(size_t)b * a.nblk + blockIdx.x] = s_v[0] + s_v[1] + s_v[2] + s_v[3];
    a.blk_f[(size_t)b * a.nblk + blockIdx.x] = s_f[0] + s_f[1] + s_f[2] + s_f[3];
  }
}

// exclusive scan of a sample's block totals, in place; thread t owns blocks [t per, (t + 1) per)
__global__ __launch_bounds__(ISO_T) void iso_scan_kernel(const IsoArgs a) {
  __shared__ int s4[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int per = (a.nblk + ISO_T - 1) / ISO_T, k0 = min(tid * per, a.nblk), k1 = min(k0 + per, a.nblk);
  for (int which = 0; which < 2; ++which) {
    int32_t* blk = (which ? a.blk_f : a.blk_v) + (size_t)b * a.nblk;
    int run = 0;
    for (int k = k0; k < k1; ++k) run += blk[k];
    int total;
    int off = block_exclusive_scan(run, s4, &total);
    for (int k = k0; k < k1; ++k) { const int x = blk[k]; blk[k] = off; off += x; }
    if (tid == 0) (which ? a.n_faces : a.n_verts)[b] = total;
  }
}

__global__ __launch_bounds__(ISO_T) void iso_vertex_kernel(const IsoArgs a) {
  __shared__ int s4[4];
  const int b = blockIdx.y, i = blockIdx.x * ISO_T + threadIdx.x, n = a.n, N = n * n * n;
  NodeView w;
  w.mask = 0;
  if (i < N) w = node_view(a.values + (size_t)b * N * a.ld, a.ld, n, i, a.iso);
  const int first = a.blk_v[(size_t)b * a.nblk + blockIdx.x] + block_exclusive_scan(__popc(w.mask), s4, nullptr);
  if (i >= N) return;
  a.word[(size_t)b * N + i] = (uint32_t)first << 7 | (uint32_t)w.mask;
  if (!a.verts || !w.mask) return;
  const float* g = a.grid + (size_t)b * 8;
  const int pc[3] = {w.ix, w.iy, w.iz};
  float px[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) px[k] = node_coord(g[k], pc[k], g[3 + k]);
  const bool p_in = w.inside & 1;
  int id = first;
#pragma unroll
  for (int e = 0; e < 7; ++e) {
    if (!(w.mask >> e & 1)) continue;
    if (id >= a.max_verts) break;                            // rows beyond the capacity are not written
    constexpr int DIR_OF_EDGE[7] = {1, 2, 4, 3, 5, 6, 7};
    const int d = DIR_OF_EDGE[e];
    const float vp = w.v[0], vq = w.v[d];
    const float va = p_in ? vp : vq, vb = p_in ? vq : vp;     // a = the inside end
    float out[3];
    {
#pragma clang fp contract(off)
      const float t = (a.iso - va) / (vb - va);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float xq = (d >> k & 1) ? node_coord(g[k], pc[k] + 1, g[3 + k]) : px[k];
        const float xa = p_in ? px[k] : xq, xb = p_in ? xq : px[k];
        const float step = t * (xb - xa);
        float x = xa + step;
        if (a.out_shift) {
          const float s = x * a.out_scale;
          x = s + a.out_shift[(size_t)b * 3 + k];
        }
        out[k] = x;
      }
    }
    float* o = a.verts + ((size_t)b * a.max_verts + id) * 3;
    o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
    ++id;
  }
}

__global__ __launch_bounds__(ISO_T) void iso_face_kernel(const IsoArgs a) {
  __shared__ int s4[4];
  const int b = blockIdx.y, i = blockIdx.x * ISO_T + threadIdx.x, n = a.n, N = n * n * n;
  NodeView w;
  w.ntri = 0;
  if (i < N) w = node_view(a.values + (size_t)b * N * a.ld, a.ld, n, i, a.iso);
  int id = a.blk_f[(size_t)b * a.nblk + blockIdx.x] + block_exclusive_scan(w.ntri, s4, nullptr);
  if (i >= N || !w.ntri) return;                             // ntri > 0: all 8 corners exist
  const uint32_t* word = a.word + (size_t)b * N;
  uint32_t cw[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) cw[c] = word[i + (c & 1) + n * ((c >> 1 & 1) + n * (c >> 2))];
  for (int k = 0; k < 6; ++k) {
    int cs = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) cs |= (w.inside >> TET_CORNER[k][c] & 1) << c;
    const int nt = case_tris(cs);
    for (int t = 0; t < nt; ++t, ++id) {
      if (id >= a.max_faces) return;
      int vid[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int te = CASE_TRI[cs][t][j];
        const int c0 = TET_CORNER[k][TET_EDGE[te][0]], c1 = TET_CORNER[k][TET_EDGE[te][1]];
        const int e = EDGE_OF_DIR[c0 ^ c1];                   // c1 contains c0's bits: the xor is the direction
        uint32_t x = cw[0];
#pragma unroll
        for (int c = 1; c < 8; ++c) x = c0 == c ? cw[c] : x;  // selects: cw stays in registers
        vid[j] = (int)(x >> 7) + __popc(x & ((1u << e) - 1u));
      }
      int32_t* o = a.faces + ((size_t)b * a.max_faces + id) * 3;
      const bool odd = TET_ODD[k];
      o[0] = vid[0]; o[1] = odd ? vid[2] : vid[1]; o[2] = odd ? vid[1] : vid[2];
    }
  }
}

static bool iso_shape_ok(const char* what, int B, int n) {
  if (B < 0 || B > 65535 || n < 2 || n > HOISDF_ISO_MAX_GRID) {
    set_error("%s: B=%d (0 .. 65535) n=%d (2 .. %d)", what, B, n, HOISDF_ISO_MAX_GRID);
    return false;
  }
  return true;
}
static long iso_nodes(int n) { return (long)n * n * n; }
// workspace of hoisdf_iso_extract: the per-block vertex and face counts, then one word per node
struct IsoWorkspace { int32_t *blk_v, *blk_f; uint32_t* word; };
static IsoWorkspace iso_workspace(Bump& w, long B, int n) {
  const long nblk = cdiv(iso_nodes(n), ISO_T);
  IsoWorkspace s;
  s.blk_v = w.ints(B * nblk);
  s.blk_f = w.ints(B * nblk);
  s.word = (uint32_t*)w.take(B * iso_nodes(n) * 4);
  return s;
}

// ---- d. Chamfer distance of predicted vertices to a ground-truth mesh -------------------------------------------------------------------
constexpr float SURF_FAR = 1e18f;            // padding of a partial tile: (q - FAR)^2 is finite and never the minimum

__device__ __forceinline__ int sample_verts(const int32_t* n_verts, int b, int max_verts) {
  const int n = n_verts[b];
  return n < 0 ? 0 : (n > max_verts ? max_verts : n);
}

__global__ __launch_bounds__(ISO_T) void surf_nn_kernel(const float* __restrict__ samples, int n_samples, const float* __restrict__ pred,
                                                       const int32_t* __restrict__ pred_n, int max_verts, float* __restrict__ d2_out,
                                                       int32_t* __restrict__ nearest_out) {
  __shared__ float tile[3][ISO_T];
  const int b = blockIdx.y, tid = threadIdx.x, i = blockIdx.x * ISO_T + tid;
  const int nv = sample_verts(pred_n, b, max_verts);
  const float* pv = pred + (size_t)b * max_verts * 3;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (i < n_samples) {
    const float* q = samples + ((size_t)b * n_samples + i) * 3;
    qx = q[0]; qy = q[1]; qz = q[2];
  }
  float best = 3.0e38f;
  int bi = -1;
  for (int j0 = 0; j0 < nv; j0 += ISO_T) {
    __syncthreads();                                         // the previous tile has been read
    const int j = j0 + tid;
    float x = SURF_FAR, y = SURF_FAR, z = SURF_FAR;
    if (j < nv) { x = pv[(size_t)j * 3]; y = pv[(size_t)j * 3 + 1]; z = pv[(size_t)j * 3 + 2]; }
    tile[0][tid] = x; tile[1][tid] = y; tile[2][tid] = z;
    __syncthreads();
    const int cnt = min(ISO_T, nv - j0);
    for (int k = 0; k < cnt; ++k) {
      const float dx = qx - tile[0][k], dy = qy - tile[1][k], dz = qz - tile[2][k];
      const float dd = dx * dx + dy * dy + dz * dz;
      if (dd < best) { best = dd; bi = j0 + k; }             // strict, ascending: the lowest index wins an exact tie
    }
  }
  if (i >= n_samples) return;
  d2_out[(size_t)b * n_samples + i] = best;
  if (nearest_out) nearest_out[(size_t)b * n_samples + i] = bi;
}

// fixed-order fp64 sum over the block: xor tree inside a wave, then the waves in order; the result is in every thread
__device__ __forceinline__ double block_sum_f64(double v, double* red4) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

__global__ __launch_bounds__(ISO_T) void surf_reduce_kernel(const float* __restrict__ sdf, const int32_t* __restrict__ pred_n, int max_verts,
                                                           const float* __restrict__ d2, int n_samples, const float* __restrict__ box,
                                                           float* __restrict__ pred_to_gt, float* __restrict__ gt_to_pred,
                                                           float* __restrict__ chamfer, int32_t* __restrict__ n_used) {
  __shared__ double red4[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nv = sample_verts(pred_n, b, max_verts);
  const bool usable = nv > 0 && box[(size_t)b * 8 + 3] > 0.f;  // a ground-truth mesh without area has no usable face
  double s1 = 0.0, s2 = 0.0;
  if (usable) {                                              // the same for the whole block
    for (int v = tid; v < nv; v += ISO_T) { const double d = (double)sdf[(size_t)b * max_verts + v]; s1 += d * d; }
    for (int k = tid; k < n_samples; k += ISO_T) s2 += (double)d2[(size_t)b * n_samples + k];
  }
  s1 = block_sum_f64(s1, red4);
  s2 = block_sum_f64(s2, red4);
  if (tid != 0) return;
  const double m1 = usable ? s1 / (double)nv : 0.0, m2 = usable ? s2 / (double)n_samples : 0.0;
  pred_to_gt[b] = (float)m1;
  gt_to_pred[b] = (float)m2;
  chamfer[b] = (float)(m1 + m2);
  n_used[b] = usable ? nv : 0;
}

// workspace of hoisdf_eval_surface: the prepared mesh, a distance per predicted vertex, the surface samples, their squared distances
struct SurfWorkspace { MeshBuffers m; float *sdf, *samples, *d2; };
static SurfWorkspace surf_workspace(Bump& w, long B, long max_verts, long max_faces, long n_samples) {
  SurfWorkspace s;
  s.m = mesh_buffers(w, B, max_faces);
  s.sdf = w.floats(B * max_verts);
  s.samples = w.floats(B * n_samples * 3);
  s.d2 = w.floats(B * n_samples);
  return s;
}
static bool surf_shape_ok(const char* what, int B, int max_verts, int max_faces, int n_samples) {
  if (!mesh_shape_ok(what, B, 0, max_faces)) return false;
  if (max_verts < 0 || max_verts > (1 << 24) || n_samples < 1 || n_samples > (1 << 24)) {
    set_error("%s: max_verts=%d (0 .. 2^24) n_samples=%d (1 .. 2^24)", what, max_verts, n_samples);
    return false;
  }
  return true;
}

}  // namespace hoisdf

using namespace hoisdf;

extern "C" int hoisdf_iso_grid_points(const float* grid, int n, int B, float* points, int32_t* sample_idx, void* stream) {
  if (!iso_shape_ok("iso_grid_points", B, n)) return HOISDF_ERR_INVALID;
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(grid && points, HOISDF_ERR_INVALID, "iso_grid_points: null pointer (grid, points)");
  hipLaunchKernelGGL(iso_points_kernel, dim3(cdiv(iso_nodes(n), ISO_T), B), dim3(ISO_T), 0, as_stream(stream), grid, n, points, sample_idx);
  return check_launch("iso_grid_points");
}

extern "C" int hoisdf_iso_refine_grid(const float* values, int ld, const float* grid_in, int n, int B, float iso, int pad_cells,
                                      int n_out, float* grid_out, void* stream) {
  if (!iso_shape_ok("iso_refine_grid", B, n)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(ld >= 1, HOISDF_ERR_INVALID, "iso_refine_grid: ld=%d (>= 1)", ld);
  HOISDF_REQUIRE(pad_cells >= 0 && pad_cells <= HOISDF_ISO_MAX_GRID, HOISDF_ERR_INVALID, "iso_refine_grid: pad_cells=%d (0 .. %d)",
                 pad_cells, HOISDF_ISO_MAX_GRID);
  HOISDF_REQUIRE(n_out >= 2 && n_out <= HOISDF_ISO_MAX_GRID, HOISDF_ERR_INVALID, "iso_refine_grid: n_out=%d (2 .. %d)", n_out,
                 HOISDF_ISO_MAX_GRID);
  HOISDF_REQUIRE(iso == iso, HOISDF_ERR_INVALID, "iso_refine_grid: iso is not a number");
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(values && grid_in && grid_out, HOISDF_ERR_INVALID, "iso_refine_grid: null pointer (values, grid_in, grid_out)");
  hipLaunchKernelGGL(iso_refine_kernel, dim3(B), dim3(ISO_T), 0, as_stream(stream), values, ld, grid_in, n, iso, pad_cells, n_out, grid_out);
  return check_launch("iso_refine_grid");
}

extern "C" long hoisdf_iso_extract_workspace_bytes(int B, int n) {
  if (!iso_shape_ok("iso_extract_workspace_bytes", B, n)) return -1;
  Bump w(nullptr, 0);
  iso_workspace(w, B, n);
  return w.bytes();
}

extern "C" int hoisdf_iso_extract(const float* values, int ld, const float* grid, int n, int B, float iso, float out_scale,
                                  const float* out_shift, float* verts, int max_verts, int32_t* faces, int max_faces, int32_t* n_verts,
                                  int32_t* n_faces, void* workspace, long workspace_bytes, void* stream) {
  if (!iso_shape_ok("iso_extract", B, n)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(ld >= 1, HOISDF_ERR_INVALID, "iso_extract: ld=%d (>= 1)", ld);
  HOISDF_REQUIRE(max_verts >= 0 && max_faces >= 0, HOISDF_ERR_INVALID, "iso_extract: max_verts=%d max_faces=%d (>= 0)", max_verts, max_faces);
  HOISDF_REQUIRE(iso == iso, HOISDF_ERR_INVALID, "iso_extract: iso is not a number");
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(values && grid && n_verts && n_faces, HOISDF_ERR_INVALID, "iso_extract: null pointer (values, grid, n_verts, n_faces)");
  HOISDF_REQUIRE(workspace, HOISDF_ERR_INVALID, "iso_extract: null pointer (workspace)");
  Bump w(workspace, workspace_bytes);
  const IsoWorkspace s = iso_workspace(w, B, n);
  HOISDF_REQUIRE(workspace_bytes >= w.bytes(), HOISDF_ERR_INVALID, "iso_extract: workspace of %ld bytes, %ld needed", workspace_bytes, w.bytes());
  hipStream_t st = as_stream(stream);
  const int nblk = cdiv(iso_nodes(n), ISO_T);
  IsoArgs a;
  a.values = values; a.ld = ld; a.grid = grid; a.n = n; a.iso = iso;
  a.blk_v = s.blk_v; a.blk_f = s.blk_f; a.nblk = nblk;
  a.word = s.word;
  a.out_scale = out_scale; a.out_shift = out_shift;
  a.verts = verts; a.max_verts = verts ? max_verts : 0;
  a.faces = faces; a.max_faces = faces ? max_faces : 0;
  a.n_verts = n_verts; a.n_faces = n_faces;
  hipLaunchKernelGGL(iso_count_kernel, dim3(nblk, B), dim3(ISO_T), 0, st, a);
  hipLaunchKernelGGL(iso_scan_kernel, dim3(B), dim3(ISO_T), 0, st, a);
  if (verts || faces) hipLaunchKernelGGL(iso_vertex_kernel, dim3(nblk, B), dim3(ISO_T), 0, st, a);   // the faces need the node words
  if (faces) hipLaunchKernelGGL(iso_face_kernel, dim3(nblk, B), dim3(ISO_T), 0, st, a);
  return check_launch("iso_extract");
}

extern "C" long hoisdf_eval_surface_workspace_bytes(int B, int max_verts, int gt_max_faces, int n_samples) {
  if (!surf_shape_ok("eval_surface_workspace_bytes", B, max_verts, gt_max_faces, n_samples)) return -1;
  Bump w(nullptr, 0);
  surf_workspace(w, B, max_verts, gt_max_faces, n_samples);
  return w.bytes();
}

extern "C" int hoisdf_eval_surface(const float* pred_verts, const int32_t* pred_n_verts, int max_verts, const hoisdf_mesh* gt, int B,
                                   int n_samples, uint64_t seed, float* pred_to_gt, float* gt_to_pred, float* chamfer, int32_t* n_used,
                                   float* samples_out, int32_t* nearest_out, void* workspace, long workspace_bytes, void* stream) {
  if (!mesh_desc_ok("eval_surface", "gt", gt, B) || !surf_shape_ok("eval_surface", B, max_verts, gt->max_faces, n_samples))
    return HOISDF_ERR_INVALID;
  if (B == 0) return HOISDF_OK;
  if (!mesh_data_ok("eval_surface", "gt", gt)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(pred_n_verts && (max_verts == 0 || pred_verts), HOISDF_ERR_INVALID, "eval_surface: null pointer (pred_verts, pred_n_verts)");
  HOISDF_REQUIRE(pred_to_gt && gt_to_pred && chamfer && n_used, HOISDF_ERR_INVALID,
                 "eval_surface: null pointer (pred_to_gt, gt_to_pred, chamfer, n_used)");
  HOISDF_REQUIRE(workspace, HOISDF_ERR_INVALID, "eval_surface: null pointer (workspace)");
  Bump w(workspace, workspace_bytes);
  const SurfWorkspace s = surf_workspace(w, B, max_verts, gt->max_faces, n_samples);
  HOISDF_REQUIRE(workspace_bytes >= w.bytes(), HOISDF_ERR_INVALID, "eval_surface: workspace of %ld bytes, %ld needed", workspace_bytes, w.bytes());
  hipStream_t st = as_stream(stream);
  float* samples = samples_out ? samples_out : s.samples;
  launch_prepare(*gt, B, s.m, st);
  // every row of pred_verts against the mesh (rows from pred_n_verts[b] on are left out in the reduction)
  if (max_verts) launch_sdf(sdf_args(pred_verts, 3, max_verts, s.m, gt->n_faces, gt->max_faces, s.sdf, 1), B, st);
  // sigma 0 and no box points: a + s (b - a) ... in barycentric form + 0 x noise, exactly a point of the face drawn by area
  launch_sample(s.m, gt->n_faces, gt->max_faces, B, n_samples, 0.f, 0.f, 0, 0.f, seed, samples, (long)n_samples * 3, 3, nullptr, st);
  hipLaunchKernelGGL(surf_nn_kernel, dim3(cdiv(n_samples, ISO_T), B), dim3(ISO_T), 0, st, samples, n_samples, pred_verts, pred_n_verts,
                     max_verts, s.d2, nearest_out);
  hipLaunchKernelGGL(surf_reduce_kernel, dim3(B), dim3(ISO_T), 0, st, s.sdf, pred_n_verts, max_verts, s.d2, n_samples, s.m.box, pred_to_gt,
                     gt_to_pred, chamfer, n_used);
  return check_launch("eval_surface");
}
