// Mesh rasteriser (include/hoisdf.h "raster"): the posed hand and object meshes of a step -> per pixel the nearest covering face
// (id, depth), the two modal masks folded to the heat-map size, the visible pixel counts; a flat-colour overlay of such ids on a
// u8 image; intersection / union counts of two pairs of masks.  Coverage is integer arithmetic on corners snapped to 1/256 pixel,
// depth is fp64 in one fixed order, so hoisdf_amd/raster_oracle.py reproduces every output bit for bit.
//   raster_setup_kernel   one face per thread: project and snap the three corners (fp64, no product fused into a sum), the
//                         skipped-face rule, corners 1 and 2 swapped where the doubled area is negative -> a 64-byte record: snapped
//                         corners, pixel box clipped to the image (empty: skipped), doubled area, the three 1 / z.  Zeroes counts.
//   raster_kernel         tile-major: a workgroup of 256 threads owns a 32 x 32 tile of one sample, wave w its rows 8 w .. 8 w + 7,
//                         a thread the 4 pixels (lx, 8 w + (lane >> 5) + 2 j).  The sample's records (hand, then object: ascending
//                         key) pass through LDS in chunks of 256 (16 KiB, copied as 1024 uint4: coalesced, no bank conflict); a wave
//                         tests 64 boxes against its 32 x 8 strip, one per lane, and walks the ballot's set bits: the face is then
//                         uniform across the wave (its record is an LDS broadcast, the edge set-up scalar work).  Per pixel three
//                         int64 edge values (two 32 x 32 -> 64 multiply-adds each for the first row, one add per further row); a
//                         covered pixel pays four fp64 divisions.  A pixel belongs to one thread and the records arrive in ascending
//                         key order, so "strictly nearer replaces" IS the smallest (depth, mesh, face) key: no atomic on the way to
//                         a pixel, no second pass, the same bits on every call.  The counts are integer sums: per workgroup in LDS,
//                         then one integer atomic add per mesh (independent of the order).
//   overlay_kernel        one pixel per thread, 3 bytes in, 3 bytes out (in place allowed: a thread reads its bytes before it writes)
//   silhouette_kernel     one workgroup per sample: four integer sums
#include "mesh.h"

namespace hoisdf {

constexpr int RASTER_TILE = 32, RASTER_CHUNK = 256, RASTER_T = 256;
constexpr int RASTER_ROWS = RASTER_TILE * RASTER_TILE / RASTER_T;          // pixels per thread: rows ly, ly + 2, ly + 4, ly + 6 of the strip
static_assert(HOISDF_RASTER_TILE == RASTER_TILE && HOISDF_RASTER_CHUNK == RASTER_CHUNK, "the header states the tile and the chunk the tests aim at");
static_assert(RASTER_TILE == 32 && RASTER_T == 256 && RASTER_ROWS == 4 && RASTER_CHUNK % 64 == 0, "the thread -> pixel map below");
constexpr int RASTER_SUB = 256;                                          // sub-pixel positions per pixel
constexpr double RASTER_GUARD = 16384.0;                                 // |u|, |v| below this: |X|, |Y| <= 2^22

struct alignas(16) RasterRec {
  int32_t X[3], Y[3];          // snapped corners, wound so that A2 > 0
  int16_t x0, x1, y0, y1;      // pixels whose sample point can be covered, clipped to the image; x0 > x1: the face is skipped
  int64_t A2;
  double iz[3];                // 1 / z of the corners
};
static_assert(sizeof(RasterRec) == 64, "four uint4 per record");

struct RasterMesh {            // a hoisdf_mesh by value (all NULL / 0: the mesh is absent)
  const float* verts; const int32_t* faces; const int32_t* n_faces; long stride; int V, max_faces;
};
struct RasterArgs {
  RasterMesh mesh[2];
  const float* K; double near;
  int width, height, off;      // off = 128 half_pixel
  int tiles_x, nrec;           // nrec = hand max_faces + obj max_faces records per sample
  RasterRec* recs;
  int32_t* id_out; float* depth_out; float* seg[2]; int hm_w, hm_h; int32_t* counts;
};

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) <= 3.4028234664e38f; }   // false for NaN and the infinities

// one corner: false where the skipped-face rule drops the face
__device__ __forceinline__ bool raster_corner(const float* __restrict__ K, const float* __restrict__ p, double near, int32_t* X, int32_t* Y,
                                              double* iz) {
#pragma clang fp contract(off)
  if (!finite_f(p[0]) || !finite_f(p[1]) || !finite_f(p[2])) return false;
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  if (z < near) return false;
  const double u = (((double)K[0] * x + (double)K[1] * y) + (double)K[2] * z) / z;
  const double v = (((double)K[3] * x + (double)K[4] * y) + (double)K[5] * z) / z;
  if (!(fabs(u) < RASTER_GUARD) || !(fabs(v) < RASTER_GUARD)) return false;      // also a K that is not finite
  *X = (int32_t)rint((double)RASTER_SUB * u);                                    // round half to even
  *Y = (int32_t)rint((double)RASTER_SUB * v);
  *iz = 1.0 / z;
  return true;
}

__global__ __launch_bounds__(RASTER_T) void raster_setup_kernel(const RasterArgs a) {
  const int b = blockIdx.y, r = blockIdx.x * RASTER_T + threadIdx.x;
  if (a.counts && blockIdx.x == 0 && threadIdx.x < 2) a.counts[(size_t)b * 2 + threadIdx.x] = 0;
  if (r >= a.nrec) return;
  const int which = r >= a.mesh[0].max_faces ? 1 : 0, f = which ? r - a.mesh[0].max_faces : r;
  const RasterMesh& m = a.mesh[which];
  RasterRec rec;
  rec.x0 = rec.y0 = 0x7fff; rec.x1 = rec.y1 = -1;
  rec.A2 = 1;
#pragma unroll
  for (int c = 0; c < 3; ++c) { rec.X[c] = rec.Y[c] = 0; rec.iz[c] = 0.0; }
  bool ok = f < sample_faces(m.n_faces, b, m.max_faces);
  int idx[3] = {0, 0, 0};
  if (ok) {
    const int32_t* fr = m.faces + (size_t)b * m.stride + (size_t)f * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) { idx[c] = fr[c]; ok = ok && idx[c] >= 0 && idx[c] < m.V; }
  }
  if (ok) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      ok = raster_corner(a.K + (size_t)b * 6, m.verts + ((size_t)b * m.V + idx[c]) * 3, a.near, &rec.X[c], &rec.Y[c], &rec.iz[c]) && ok;
  }
  if (ok) {
    int64_t A2 = (int64_t)(rec.X[1] - rec.X[0]) * (rec.Y[2] - rec.Y[0]) - (int64_t)(rec.X[2] - rec.X[0]) * (rec.Y[1] - rec.Y[0]);
    if (A2 < 0) {
      const int32_t tx = rec.X[1], ty = rec.Y[1];
      const double tz = rec.iz[1];
      rec.X[1] = rec.X[2]; rec.Y[1] = rec.Y[2]; rec.iz[1] = rec.iz[2];
      rec.X[2] = tx; rec.Y[2] = ty; rec.iz[2] = tz;
      A2 = -A2;
    }
    ok = A2 != 0;
    if (ok) {
      rec.A2 = A2;
      // pixels px with X_min <= 256 px + off <= X_max (arithmetic shifts: ceil and floor), then the image
      const int xa = min(rec.X[0], min(rec.X[1], rec.X[2])) - a.off, xb = max(rec.X[0], max(rec.X[1], rec.X[2])) - a.off;
      const int ya = min(rec.Y[0], min(rec.Y[1], rec.Y[2])) - a.off, yb = max(rec.Y[0], max(rec.Y[1], rec.Y[2])) - a.off;
      const int x0 = max((xa + RASTER_SUB - 1) >> 8, 0), x1 = min(xb >> 8, a.width - 1);
      const int y0 = max((ya + RASTER_SUB - 1) >> 8, 0), y1 = min(yb >> 8, a.height - 1);
      if (x0 <= x1 && y0 <= y1) { rec.x0 = (int16_t)x0; rec.x1 = (int16_t)x1; rec.y0 = (int16_t)y0; rec.y1 = (int16_t)y1; }
    }
  }
  a.recs[(size_t)b * a.nrec + r] = rec;
}

// z of a covered sample point: perspective-correct, fp64, one order
__device__ __forceinline__ float raster_depth(int64_t e0, int64_t e1, int64_t e2, double A2, double iz0, double iz1, double iz2) {
#pragma clang fp contract(off)
  const double l0 = (double)e0 / A2, l1 = (double)e1 / A2, l2 = (double)e2 / A2;
  const double p0 = l0 * iz0, p1 = l1 * iz1, p2 = l2 * iz2;
  const double invz = (p0 + p1) + p2;
  return (float)(1.0 / invz);
}

__global__ __launch_bounds__(RASTER_T) void raster_kernel(const RasterArgs a) {
  __shared__ RasterRec s_rec[RASTER_CHUNK];
  __shared__ int s_cnt[2][RASTER_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
  const int tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
  const int px = tx * RASTER_TILE + (tid & 31), py0 = ty * RASTER_TILE + wv * 8 + (lane >> 5);
  const int wx0 = tx * RASTER_TILE, wx1 = wx0 + RASTER_TILE - 1, wy0 = ty * RASTER_TILE + wv * 8, wy1 = wy0 + 7;   // the wave's strip
  const int sx = RASTER_SUB * px + a.off, sy = RASTER_SUB * py0 + a.off;                                        // < 2^21
  const int Fh = a.mesh[0].max_faces;
  float best[RASTER_ROWS];
  int id[RASTER_ROWS];
#pragma unroll
  for (int j = 0; j < RASTER_ROWS; ++j) { best[j] = __int_as_float(0x7f800000); id[j] = -1; }

  const uint4* src = reinterpret_cast<const uint4*>(a.recs + (size_t)b * a.nrec);
  uint4* dst = reinterpret_cast<uint4*>(s_rec);
  for (int c0 = 0; c0 < a.nrec; c0 += RASTER_CHUNK) {
    const int cnt = min(RASTER_CHUNK, a.nrec - c0);
    __syncthreads();                                          // the previous chunk has been read
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = q * RASTER_T + tid;
      if (i < cnt * 4) dst[i] = src[(size_t)c0 * 4 + i];
    }
    __syncthreads();
    for (int g0 = 0; g0 < cnt; g0 += 64) {
      const int k = g0 + lane;
      bool hit = false;
      if (k < cnt) {
        const RasterRec& q = s_rec[k];
        hit = q.x0 <= wx1 && q.x1 >= wx0 && q.y0 <= wy1 && q.y1 >= wy0;
      }
      unsigned long long todo = __ballot(hit);
      while (todo) {
        const int kk = g0 + __builtin_ctzll(todo);            // the same in every lane
        todo &= todo - 1;
        const RasterRec& R = s_rec[kk];
        const int r = c0 + kk, key = r < Fh ? r : (1 << 16 | (r - Fh));
        // edge i is opposite corner i: from corner i + 1 to corner i + 2
        // e[i] = the edge value minus bias[i]: a point on the edge counts for a left edge (dy < 0: the interior at larger x) or a
        // top edge (dy = 0, dx > 0), so the test is E >= 0 for those (bias 0) and E >= 1 for the others (bias 1)
        int64_t e[3], step[3];
        int bias[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const int j = (i + 1) % 3, k2 = (i + 2) % 3;
          const int dx = R.X[k2] - R.X[j], dy = R.Y[k2] - R.Y[j];                 // |.| <= 2^23
          bias[i] = (dy < 0 || (dy == 0 && dx > 0)) ? 0 : 1;
          e[i] = (int64_t)dx * (int64_t)(sy - R.Y[j]) - (int64_t)dy * (int64_t)(sx - R.X[j]) - bias[i];
          step[i] = (int64_t)dx * (2 * RASTER_SUB);                                // two rows down
        }
        const double A2 = (double)R.A2;
#pragma unroll
        for (int j = 0; j < RASTER_ROWS; ++j) {
          if ((e[0] | e[1] | e[2]) >= 0) {                                         // all three sign bits clear
            const float z = raster_depth(e[0] + bias[0], e[1] + bias[1], e[2] + bias[2], A2, R.iz[0], R.iz[1], R.iz[2]);
            if (z < best[j]) { best[j] = z; id[j] = key; }                         // ascending keys: the smallest wins a tie
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) e[i] += step[i];
        }
      }
    }
  }

  int c_hand = 0, c_obj = 0;
  const int fx = a.seg[0] || a.seg[1] ? a.width / a.hm_w : 1, fy = a.seg[0] || a.seg[1] ? a.height / a.hm_h : 1;
#pragma unroll
  for (int j = 0; j < RASTER_ROWS; ++j) {
    const int py = py0 + 2 * j;
    if (px >= a.width || py >= a.height) continue;
    const size_t o = ((size_t)b * a.height + py) * a.width + px;
    const int which = id[j] < 0 ? -1 : id[j] >> 16;
    if (a.id_out) a.id_out[o] = id[j];
    if (a.depth_out) a.depth_out[o] = which < 0 ? 0.f : best[j];
    c_hand += which == 0;
    c_obj += which == 1;
    if ((a.seg[0] || a.seg[1]) && px % fx == fx / 2 && py % fy == fy / 2) {        // the raster pixel mask pixel (px / fx, py / fy) reads
      const size_t mo = ((size_t)b * a.hm_h + py / fy) * a.hm_w + px / fx;
      if (a.seg[0]) a.seg[0][mo] = which == 0 ? 1.f : 0.f;
      if (a.seg[1]) a.seg[1][mo] = which == 1 ? 1.f : 0.f;
    }
  }
  if (!a.counts) return;                                                           // the same for the whole grid
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { c_hand += __shfl_xor(c_hand, o, 64); c_obj += __shfl_xor(c_obj, o, 64); }
  if (lane == 0) { s_cnt[0][wv] = c_hand; s_cnt[1][wv] = c_obj; }
  __syncthreads();
  if (tid < 2) {
    const int n = s_cnt[tid][0] + s_cnt[tid][1] + s_cnt[tid][2] + s_cnt[tid][3];
    if (n) atomicAdd(a.counts + (size_t)b * 2 + tid, n);
  }
}

struct OverlayColour { uint8_t c[2][3]; };

__global__ __launch_bounds__(RASTER_T) void overlay_kernel(const int32_t* __restrict__ id, const uint8_t* image_in, uint8_t* image_out,
                                                           OverlayColour col, int alpha, long n_pixels) {
  const long i = (long)blockIdx.x * RASTER_T + threadIdx.x;
  if (i >= n_pixels) return;
  const int k = id[i];
  const int which = k < 0 ? -1 : (k >> 16) & 1;
  int v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = image_in[i * 3 + c];
  if (which >= 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (alpha * col.c[which][c] + (256 - alpha) * v[c] + 128) >> 8;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) image_out[i * 3 + c] = (uint8_t)v[c];
}

__global__ __launch_bounds__(RASTER_T) void silhouette_kernel(const float* __restrict__ pred_hand, const float* __restrict__ pred_obj,
                                                              const float* __restrict__ gt_hand, const float* __restrict__ gt_obj, int n,
                                                              int32_t* __restrict__ counts) {
  __shared__ int s[4][RASTER_T / 64];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t base = (size_t)b * n;
  int c[4] = {0, 0, 0, 0};
  for (int i = tid; i < n; i += RASTER_T) {
    const bool ph = pred_hand[base + i] > 0.5f, gh = gt_hand[base + i] > 0.5f, po = pred_obj[base + i] > 0.5f, go = gt_obj[base + i] > 0.5f;
    c[0] += ph && gh; c[1] += ph || gh; c[2] += po && go; c[3] += po || go;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c[k] += __shfl_xor(c[k], o, 64);
    if ((tid & 63) == 0) s[k][tid >> 6] = c[k];
  }
  __syncthreads();
  if (tid < 4) counts[(size_t)b * 4 + tid] = s[tid][0] + s[tid][1] + s[tid][2] + s[tid][3];
}

// the workspace is one array of records: a Bump of one piece, so that it rounds as every other workspace does
static long raster_workspace_bytes(long B, long nrec) {
  Bump w(nullptr, 0);
  w.take(B * nrec * (long)sizeof(RasterRec));
  return w.bytes();
}
static RasterMesh raster_mesh(const hoisdf_mesh* m) {
  if (!m) return {nullptr, nullptr, nullptr, 0, 0, 0};
  return {m->verts, m->faces, m->n_faces, m->face_batch_stride, m->V, m->max_faces};
}

}  // namespace hoisdf

using namespace hoisdf;

extern "C" long hoisdf_raster_workspace_bytes(int B, int hand_max_faces, int obj_max_faces) {
  if (!mesh_shape_ok("raster_workspace_bytes (hand)", B, 0, hand_max_faces) || !mesh_shape_ok("raster_workspace_bytes (obj)", B, 0, obj_max_faces))
    return -1;
  return raster_workspace_bytes(B, (long)hand_max_faces + obj_max_faces);
}

extern "C" int hoisdf_raster_meshes(const hoisdf_mesh* hand, const hoisdf_mesh* obj, const float* K, int B, int width, int height,
                                    int half_pixel, float near, int32_t* id_out, float* depth_out, float* hand_seg, float* obj_seg,
                                    int hm_w, int hm_h, int32_t* counts, void* workspace, long workspace_bytes, void* stream) {
  HOISDF_REQUIRE(hand || obj, HOISDF_ERR_INVALID, "raster_meshes: null pointer (hand and obj: one mesh at least)");
  HOISDF_REQUIRE(B >= 0 && B <= 65535, HOISDF_ERR_INVALID, "raster_meshes: B=%d (0 .. 65535)", B);
  if (!mesh_desc_ok("raster_meshes", "hand", hand, B, true) || !mesh_desc_ok("raster_meshes", "obj", obj, B, true)) return HOISDF_ERR_INVALID;
  HOISDF_REQUIRE(width >= 1 && width <= HOISDF_RASTER_MAX_SIZE && height >= 1 && height <= HOISDF_RASTER_MAX_SIZE, HOISDF_ERR_INVALID,
                 "raster_meshes: width=%d height=%d (1 .. %d)", width, height, HOISDF_RASTER_MAX_SIZE);
  HOISDF_REQUIRE(half_pixel == 0 || half_pixel == 1, HOISDF_ERR_INVALID, "raster_meshes: half_pixel=%d (0 or 1)", half_pixel);
  HOISDF_REQUIRE(near > 0.f && near <= 3.4028234664e38f, HOISDF_ERR_INVALID, "raster_meshes: near=%g (finite, > 0)", (double)near);
  HOISDF_REQUIRE(id_out || depth_out || hand_seg || obj_seg || counts, HOISDF_ERR_INVALID,
                 "raster_meshes: null pointer (id_out, depth_out, hand_seg, obj_seg, counts: one output at least)");
  if (hand_seg || obj_seg)
    HOISDF_REQUIRE(hm_w >= 1 && hm_h >= 1 && width % hm_w == 0 && height % hm_h == 0, HOISDF_ERR_INVALID,
                   "raster_meshes: hm_w=%d hm_h=%d (>= 1, dividing width=%d and height=%d)", hm_w, hm_h, width, height);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(K, HOISDF_ERR_INVALID, "raster_meshes: null pointer (K)");
  if (!mesh_data_ok("raster_meshes", "hand", hand) || !mesh_data_ok("raster_meshes", "obj", obj)) return HOISDF_ERR_INVALID;
  const long nrec = (long)(hand ? hand->max_faces : 0) + (obj ? obj->max_faces : 0);
  const long need = raster_workspace_bytes(B, nrec);
  HOISDF_REQUIRE(workspace || need == 0, HOISDF_ERR_INVALID, "raster_meshes: null pointer (workspace)");
  HOISDF_REQUIRE(workspace_bytes >= need, HOISDF_ERR_INVALID, "raster_meshes: workspace of %ld bytes, %ld needed", workspace_bytes, need);
  RasterArgs a;
  a.mesh[0] = raster_mesh(hand); a.mesh[1] = raster_mesh(obj);
  a.K = K; a.near = (double)near;
  a.width = width; a.height = height; a.off = half_pixel ? RASTER_SUB / 2 : 0;
  a.tiles_x = cdiv(width, RASTER_TILE); a.nrec = (int)nrec;
  a.recs = (RasterRec*)workspace;
  a.id_out = id_out; a.depth_out = depth_out; a.seg[0] = hand_seg; a.seg[1] = obj_seg; a.hm_w = hm_w; a.hm_h = hm_h; a.counts = counts;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(raster_setup_kernel, dim3(nrec ? cdiv(nrec, RASTER_T) : 1, B), dim3(RASTER_T), 0, st, a);
  hipLaunchKernelGGL(raster_kernel, dim3(a.tiles_x * cdiv(height, RASTER_TILE), B), dim3(RASTER_T), 0, st, a);
  return check_launch("raster_meshes");
}

extern "C" int hoisdf_raster_overlay(const int32_t* id, const uint8_t* image_in, uint8_t* image_out, const uint8_t* colour, int alpha,
                                     int B, int width, int height, void* stream) {
  HOISDF_REQUIRE(B >= 0 && B <= 65535, HOISDF_ERR_INVALID, "raster_overlay: B=%d (0 .. 65535)", B);
  HOISDF_REQUIRE(width >= 1 && width <= HOISDF_RASTER_MAX_SIZE && height >= 1 && height <= HOISDF_RASTER_MAX_SIZE, HOISDF_ERR_INVALID,
                 "raster_overlay: width=%d height=%d (1 .. %d)", width, height, HOISDF_RASTER_MAX_SIZE);
  HOISDF_REQUIRE(alpha >= 0 && alpha <= 256, HOISDF_ERR_INVALID, "raster_overlay: alpha=%d (0 .. 256)", alpha);
  HOISDF_REQUIRE(colour, HOISDF_ERR_INVALID, "raster_overlay: null pointer (colour)");
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(id && image_in && image_out, HOISDF_ERR_INVALID, "raster_overlay: null pointer (id, image_in, image_out)");
  OverlayColour col;
  for (int m = 0; m < 2; ++m)
    for (int c = 0; c < 3; ++c) col.c[m][c] = colour[m * 3 + c];
  const long n = (long)B * width * height;                   // <= 65535 x 2^24 pixels: the grid stays below 2^31 blocks
  hipLaunchKernelGGL(overlay_kernel, dim3((unsigned)((n + RASTER_T - 1) / RASTER_T)), dim3(RASTER_T), 0, as_stream(stream), id, image_in,
                     image_out, col, alpha, n);
  return check_launch("raster_overlay");
}

extern "C" int hoisdf_eval_silhouette(const float* pred_hand, const float* pred_obj, const float* gt_hand, const float* gt_obj, int B, int n,
                                      int32_t* counts, void* stream) {
  HOISDF_REQUIRE(B >= 0 && B <= 65535, HOISDF_ERR_INVALID, "eval_silhouette: B=%d (0 .. 65535)", B);
  HOISDF_REQUIRE(n >= 1 && n <= (1 << 24), HOISDF_ERR_INVALID, "eval_silhouette: n=%d (1 .. 2^24)", n);
  if (B == 0) return HOISDF_OK;
  HOISDF_REQUIRE(pred_hand && pred_obj && gt_hand && gt_obj && counts, HOISDF_ERR_INVALID,
                 "eval_silhouette: null pointer (pred_hand, pred_obj, gt_hand, gt_obj, counts)");
  hipLaunchKernelGGL(silhouette_kernel, dim3(B), dim3(RASTER_T), 0, as_stream(stream), pred_hand, pred_obj, gt_hand, gt_obj, n, counts);
  return check_launch("eval_silhouette");
}
