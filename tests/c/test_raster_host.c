/* A C host with no Python and no torch renders two posed meshes through include/hoisdf.h:
 *   hoisdf_raster_workspace_bytes -> hoisdf_raster_meshes (ids, depth, the two folded masks, the counts) -> hoisdf_raster_overlay
 * checks on the host that the outputs agree with each other, and writes what it got;
 * tests/test_gpu_raster.py::test_the_c_host_reproduces_the_python_call_bit_for_bit compares it with ops.raster_meshes on the same inputs.
 * Input file (little-endian): int32 B, width, height, hm_w, hm_h, Vh, Fh, Vo, Fo, half_pixel; then K float32 [B][6], hand verts
 * float32 [B][Vh][3], hand faces int32 [Fh][3], object verts float32 [B][Vo][3], object faces int32 [Fo][3].
 * Output file: ids int32 [B][height][width], depth float32 (same), hand_seg float32 [B][hm_h][hm_w], obj_seg (same), counts int32 [B][2]. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hoisdf.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "hip error line %d\n", __LINE__); return 2; } } while (0)
#define CALL(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "line %d: status %d: %s\n", __LINE__, rc_, hoisdf_last_error()); return 1; } } while (0)

static FILE* f;
/* the next `n` 4-byte words of the file, uploaded */
static void* rd(long n) {
  void* h = malloc(4 * (size_t)n + 4);
  if (fread(h, 4, n, f) != (size_t)n) { fprintf(stderr, "short read\n"); exit(2); }
  void* d = NULL;
  if (hipMalloc(&d, 4 * (size_t)n + 4) != hipSuccess || hipMemcpy(d, h, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) exit(2);
  free(h);
  return d;
}
static void* down(const void* dev, size_t bytes) {
  void* h = malloc(bytes);
  if (hipMemcpy(h, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "copy back failed\n"); exit(2); }
  return h;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <inputs.bin> <outputs.bin>\n", argv[0]); return 2; }
  f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  int32_t hd[10];
  if (fread(hd, sizeof(int32_t), 10, f) != 10) return 2;
  const int B = hd[0], W = hd[1], H = hd[2], hm_w = hd[3], hm_h = hd[4], Vh = hd[5], Fh = hd[6], Vo = hd[7], Fo = hd[8], half = hd[9];
  if (B < 1 || B > 64 || W < 1 || W > HOISDF_RASTER_MAX_SIZE || H < 1 || H > HOISDF_RASTER_MAX_SIZE || hm_w < 1 || hm_h < 1 || Vh < 1 ||
      Vh > 100000 || Vo < 1 || Vo > 100000 || Fh < 1 || Fh > HOISDF_MESH_MAX_FACES || Fo < 1 || Fo > HOISDF_MESH_MAX_FACES) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  float* K = (float*)rd((long)B * 6);
  hoisdf_mesh hand = {0}, obj = {0};
  hand.verts = (const float*)rd((long)B * Vh * 3);
  hand.faces = (const int32_t*)rd((long)Fh * 3);
  hand.V = Vh; hand.max_faces = Fh;                       /* n_faces NULL: every row; face_batch_stride 0: one table for the batch */
  obj.verts = (const float*)rd((long)B * Vo * 3);
  obj.faces = (const int32_t*)rd((long)Fo * 3);
  obj.V = Vo; obj.max_faces = Fo;
  fclose(f);

  const size_t n_px = (size_t)B * H * W, n_hm = (size_t)B * hm_h * hm_w;
  const long nws = hoisdf_raster_workspace_bytes(B, Fh, Fo);
  if (nws < 0) { fprintf(stderr, "workspace: %s\n", hoisdf_last_error()); return 1; }
  int32_t *ids, *counts;
  float *depth, *hseg, *oseg;
  uint8_t* image;
  void* ws;
  CHECK(hipMalloc((void**)&ids, 4 * n_px));
  CHECK(hipMalloc((void**)&depth, 4 * n_px));
  CHECK(hipMalloc((void**)&hseg, 4 * n_hm));
  CHECK(hipMalloc((void**)&oseg, 4 * n_hm));
  CHECK(hipMalloc((void**)&counts, 8 * (size_t)B));
  CHECK(hipMalloc((void**)&image, 3 * n_px));
  CHECK(hipMalloc(&ws, (size_t)nws + 1));
  CHECK(hipMemset(image, 100, 3 * n_px));
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  CALL(hoisdf_raster_meshes(&hand, &obj, K, B, W, H, half, 0.01f, ids, depth, hseg, oseg, hm_w, hm_h, counts, ws, nws, st));
  const uint8_t colour[2][3] = {{70, 130, 255}, {255, 160, 40}};
  CALL(hoisdf_raster_overlay(ids, image, image, &colour[0][0], 256, B, W, H, st));      /* in place, opaque */
  CHECK(hipStreamSynchronize(st));

  int32_t* h_ids = (int32_t*)down(ids, 4 * n_px);
  float* h_depth = (float*)down(depth, 4 * n_px);
  float* h_hseg = (float*)down(hseg, 4 * n_hm);
  float* h_oseg = (float*)down(oseg, 4 * n_hm);
  int32_t* h_counts = (int32_t*)down(counts, 8 * (size_t)B);
  uint8_t* h_image = (uint8_t*)down(image, 3 * n_px);
  /* the outputs agree with each other: counts = ids per mesh, depth > 0 exactly where an id is, the overlay shows the id's colour,
   * a mask pixel is the id of the raster pixel it reads */
  for (int b = 0; b < B; ++b) {
    long n[2] = {0, 0};
    for (long i = (long)b * H * W; i < (long)(b + 1) * H * W; ++i) {
      const int id = h_ids[i], m = id < 0 ? -1 : id >> 16;
      if (id < -1 || m > 1 || (m == 0 && (id & 0xffff) >= Fh) || (m == 1 && (id & 0xffff) >= Fo)) { fprintf(stderr, "id %d\n", id); return 1; }
      if ((m >= 0) != (h_depth[i] > 0.f)) { fprintf(stderr, "depth %g at id %d\n", (double)h_depth[i], id); return 1; }
      if (m >= 0) ++n[m];
      for (int c = 0; c < 3; ++c)
        if (h_image[3 * i + c] != (m < 0 ? 100 : colour[m][c])) { fprintf(stderr, "overlay at pixel %ld\n", i); return 1; }
    }
    if (n[0] != h_counts[2 * b] || n[1] != h_counts[2 * b + 1]) { fprintf(stderr, "counts of sample %d\n", b); return 1; }
    for (int j = 0; j < hm_h; ++j)
      for (int i = 0; i < hm_w; ++i) {
        const int px = (int)(((2 * i + 1) * (long)W) / (2 * hm_w)), py = (int)(((2 * j + 1) * (long)H) / (2 * hm_h));
        const int id = h_ids[((long)b * H + py) * W + px], m = id < 0 ? -1 : id >> 16;
        const long o = ((long)b * hm_h + j) * hm_w + i;
        if (h_hseg[o] != (m == 0 ? 1.f : 0.f) || h_oseg[o] != (m == 1 ? 1.f : 0.f)) { fprintf(stderr, "mask pixel %d %d\n", i, j); return 1; }
      }
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror("open"); return 2; }
  if (fwrite(h_ids, 4, n_px, o) != n_px || fwrite(h_depth, 4, n_px, o) != n_px || fwrite(h_hseg, 4, n_hm, o) != n_hm ||
      fwrite(h_oseg, 4, n_hm, o) != n_hm || fwrite(h_counts, 4, 2 * (size_t)B, o) != 2 * (size_t)B) {
    fprintf(stderr, "writing the outputs failed\n");
    return 2;
  }
  fclose(o);
  printf("c host raster ok: %d samples, %d + %d faces, %d x %d pixels, %d + %d visible in sample 0\n", B, Fh, Fo, W, H, h_counts[0], h_counts[1]);
  return 0;
}
