/* A C host with no Python and no torch holds a projected point set to a pair of masks, through include/hoisdf.h:
 *   hoisdf_mask_edt -> hoisdf_silhouette_loss_workspace_bytes -> hoisdf_silhouette_loss_fwd -> hoisdf_silhouette_loss_bwd (one call
 *   each for the batch)
 * prints what it got and writes it; tests/test_gpu_silhouette_loss.py::test_c_host_silhouette_loss compares it with the numpy
 * restatement and, bit for bit, with ops.mask_edt / ops.silhouette_loss and its backward on the same inputs.
 * Input file (little-endian): int32 B, V, w, h; float32 near; then arrays, each as int64 count + 4-byte data: verts float32
 * [B][V][3], n_verts int32 [B], K float32 [B][6], allow mask float32 [B][h][w], cover mask float32 [B][h][w], weight float32 [B][V],
 * upstream gradients float32 [2][B] (inside, cover).
 * Output file: d2 int32 [B][h][w]; inside, cover float32 [B] each; d_verts float32 [B][V][3]. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hoisdf.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "hip error line %d\n", __LINE__); return 2; } } while (0)
#define CALL(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "line %d: status %d: %s\n", __LINE__, rc_, hoisdf_last_error()); return 1; } } while (0)

static FILE* f;
/* next array of the file: `expect` 4-byte words, uploaded */
static void* rd(long expect) {
  int64_t n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1 || n != expect) { fprintf(stderr, "array of %ld words, expected %ld\n", (long)n, expect); exit(2); }
  void* h = malloc(4 * (size_t)n + 4);
  if (fread(h, 4, n, f) != (size_t)n) { fprintf(stderr, "short read\n"); exit(2); }
  void* d = NULL;
  if (hipMalloc(&d, 4 * (size_t)n + 4) != hipSuccess || hipMemcpy(d, h, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) exit(2);
  free(h);
  return d;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <inputs.bin> <outputs.bin>\n", argv[0]); return 2; }
  f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  int32_t hd[4];
  float near;
  if (fread(hd, sizeof(int32_t), 4, f) != 4 || fread(&near, sizeof(float), 1, f) != 1) return 2;
  const int B = hd[0], V = hd[1], w = hd[2], h = hd[3];
  if (B < 1 || B > 64 || V < 1 || V > 100000 || w < 1 || w > HOISDF_EDT_MAX_SIZE || h < 1 || h > HOISDF_EDT_MAX_SIZE) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  const long npix = (long)B * h * w;
  const float* verts = (const float*)rd((long)B * V * 3);
  const int32_t* n_verts = (const int32_t*)rd(B);
  const float* K = (const float*)rd(6L * B);
  const float* allow = (const float*)rd(npix);
  const float* cover = (const float*)rd(npix);
  const float* weight = (const float*)rd((long)B * V);
  const float* g = (const float*)rd(2L * B);
  fclose(f);

  const long nws = hoisdf_silhouette_loss_workspace_bytes(B, V, w, h);
  if (nws < 0) { fprintf(stderr, "workspace: %s\n", hoisdf_last_error()); return 1; }
  const long n_out = npix + 2L * B + 3L * B * V;
  int32_t* out;   /* d2 [B][h][w], then as floats inside [B], cover [B], d_verts [B][V][3] */
  void* ws;
  CHECK(hipMalloc((void**)&out, 4 * (size_t)n_out));
  CHECK(hipMalloc(&ws, nws > 0 ? (size_t)nws : 1));
  float* vals = (float*)(out + npix);
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  CALL(hoisdf_mask_edt(allow, NULL, B, w, h, out, NULL, st));
  CALL(hoisdf_silhouette_loss_fwd(verts, n_verts, V, K, B, out, cover, w, h, near, weight, V, vals, vals + B, ws, nws, st));
  CALL(hoisdf_silhouette_loss_bwd(verts, n_verts, V, K, B, out, cover, w, h, near, weight, V, g, g + B, vals + 2 * B, ws, nws, st));
  CHECK(hipStreamSynchronize(st));

  int32_t* hst = (int32_t*)malloc(4 * (size_t)n_out);
  CHECK(hipMemcpy(hst, out, 4 * (size_t)n_out, hipMemcpyDeviceToHost));
  const float* hv = (const float*)(hst + npix);
  for (int b = 0; b < B; ++b) {
    double n2 = 0;
    int far = 0;
    for (long i = 0; i < 3L * V; ++i) n2 += (double)hv[2 * B + (long)b * V * 3 + i] * hv[2 * B + (long)b * V * 3 + i];
    for (long i = 0; i < (long)h * w; ++i) far = hst[(long)b * h * w + i] > far ? hst[(long)b * h * w + i] : far;
    printf("sample %d: inside %.6f px, cover %.6f px, |d_verts|^2 %.4g, largest d2 %d\n", b, hv[b], hv[B + b], n2, far);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror("open"); return 2; }
  if (fwrite(hst, 4, n_out, o) != (size_t)n_out) {
    fprintf(stderr, "writing the outputs failed\n");
    return 2;
  }
  fclose(o);
  printf("c host silhouette loss ok: %d samples\n", B);
  return 0;
}
