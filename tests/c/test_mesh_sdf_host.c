/* A C host with no Python and no torch computes signed distances to a mesh through include/hoisdf.h:
 *   hoisdf_mesh_prepare (once per batch of meshes) -> hoisdf_mesh_sdf (per set of query points)
 * and writes what it got; tests/test_gpu_mesh_sdf.py::test_c_host_mesh_sdf compares it bit for bit with ops.mesh_sdf on the same inputs.
 * Input file (little-endian): int32 B, V, F, N, per_sample (1: one face table per sample); then arrays, each as int64 count + 4-byte
 * data: verts float32 [B][V][3], faces int32 [F][3] or [B][F][3], n_faces int32 [B], points float32 [B][N][3], vert_label int32 [V].
 * Output file: sdf float32 [B][N], then face int32 [B][N], then label int32 [B][N]. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
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
static int wr(FILE* o, const void* dev, size_t bytes) {
  void* h = malloc(bytes);
  int ok = hipMemcpy(h, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess && fwrite(h, 1, bytes, o) == bytes;
  free(h);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <inputs.bin> <outputs.bin>\n", argv[0]); return 2; }
  f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  int32_t hd[5];
  if (fread(hd, sizeof(int32_t), 5, f) != 5) return 2;
  const int B = hd[0], V = hd[1], F = hd[2], N = hd[3], per_sample = hd[4];
  if (B < 1 || B > 1024 || V < 1 || V > 100000 || F < 1 || F > HOISDF_MESH_MAX_FACES || N < 1 || N > 1000000) { fprintf(stderr, "bad header\n"); return 2; }
  float* verts = (float*)rd((long)B * V * 3);
  int32_t* faces = (int32_t*)rd((per_sample ? (long)B : 1L) * F * 3);
  int32_t* n_faces = (int32_t*)rd(B);
  float* points = (float*)rd((long)B * N * 3);
  int32_t* vert_label = (int32_t*)rd(V);
  fclose(f);

  float *tris, *area, *cdf, *box, *sdf;
  int32_t *face, *label;
  CHECK(hipMalloc((void**)&tris, sizeof(float) * 12 * B * F));
  CHECK(hipMalloc((void**)&area, sizeof(float) * B * F));
  CHECK(hipMalloc((void**)&cdf, sizeof(float) * B * F));
  CHECK(hipMalloc((void**)&box, sizeof(float) * 8 * B));
  CHECK(hipMalloc((void**)&sdf, sizeof(float) * B * N));
  CHECK(hipMalloc((void**)&face, sizeof(int32_t) * B * N));
  CHECK(hipMalloc((void**)&label, sizeof(int32_t) * B * N));
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  CALL(hoisdf_mesh_prepare(verts, B, V, faces, per_sample ? 3L * F : 0L, n_faces, F, tris, area, cdf, box, st));
  CALL(hoisdf_mesh_sdf(points, 3, B, N, tris, box, n_faces, F, vert_label, 0, sdf, 1, face, NULL, NULL, label, st));
  CHECK(hipStreamSynchronize(st));

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror("open"); return 2; }
  if (!wr(o, sdf, sizeof(float) * B * N) || !wr(o, face, sizeof(int32_t) * B * N) || !wr(o, label, sizeof(int32_t) * B * N)) {
    fprintf(stderr, "writing the outputs failed\n");
    return 2;
  }
  fclose(o);
  printf("c host mesh sdf ok: %d meshes, %d faces, %d points each\n", B, F, N);
  return 0;
}
