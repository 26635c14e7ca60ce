/* A C host with no Python and no torch turns a sampled field into a triangle mesh through include/hoisdf.h:
 *   hoisdf_iso_extract_workspace_bytes -> hoisdf_iso_extract (count only) -> one read of the counts -> hoisdf_iso_extract
 * The field is a sphere of radius 0.3 sampled on the host on n nodes per axis over [-0.5, 0.5]^3.  The host then checks what it got
 * itself: every directed edge occurs once and its reverse once (closed, consistently oriented), and the signed volume by the
 * divergence theorem is positive (outward winding) and near 4/3 pi r^3.  tests/test_gpu_isosurf.py::test_c_host_iso_surface compares
 * the file it writes bit for bit with the numpy oracle on the same field.
 * usage: test_iso_surface_host <n> <outputs.bin>
 * Output file (little-endian): int32 n, n_verts, n_faces; the field float32 [n^3]; verts float32 [n_verts][3]; faces int32 [n_faces][3]. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hoisdf.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "hip error line %d\n", __LINE__); return 2; } } while (0)
#define CALL(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "line %d: status %d: %s\n", __LINE__, rc_, hoisdf_last_error()); return 1; } } while (0)

static int cmp_i64(const void* a, const void* b) {
  const int64_t x = *(const int64_t*)a, y = *(const int64_t*)b;
  return x < y ? -1 : x > y;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s <n> <outputs.bin>\n", argv[0]); return 2; }
  const int n = atoi(argv[1]);
  if (n < 2 || n > HOISDF_ISO_MAX_GRID) { fprintf(stderr, "n = 2 .. %d\n", HOISDF_ISO_MAX_GRID); return 2; }
  const long N = (long)n * n * n;
  const double r = 0.3;
  const float lo = -0.5f, cell = 1.0f / (float)(n - 1);
  const float grid[8] = {lo, lo, lo, cell, cell, cell, 0.f, 0.f};
  float* field = (float*)malloc(sizeof(float) * N);
  for (int iz = 0; iz < n; ++iz)
    for (int iy = 0; iy < n; ++iy)
      for (int ix = 0; ix < n; ++ix) {
        const double x = lo + (double)ix * cell, y = lo + (double)iy * cell, z = lo + (double)iz * cell;
        field[ix + (long)n * (iy + (long)n * iz)] = (float)(sqrt(x * x + y * y + z * z) - r);
      }

  float *d_field, *d_grid, *d_verts = NULL;
  int32_t *d_counts, *d_faces = NULL;
  void* ws;
  const long nws = hoisdf_iso_extract_workspace_bytes(1, n);
  if (nws < 0) { fprintf(stderr, "workspace: %s\n", hoisdf_last_error()); return 1; }
  CHECK(hipMalloc((void**)&d_field, sizeof(float) * N));
  CHECK(hipMalloc((void**)&d_grid, sizeof(grid)));
  CHECK(hipMalloc((void**)&d_counts, 2 * sizeof(int32_t)));
  CHECK(hipMalloc(&ws, (size_t)nws));
  CHECK(hipMemcpy(d_field, field, sizeof(float) * N, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_grid, grid, sizeof(grid), hipMemcpyHostToDevice));
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  /* 1. count only: both outputs NULL */
  CALL(hoisdf_iso_extract(d_field, 1, d_grid, n, 1, 0.f, 1.f, NULL, NULL, 0, NULL, 0, d_counts, d_counts + 1, ws, nws, st));
  int32_t counts[2];
  CHECK(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
  CHECK(hipStreamSynchronize(st));
  const int nv = counts[0], nf = counts[1];
  if (nv <= 0 || nf <= 0) { fprintf(stderr, "empty surface: %d vertices, %d faces\n", nv, nf); return 1; }
  /* 2. exact allocation, extraction */
  CHECK(hipMalloc((void**)&d_verts, sizeof(float) * 3 * nv));
  CHECK(hipMalloc((void**)&d_faces, sizeof(int32_t) * 3 * nf));
  CALL(hoisdf_iso_extract(d_field, 1, d_grid, n, 1, 0.f, 1.f, NULL, d_verts, nv, d_faces, nf, d_counts, d_counts + 1, ws, nws, st));
  float* v = (float*)malloc(sizeof(float) * 3 * nv);
  int32_t* fc = (int32_t*)malloc(sizeof(int32_t) * 3 * nf);
  CHECK(hipMemcpyAsync(v, d_verts, sizeof(float) * 3 * nv, hipMemcpyDeviceToHost, st));
  CHECK(hipMemcpyAsync(fc, d_faces, sizeof(int32_t) * 3 * nf, hipMemcpyDeviceToHost, st));
  CHECK(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, st));
  CHECK(hipStreamSynchronize(st));
  if (counts[0] != nv || counts[1] != nf) { fprintf(stderr, "the two calls disagree on the counts\n"); return 1; }

  /* closed and consistently oriented: the sorted list of directed edges has no duplicate and contains every edge's reverse */
  int64_t* e = (int64_t*)malloc(sizeof(int64_t) * 3 * nf);
  double vol = 0.0;
  for (int t = 0; t < nf; ++t) {
    const int32_t* q = fc + 3 * t;
    for (int k = 0; k < 3; ++k) {
      if (q[k] < 0 || q[k] >= nv) { fprintf(stderr, "face %d names vertex %d of %d\n", t, q[k], nv); return 1; }
      e[3 * t + k] = (int64_t)q[k] * nv + q[(k + 1) % 3];
    }
    const float *a = v + 3 * q[0], *b = v + 3 * q[1], *c = v + 3 * q[2];
    vol += ((double)a[0] * ((double)b[1] * c[2] - (double)b[2] * c[1]) + (double)a[1] * ((double)b[2] * c[0] - (double)b[0] * c[2]) +
            (double)a[2] * ((double)b[0] * c[1] - (double)b[1] * c[0])) / 6.0;
  }
  qsort(e, 3 * (size_t)nf, sizeof(int64_t), cmp_i64);
  for (long i = 0; i < 3L * nf; ++i) {
    if (i && e[i] == e[i - 1]) { fprintf(stderr, "a directed edge occurs twice: not consistently oriented\n"); return 1; }
    const int64_t rev = (e[i] % nv) * nv + e[i] / nv;
    if (!bsearch(&rev, e, 3 * (size_t)nf, sizeof(int64_t), cmp_i64)) { fprintf(stderr, "an edge without its reverse: not closed\n"); return 1; }
  }
  const double exact = 4.0 / 3.0 * 3.14159265358979323846 * r * r * r;
  printf("n %d: %d vertices, %d faces, euler %d, volume %.6f (sphere %.6f)\n", n, nv, nf, nv - 3 * nf / 2 + nf, vol, exact);
  if (nv - 3 * nf / 2 + nf != 2) { fprintf(stderr, "euler characteristic is not 2\n"); return 1; }
  /* the surface is inscribed (too small) and converges at second order: the numpy oracle in float64 is 4 pi r h^2 / 6 short
   * (h = the cell; 9.96e-3, 2.43e-3, 6.12e-4 at n = 9, 17, 33); the bar is twice that */
  if (!(vol > 0.0 && vol < exact && exact - vol < 4.0 * 3.14159265358979323846 * r * (double)cell * cell / 3.0)) {
    fprintf(stderr, "volume %.6f against %.6f\n", vol, exact);
    return 1;
  }

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror("open"); return 2; }
  const int32_t hd[3] = {n, nv, nf};
  if (fwrite(hd, sizeof(int32_t), 3, o) != 3 || fwrite(field, sizeof(float), N, o) != (size_t)N ||
      fwrite(v, sizeof(float), 3 * (size_t)nv, o) != 3 * (size_t)nv || fwrite(fc, sizeof(int32_t), 3 * (size_t)nf, o) != 3 * (size_t)nf) {
    fprintf(stderr, "writing the outputs failed\n");
    return 2;
  }
  fclose(o);
  printf("c host iso surface ok\n");
  return 0;
}
