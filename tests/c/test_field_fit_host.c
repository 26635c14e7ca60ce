/* A C host with no Python and no torch moves a point set onto the zero level set of a sampled field through include/hoisdf.h:
 *   hoisdf_field_fit_workspace_bytes -> hoisdf_field_fit (hoisdf_field_fit_launch_count(iters) launches, one synchronisation here)
 * The field is tanh of the distance to a sphere of radius 0.3, sampled on the host on n nodes per axis over [-0.5, 0.5]^3.  The
 * points are V points of that sphere (a Fibonacci lattice) moved by a known translation; the rotation of a sphere is unobservable,
 * so the host checks the translation alone: it comes back to a quarter of a cell (the interpolant's zero level set is the sphere up
 * to second order in the cell, and the error is symmetric about the centre), the posed points lie on the sphere to the same bar, the
 * rotation is orthonormal, the cost fell, and info is sane: every point took part at both ends, 1 <= accepted <= tried <= iters.
 * usage: test_field_fit_host <n> */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hoisdf.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "hip error line %d\n", __LINE__); return 2; } } while (0)
#define CALL(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "line %d: status %d: %s\n", __LINE__, rc_, hoisdf_last_error()); return 1; } } while (0)

enum { V = 400, ITERS = 32 };

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <n>\n", argv[0]); return 2; }
  const int n = atoi(argv[1]);
  if (n < 2 || n > HOISDF_ISO_MAX_GRID) { fprintf(stderr, "n = 2 .. %d\n", HOISDF_ISO_MAX_GRID); return 2; }
  const long N = (long)n * n * n;
  const double r = 0.3, shift[3] = {0.04, -0.03, 0.02};
  const float lo = -0.5f, cell = 1.0f / (float)(n - 1);
  const float grid[8] = {lo, lo, lo, cell, cell, cell, 0.f, 0.f};
  float* field = (float*)malloc(sizeof(float) * N);
  for (int iz = 0; iz < n; ++iz)
    for (int iy = 0; iy < n; ++iy)
      for (int ix = 0; ix < n; ++ix) {
        const double x = lo + (double)ix * cell, y = lo + (double)iy * cell, z = lo + (double)iz * cell;
        field[ix + (long)n * (iy + (long)n * iz)] = (float)tanh(sqrt(x * x + y * y + z * z) - r);
      }
  float pts[V][3];
  for (int i = 0; i < V; ++i) {                                 /* Fibonacci lattice on the sphere, then the known translation */
    const double z = 1.0 - (2.0 * i + 1.0) / V, rho = sqrt(1.0 - z * z), phi = i * 2.39996322972865332;
    pts[i][0] = (float)(r * rho * cos(phi) + shift[0]);
    pts[i][1] = (float)(r * rho * sin(phi) + shift[1]);
    pts[i][2] = (float)(r * z + shift[2]);
  }

  if (hoisdf_field_fit_launch_count(ITERS) != ITERS + 2) { fprintf(stderr, "launch count: %s\n", hoisdf_last_error()); return 1; }
  const long nws = hoisdf_field_fit_workspace_bytes(1);
  if (nws < 0) { fprintf(stderr, "workspace: %s\n", hoisdf_last_error()); return 1; }
  float *d_field, *d_grid, *d_pts, *d_rot, *d_trans, *d_out;
  double* d_cost;
  int32_t* d_info;
  void* ws;
  CHECK(hipMalloc((void**)&d_field, sizeof(float) * N));
  CHECK(hipMalloc((void**)&d_grid, sizeof(grid)));
  CHECK(hipMalloc((void**)&d_pts, sizeof(pts)));
  CHECK(hipMalloc((void**)&d_out, sizeof(pts)));
  CHECK(hipMalloc((void**)&d_rot, 9 * sizeof(float)));
  CHECK(hipMalloc((void**)&d_trans, 3 * sizeof(float)));
  CHECK(hipMalloc((void**)&d_cost, 2 * sizeof(double)));
  CHECK(hipMalloc((void**)&d_info, 4 * sizeof(int32_t)));
  CHECK(hipMalloc(&ws, (size_t)nws));
  CHECK(hipMemcpy(d_field, field, sizeof(float) * N, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_grid, grid, sizeof(grid), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_pts, pts, sizeof(pts), hipMemcpyHostToDevice));
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  CALL(hoisdf_field_fit(d_field, N, d_grid, n, d_pts, V, NULL, NULL, 1, ITERS, 0.1f, 1e-3f, 1e-7f, 50, d_rot, d_trans, d_out, d_cost,
                        d_info, NULL, NULL, ws, nws, st));
  float rot[9], trans[3], out[V][3];
  double cost[2];
  int32_t info[4];
  CHECK(hipMemcpyAsync(rot, d_rot, sizeof(rot), hipMemcpyDeviceToHost, st));
  CHECK(hipMemcpyAsync(trans, d_trans, sizeof(trans), hipMemcpyDeviceToHost, st));
  CHECK(hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, st));
  CHECK(hipMemcpyAsync(cost, d_cost, sizeof(cost), hipMemcpyDeviceToHost, st));
  CHECK(hipMemcpyAsync(info, d_info, sizeof(info), hipMemcpyDeviceToHost, st));
  CHECK(hipStreamSynchronize(st));

  const double bar = 0.25 * (double)cell;
  double terr = 0.0, serr = 0.0, oerr = 0.0;
  for (int k = 0; k < 3; ++k) terr = fmax(terr, fabs((double)trans[k] + shift[k]));
  for (int i = 0; i < V; ++i)
    serr = fmax(serr, fabs(sqrt((double)out[i][0] * out[i][0] + (double)out[i][1] * out[i][1] + (double)out[i][2] * out[i][2]) - r));
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double d = i == j ? -1.0 : 0.0;
      for (int k = 0; k < 3; ++k) d += (double)rot[3 * i + k] * rot[3 * j + k];
      oerr = fmax(oerr, fabs(d));
    }
  printf("n %d (cell %.4f): translation error %.2e, points off the sphere %.2e (bar %.2e), |R R^T - I| %.1e, cost %.3e -> %.3e, "
         "info %d %d %d %d\n", n, (double)cell, terr, serr, bar, oerr, cost[0], cost[1], info[0], info[1], info[2], info[3]);
  if (!(terr < bar)) { fprintf(stderr, "the translation did not come back\n"); return 1; }
  if (!(serr < bar)) { fprintf(stderr, "the posed points are off the sphere\n"); return 1; }
  if (!(oerr < 1e-5)) { fprintf(stderr, "the rotation is not orthonormal\n"); return 1; }
  if (!(cost[1] < cost[0] && cost[1] >= 0.0)) { fprintf(stderr, "the cost did not fall\n"); return 1; }
  if (info[0] != V || info[1] != V || info[3] < 1 || info[3] > info[2] || info[2] > ITERS) { fprintf(stderr, "info is not sane\n"); return 1; }
  printf("c host field fit ok\n");
  return 0;
}
