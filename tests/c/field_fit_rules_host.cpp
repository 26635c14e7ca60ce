// The whole field fit on the host, through the text the kernels compile: hoisdf_amd/csrc/field_fit_rules.h with its qualifiers
// defined away, and the 256-lane summation order of csrc/field_fit.hip as plain loops.  No GPU, no library: this program exists
// so that tests/test_field_fit_rules_host.py can hold the rules header to hoisdf_amd/field_fit_oracle.py on a CPU (and so that the
// header can run under a host sanitizer).  Build: g++ -O2 -ffp-contract=off -I hoisdf_amd/csrc.
//   usage: field_fit_rules_host CASE.bin   ->  the result on stdout, doubles as C99 hex floats
//   CASE.bin: int32 n, V, n_points (< 0: none), has_pivot, iters, min_used_percent; float32 huber, lambda0, step_tol; float32 grid[8],
//   pivot[3], values[n^3], points[V][3]
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "field_fit_rules.h"

enum { LANES = 256, WAVE = 64 };

// lanes[l][k] -> out[k]: xor tree within each wave of 64, then ((w0 + w1) + w2) + w3
static void lane_tree(std::vector<double>& lanes, int K, double* out) {
  double wave[LANES / WAVE];
  for (int k = 0; k < K; ++k) {
    for (int w = 0; w < LANES / WAVE; ++w) {
      double v[WAVE], y[WAVE];
      for (int l = 0; l < WAVE; ++l) v[l] = lanes[(size_t)(w * WAVE + l) * K + k];
      for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < WAVE; ++l) y[l] = v[l] + v[l ^ o];
        for (int l = 0; l < WAVE; ++l) v[l] = y[l];
      }
      wave[w] = v[0];
    }
    out[k] = ((wave[0] + wave[1]) + wave[2]) + wave[3];
  }
}

// the sums of pose (R, t): lane l takes points l, l + 256, ... ascending
static int pose_sums(const float* val, const float* grid, int n, const float* pts, int nv, const double* R, const double* t,
                     const double* c, double huber, double* sums, double* sums_abs) {
  std::vector<double> acc((size_t)LANES * FF_TERMS, 0.0), acc_abs((size_t)LANES * FF_TERMS, 0.0);
  int used = 0;
  for (int l = 0; l < LANES; ++l)
    for (int i = l; i < nv; i += LANES) {
      const double p[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
      double term[FF_TERMS];
      if (!ff_point_terms(val, grid, n, R, t, c, p, huber, term)) continue;
      ++used;
      for (int k = 0; k < FF_TERMS; ++k) {
        acc[(size_t)l * FF_TERMS + k] = acc[(size_t)l * FF_TERMS + k] + term[k];
        acc_abs[(size_t)l * FF_TERMS + k] = acc_abs[(size_t)l * FF_TERMS + k] + fabs(term[k]);
      }
    }
  lane_tree(acc, FF_TERMS, sums);
  if (sums_abs) lane_tree(acc_abs, FF_TERMS, sums_abs);
  return used;
}

static void print_doubles(const char* name, const double* v, size_t n) {
  printf("%s", name);
  for (size_t k = 0; k < n; ++k) printf(" %a", v[k]);
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s CASE.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  int32_t head[6];
  float par[3], grid[8], pivot[3];
  if (fread(head, 4, 6, f) != 6 || fread(par, 4, 3, f) != 3 || fread(grid, 4, 8, f) != 8 || fread(pivot, 4, 3, f) != 3) return 2;
  const int n = head[0], V = head[1];
  if (n < 2 || n > 128 || V < 0 || V > (1 << 24)) return 2;
  std::vector<float> val((size_t)n * n * n), pts((size_t)V * 3 + 1);
  if (fread(val.data(), 4, val.size(), f) != val.size() || fread(pts.data(), 4, (size_t)V * 3, f) != (size_t)V * 3) return 2;
  fclose(f);
  const int nv = head[2] < 0 ? V : (head[2] > V ? V : head[2]);
  FFParams p;
  p.n = n; p.iters = head[4]; p.min_used_percent = head[5];
  p.huber = (double)par[0]; p.lambda0 = (double)par[1]; p.step_tol = (double)par[2];

  FFState s;
  // init: the pivot (the given one, or the mean in lane order), the extent, the sums of the start pose, the first plan
  std::vector<double> m((size_t)LANES * 3, 0.0);
  for (int l = 0; l < LANES; ++l)
    for (int i = l; i < nv; i += LANES)
      for (int k = 0; k < 3; ++k) m[(size_t)l * 3 + k] = m[(size_t)l * 3 + k] + (double)pts[3 * i + k];
  double mean[3];
  lane_tree(m, 3, mean);
  for (int k = 0; k < 3; ++k) s.c[k] = head[3] ? (double)pivot[k] : mean[k] / (double)(nv > 1 ? nv : 1);
  s.extent = 0.0;
  for (int i = 0; i < nv; ++i)
    for (int k = 0; k < 3; ++k) {
      const double q = fabs((double)pts[3 * i + k] - s.c[k]);
      s.extent = q > s.extent ? q : s.extent;
    }
  const double I[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, zero[3] = {0.0, 0.0, 0.0};
  double sums[FF_TERMS], sums_abs[FF_TERMS], normal[2 * FF_TERMS];
  const int n0 = pose_sums(val.data(), grid, n, pts.data(), nv, I, zero, s.c, p.huber, sums, sums_abs);
  ff_start(&s, &p, sums, n0);
  for (int k = 0; k < FF_TERMS; ++k) {
    normal[k] = n0 ? sums[k] : 0.0;
    normal[FF_TERMS + k] = n0 ? sums_abs[k] / (double)(n0 > 1 ? n0 : 1) : 0.0;
  }
  // rounds: what hoisdf_field_fit enqueues as `iters` launches; a stopped sample does nothing
  std::vector<char> decisions;
  for (int r = 0; r < p.iters; ++r) {
    if (s.status != FF_ACTIVE) continue;
    const int used = pose_sums(val.data(), grid, n, pts.data(), nv, s.R1, s.t1, s.c, p.huber, sums, nullptr);
    decisions.push_back(ff_decide(&s, &p, sums, used) ? '1' : '0');
  }
  decisions.push_back('\0');
  // finish
  const bool empty = s.status == FF_EMPTY;
  const double cost[2] = {empty ? 0.0 : s.cost0, empty ? 0.0 : s.sums[27]};
  print_doubles("normal", normal, 2 * FF_TERMS);
  printf("info %d %d %d %d\n", s.n0, s.n_used, s.tried, s.accepted);
  printf("status %d\n", s.status);
  printf("decisions [%s]\n", decisions.data());
  print_doubles("rot", s.R, 9);
  print_doubles("trans", s.t, 3);
  print_doubles("cost", cost, 2);
  std::vector<double> out((size_t)nv * 3);
  for (int i = 0; i < nv; ++i) {
    const double q[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
    double rq[3];
    ff_pose(s.R, s.t, s.c, q, rq, &out[(size_t)i * 3]);
  }
  print_doubles("points", out.data(), out.size());
  return 0;
}
