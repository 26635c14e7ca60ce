// The rules of the rigid fit of a point set to a sampled signed-distance field (hoisdf_amd/field_fit_oracle.py states them; include/
// hoisdf.h "field fit" repeats them) as plain functions: the per-point term (pose -> trilinear read -> the 28 terms of the normal
// equations) and the serial part one lane does per step (start, decide, plan: the stop tests, the damped 6 x 6 Cholesky solve,
// Rodrigues, the 3 x 3 product).  fp64 on the f32 inputs, every product and sum rounded on its own, in the oracle's order.
// Compiled twice: by field_fit.hip for the device (FF_FN = __device__ __forceinline__) and, with FF_FN left to its default, by a
// plain C++ host program (tests/c/field_fit_rules_host.cpp, built with -ffp-contract=off) that holds this text to the oracle without
// a GPU.  The library itself has no CPU path.  Nothing here synchronises or knows about lanes: the summation order is the caller's.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef FF_FN
#define FF_FN static inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#define FF_UNROLL _Pragma("unroll")
#else
#define FF_UNROLL
#endif

enum { FF_TERMS = 28 };                   // H's upper triangle row-major (21), b (6), rho (1)
enum { FF_ACTIVE = 0, FF_BY_ITERS = 1, FF_BY_STEP = 2, FF_BY_LAMBDA = 3, FF_EMPTY = 4 };   // the status word: 0 = a trial pose waits

struct FFParams {
  int n, iters, min_used_percent;
  double huber, lambda0, step_tol;        // the caller's floats, widened
};

// per-sample state between the launches (the device workspace holds one per sample)
struct FFState {
  double c[3], extent, R[9], t[3], lam;
  double sums[FF_TERMS];                  // of the current pose, divided by its n_used: H (21), b (6), cost
  double R1[9], t1[3];                    // the trial pose
  double cost0;
  int32_t n0, n_used, tried, accepted, status, pad;
};

// python's max(a, b) of two floats: b only when b > a
FF_FN double ff_max(double a, double b) { return b > a ? b : a; }
// numpy's max: a NaN wins
FF_FN double ff_npmax(double a, double b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }
FF_FN bool ff_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// x = R (p - c) + c + t: rq = the rotated offset, x the posed point
FF_FN void ff_pose(const double* R, const double* t, const double* c, const double* p, double* rq, double* x) {
  const double q0 = p[0] - c[0], q1 = p[1] - c[1], q2 = p[2] - c[2];
  FF_UNROLL
  for (int k = 0; k < 3; ++k) {
    rq[k] = (R[3 * k] * q0 + R[3 * k + 1] * q1) + R[3 * k + 2] * q2;
    x[k] = (rq[k] + c[k]) + t[k];
  }
}

// the trilinear read at x and its gradient; false: the point takes no part (outside, NaN, or a corner that is not finite).
// val: the sample's n^3 values, unit stride; grid: lo xyz, cell xyz
FF_FN bool ff_field_read(const float* val, const float* grid, int n, const double* x, double* f, double* g) {
  double u[3], fr[3], cell[3];
  int idx[3];
  bool ok = true;
  FF_UNROLL
  for (int k = 0; k < 3; ++k) {
    cell[k] = (double)grid[3 + k];
    u[k] = (x[k] - (double)grid[k]) / cell[k];
    ok = ok && u[k] >= 0.0 && u[k] <= (double)(n - 1);
  }
  if (!ok) return false;
  FF_UNROLL
  for (int k = 0; k < 3; ++k) {
    const double fl = floor(u[k]);
    idx[k] = fl < (double)(n - 2) ? (int)fl : n - 2;
    fr[k] = u[k] - (double)idx[k];
  }
  const long base = idx[0] + (long)n * (idx[1] + (long)n * idx[2]);
  double v[8];                            // by dx | dy << 1 | dz << 2
  FF_UNROLL
  for (int cn = 0; cn < 8; ++cn) {
    v[cn] = (double)val[base + (cn & 1) + (long)n * ((cn >> 1 & 1) + (long)n * (cn >> 2))];
    ok = ok && ff_finite(v[cn]);
  }
  if (!ok) return false;
  const double fx = fr[0], fy = fr[1], fz = fr[2];
  const double d00 = v[1] - v[0], d10 = v[3] - v[2], d01 = v[5] - v[4], d11 = v[7] - v[6];
  const double c00 = v[0] + fx * d00, c10 = v[2] + fx * d10, c01 = v[4] + fx * d01, c11 = v[6] + fx * d11;
  const double c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
  *f = c0 + fz * (c1 - c0);
  const double e0 = d00 + fy * (d10 - d00), e1 = d01 + fy * (d11 - d01);
  g[0] = (e0 + fz * (e1 - e0)) / cell[0];
  const double h0 = c10 - c00, h1 = c11 - c01;
  g[1] = (h0 + fz * (h1 - h0)) / cell[1];
  g[2] = (c1 - c0) / cell[2];
  return true;
}

// one point under the pose (R, t) about c: its 28 terms; false (terms untouched): it takes no part
FF_FN bool ff_point_terms(const float* val, const float* grid, int n, const double* R, const double* t, const double* c,
                          const double* p, double huber, double* term) {
  double rq[3], x[3], f, g[3], J[6];
  ff_pose(R, t, c, p, rq, x);
  if (!ff_field_read(val, grid, n, x, &f, g)) return false;
  const double a = fabs(f);
  const bool small = a <= huber;
  const double w = small ? 1.0 : huber / a;
  const double rho = small ? 0.5 * f * f : huber * (a - 0.5 * huber);
  J[0] = g[0]; J[1] = g[1]; J[2] = g[2];
  J[3] = rq[1] * g[2] - rq[2] * g[1];
  J[4] = rq[2] * g[0] - rq[0] * g[2];
  J[5] = rq[0] * g[1] - rq[1] * g[0];
  const double wf = w * f;
  int k = 0;
  FF_UNROLL
  for (int i = 0; i < 6; ++i) {
    const double wJ = w * J[i];
    FF_UNROLL
    for (int j = i; j < 6; ++j) term[k++] = wJ * J[j];
  }
  FF_UNROLL
  for (int i = 0; i < 6; ++i) term[21 + i] = wf * J[i];
  term[27] = rho;
  return true;
}

// (H + lam diag(H) + 1e-12 I) d = -b by Cholesky, ascending; false: a pivot was not positive
FF_FN bool ff_solve(const double* H21, const double* b, double lam, double* d) {
  double A[6][6], L[6][6], y[6];
  int k = 0;
  FF_UNROLL
  for (int i = 0; i < 6; ++i) {
    FF_UNROLL
    for (int j = i; j < 6; ++j) { A[i][j] = H21[k]; A[j][i] = H21[k]; ++k; }
  }
  FF_UNROLL
  for (int i = 0; i < 6; ++i) A[i][i] = (A[i][i] + lam * A[i][i]) + 1e-12;
  FF_UNROLL
  for (int j = 0; j < 6; ++j) {
    double s = A[j][j];
    FF_UNROLL
    for (int m = 0; m < j; ++m) s = s - L[j][m] * L[j][m];
    if (!(s > 0.0)) return false;
    L[j][j] = sqrt(s);
    FF_UNROLL
    for (int i = j + 1; i < 6; ++i) {
      s = A[i][j];
      FF_UNROLL
      for (int m = 0; m < j; ++m) s = s - L[i][m] * L[j][m];
      L[i][j] = s / L[j][j];
    }
  }
  FF_UNROLL
  for (int i = 0; i < 6; ++i) {
    double s = -b[i];
    FF_UNROLL
    for (int m = 0; m < i; ++m) s = s - L[i][m] * y[m];
    y[i] = s / L[i][i];
  }
  FF_UNROLL
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    FF_UNROLL
    for (int m = i + 1; m < 6; ++m) s = s - L[m][i] * d[m];
    d[i] = s / L[i][i];
  }
  return true;
}

// exp of the rotation vector w: I + a K + b K^2
FF_FN void ff_rodrigues(const double* w, double* E) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  const double th = sqrt(th2);
  double a = 1.0, b = 0.5;
  if (th > 0.0) {
    const double h = 0.5 * th;
    const double sh = sin(h) / h;
    a = sin(th) / th;
    b = 0.5 * sh * sh;
  }
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  FF_UNROLL
  for (int i = 0; i < 3; ++i) {
    FF_UNROLL
    for (int j = 0; j < 3; ++j)
      E[3 * i + j] = ((i == j ? 1.0 : 0.0) + a * K[3 * i + j]) + b * (w[i] * w[j] - (i == j ? th2 : 0.0));
  }
}

FF_FN void ff_matmul3(const double* E, const double* R, double* out) {
  FF_UNROLL
  for (int i = 0; i < 3; ++i) {
    FF_UNROLL
    for (int j = 0; j < 3; ++j) out[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
  }
}

// the next step of a sample that has not stopped: the stop test first, lambda grown over factorisations that fail (each a tried,
// rejected step), then either a stop (status) or the trial pose R1, t1 (status stays FF_ACTIVE)
FF_FN void ff_plan(FFState* s, const FFParams* p) {
  for (;;) {
    if (s->tried >= p->iters) { s->status = FF_BY_ITERS; return; }
    double d[6];
    if (!ff_solve(s->sums, s->sums + 21, s->lam, d)) {
      s->tried += 1;
      s->lam = 10.0 * s->lam;
      if (s->lam > 1e9) { s->status = FF_BY_LAMBDA; return; }
      continue;
    }
    const double dmax = ff_npmax(ff_npmax(fabs(d[0]), fabs(d[1])), fabs(d[2]));
    const double wmax = ff_npmax(ff_npmax(fabs(d[3]), fabs(d[4])), fabs(d[5]));
    const double size = ff_max(dmax, wmax * s->extent);
    if (size < p->step_tol) { s->status = FF_BY_STEP; return; }
    s->tried += 1;
    double E[9];
    ff_rodrigues(d + 3, E);
    ff_matmul3(E, s->R, s->R1);
    FF_UNROLL
    for (int k = 0; k < 3; ++k) s->t1[k] = s->t[k] + d[k];
    return;
  }
}

// after the sums of the START pose (raw, not yet divided): the state of the sample and its first plan.  c and extent are set.
FF_FN void ff_start(FFState* s, const FFParams* p, double* sums, int n_used) {
  const double div = (double)(n_used > 1 ? n_used : 1);
  FF_UNROLL
  for (int k = 0; k < 9; ++k) s->R[k] = s->R1[k] = (k % 4 == 0) ? 1.0 : 0.0;
  FF_UNROLL
  for (int k = 0; k < 3; ++k) s->t[k] = s->t1[k] = 0.0;
  FF_UNROLL
  for (int k = 0; k < FF_TERMS; ++k) { sums[k] = sums[k] / div; s->sums[k] = n_used ? sums[k] : 0.0; }
  s->lam = p->lambda0;
  s->n0 = s->n_used = n_used;
  s->tried = s->accepted = 0;
  s->pad = 0;
  s->cost0 = s->sums[27];
  s->status = FF_ACTIVE;
  if (n_used == 0) { s->status = FF_EMPTY; return; }
  ff_plan(s, p);
}

// after the sums of the trial pose (raw): accept or reject, lambda, the counters, the next plan -> whether it was accepted
FF_FN bool ff_decide(FFState* s, const FFParams* p, double* sums, int n_used) {
  const double div = (double)(n_used > 1 ? n_used : 1);
  FF_UNROLL
  for (int k = 0; k < FF_TERMS; ++k) sums[k] = sums[k] / div;
  const bool ok = (long)n_used * 100 >= (long)p->min_used_percent * (long)s->n0 && n_used > 0 && sums[27] < s->sums[27];
  if (ok) {
    FF_UNROLL
    for (int k = 0; k < 9; ++k) s->R[k] = s->R1[k];
    FF_UNROLL
    for (int k = 0; k < 3; ++k) s->t[k] = s->t1[k];
    FF_UNROLL
    for (int k = 0; k < FF_TERMS; ++k) s->sums[k] = sums[k];
    s->n_used = n_used;
    s->accepted += 1;
    s->lam = ff_max(s->lam / 10.0, 1e-9);
  } else {
    s->lam = 10.0 * s->lam;
    if (s->lam > 1e9) { s->status = FF_BY_LAMBDA; return ok; }
  }
  ff_plan(s, p);
  return ok;
}
