/* A C host with no Python and no torch turns dumped predictions into the numbers of results.txt through include/hoisdf.h:
 *   per batch hoisdf_eval_object, hoisdf_eval_hand_joints, hoisdf_eval_mesh, hoisdf_eval_accum_feed (raw and aligned); at the end
 *   hoisdf_eval_accum_finish twice and the file in the reference's layout (main/test.py:229-261, the dexycb form).
 * tests/test_gpu_eval_native.py::test_c_host_eval compares the raw outputs bit for bit with the Python calls on the same dump.
 * Input file (little-endian): int32 n_batches, B, P, T, V, J, NV, steps; float64 F-score thresholds [2], accumulator thresholds [steps];
 * float32 templates [T][V][3]; then per batch int32 obj_ids [B] and float32 obj_rot [B][P][3], obj_trans [B][P][3], obj_rot_gt [B][3],
 * obj_trans_gt [B][3], joints pred [B][J][3], joints gt, mesh pred [B][NV][3], mesh gt.
 * Output file: per batch float32 adds, mce, oce, mme, mje, pamje [B] each, dist_raw, dist_aligned [B][NV], fscore, fscore_aligned [B][2],
 * int32 used [B]; then float64 [2 + steps] (mean EPE, AUC, PCK curve) of the raw and of the aligned accumulator. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hoisdf.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "hip error line %d\n", __LINE__); return 2; } } while (0)
#define CALL(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "line %d: status %d: %s\n", __LINE__, rc_, hoisdf_last_error()); return 1; } } while (0)
#define NTH 2

static FILE* f;
/* the next `bytes` of the file, uploaded */
static void* rd(size_t bytes) {
  void* h = malloc(bytes);
  if (fread(h, 1, bytes, f) != bytes) { fprintf(stderr, "short read\n"); exit(2); }
  void* d = NULL;
  if (hipMalloc(&d, bytes) != hipSuccess || hipMemcpy(d, h, bytes, hipMemcpyHostToDevice) != hipSuccess) exit(2);
  free(h);
  return d;
}
static void* dalloc(size_t bytes) {
  void* d = NULL;
  if (hipMalloc(&d, bytes) != hipSuccess) { fprintf(stderr, "hipMalloc of %zu bytes failed\n", bytes); exit(2); }
  return d;
}
/* device -> the output file, and into `keep` (may be NULL) */
static int wr(FILE* o, const void* dev, size_t bytes, void* keep) {
  void* h = keep ? keep : malloc(bytes);
  int ok = hipMemcpy(h, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess && fwrite(h, 1, bytes, o) == bytes;
  if (!keep) free(h);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s <inputs.bin> <outputs.bin> <results.txt>\n", argv[0]); return 2; }
  f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  int32_t hd[8];
  if (fread(hd, sizeof(int32_t), 8, f) != 8) return 2;
  const int n_batches = hd[0], B = hd[1], P = hd[2], T = hd[3], V = hd[4], J = hd[5], NV = hd[6], steps = hd[7];
  if (n_batches < 1 || n_batches > 64 || B < 1 || B > 4096 || P < 1 || T < 1 || V < 1 || J < 1 || NV < 1 || steps < 2 || steps > 4096) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  double f_th[NTH];
  double* acc_th = (double*)malloc(sizeof(double) * steps);
  if (fread(f_th, sizeof(double), NTH, f) != NTH || fread(acc_th, sizeof(double), steps, f) != (size_t)steps) return 2;
  double *d_fth, *d_ath, *d_out;
  CHECK(hipMalloc((void**)&d_fth, sizeof(f_th)));
  CHECK(hipMalloc((void**)&d_ath, sizeof(double) * steps));
  CHECK(hipMalloc((void**)&d_out, sizeof(double) * (2 + steps)));
  CHECK(hipMemcpy(d_fth, f_th, sizeof(f_th), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_ath, acc_th, sizeof(double) * steps, hipMemcpyHostToDevice));
  float* templates = (float*)rd(sizeof(float) * T * V * 3);

  const int Vmax = V > NV ? V : NV;
  const long ws_bytes = hoisdf_eval_workspace_bytes(B, Vmax), st_bytes = hoisdf_eval_accum_state_bytes(NV, steps);
  if (ws_bytes < 0 || st_bytes < 0) { fprintf(stderr, "size query: %s\n", hoisdf_last_error()); return 1; }
  void* ws = dalloc(ws_bytes);
  void* st_raw = dalloc(st_bytes);
  void* st_al = dalloc(st_bytes);
  float* s6 = (float*)dalloc(sizeof(float) * 6 * B);              /* adds, mce, oce, mme, mje, pamje */
  float* dist = (float*)dalloc(sizeof(float) * 2 * B * NV);       /* raw, aligned */
  float* fs = (float*)dalloc(sizeof(float) * 2 * B * NTH);        /* raw, aligned */
  int32_t* used = (int32_t*)dalloc(sizeof(int32_t) * B);
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  CALL(hoisdf_eval_accum_init(st_raw, NV, steps, st));
  CALL(hoisdf_eval_accum_init(st_al, NV, steps, st));

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror("open"); return 2; }
  float* h6 = (float*)malloc(sizeof(float) * 6 * B);
  float* hfs = (float*)malloc(sizeof(float) * 2 * B * NTH);
  float* f_all = (float*)malloc(sizeof(float) * 2 * NTH * n_batches * B);     /* [raw / aligned][threshold][sample] */
  double sums[6] = {0, 0, 0, 0, 0, 0};
  long total = 0;
  for (int it = 0; it < n_batches; ++it) {
    int32_t* ids = (int32_t*)rd(sizeof(int32_t) * B);
    float* obj_rot = (float*)rd(sizeof(float) * B * P * 3);
    float* obj_trans = (float*)rd(sizeof(float) * B * P * 3);
    float* rot_gt = (float*)rd(sizeof(float) * B * 3);
    float* trans_gt = (float*)rd(sizeof(float) * B * 3);
    float* pr_j = (float*)rd(sizeof(float) * B * J * 3);
    float* gt_j = (float*)rd(sizeof(float) * B * J * 3);
    float* pr_v = (float*)rd(sizeof(float) * B * NV * 3);
    float* gt_v = (float*)rd(sizeof(float) * B * NV * 3);
    CALL(hoisdf_eval_object(obj_rot, obj_trans, P, rot_gt, trans_gt, templates, T, V, ids, B, s6, s6 + B, s6 + 2 * B, s6 + 3 * B, used, ws,
                            ws_bytes, st));
    CALL(hoisdf_eval_hand_joints(pr_j, gt_j, B, J, s6 + 4 * B, s6 + 5 * B, NULL, NULL, NULL, NULL, st));
    CALL(hoisdf_eval_mesh(pr_v, gt_v, B, NV, d_fth, NTH, dist, dist + (long)B * NV, fs, fs + B * NTH, NULL, ws, ws_bytes, st));
    CALL(hoisdf_eval_accum_feed(st_raw, dist, B, NV, d_ath, steps, st));
    CALL(hoisdf_eval_accum_feed(st_al, dist + (long)B * NV, B, NV, d_ath, steps, st));
    CHECK(hipStreamSynchronize(st));
    if (!wr(o, s6, sizeof(float) * 6 * B, h6) || !wr(o, dist, sizeof(float) * 2 * B * NV, NULL) || !wr(o, fs, sizeof(float) * 2 * B * NTH, hfs) ||
        !wr(o, used, sizeof(int32_t) * B, NULL)) { fprintf(stderr, "writing the outputs failed\n"); return 2; }
    for (int k = 0; k < 6; ++k) {                                 /* the running sums of test.py, in cm */
      double s = 0;
      for (int b = 0; b < B; ++b) s += (double)h6[k * B + b];
      sums[k] += s * 100;
    }
    for (int a = 0; a < 2; ++a)
      for (int t = 0; t < NTH; ++t)
        for (int b = 0; b < B; ++b) f_all[((long)(a * NTH + t) * n_batches + it) * B + b] = hfs[(a * B + b) * NTH + t];
    total += B;
    void* batch[9] = {ids, obj_rot, obj_trans, rot_gt, trans_gt, pr_j, gt_j, pr_v, gt_v};
    for (int k = 0; k < 9; ++k) CHECK(hipFree(batch[k]));
  }
  fclose(f);
  double* m_raw = (double*)malloc(sizeof(double) * (2 + steps));
  double* m_al = (double*)malloc(sizeof(double) * (2 + steps));
  CALL(hoisdf_eval_accum_finish(st_raw, NV, d_ath, steps, d_out, st));
  CHECK(hipStreamSynchronize(st));
  if (!wr(o, d_out, sizeof(double) * (2 + steps), m_raw)) return 2;
  CALL(hoisdf_eval_accum_finish(st_al, NV, d_ath, steps, d_out, st));
  CHECK(hipStreamSynchronize(st));
  if (!wr(o, d_out, sizeof(double) * (2 + steps), m_al)) return 2;
  fclose(o);

  FILE* r = fopen(argv[3], "w");
  if (!r) { perror("open"); return 2; }
  /* sums: adds, mce, oce, mme, mje, pamje; the file's order is that of main/test.py */
  fprintf(r, "ADDS_error :  %.17g\n", sums[0] / total);
  fprintf(r, "mano_mje :  %.17g\n", sums[4] / total);
  fprintf(r, "mano_pamje :  %.17g\n", sums[5] / total);
  fprintf(r, "OCE_error :  %.17g\n", sums[2] / total);
  fprintf(r, "MCE_error :  %.17g\n", sums[1] / total);
  fprintf(r, "Evaluation 3D MESH results:\n");
  fprintf(r, "auc=%.3f, mean_vert3d_avg=%.2f cm\n", m_raw[1], m_raw[0] * 100.0);
  fprintf(r, "Evaluation 3D MESH ALIGNED results:\n");
  fprintf(r, "auc=%.3f, mean_vert3d_avg=%.2f cm\n\n", m_al[1], m_al[0] * 100.0);
  fprintf(r, "F-scores\n");
  for (int t = 0; t < NTH; ++t) {
    float m[2];
    for (int a = 0; a < 2; ++a) {                                 /* a float32 mean, as numpy takes it of the float32 scores */
      float s = 0.f;
      for (long i = 0; i < (long)n_batches * B; ++i) s += f_all[(long)(a * NTH + t) * n_batches * B + i];
      m[a] = s / (float)(n_batches * B);
    }
    fprintf(r, "F@%.1fmm = %.3f \tF_aligned@%.1fmm = %.3f\n", f_th[t] * 1000, m[0], f_th[t] * 1000, m[1]);
  }
  fclose(r);
  printf("c host eval ok: %d batches of %d samples\n", n_batches, B);
  return 0;
}
