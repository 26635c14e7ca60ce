/* A C host with no Python and no torch runs the IK variant's post-process through include/hoisdf.h:
 *   hoisdf_mano_prepare (once per set of MANO assets) -> hoisdf_ik_mano_fwd (per batch of hands)
 * and writes what it got; tests/test_gpu_ik_native.py::test_c_host_ik compares it bit for bit with the Python call on the same inputs.
 * Input file (little-endian): int32 hands, n_joints, ldbetas; then arrays, each as int64 count + float32 data: joints
 * [hands][n_joints][3], betas [hands][ldbetas], th_shapedirs, th_posedirs, th_weights, th_v_template, th_J_regressor.
 * Output file: pose [hands][48], joints [hands][21][3], verts [hands][778][3] as raw float32, then int32 valid [hands]. */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "hoisdf.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "hip error line %d\n", __LINE__); return 2; } } while (0)
#define CALL(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "line %d: status %d: %s\n", __LINE__, rc_, hoisdf_last_error()); return 1; } } while (0)

static FILE* f;
/* next array of the file: `expect` floats, uploaded */
static float* rd(long expect) {
  int64_t n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1 || n != expect) { fprintf(stderr, "array of %ld floats, expected %ld\n", (long)n, expect); exit(2); }
  float* h = (float*)malloc(sizeof(float) * n);
  if (fread(h, sizeof(float), n, f) != (size_t)n) { fprintf(stderr, "short read\n"); exit(2); }
  float* d = NULL;
  if (hipMalloc((void**)&d, sizeof(float) * n) != hipSuccess || hipMemcpy(d, h, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess) exit(2);
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
  int32_t hd[3];
  if (fread(hd, sizeof(int32_t), 3, f) != 3) return 2;
  const int hands = hd[0], n_joints = hd[1], ldbetas = hd[2];
  if (hands < 1 || hands > 4096 || (n_joints != 20 && n_joints != 21) || ldbetas < 10 || ldbetas > 64) { fprintf(stderr, "bad header\n"); return 2; }
  float* joints = rd((long)hands * n_joints * 3);
  float* betas = rd((long)hands * ldbetas);
  float* shapedirs = rd(778L * 3 * 10);
  float* posedirs = rd(778L * 3 * 135);
  float* weights = rd(778L * 16);
  float* v_template = rd(778L * 3);
  float* j_regressor = rd(16L * 778);
  fclose(f);

  float *image, *pose, *out_joints, *verts;
  int32_t* valid;
  CHECK(hipMalloc((void**)&image, sizeof(float) * hoisdf_mano_dirs_image_floats()));
  CHECK(hipMalloc((void**)&pose, sizeof(float) * hands * 48));
  CHECK(hipMalloc((void**)&out_joints, sizeof(float) * hands * 21 * 3));
  CHECK(hipMalloc((void**)&verts, sizeof(float) * hands * 778 * 3));
  CHECK(hipMalloc((void**)&valid, sizeof(int32_t) * hands));
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  CALL(hoisdf_mano_prepare(shapedirs, posedirs, weights, image, st));
  CALL(hoisdf_ik_mano_fwd(joints, n_joints, betas, ldbetas, hands, image, v_template, j_regressor, weights, pose, verts, out_joints, valid, st));
  CHECK(hipStreamSynchronize(st));

  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror("open"); return 2; }
  if (!wr(o, pose, sizeof(float) * hands * 48) || !wr(o, out_joints, sizeof(float) * hands * 21 * 3) ||
      !wr(o, verts, sizeof(float) * hands * 778 * 3) || !wr(o, valid, sizeof(int32_t) * hands)) { fprintf(stderr, "writing the outputs failed\n"); return 2; }
  fclose(o);
  printf("c host ik ok: %d hands\n", hands);
  return 0;
}
