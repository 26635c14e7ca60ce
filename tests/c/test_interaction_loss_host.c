/* A C host with no Python and no torch trains against the compatibility of a hand mesh and an object mesh, through include/hoisdf.h:
 *   hoisdf_interaction_loss_workspace_bytes -> hoisdf_interaction_loss_fwd -> hoisdf_interaction_loss_bwd (one call each for the batch)
 * prints what it got and writes it; tests/test_gpu_interaction_loss.py::test_c_host_interaction_loss compares it bit for bit with
 * ops.interaction_loss and its backward on the same inputs.
 * Input file (little-endian): int32 B, Vh, Fh, Vo, Fo; float32 alpha; then arrays, each as int64 count + 4-byte data: hand verts
 * float32 [B][Vh][3], hand faces int32 [Fh][3] (shared), object verts float32 [B][Vo][3], object faces int32 [B][Fo][3], object
 * n_faces int32 [B], object n_verts int32 [B], rep_w_hand, att_w_hand float32 [B][Vh], rep_w_obj float32 [B][Vo], upstream gradients
 * float32 [3][B] (rep_hand, att, rep_obj).
 * Output file: rep_hand, att, rep_obj float32 [B] each; d_hand_verts float32 [B][Vh][3]; d_obj_verts float32 [B][Vo][3]. */
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
  int32_t hd[5];
  float alpha;
  if (fread(hd, sizeof(int32_t), 5, f) != 5 || fread(&alpha, sizeof(float), 1, f) != 1) return 2;
  const int B = hd[0], Vh = hd[1], Fh = hd[2], Vo = hd[3], Fo = hd[4];
  if (B < 1 || B > 64 || Vh < 1 || Vh > 100000 || Vo < 1 || Vo > 100000 || Fh < 1 || Fh > HOISDF_MESH_MAX_FACES || Fo < 1 ||
      Fo > HOISDF_MESH_MAX_FACES) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  hoisdf_mesh hand, obj;
  hand.verts = (const float*)rd((long)B * Vh * 3);
  hand.faces = (const int32_t*)rd((long)Fh * 3);
  hand.n_faces = NULL;
  hand.face_batch_stride = 0;
  hand.V = Vh;
  hand.max_faces = Fh;
  obj.verts = (const float*)rd((long)B * Vo * 3);
  obj.faces = (const int32_t*)rd((long)B * Fo * 3);
  obj.n_faces = (const int32_t*)rd(B);
  obj.face_batch_stride = 3L * Fo;
  obj.V = Vo;
  obj.max_faces = Fo;
  const int32_t* obj_n_verts = (const int32_t*)rd(B);
  const float* wr = (const float*)rd((long)B * Vh);
  const float* wa = (const float*)rd((long)B * Vh);
  const float* wo = (const float*)rd((long)B * Vo);
  const float* g = (const float*)rd(3L * B);
  fclose(f);

  const long nws = hoisdf_interaction_loss_workspace_bytes(B, Vh, Fh, Vo, Fo);
  if (nws < 0) { fprintf(stderr, "workspace: %s\n", hoisdf_last_error()); return 1; }
  const long n_out = 3L * B + 3L * B * Vh + 3L * B * Vo;
  float* out;     /* rep_hand, att, rep_obj [B] each, then d_hand_verts, then d_obj_verts */
  void* ws;
  CHECK(hipMalloc((void**)&out, sizeof(float) * n_out));
  CHECK(hipMalloc(&ws, nws > 0 ? (size_t)nws : 1));
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  CALL(hoisdf_interaction_loss_fwd(&hand, &obj, obj_n_verts, B, wr, Vh, wa, Vh, wo, Vo, alpha, out, out + B, out + 2 * B, ws, nws, st));
  CALL(hoisdf_interaction_loss_bwd(&hand, &obj, obj_n_verts, B, wr, Vh, wa, Vh, wo, Vo, alpha, g, g + B, g + 2 * B, out + 3 * B,
                                   out + 3 * B + 3L * B * Vh, ws, nws, st));
  CHECK(hipStreamSynchronize(st));

  float* h = (float*)malloc(sizeof(float) * n_out);
  CHECK(hipMemcpy(h, out, sizeof(float) * n_out, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    double nh = 0, no = 0;
    for (long i = 0; i < 3L * Vh; ++i) nh += (double)h[3 * B + (long)b * Vh * 3 + i] * h[3 * B + (long)b * Vh * 3 + i];
    for (long i = 0; i < 3L * Vo; ++i) no += (double)h[3 * B + 3L * B * Vh + (long)b * Vo * 3 + i] * h[3 * B + 3L * B * Vh + (long)b * Vo * 3 + i];
    printf("sample %d: rep_hand %.7f m, att %.7f m, rep_obj %.7f m, |d_hand|^2 %.4g, |d_obj|^2 %.4g\n", b, h[b], h[B + b], h[2 * B + b], nh, no);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror("open"); return 2; }
  if (fwrite(h, sizeof(float), n_out, o) != (size_t)n_out) {
    fprintf(stderr, "writing the outputs failed\n");
    return 2;
  }
  fclose(o);
  printf("c host interaction loss ok: %d samples\n", B);
  return 0;
}
