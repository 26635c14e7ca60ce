/* A C host with no Python and no torch asks whether a hand mesh and an object mesh are compatible, through include/hoisdf.h:
 *   hoisdf_eval_interaction_workspace_bytes -> hoisdf_eval_interaction (one call for the batch)
 * prints what it got and writes it; tests/test_gpu_interaction.py::test_c_host_interaction compares it bit for bit with
 * ops.eval_interaction on the same inputs.
 * Input file (little-endian): int32 B, Vh, Fh, Vo, Fo; float32 contact_dist, voxel; then arrays, each as int64 count + 4-byte data:
 * hand verts float32 [B][Vh][3], hand faces int32 [B][Fh][3], hand n_faces int32 [B], object verts float32 [B][Vo][3], object faces
 * int32 [B][Fo][3], object n_faces int32 [B], object n_verts int32 [B].
 * Output file: pen_hand, pen_obj, min_dist, volume float32 [B] each; contact_verts, in_contact, inside_count int32 [B] each; grid
 * float32 [B][8]; the number of inside bytes set in each sample's mask, int32 [B]. */
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
  float par[2];
  if (fread(hd, sizeof(int32_t), 5, f) != 5 || fread(par, sizeof(float), 2, f) != 2) return 2;
  const int B = hd[0], Vh = hd[1], Fh = hd[2], Vo = hd[3], Fo = hd[4];
  if (B < 1 || B > 64 || Vh < 1 || Vh > 100000 || Vo < 1 || Vo > 100000 || Fh < 1 || Fh > HOISDF_MESH_MAX_FACES || Fo < 1 ||
      Fo > HOISDF_MESH_MAX_FACES) {
    fprintf(stderr, "bad header\n");
    return 2;
  }
  hoisdf_mesh hand, obj;
  hand.verts = (const float*)rd((long)B * Vh * 3);
  hand.faces = (const int32_t*)rd((long)B * Fh * 3);
  hand.n_faces = (const int32_t*)rd(B);
  hand.face_batch_stride = 3L * Fh;
  hand.V = Vh;
  hand.max_faces = Fh;
  obj.verts = (const float*)rd((long)B * Vo * 3);
  obj.faces = (const int32_t*)rd((long)B * Fo * 3);
  obj.n_faces = (const int32_t*)rd(B);
  obj.face_batch_stride = 3L * Fo;
  obj.V = Vo;
  obj.max_faces = Fo;
  const int32_t* obj_n_verts = (const int32_t*)rd(B);
  fclose(f);

  const long cells = (long)HOISDF_INTERACT_MAX_GRID * HOISDF_INTERACT_MAX_GRID * HOISDF_INTERACT_MAX_GRID;
  const long nws = hoisdf_eval_interaction_workspace_bytes(B, Vh, Fh, Vo, Fo);
  if (nws < 0) { fprintf(stderr, "workspace: %s\n", hoisdf_last_error()); return 1; }
  float* fo;      /* pen_hand, pen_obj, min_dist, volume [B] each, then grid [B][8] */
  int32_t* io;    /* contact_verts, in_contact, inside_count [B] each */
  uint8_t* mask;
  void* ws;
  CHECK(hipMalloc((void**)&fo, sizeof(float) * 12 * B));
  CHECK(hipMalloc((void**)&io, sizeof(int32_t) * 3 * B));
  CHECK(hipMalloc((void**)&mask, (size_t)cells * B));
  CHECK(hipMemset(mask, 0, (size_t)cells * B));
  CHECK(hipMalloc(&ws, nws > 0 ? (size_t)nws : 1));
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  CALL(hoisdf_eval_interaction(&hand, &obj, obj_n_verts, B, par[0], par[1], fo, fo + B, fo + 2 * B, io, io + B, fo + 3 * B, io + 2 * B, mask,
                               fo + 4 * B, ws, nws, st));
  CHECK(hipStreamSynchronize(st));

  float* hf = (float*)malloc(sizeof(float) * 12 * B);
  int32_t* hi = (int32_t*)malloc(sizeof(int32_t) * 4 * B);
  uint8_t* hm = (uint8_t*)malloc((size_t)cells);
  CHECK(hipMemcpy(hf, fo, sizeof(float) * 12 * B, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hi, io, sizeof(int32_t) * 3 * B, hipMemcpyDeviceToHost));
  for (int b = 0; b < B; ++b) {
    CHECK(hipMemcpy(hm, mask + (size_t)b * cells, (size_t)cells, hipMemcpyDeviceToHost));
    int32_t set = 0;
    for (long i = 0; i < cells; ++i) set += hm[i] != 0;
    hi[3 * B + b] = set;
    int32_t n;
    memcpy(&n, &hf[4 * B + 8 * b + 6], sizeof(n));
    printf("sample %d: pen_hand %.6f m, pen_obj %.6f m, min_dist %.6g m, contact_verts %d, in_contact %d, inside %d of %d x %d x %d cells, "
           "volume %.4g m^3, mask bytes set %d\n", b, hf[b], hf[B + b], hf[2 * B + b], hi[b], hi[B + b], hi[2 * B + b], n & 255, (n >> 8) & 255,
           (n >> 16) & 255, hf[3 * B + b], set);
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { perror("open"); return 2; }
  if (fwrite(hf, sizeof(float), 4 * B, o) != (size_t)(4 * B) || fwrite(hi, sizeof(int32_t), 3 * B, o) != (size_t)(3 * B) ||
      fwrite(hf + 4 * B, sizeof(float), 8 * B, o) != (size_t)(8 * B) || fwrite(hi + 3 * B, sizeof(int32_t), B, o) != (size_t)B) {
    fprintf(stderr, "writing the outputs failed\n");
    return 2;
  }
  fclose(o);
  printf("c host interaction ok: %d samples\n", B);
  return 0;
}
