/* A C host with no Python and no torch takes ONE CAMERA FRAME TO ONE POSE through include/hoisdf.h alone - the call sequence of
 * INTEGRATION.md "from a camera frame to the model input" in front of "image to pose from C":
 *   hoisdf_crop_params_dexycb (host arithmetic) -> hoisdf_image_crop (the NHWC model input, both heat-map masks) ->
 *   hoisdf_pose_infer_begin -> hoisdf_encoder_infer -> hoisdf_pose_infer, all on one stream,
 * and compares joints / MANO mesh / MANO joints / the per-point object outputs with what the Python native path
 * (ImagePipeline.eval_batch + Model.encode_native + Model.infer_native) produced from the same frames: the same kernels in the same
 * order, so 1e-6 m.  File layout (little-endian), written by tests/test_gpu_image.py::test_c_host_frame_to_pose: as
 * tests/c/test_image_to_pose_host.c up to the MANO assets; then the frame size (two int64), and per sample the uint8 frame and two
 * uint8 byte masks (int64 count + bytes each); then float32 arrays: joints_uv [B][21][2], p2d [B][21][2], K [B][9], flip [B],
 * centres, expected outputs. */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hoisdf.h"

#define CHECK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "hip error line %d\n", __LINE__); return 2; } } while (0)
#define CALL(x) do { int rc_ = (x); if (rc_) { fprintf(stderr, "line %d: status %d: %s\n", __LINE__, rc_, hoisdf_last_error()); return 1; } } while (0)

static FILE* f;
/* next array of the file: `expect` floats (0 = any), uploaded; *host (optional) keeps the host copy */
static float* rd(long expect, float** host) {
  int64_t n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1 || n <= 0 || (expect && n != expect)) { fprintf(stderr, "array of %ld floats, expected %ld\n", (long)n, expect); exit(2); }
  float* h = (float*)malloc(sizeof(float) * n);
  if (fread(h, sizeof(float), n, f) != (size_t)n) { fprintf(stderr, "short read\n"); exit(2); }
  float* d = NULL;
  if (hipMalloc((void**)&d, sizeof(float) * n) != hipSuccess || hipMemcpy(d, h, sizeof(float) * n, hipMemcpyHostToDevice) != hipSuccess) exit(2);
  if (host) *host = h; else free(h);
  return d;
}
static uint8_t* rd_u8(long expect) {
  int64_t n = 0;
  if (fread(&n, sizeof(n), 1, f) != 1 || n != expect) { fprintf(stderr, "array of %ld bytes, expected %ld\n", (long)n, expect); exit(2); }
  uint8_t* h = (uint8_t*)malloc(n);
  if (fread(h, 1, n, f) != (size_t)n) { fprintf(stderr, "short read\n"); exit(2); }
  uint8_t* d = NULL;
  if (hipMalloc((void**)&d, n) != hipSuccess || hipMemcpy(d, h, n, hipMemcpyHostToDevice) != hipSuccess) exit(2);
  free(h);
  return d;
}
static void rd_mlp(hoisdf_mlp* m, int n_layers, const int* dims, int act_last) {
  memset(m, 0, sizeof(*m));
  m->n_layers = n_layers; m->act_last = act_last;
  for (int i = 0; i <= n_layers; ++i) m->dims[i] = dims[i];
  for (int i = 0; i < n_layers; ++i) { m->w[i] = rd((long)dims[i + 1] * dims[i], NULL); m->b[i] = rd(dims[i + 1], NULL); }
}
static void rd_sdf_decoder(hoisdf_sdf_decoder_params* p) {
  static const int out[4] = {512, 223, 512, 512}, in[4] = {289, 512, 512, 512};
  for (int i = 0; i < 4; ++i) { p->weight_v[i] = rd((long)out[i] * in[i], NULL); p->weight_g[i] = rd(out[i], NULL); p->bias[i] = rd(out[i], NULL); }
  p->linh4_weight = rd(512, NULL); p->linh4_bias = rd(1, NULL);
}
static void rd_encoder(hoisdf_encoder_layer_weights* w, int L, long E, long F) {
  for (int i = 0; i < L; ++i) {
    w[i].w_in = rd(3 * E * E, NULL); w[i].b_in = rd(3 * E, NULL); w[i].w_out = rd(E * E, NULL); w[i].b_out = rd(E, NULL);
    w[i].g1 = rd(E, NULL); w[i].be1 = rd(E, NULL); w[i].w1 = rd(F * E, NULL); w[i].b1 = rd(F, NULL);
    w[i].w2 = rd(E * F, NULL); w[i].b2 = rd(E, NULL); w[i].g2 = rd(E, NULL); w[i].be2 = rd(E, NULL);
  }
  const float* g3 = rd(E, NULL); const float* be3 = rd(E, NULL);          /* the stack's inter_norm */
  for (int i = 0; i < L; ++i) { w[i].g3 = g3; w[i].be3 = be3; }
}
static double max_err(const float* a, const float* b, long n) {
  double e = 0;
  for (long i = 0; i < n; ++i) { double d = fabs((double)a[i] - b[i]); if (!(d <= e)) e = d; }
  return e;
}
int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <dump.bin>\n", argv[0]); return 2; }
  f = fopen(argv[1], "rb");
  if (!f) { perror("open"); return 2; }
  hoisdf_encoder_desc ed;
  hoisdf_pose_desc d;
  if (fread(&ed, sizeof(ed), 1, f) != 1 || fread(&d, sizeof(d), 1, f) != 1) return 2;
  if (d.use_inverse_kinematics || ed.B != d.B) { fprintf(stderr, "this host checks the MANO-head variant, one batch size\n"); return 2; }
  const int B = d.B, nh = d.num_samp_hand, no = d.num_samp_obj, E = d.hidden_dim, F = d.dim_feedforward, C = d.C;

  /* ---- the encoder's tensors, in table order (a real host looks each name up in its checkpoint) ---- */
  const int nt = hoisdf_encoder_tensor_count(&ed);
  if (nt <= 0) { fprintf(stderr, "tensor_count: %s\n", hoisdf_last_error()); return 1; }
  const float** enc = (const float**)malloc(sizeof(float*) * nt);
  for (int i = 0; i < nt; ++i) {
    if (!hoisdf_encoder_tensor_name(&ed, i)) { fprintf(stderr, "tensor_name: %s\n", hoisdf_last_error()); return 1; }
    enc[i] = rd(hoisdf_encoder_tensor_numel(&ed, i), NULL);
  }

  /* ---- weights, named after the checkpoint keys ---- */
  static hoisdf_pose_weights w;
  memset(&w, 0, sizeof(w));
  { const int ds[3] = {C, 512, 256}; rd_mlp(&w.linear_sdfin, 2, ds, 1); }
  rd_sdf_decoder(&w.hand_sdf_decoder);
  rd_sdf_decoder(&w.obj_sdf_decoder);
  { const int ds[5] = {C, 1024, 512, 256, E - 33}; rd_mlp(&w.linear_transformerin, 4, ds, 1); }
  w.hand_sigmoid_beta = rd(1, NULL); w.obj_sigmoid_beta = rd(1, NULL);
  rd_encoder(w.hand_encoder, d.enc_layers, E, F);
  rd_encoder(w.obj_encoder, d.enc_layers / 2, E, F);
  for (int i = 0; i < d.dec_layers; ++i) {
    hoisdf_decoder_layer_weights* l = &w.hand_decoder[i];
    const long e = E, ff = F;
    l->sa_w_in = rd(3 * e * e, NULL); l->sa_b_in = rd(3 * e, NULL); l->sa_w_out = rd(e * e, NULL); l->sa_b_out = rd(e, NULL);
    l->ca_w_in = rd(3 * e * e, NULL); l->ca_b_in = rd(3 * e, NULL); l->ca_w_out = rd(e * e, NULL); l->ca_b_out = rd(e, NULL);
    l->w1 = rd(ff * e, NULL); l->b1 = rd(ff, NULL); l->w2 = rd(e * ff, NULL); l->b2 = rd(e, NULL);
    l->g1 = rd(e, NULL); l->be1 = rd(e, NULL); l->g2 = rd(e, NULL); l->be2 = rd(e, NULL); l->g3 = rd(e, NULL); l->be3 = rd(e, NULL);
  }
  { const float* g4 = rd(E, NULL); const float* be4 = rd(E, NULL);        /* decoder.norm */
    for (int i = 0; i < d.dec_layers; ++i) { w.hand_decoder[i].g4 = g4; w.hand_decoder[i].be4 = be4; } }
  w.mano_query_embed = rd(17L * E, NULL);
  { const int d6[4] = {E, E, E, 6}, d10[4] = {E, E, E, 10}, dv[5] = {E, E, E, E, 60}, dc[4] = {E, E, E, 20}, d3[4] = {E, E, E, 3};
    rd_mlp(&w.linear_pose, 3, d6, 0); rd_mlp(&w.linear_shape, 3, d10, 0); rd_mlp(&w.linear_handvote, 4, dv, 0);
    rd_mlp(&w.linear_handcls, 3, dc, 0); rd_mlp(&w.linear_obj_rot, 3, d3, 0); rd_mlp(&w.linear_obj_rel_trans, 3, d3, 0); }
  w.mano_shapedirs = rd(778L * 3 * 10, NULL); w.mano_posedirs = rd(778L * 3 * 135, NULL); w.mano_weights = rd(778L * 16, NULL);
  w.mano_v_template = rd(778L * 3, NULL); w.mano_j_regressor = rd(16L * 778, NULL); w.mano_hands_mean = rd(45, NULL);

  /* ---- the frames and their 2D labels; the Python native path's outputs ---- */
  int64_t hw[2];
  if (fread(hw, sizeof(int64_t), 2, f) != 2 || hw[0] <= 0 || hw[1] <= 0) return 2;
  const int FH = (int)hw[0], FW = (int)hw[1], res = ed.img_h, hm = res / 2;
  hoisdf_frame* frames = (hoisdf_frame*)calloc(B, sizeof(hoisdf_frame));
  for (int b = 0; b < B; ++b) {
    frames[b].frame = rd_u8((long)FH * FW * 3); frames[b].hand_mask = rd_u8((long)FH * FW); frames[b].obj_mask = rd_u8((long)FH * FW);
    frames[b].H = FH; frames[b].W = FW; frames[b].mask_packed = 0;
  }
  float *joints_uv, *p2d, *K, *flip;
  (void)rd(B * 42L, &joints_uv); (void)rd(B * 42L, &p2d); (void)rd(B * 9L, &K); (void)rd(B, &flip);
  const float* center_hand = rd(B * 3L, NULL); const float* center_obj = rd(B * 3L, NULL);
  float *e_joints, *e_rot, *e_trans, *e_mesh, *e_mj;
  (void)rd(B * 60L, &e_joints); (void)rd((long)B * no * 3, &e_rot); (void)rd((long)B * no * 3, &e_trans); (void)rd(B * 778L * 3, &e_mesh);
  (void)rd(B * 63L, &e_mj);
  fclose(f);

  hipStream_t stream, side;
  CHECK(hipStreamCreate(&stream)); CHECK(hipStreamCreate(&side));

  /* ---- per frame, host: the crop and the camera it leaves behind ---- */
  hoisdf_crop* crops = (hoisdf_crop*)calloc(B, sizeof(hoisdf_crop));
  float* cam_h = (float*)malloc(sizeof(float) * B * 17);
  for (int b = 0; b < B; ++b) {
    double p[42], k[9];
    for (int i = 0; i < 42; ++i) p[i] = (double)p2d[b * 42 + i];
    for (int i = 0; i < 9; ++i) k[i] = (double)K[b * 9 + i];
    CALL(hoisdf_crop_params_dexycb(joints_uv + b * 42, 21, p, 21, k, FW, FH, flip[b] != 0.f, res, hm, &crops[b]));
    for (int i = 0; i < 9; ++i) cam_h[b * 9 + i] = (float)crops[b].K[i];
    for (int i = 0; i < 4; ++i) { cam_h[B * 9 + b * 4 + i] = (float)crops[b].bbox_hand[i]; cam_h[B * 13 + b * 4 + i] = (float)crops[b].bbox_obj[i]; }
  }
  float* cam_d;
  CHECK(hipMalloc((void**)&cam_d, sizeof(float) * B * 17));
  CHECK(hipMemcpy(cam_d, cam_h, sizeof(float) * B * 17, hipMemcpyHostToDevice));
  const float *cam_intr = cam_d, *bbox_hand = cam_d + B * 9, *bbox_obj = cam_d + B * 13;
  float *img, *hand_seg, *obj_seg;
  CHECK(hipMalloc((void**)&img, sizeof(float) * B * res * res * 3));
  CHECK(hipMalloc((void**)&hand_seg, sizeof(float) * B * hm * hm)); CHECK(hipMalloc((void**)&obj_seg, sizeof(float) * B * hm * hm));
  CALL(hoisdf_image_crop(frames, crops, B, res, hm, 0, img, NULL, hand_seg, obj_seg, stream));    /* NHWC: what the encoder reads */
  /* ---- once: everything that depends on the weights alone ---- */
  const long nenc = hoisdf_encoder_prepared_bytes(&ed), nprep = hoisdf_pose_prepared_bytes(&d), news = hoisdf_encoder_infer_workspace(&ed);
  if (nenc <= 0 || nprep <= 0 || news <= 0) { fprintf(stderr, "size query: %s\n", hoisdf_last_error()); return 1; }
  void *enc_prepared, *prepared, *enc_ws;
  CHECK(hipMalloc(&enc_prepared, nenc)); CHECK(hipMalloc(&prepared, nprep)); CHECK(hipMalloc(&enc_ws, news));
  CALL(hoisdf_encoder_prepare(&ed, enc, nt, enc_prepared, nenc, stream));
  CALL(hoisdf_pose_prepare(&d, &w, prepared, nprep, stream));
  hoisdf_pyramid pyr;
  CALL(hoisdf_encoder_pyramid_shape(&ed, &pyr));
  float* levels[HOISDF_MAX_LEVELS];
  int ctot = 0;
  for (int l = 0; l < pyr.n_levels; ++l) {
    CHECK(hipMalloc((void**)&levels[l], sizeof(float) * B * pyr.C[l] * pyr.H[l] * pyr.W[l]));
    pyr.data[l] = levels[l];
    ctot += pyr.C[l];
  }
  if (ctot != C) { fprintf(stderr, "the encoder's pyramid has %d channels, the pose descriptor %d\n", ctot, C); return 2; }

  /* ---- per frame ---- */
  int32_t *counts_dev, *counts_host;
  CHECK(hipMalloc((void**)&counts_dev, sizeof(int32_t) * 2 * B));
  CHECK(hipHostMalloc((void**)&counts_host, sizeof(int32_t) * 2 * B, hipHostMallocDefault));
  hipEvent_t counted;
  CHECK(hipEventCreateWithFlags(&counted, hipEventDisableTiming));
  CALL(hoisdf_pose_infer_begin(&d, center_hand, center_obj, cam_intr, bbox_hand, bbox_obj, counts_dev, counts_host, stream));
  CHECK(hipEventRecord(counted, stream));
  CALL(hoisdf_encoder_infer(&ed, enc_prepared, img, levels, NULL, enc_ws, news, stream));       /* only enqueues: the counts arrive meanwhile */
  CHECK(hipEventSynchronize(counted));                                   /* the one host read of the path: 2 B integers */
  const long nws = hoisdf_pose_infer_workspace(&d, counts_host);
  if (nws <= 0) { fprintf(stderr, "infer_workspace: %s\n", hoisdf_last_error()); return 1; }
  void* ws;
  CHECK(hipMalloc(&ws, nws));
  hoisdf_pose_outputs out;
  memset(&out, 0, sizeof(out));
  CHECK(hipMalloc((void**)&out.hand_joints_out, sizeof(float) * B * 60)); CHECK(hipMalloc((void**)&out.obj_rot_out, sizeof(float) * B * no * 3));
  CHECK(hipMalloc((void**)&out.obj_trans_out, sizeof(float) * B * no * 3)); CHECK(hipMalloc((void**)&out.mano_mesh_out, sizeof(float) * B * 778 * 3));
  CHECK(hipMalloc((void**)&out.mano_joints_out, sizeof(float) * B * 63));
  CALL(hoisdf_pose_infer(&d, prepared, &pyr, center_hand, center_obj, cam_intr, bbox_hand, bbox_obj, counts_dev, counts_host, &out, ws, nws, side,
                         stream));
  CHECK(hipStreamSynchronize(stream));                                   /* `stream` is ordered behind the side stream's work */

  long nmax = B * 778L * 3;
  if ((long)B * no * 3 > nmax) nmax = (long)B * no * 3;
  float* h = (float*)malloc(sizeof(float) * nmax);
  CHECK(hipMemcpy(h, out.hand_joints_out, sizeof(float) * B * 60, hipMemcpyDeviceToHost));
  const double ej = max_err(h, e_joints, B * 60L);
  CHECK(hipMemcpy(h, out.mano_mesh_out, sizeof(float) * B * 778 * 3, hipMemcpyDeviceToHost));
  const double em = max_err(h, e_mesh, B * 778L * 3);
  CHECK(hipMemcpy(h, out.mano_joints_out, sizeof(float) * B * 63, hipMemcpyDeviceToHost));
  const double emj = max_err(h, e_mj, B * 63L);
  CHECK(hipMemcpy(h, out.obj_rot_out, sizeof(float) * B * no * 3, hipMemcpyDeviceToHost));
  const double er = max_err(h, e_rot, (long)B * no * 3);
  CHECK(hipMemcpy(h, out.obj_trans_out, sizeof(float) * B * no * 3, hipMemcpyDeviceToHost));
  const double et = max_err(h, e_trans, (long)B * no * 3);
  printf("survivors hand %d obj %d (of %d + %d wanted); encoder: %d tensors, blob %ld bytes, workspace %ld bytes, %d launches; pose: blob %ld, workspace %ld\n",
         counts_host[0], counts_host[B], nh, no, nt, nenc, news, hoisdf_encoder_launch_count(&ed), nprep, nws);
  printf("max abs diff to the Python native path: hand_joints %.3e mano_mesh %.3e mano_joints %.3e obj_rot %.3e obj_trans %.3e\n", ej, em, emj, er, et);
  const double tol = 1e-6;
  if (!(ej <= tol && em <= tol && emj <= tol && er <= tol && et <= tol)) { fprintf(stderr, "above the 1e-6 bar\n"); return 1; }
  printf("c host frame to pose ok\n");
  return 0;
}
