/* Crop and augmentation parameters of the image pipeline (include/hoisdf.h, "image preparation"): host arithmetic only, plain C,
 * no GPU call.  Restates data/dataset_util.py get_bbox_joints, fuse_bbox, get_affine_trans_no_rot, get_affine_transform,
 * transform_coords and normalize_joints as data/dexycb.py:249-305, :355-404 and data/ho3d.py:399-427 call them, with the
 * reference's number formats: `float` where numpy computes in float32, `double` elsewhere (compiled with -ffp-contract=off, so a
 * product and a sum never fuse).  hoisdf_amd/image_oracle.py is the same arithmetic in numpy. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../../include/hoisdf.h"

void hoisdf_internal_set_error(const char* msg); /* imgprep.hip: the library's thread-local message */

static int fail(const char* what, const char* msg) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", what, msg);
  hoisdf_internal_set_error(buf);
  return HOISDF_ERR_INVALID;
}

/* get_bbox_joints on float32 points: float32 arithmetic, the centre truncated; the box itself is float32 */
static void bbox_f32(const float* p, int n, float factor, float box[4]) {
  float mn[2] = {p[0], p[1]}, mx[2] = {p[0], p[1]};
  for (int i = 1; i < n; ++i)
    for (int a = 0; a < 2; ++a) {
      if (p[2 * i + a] < mn[a]) mn[a] = p[2 * i + a];
      if (p[2 * i + a] > mx[a]) mx[a] = p[2 * i + a];
    }
  for (int a = 0; a < 2; ++a) {
    const float half = (mx[a] + mn[a]) / 2.f;
    const double c = (double)(long)half;
    float d = (mx[a] - mn[a]) * factor;
    d = d / 2.f;
    box[a] = (float)(c - (double)d);
    box[2 + a] = (float)(c + (double)d);
  }
}
/* ... on float64 points */
static void bbox_f64(const double* p, int n, double factor, float box[4]) {
  double mn[2] = {p[0], p[1]}, mx[2] = {p[0], p[1]};
  for (int i = 1; i < n; ++i)
    for (int a = 0; a < 2; ++a) {
      if (p[2 * i + a] < mn[a]) mn[a] = p[2 * i + a];
      if (p[2 * i + a] > mx[a]) mx[a] = p[2 * i + a];
    }
  for (int a = 0; a < 2; ++a) {
    const double c = (double)(long)((mx[a] + mn[a]) / 2.0);
    const double d = (mx[a] - mn[a]) * factor / 2.0;
    box[a] = (float)(c - d);
    box[2 + a] = (float)(c + d);
  }
}

/* fuse_bbox: x is clamped to img_size[0] = W and y to img_size[1] = H, the axes as the reference has them */
static int fuse(const float a[4], const float b[4], int W, int H, double center[2], float* scale) {
  const float lim[2] = {(float)W, (float)H};
  float delta[2];
  for (int k = 0; k < 2; ++k) {
    float mn = fminf(fminf(a[k], a[2 + k]), fminf(b[k], b[2 + k]));
    float mx = fmaxf(fmaxf(a[k], a[2 + k]), fmaxf(b[k], b[2 + k]));
    if (!(mn == mn) || !(mx == mx) || isinf(mn) || isinf(mx)) return 0;
    if (mn < 0.f) mn = 0.f;
    if (mx > lim[k]) mx = lim[k];
    center[k] = (double)(long)((mx + mn) / 2.f);
    delta[k] = mx - mn;
  }
  *scale = delta[0] > delta[1] ? delta[0] : delta[1];
  return *scale > 0.f;
}

static void no_rot_f32(double cx, double cy, float scale, int res, double A[9]) {
  memset(A, 0, 9 * sizeof(double));
  const float r = (float)res;
  A[0] = A[4] = (double)(r / scale);
  float tx = (float)(-cx) / scale;
  tx = tx + 0.5f;
  float ty = (float)(-cy) / scale;
  ty = ty + 0.5f;
  A[2] = (double)(r * tx);
  A[5] = (double)(r * ty);
  A[8] = 1.0;
}
static void no_rot_f64(double cx, double cy, double scale, int res, double A[9]) {
  memset(A, 0, 9 * sizeof(double));
  A[0] = A[4] = (double)res / scale;
  A[2] = (double)res * (-cx / scale + 0.5);
  A[5] = (double)res * (-cy / scale + 0.5);
  A[8] = 1.0;
}
static void mm3(const double* a, const double* b, double* c) { /* k = 0, 1, 2 in order */
  double t[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) t[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
  memcpy(c, t, sizeof(t));
}
static void mv3(const double* a, const double* v, double* o) {
  double t[3];
  for (int i = 0; i < 3; ++i) t[i] = a[3 * i] * v[0] + a[3 * i + 1] * v[1] + a[3 * i + 2] * v[2];
  memcpy(o, t, sizeof(t));
}

/* get_affine_transform: scale_is_f32 selects the float32 form of get_affine_trans_no_rot (the evaluation crops) */
static void affine(const double center[2], double scale, int scale_is_f32, int res, double rot, const double* K, hoisdf_crop* o) {
  const double sn = sin(rot), cs = cos(rot);
  const double R[9] = {cs, -sn, 0, sn, cs, 0, 0, 0, 1};
  const double c1[3] = {center[0], center[1], 1.0};
  double rc[3], A[9], T[9];
  mv3(R, c1, rc);
  if (scale_is_f32) no_rot_f32(rc[0], rc[1], (float)scale, res, A); else no_rot_f64(rc[0], rc[1], scale, res, A);
  mm3(A, R, T);
  for (int i = 0; i < 9; ++i) { o->affine[i] = (float)T[i]; o->rot_mat[i] = (float)R[i]; }
  if (K) {
    const double t_mat[9] = {1, 0, -K[2], 0, 1, -K[5], 0, 0, 1}, t_inv[9] = {1, 0, K[2], 0, 1, K[5], 0, 0, 1};
    double M[9], tc[3];
    mm3(t_inv, R, M);
    mm3(M, t_mat, M);
    mv3(M, c1, tc);
    if (scale_is_f32) no_rot_f32(tc[0], tc[1], (float)scale, res, A); else no_rot_f64(tc[0], tc[1], scale, res, A);
    for (int i = 0; i < 9; ++i) o->post_rot_trans[i] = (float)A[i];
  } else {
    memcpy(o->post_rot_trans, o->affine, sizeof(o->affine));
  }
}

static int invert(hoisdf_crop* o) {
  double a[9];
  for (int i = 0; i < 9; ++i) a[i] = (double)o->affine[i];
  const double det = a[0] * a[4] - a[1] * a[3];
  if (!(det == det) || isinf(det) || det == 0.0) return 0;
  o->inverse[0] = a[4] / det;
  o->inverse[1] = -a[1] / det;
  o->inverse[2] = (a[1] * a[5] - a[4] * a[2]) / det;
  o->inverse[3] = -a[3] / det;
  o->inverse[4] = a[0] / det;
  o->inverse[5] = (a[3] * a[2] - a[0] * a[5]) / det;
  for (int i = 0; i < 6; ++i)
    if (!(o->inverse[i] == o->inverse[i]) || isinf(o->inverse[i])) return 0;
  return 1;
}

static void xform(const float* A, double x, double y, double* ox, double* oy) { /* transform_coords, float64 */
  *ox = (double)A[0] * x + (double)A[1] * y + (double)A[2];
  *oy = (double)A[3] * x + (double)A[4] * y + (double)A[5];
}
static void xform_box(const float* A, const float box[4], double out[4]) {
  xform(A, (double)box[0], (double)box[1], &out[0], &out[1]);
  xform(A, (double)box[2], (double)box[3], &out[2], &out[3]);
}
static void k_prime(const float* M, const double* K, double* out) {
  double m[9];
  for (int i = 0; i < 9; ++i) m[i] = (double)M[i];
  mm3(m, K, out);
}

static int check_common(const char* what, const void* p2d, int n_corners, const void* K, int W, int H, int res, int hm, const void* out) {
  if (!p2d || !K || !out) return fail(what, "null pointer");
  if (n_corners < 1 || n_corners > HOISDF_CROP_MAX_POINTS) return fail(what, "n_corners outside 1 .. HOISDF_CROP_MAX_POINTS");
  if (W <= 0 || H <= 0) return fail(what, "frame size <= 0");
  if (res <= 0 || hm <= 0) return fail(what, "res / hm <= 0");
  return HOISDF_OK;
}

/* the left-hand flip on the 2D inputs: float32 joints in float32, corners and K in float64 */
static void flip_inputs(int flip, int W, const float* joints_uv, int nj, const double* p2d, int nc, const double* K, float* j, double* p,
                        double* k) {
  memcpy(j, joints_uv, sizeof(float) * 2 * nj);
  memcpy(p, p2d, sizeof(double) * 2 * nc);
  memcpy(k, K, sizeof(double) * 9);
  if (!flip) return;
  for (int i = 0; i < nj; ++i) {
    float u = (float)W - j[2 * i];
    j[2 * i] = u - 1.f;
  }
  for (int i = 0; i < nc; ++i) p[2 * i] = (double)W - p[2 * i] - 1.0;
  k[2] = (double)W - k[2] - 1.0;
}

int hoisdf_crop_params_dexycb(const float* joints_uv, int n_joints, const double* p2d, int n_corners, const double* K, int frame_w,
                              int frame_h, int flip, int res, int hm, hoisdf_crop* out) {
  const char* what = "crop_params_dexycb";
  if (!joints_uv) return fail(what, "null pointer");
  int rc = check_common(what, p2d, n_corners, K, frame_w, frame_h, res, hm, out);
  if (rc) return rc;
  if (n_joints < 1 || n_joints > HOISDF_CROP_MAX_POINTS) return fail(what, "n_joints outside 1 .. HOISDF_CROP_MAX_POINTS");
  float j[2 * HOISDF_CROP_MAX_POINTS], crop_hand[4], crop_obj[4], bh[4], bo[4], scale;
  double p[2 * HOISDF_CROP_MAX_POINTS], k[9], center[2];
  flip_inputs(flip, frame_w, joints_uv, n_joints, p2d, n_corners, K, j, p, k);
  bbox_f32(j, n_joints, 1.5f, crop_hand);
  bbox_f64(p, n_corners, 1.5, crop_obj);
  bbox_f32(j, n_joints, 1.1f, bh);
  bbox_f64(p, n_corners, 1.0, bo);
  if (!fuse(crop_hand, crop_obj, frame_w, frame_h, center, &scale)) return fail(what, "the fused box is empty or not finite");
  memset(out, 0, sizeof(*out));
  affine(center, (double)scale, 1, res, 0.0, k, out);
  if (!invert(out)) return fail(what, "the affine is not invertible");
  xform_box(out->affine, bh, out->bbox_hand);
  xform_box(out->affine, bo, out->bbox_obj);
  k_prime(out->post_rot_trans, k, out->K);
  out->n_joints = n_joints;
  out->n_corners = n_corners;
  out->flip = flip != 0;
  for (int i = 0; i < n_joints; ++i) {
    double x, y;
    xform(out->affine, (double)j[2 * i], (double)j[2 * i + 1], &x, &y);
    out->joints_uv[i][0] = x / (double)res * (double)hm;
    out->joints_uv[i][1] = y / (double)res * (double)hm;
  }
  for (int i = 0; i < n_corners; ++i) {
    double x, y;
    xform(out->affine, p[2 * i], p[2 * i + 1], &x, &y);
    out->p2d[i][0] = (x - out->bbox_obj[0]) / (out->bbox_obj[2] - out->bbox_obj[0]);
    out->p2d[i][1] = (y - out->bbox_obj[1]) / (out->bbox_obj[3] - out->bbox_obj[1]);
  }
  return HOISDF_OK;
}

int hoisdf_crop_params_ho3d(const double* bbox_hand, const double* p2d, int n_corners, const double* K, int frame_w, int frame_h,
                            int res, int hm, hoisdf_crop* out) {
  const char* what = "crop_params_ho3d";
  if (!bbox_hand) return fail(what, "null pointer");
  int rc = check_common(what, p2d, n_corners, K, frame_w, frame_h, res, hm, out);
  if (rc) return rc;
  float crop_hand[4], crop_obj[4], bh[4], bo[4], scale;
  double center[2];
  bbox_f64(bbox_hand, 2, 1.5, crop_hand);
  bbox_f64(p2d, n_corners, 1.5, crop_obj);
  bbox_f64(bbox_hand, 2, 1.2, bh);
  bbox_f64(p2d, n_corners, 1.0, bo);
  if (!fuse(crop_hand, crop_obj, frame_w, frame_h, center, &scale)) return fail(what, "the fused box is empty or not finite");
  memset(out, 0, sizeof(*out));
  affine(center, (double)scale, 1, res, 0.0, NULL, out);
  if (!invert(out)) return fail(what, "the affine is not invertible");
  xform_box(out->affine, bh, out->bbox_hand);
  xform_box(out->affine, bo, out->bbox_obj);
  k_prime(out->affine, K, out->K);
  return HOISDF_OK;
}

int hoisdf_aug_params_dexycb(const float* joints_uv, int n_joints, const double* p2d, int n_corners, const double* K, int frame_w,
                             int frame_h, int flip, int res, int hm, double center_jittering, const double* center_u,
                             double scale_jitter, double rot, hoisdf_crop* out) {
  const char* what = "aug_params_dexycb";
  if (!joints_uv || !center_u) return fail(what, "null pointer");
  int rc = check_common(what, p2d, n_corners, K, frame_w, frame_h, res, hm, out);
  if (rc) return rc;
  if (n_joints < 1 || n_joints > HOISDF_CROP_MAX_POINTS) return fail(what, "n_joints outside 1 .. HOISDF_CROP_MAX_POINTS");
  if (!(scale_jitter > 0.0) || isinf(scale_jitter) || !(rot == rot) || isinf(rot) || !(center_jittering == center_jittering) ||
      !(center_u[0] == center_u[0]) || !(center_u[1] == center_u[1]))
    return fail(what, "scale_jitter <= 0 or a jitter number that is not finite");
  float j[2 * HOISDF_CROP_MAX_POINTS], crop_hand[4], crop_obj[4], scale;
  double p[2 * HOISDF_CROP_MAX_POINTS], k[9], center[2], tj[2 * HOISDF_CROP_MAX_POINTS], tp[2 * HOISDF_CROP_MAX_POINTS];
  flip_inputs(flip, frame_w, joints_uv, n_joints, p2d, n_corners, K, j, p, k);
  bbox_f32(j, n_joints, 1.5f, crop_hand);
  bbox_f64(p, n_corners, 1.5, crop_obj);
  if (!fuse(crop_hand, crop_obj, frame_w, frame_h, center, &scale)) return fail(what, "the fused box is empty or not finite");
  const float cs = (float)center_jittering * scale;
  center[0] = center[0] + (double)cs * center_u[0];
  center[1] = center[1] + (double)cs * center_u[1];
  const double scale64 = (double)scale * scale_jitter;
  memset(out, 0, sizeof(*out));
  affine(center, scale64, 0, res, rot, k, out);
  if (!invert(out)) return fail(what, "the affine is not invertible");
  for (int i = 0; i < n_joints; ++i) xform(out->affine, (double)j[2 * i], (double)j[2 * i + 1], &tj[2 * i], &tj[2 * i + 1]);
  for (int i = 0; i < n_corners; ++i) xform(out->affine, p[2 * i], p[2 * i + 1], &tp[2 * i], &tp[2 * i + 1]);
  float bh[4], bo[4];
  bbox_f64(tj, n_joints, 1.1, bh);
  bbox_f64(tp, n_corners, 1.0, bo);
  for (int i = 0; i < 4; ++i) { out->bbox_hand[i] = (double)bh[i]; out->bbox_obj[i] = (double)bo[i]; }
  k_prime(out->post_rot_trans, k, out->K);
  out->n_joints = n_joints;
  out->n_corners = n_corners;
  out->flip = flip != 0;
  for (int i = 0; i < n_joints; ++i) {
    out->joints_uv[i][0] = tj[2 * i] / (double)res * (double)hm;
    out->joints_uv[i][1] = tj[2 * i + 1] / (double)res * (double)hm;
  }
  for (int i = 0; i < n_corners; ++i) {
    out->p2d[i][0] = (tp[2 * i] - out->bbox_obj[0]) / (out->bbox_obj[2] - out->bbox_obj[0]);
    out->p2d[i][1] = (tp[2 * i + 1] - out->bbox_obj[1]) / (out->bbox_obj[3] - out->bbox_obj[1]);
  }
  return HOISDF_OK;
}
