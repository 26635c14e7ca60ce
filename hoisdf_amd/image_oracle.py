"""numpy restatement of the image half of the reference's ``__getitem__`` (data/dexycb.py:219-404, data/ho3d.py:399-427,
data/dataset_util.py): crop parameters, the nearest-neighbour affine warp, the 8-bit photometric chain and the labels that move
with them.  It is the DEFINITION csrc/imgprep.hip and csrc/imgprep_params.c are held to (tests/test_gpu_image.py,
tests/test_image_oracle.py); it is not a product path and imports neither PIL nor torch.

Number formats follow the reference under numpy's scalar rules (a Python number next to a float32 stays float32): boxes of
float32 joints and the evaluation crop's affine are float32 arithmetic, everything downstream of a float64 operand is float64,
``get_affine_transform`` returns float32 matrices.  Deviations from the reference's image libraries, all deliberate (DESIGN.md,
"Image preparation on the device"): the warp evaluates PIL's nearest rule in float64 from the float64 inverse of the float32
affine; the blur is a true 7-tap Gaussian, not PIL's box approximation.  Brightness / contrast / saturation are the floor of
PIL's blend in float32, the RGB <-> HSV pair reproduces PIL's conversion for all 2^24 colours in both directions.
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
f64 = np.float64
OPS = ("brightness", "contrast", "saturation", "hue")          # op ids 0..3 of hoisdf_photo.order


# ---------------------------------------------------------------------------------------------- boxes and affines
def get_bbox_joints(pts, bbox_factor):
    """dataset_util.get_bbox_joints: arithmetic in the dtype of ``pts`` (float32 joints stay float32), centre truncated."""
    pts = np.asarray(pts)
    t = pts.dtype.type
    mn, mx = pts.min(0), pts.max(0)
    c = np.array([int((mx[0] + mn[0]) / t(2)), int((mx[1] + mn[1]) / t(2))], dtype=f64)
    delta = ((mx - mn) * t(bbox_factor) / t(2)).astype(f64)
    return np.concatenate([c - delta, c + delta]).astype(f32)


def fuse_bbox(b1, b2, img_size):
    """dataset_util.fuse_bbox on two float32 boxes; ``img_size`` = (W, H) and x is clamped to img_size[0], as the reference has it."""
    b = np.concatenate([np.asarray(b1, f32).reshape(2, 2), np.asarray(b2, f32).reshape(2, 2)], 0)
    mn, mx = b.min(0), b.max(0)
    min_x, min_y = max(f32(0), mn[0]), max(f32(0), mn[1])
    max_x, max_y = min(mx[0], f32(img_size[0])), min(mx[1], f32(img_size[1]))
    center = np.array([int((max_x + min_x) / f32(2)), int((max_y + min_y) / f32(2))], dtype=f64)
    scale = max(f32(max_x - min_x), f32(max_y - min_y))
    return center, f32(scale)


def affine_no_rot(center, scale, res):
    """get_affine_trans_no_rot; a float32 ``scale`` makes the entries float32 arithmetic (the evaluation crops)."""
    a = np.zeros((3, 3), f64)
    if isinstance(scale, np.float32):
        a[0, 0] = a[1, 1] = f32(res) / scale
        a[0, 2] = f32(res) * (f32(-float(center[0])) / scale + f32(0.5))
        a[1, 2] = f32(res) * (f32(-float(center[1])) / scale + f32(0.5))
    else:
        a[0, 0] = a[1, 1] = float(res) / scale
        a[0, 2] = res * (-float(center[0]) / scale + 0.5)
        a[1, 2] = res * (-float(center[1]) / scale + 0.5)
    a[2, 2] = 1
    return a


def _mm(a, b):
    """3 x 3 (or 3 x 3 by 3) product, k = 0, 1, 2 summed in order, no fused multiply-add: what csrc/imgprep_params.c does"""
    a, b = np.asarray(a, f64), np.asarray(b, f64)
    return a[:, 0, None] * b[0] + a[:, 1, None] * b[1] + a[:, 2, None] * b[2] if b.ndim == 2 else a[:, 0] * b[0] + a[:, 1] * b[1] + a[:, 2] * b[2]


def get_affine_transform(center, scale, res, rot=0.0, K=None):
    """-> (affine f32, post_rot_trans f32 or None, rot_mat f32)"""
    sn, cs = np.sin(f64(rot)), np.cos(f64(rot))
    rot_mat = np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1]], f64)
    c1 = np.array([center[0], center[1], 1.0], f64)
    total = _mm(affine_no_rot(_mm(rot_mat, c1)[:2], scale, res), rot_mat)
    post = None
    if K is not None:
        t_mat, t_inv = np.eye(3), np.eye(3)
        t_mat[0, 2], t_mat[1, 2] = -K[0, 2], -K[1, 2]
        t_inv[0, 2], t_inv[1, 2] = K[0, 2], K[1, 2]
        tc = _mm(_mm(_mm(t_inv, rot_mat), t_mat), c1)
        post = affine_no_rot(tc[:2], scale, res).astype(f32)
    return total.astype(f32), post, rot_mat.astype(f32)


def invert_affine(affine):
    """float64 inverse (first two rows) of a float32 affine whose last row is (0, 0, 1); None when it is singular"""
    a = np.asarray(affine, f32).astype(f64)
    det = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
    if not np.isfinite(det) or det == 0.0:
        return None
    return np.array([[a[1, 1] / det, -a[0, 1] / det, (a[0, 1] * a[1, 2] - a[1, 1] * a[0, 2]) / det],
                     [-a[1, 0] / det, a[0, 0] / det, (a[1, 0] * a[0, 2] - a[0, 0] * a[1, 2]) / det]], f64)


def transform_coords(pts, affine):
    pts, a = np.asarray(pts, f64), np.asarray(affine, f64)
    return np.stack([a[0, 0] * pts[:, 0] + a[0, 1] * pts[:, 1] + a[0, 2], a[1, 0] * pts[:, 0] + a[1, 1] * pts[:, 1] + a[1, 2]], 1)


def normalize_joints(pts, bbox):
    b = np.asarray(bbox).reshape(2, 2).astype(f64)
    return (np.asarray(pts, f64) - b[0]) / (b[1] - b[0])


def flip_inputs(joints_uv, p2d, K, W):
    """the left-hand flip of data/dexycb.py:462-465, :501 on the 2D inputs: float32 joints in float32, the rest float64"""
    j = np.asarray(joints_uv, f32).copy()
    j[:, 0] = f32(W) - j[:, 0] - f32(1)
    p = np.asarray(p2d, f64).copy()
    p[:, 0] = W - p[:, 0] - 1
    K = np.asarray(K, f64).copy()
    K[0, 2] = W - K[0, 2] - 1
    return j, p, K


def _finish(out, affine, res, hm):
    out["affine"] = affine
    out["inverse"] = invert_affine(affine)
    return out


def crop_params_dexycb(joints_uv, p2d, K, W, H, flip, res, hm):
    """data/dexycb.py:355-404 (and the flip of :427-512 before it)"""
    joints_uv, p2d, K = np.asarray(joints_uv, f32), np.asarray(p2d, f64), np.asarray(K, f64)
    if flip:
        joints_uv, p2d, K = flip_inputs(joints_uv, p2d, K, W)
    crop_hand, crop_obj = get_bbox_joints(joints_uv, 1.5), get_bbox_joints(p2d, 1.5)
    bbox_hand, bbox_obj = get_bbox_joints(joints_uv, 1.1), get_bbox_joints(p2d, 1.0)
    center, scale = fuse_bbox(crop_hand, crop_obj, (W, H))
    affine, post, rot_mat = get_affine_transform(center, scale, res, 0.0, K)
    bbox_hand = transform_coords(bbox_hand.reshape(2, 2), affine).flatten()
    bbox_obj = transform_coords(bbox_obj.reshape(2, 2), affine).flatten()
    out = dict(post_rot_trans=post, rot_mat=rot_mat, K=_mm(post, K), bbox_hand=bbox_hand, bbox_obj=bbox_obj, flip=int(bool(flip)),
               joints_uv=transform_coords(joints_uv, affine) / res * hm,
               p2d=normalize_joints(transform_coords(p2d, affine), bbox_obj))
    return _finish(out, affine, res, hm)


def crop_params_ho3d(bbox_hand, p2d, K, W, H, res, hm):
    """data/ho3d.py:399-427: the hand is a box, K' = affine . K"""
    box, p2d, K = np.asarray(bbox_hand, f64).reshape(2, 2), np.asarray(p2d, f64), np.asarray(K, f64)
    crop_hand, crop_obj = get_bbox_joints(box, 1.5), get_bbox_joints(p2d, 1.5)
    bbox_hand, bbox_obj = get_bbox_joints(box, 1.2), get_bbox_joints(p2d, 1.0)
    center, scale = fuse_bbox(crop_hand, crop_obj, (W, H))
    affine, _, rot_mat = get_affine_transform(center, scale, res, 0.0, None)
    out = dict(post_rot_trans=affine.copy(), rot_mat=rot_mat, K=_mm(affine, K), flip=0,
               bbox_hand=transform_coords(bbox_hand.reshape(2, 2), affine).flatten(),
               bbox_obj=transform_coords(bbox_obj.reshape(2, 2), affine).flatten(),
               joints_uv=np.zeros((0, 2)), p2d=np.zeros((0, 2)))
    return _finish(out, affine, res, hm)


def aug_params_dexycb(joints_uv, p2d, K, W, H, flip, res, hm, center_jittering, center_u, scale_jitter, rot):
    """data/dexycb.py:249-305 with the random numbers given: centre offset = center_jittering * scale * center_u, scale *= scale_jitter,
    rotation ``rot`` in radians"""
    joints_uv, p2d, K = np.asarray(joints_uv, f32), np.asarray(p2d, f64), np.asarray(K, f64)
    if flip:
        joints_uv, p2d, K = flip_inputs(joints_uv, p2d, K, W)
    center, scale = fuse_bbox(get_bbox_joints(joints_uv, 1.5), get_bbox_joints(p2d, 1.5), (W, H))
    center = center + f64(f32(center_jittering) * scale) * np.asarray(center_u, f64)
    scale = f64(scale) * f64(scale_jitter)
    affine, post, rot_mat = get_affine_transform(center, scale, res, rot, K)
    juv = transform_coords(joints_uv, affine)
    p2 = transform_coords(p2d, affine)
    bbox_obj = get_bbox_joints(p2, 1.0)
    out = dict(post_rot_trans=post, rot_mat=rot_mat, K=_mm(post, K), bbox_hand=get_bbox_joints(juv, 1.1).astype(f64),
               bbox_obj=bbox_obj.astype(f64), flip=int(bool(flip)), joints_uv=juv / res * hm, p2d=normalize_joints(p2, bbox_obj))
    return _finish(out, affine, res, hm)


# ---------------------------------------------------------------------------------------------- 3D labels
def rodrigues(v):
    """axis-angle (3,) -> rotation matrix, float64"""
    v = np.asarray(v, f64).reshape(3)
    th = np.sqrt(v @ v)
    if th < 1e-12:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def rodrigues_inv(R):
    """rotation matrix -> axis-angle (3,), angle in [0, pi]"""
    R = np.asarray(R, f64)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.sqrt(w @ w), np.clip(0.5 * (np.trace(R) - 1), -1, 1)
    th = np.arctan2(s, c)
    if s > 1e-9:
        return w * (th / (2 * s))
    if c > 0:
        return np.zeros(3)
    d = np.sqrt(np.maximum((np.diag(R) + 1) * 0.5, 0))             # angle = pi: the axis from R + I, signs from the off-diagonals
    i = int(np.argmax(d))
    ax = np.array([(R[i, j] + R[j, i]) * 0.25 / d[i] if j != i else d[i] for j in range(3)])
    return ax / np.sqrt(ax @ ax) * th


def rotate_labels(rot_mat, joints_3d, p3d, mano_root, obj_rot, obj_trans):
    """data/dexycb.py:279-293: the in-plane rotation applied to the 3D labels"""
    R = np.asarray(rot_mat, f64)
    return dict(joints_3d=np.asarray(joints_3d, f64) @ R.T, p3d=np.asarray(p3d, f64) @ R.T,
                mano_root=rodrigues_inv(R @ rodrigues(mano_root)), obj_rot=rodrigues_inv(R @ rodrigues(obj_rot)),
                obj_trans=R @ np.asarray(obj_trans, f64))


# ---------------------------------------------------------------------------------------------- warp
def unpack_mask(packed, H, W):
    return np.unpackbits(np.asarray(packed, np.uint8))[:H * W].reshape(H, W)


def source_pixels(inverse, n, step=1.0):
    """source (sx, sy, inside-independent) of the n x n output grid whose pixel i sits at crop pixel floor((i + .5) * step)"""
    t = np.asarray(inverse, f64)
    i = np.floor((np.arange(n, dtype=f64) + 0.5) * step)
    xc, yc = np.meshgrid(i + 0.5, i + 0.5)
    sx = np.floor(t[0, 0] * xc + t[0, 1] * yc + t[0, 2])
    sy = np.floor(t[1, 0] * xc + t[1, 1] * yc + t[1, 2])
    return sx, sy


def _gather(img, sx, sy, flip):
    H, W = img.shape[:2]
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    xi, yi = np.where(ok, sx, 0).astype(np.int64), np.where(ok, sy, 0).astype(np.int64)
    if flip:
        xi = W - 1 - xi
    out = img[yi, xi]
    return np.where(ok.reshape(ok.shape + (1,) * (img.ndim - 2)), out, 0).astype(img.dtype)


def warp(frame, inverse, res, flip=False):
    """u8 [H][W][3] RAW (unflipped) frame -> u8 [res][res][3] crop"""
    sx, sy = source_pixels(inverse, res)
    return _gather(np.asarray(frame), sx, sy, flip)


def warp_mask(mask, inverse, res, hm, flip=False):
    """u8 [H][W] raw mask -> float32 [hm][hm]: the crop's warp and its NEAREST resize in one gather"""
    sx, sy = source_pixels(inverse, hm, res / hm)
    return _gather(np.asarray(mask), sx, sy, flip).astype(f32)


# ---------------------------------------------------------------------------------------------- photometric chain (8-bit levels)
def luma(img):
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def _blend(x, deg, f):
    x, deg, f = x.astype(f32), np.asarray(deg).astype(f32), f32(f)
    return np.trunc(np.clip(deg + f * (x - deg), f32(0), f32(255))).astype(np.uint8)


def brightness(img, f):
    return _blend(img, np.zeros((), f32), f)


def contrast_degenerate(img):
    return int(int(luma(img).sum()) / (img.shape[0] * img.shape[1]) + 0.5)


def contrast(img, f):
    return _blend(img, f32(contrast_degenerate(img)), f)


def saturation(img, f):
    return _blend(img, luma(img)[..., None], f)


def rgb_to_hsv(img):
    """PIL's RGB -> HSV, equal to Image.convert for every one of the 2^24 colours"""
    r, g, b = (img[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    s = cr / np.where(maxc == 0, 1, maxc).astype(f32)
    rc, gc, bc = ((maxc - c).astype(f32) / cr for c in (r, g, b))
    rc, gc, bc = rc.astype(f64), gc.astype(f64), bc.astype(f64)
    h = np.where(r == maxc, bc - gc, np.where(g == maxc, 2.0 + rc - bc, 4.0 + gc - rc)).astype(f32)
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(f64) * 255.0).astype(np.int32), 0, 255)
    us = np.clip((s.astype(f64) * 255.0).astype(np.int32), 0, 255)
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """PIL's HSV -> RGB, equal to Image.convert for every one of the 2^24 triples"""
    h, s, v = (hsv[..., i].astype(np.int32) for i in range(3))
    fh = h.astype(f32) * f32(6) / f32(255)
    i = np.floor(fh).astype(np.int32)
    f, fs, vv = fh - i.astype(f32), s.astype(f32) / f32(255), v.astype(f32)
    rnd = lambda x: np.floor(x.astype(f64) + 0.5).astype(np.int32)
    p, q, t = rnd(vv * (f32(1) - fs)), rnd(vv * (f32(1) - fs * f)), rnd(vv * (f32(1) - fs * (f32(1) - f)))
    i = i % 6
    out = np.stack([np.choose(i, [v, q, p, p, t, v]), np.choose(i, [t, v, v, q, p, p]), np.choose(i, [p, p, t, v, v, q])], -1)
    return np.where((s == 0)[..., None], v[..., None], np.clip(out, 0, 255)).astype(np.uint8)


def hue_shift(hue_factor):
    """torchvision's uint8(hue_factor * 255): truncated toward zero, modulo 256"""
    return int(np.trunc(f64(f32(hue_factor)) * 255.0)) & 255


def hue(img, hue_factor):
    hsv = rgb_to_hsv(img).astype(np.int32)
    hsv[..., 0] = (hsv[..., 0] + hue_shift(hue_factor)) & 255
    return hsv_to_rgb(hsv.astype(np.uint8))


BLUR_TAPS = 3
BLUR_MIN_SIGMA = 0.05


def blur_weights(sigma):
    """float32 weights w[0..3] of the taps at distance 0..3, normalised over the 7 taps in float64"""
    k = np.arange(BLUR_TAPS + 1, dtype=f64)
    w = np.exp(-(k * k) / (2.0 * f64(f32(sigma)) ** 2))
    return (w / (w[0] + 2 * w[1:].sum())).astype(f32)


def gaussian_blur(img, sigma):
    if f32(sigma) < f32(BLUR_MIN_SIGMA):
        return np.asarray(img).copy()
    w = blur_weights(sigma).astype(f64)
    x = np.asarray(img).astype(f64)
    for axis in (1, 0):
        n = x.shape[axis]
        acc = np.zeros_like(x)
        for k in range(-BLUR_TAPS, BLUR_TAPS + 1):
            acc += w[abs(k)] * np.take(x, np.clip(np.arange(n) + k, 0, n - 1), axis=axis)
        x = acc
    return np.floor(x + 0.5).astype(np.uint8)


def photo_chain(crop, blur_sigma, factors, order):
    """``factors``: 4 entries in OPS order, None = that op is absent; ``order``: a permutation of 0..3.
    -> (u8 image, the contrast degenerate level or None)"""
    img = gaussian_blur(crop, blur_sigma)
    deg = None
    for op in order:
        if factors[op] is None:
            continue
        if op == 0:
            img = brightness(img, factors[0])
        elif op == 1:
            deg = contrast_degenerate(img)
            img = contrast(img, factors[1])
        elif op == 2:
            img = saturation(img, factors[2])
        else:
            img = hue(img, factors[3])
    return img, deg


def to_float(img_u8, nchw=False):
    x = img_u8.astype(f32) / f32(255)
    return np.ascontiguousarray(np.moveaxis(x, -1, -3)) if nchw else x
