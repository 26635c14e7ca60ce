"""numpy restatement of the raster rules of include/hoisdf.h ("raster"): the yardstick of tests/test_raster_oracle.py and
tests/test_gpu_raster.py.  It follows the rules as the header states them - projection in float64 with every product rounded on
its own, corners snapped to 1/256 pixel, int64 edge functions with the top-left rule, perspective-correct float64 depth in one
order, the smallest (depth, mesh, face) key - one face at a time over whole pixel arrays, so ids, the bits of the depth, masks and
counts can be compared exactly with csrc/raster.hip.  ``raycast`` is an independent float64 ray caster, used by the tests only.
Not a fallback: nothing on the model's path imports it."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

SUB = 256                 # sub-pixel positions per pixel
GUARD = 16384.0           # |u|, |v| below this
MAX_SIZE = 4096


def project(verts, K) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """verts (V, 3), K (6,), both taken as float32 and widened -> u, v, z (V,) float64: u = ((K0 x + K1 y) + K2 z) / z"""
    p = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    k = np.asarray(K, np.float32).astype(np.float64).reshape(6)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        u = ((k[0] * x + k[1] * y) + k[2] * z) / z
        v = ((k[3] * x + k[4] * y) + k[5] * z) / z
    return u, v, z


def raster(meshes: Sequence[Optional[Tuple]], K, width: int, height: int, half_pixel: int = 0, near: float = 0.01):
    """ONE sample.  meshes = (hand, obj), each (verts (V, 3), faces (F, 3)) or None (the caller cuts the faces to n_faces rows)
    -> ids int32 (height, width) (-1: background, else mesh << 16 | face row), depth float32 (0: background), cover int32 = how many
    faces cover each sample point (whatever their depth), counts int32 (2,) = visible pixels per mesh"""
    W, H = int(width), int(height)
    near = float(np.float32(near))
    best_z = np.full((H, W), np.inf, np.float32)
    ids = np.full((H, W), -1, np.int32)
    cover = np.zeros((H, W), np.int32)
    off = SUB // 2 if half_pixel else 0
    for m, mesh in enumerate(meshes):
        if mesh is None:
            continue
        verts = np.asarray(mesh[0], np.float32).reshape(-1, 3)
        faces = np.asarray(mesh[1], np.int64).reshape(-1, 3)
        V = len(verts)
        u, v, z = project(verts, K)
        with np.errstate(all="ignore"):
            usable = np.isfinite(verts).all(1) & ~(z < near) & (np.abs(u) < GUARD) & (np.abs(v) < GUARD)
            X = np.where(usable, np.rint(SUB * u), 0).astype(np.int64)
            Y = np.where(usable, np.rint(SUB * v), 0).astype(np.int64)
            iz = 1.0 / z
        for fi, f in enumerate(faces):
            if (f < 0).any() or (f >= V).any() or not usable[f].all():
                continue
            xs, ys, zs = [int(X[i]) for i in f], [int(Y[i]) for i in f], [iz[i] for i in f]
            A2 = (xs[1] - xs[0]) * (ys[2] - ys[0]) - (xs[2] - xs[0]) * (ys[1] - ys[0])
            if A2 == 0:
                continue
            if A2 < 0:
                xs[1], xs[2], ys[1], ys[2], zs[1], zs[2], A2 = xs[2], xs[1], ys[2], ys[1], zs[2], zs[1], -A2
            # only pixels whose sample point lies in the corners' bounding box can be covered
            x0, x1 = max(-((off - min(xs)) // SUB), 0), min((max(xs) - off) // SUB, W - 1)
            y0, y1 = max(-((off - min(ys)) // SUB), 0), min((max(ys) - off) // SUB, H - 1)
            if x0 > x1 or y0 > y1:
                continue
            px = (np.arange(x0, x1 + 1, dtype=np.int64) * SUB + off)[None, :]
            py = (np.arange(y0, y1 + 1, dtype=np.int64) * SUB + off)[:, None]
            inside = np.ones((y1 - y0 + 1, x1 - x0 + 1), bool)
            E = []
            for i in range(3):
                a, b = (i + 1) % 3, (i + 2) % 3                                  # edge i, opposite corner i: from a to b
                dx, dy = xs[b] - xs[a], ys[b] - ys[a]
                e = dx * (py - ys[a]) - dy * (px - xs[a])
                on_edge_counts = dy < 0 or (dy == 0 and dx > 0)                  # a left edge or a top edge
                inside &= (e > 0) | ((e == 0) & on_edge_counts)
                E.append(e)
            if not inside.any():
                continue
            win = (slice(y0, y1 + 1), slice(x0, x1 + 1))
            cover[win] += inside
            lam = [E[i].astype(np.float64) / float(A2) for i in range(3)]
            invz = (lam[0] * zs[0] + lam[1] * zs[1]) + lam[2] * zs[2]
            with np.errstate(all="ignore"):
                zz = (1.0 / invz).astype(np.float32)
            better = inside & (zz < best_z[win])                                 # ascending keys: strictly nearer replaces
            best_z[win][better] = zz[better]
            ids[win][better] = m << 16 | fi
    depth = np.where(ids >= 0, best_z, np.float32(0)).astype(np.float32)
    counts = np.array([((ids >= 0) & (ids >> 16 == m)).sum() for m in (0, 1)], np.int32)
    return ids, depth, cover, counts


def fold_masks(ids, hm_w: int, hm_h: int) -> Tuple[np.ndarray, np.ndarray]:
    """ids (..., height, width) -> hand_seg, obj_seg float32 (..., hm_h, hm_w): mask pixel (i, j) reads raster pixel
    (floor((i + .5) width / hm_w), floor((j + .5) height / hm_h)), the NEAREST fold of hoisdf_image_crop"""
    ids = np.asarray(ids)
    H, W = ids.shape[-2:]
    if W % hm_w or H % hm_h:
        raise ValueError(f"fold_masks: {W} x {H} does not fold to {hm_w} x {hm_h}")
    xs = np.floor((np.arange(hm_w) + 0.5) * W / hm_w).astype(np.int64)
    ys = np.floor((np.arange(hm_h) + 0.5) * H / hm_h).astype(np.int64)
    sub = ids[..., ys[:, None], xs[None, :]]
    return tuple(((sub >= 0) & (sub >> 16 == m)).astype(np.float32) for m in (0, 1))


def overlay(ids, image, colour, alpha: int) -> np.ndarray:
    """ids (..., H, W), image uint8 (..., H, W, 3), colour uint8 (2, 3), alpha 0 .. 256 -> uint8: a covered pixel becomes
    (alpha colour[mesh][c] + (256 - alpha) in + 128) >> 8, a background pixel is copied"""
    ids = np.asarray(ids)
    img = np.asarray(image, np.uint8).astype(np.int64)
    col = np.asarray(colour, np.uint8).astype(np.int64).reshape(2, 3)
    mixed = (alpha * col[np.clip(ids >> 16, 0, 1)] + (256 - alpha) * img + 128) >> 8
    return np.where((ids >= 0)[..., None], mixed, img).astype(np.uint8)


def silhouette_counts(pred_hand, pred_obj, gt_hand, gt_obj) -> np.ndarray:
    """four masks (B, ...) floats, set where > 0.5 -> int32 (B, 4): hand intersection, hand union, object intersection, object union"""
    out = []
    for p, g in ((pred_hand, gt_hand), (pred_obj, gt_obj)):
        p = np.asarray(p).reshape(len(p), -1) > 0.5
        g = np.asarray(g).reshape(len(g), -1) > 0.5
        out += [(p & g).sum(1), (p | g).sum(1)]
    return np.stack(out, 1).astype(np.int32)


def raycast(meshes: Sequence[Optional[Tuple]], K, width: int, height: int, half_pixel: int = 0):
    """float64 ground truth by other means: one ray per pixel through the inverse camera matrix, Moeller-Trumbore against every
    triangle -> ids (height, width) (the nearest hit, -1: none), t float64 = its z, near_edge bool = the pixel's sample point lies
    within 1/256 pixel of a projected (unsnapped) edge - where snapping may legitimately decide otherwise"""
    W, H = int(width), int(height)
    k = np.asarray(K, np.float32).astype(np.float64).reshape(6)
    Minv = np.linalg.inv(np.array([[k[0], k[1], k[2]], [k[3], k[4], k[5]], [0, 0, 1]]))
    c = 0.5 if half_pixel else 0.0
    uu, vv = np.meshgrid(np.arange(W) + c, np.arange(H) + c)
    d = np.stack([uu, vv, np.ones_like(uu)], -1) @ Minv.T                      # ray directions with z = 1: t is the depth
    best = np.full((H, W), np.inf)
    ids = np.full((H, W), -1, np.int64)
    near_edge = np.zeros((H, W), bool)
    for m, mesh in enumerate(meshes):
        if mesh is None:
            continue
        verts = np.asarray(mesh[0], np.float32).astype(np.float64).reshape(-1, 3)
        faces = np.asarray(mesh[1], np.int64).reshape(-1, 3)
        u, v, _ = project(verts, K)
        for fi, (a, b, c_) in enumerate(faces):
            p0, e1, e2 = verts[a], verts[b] - verts[a], verts[c_] - verts[a]
            h = np.cross(d, e2)
            det = h @ e1
            with np.errstate(all="ignore"):
                inv = 1.0 / det
                s = -p0
                bu = (h @ s) * inv
                q = np.cross(s, e1)
                bv = (d @ q) * inv
                t = (e2 @ q) * inv
            hit = (np.abs(det) > 1e-18) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0)
            upd = hit & (t < best)
            best[upd] = t[upd]
            ids[upd] = m << 16 | fi
            for i, j in ((a, b), (b, c_), (c_, a)):
                ax, ay, dx, dy = u[i], v[i], u[j] - u[i], v[j] - v[i]
                tt = np.clip(((uu - ax) * dx + (vv - ay) * dy) / max(dx * dx + dy * dy, 1e-30), 0, 1)
                near_edge |= np.hypot(uu - (ax + tt * dx), vv - (ay + tt * dy)) < 1.0 / SUB
    return ids, best, near_edge


# ---- the closed-form scenes tests/test_raster_oracle.py and tests/test_gpu_raster.py share -------------------------------------------
def quad_case():
    """a quad at z = 1 split along its diagonal; with K = [64 0 24; 0 64 24] its corners project to 8 and 40: on pixel centres for
    half_pixel = 0 -> (verts, faces, K, width, height)"""
    v = np.array([[-0.25, -0.25, 1], [0.25, -0.25, 1], [0.25, 0.25, 1], [-0.25, 0.25, 1]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([64, 0, 24, 0, 64, 24], np.float32), 48, 48


def fan_case(n: int = 7):
    """n faces around a vertex that projects to the pixel centre (24, 24); the rim lies on a circle of 15.5 pixels, every second
    face wound the other way -> (verts, faces, K, width, height)"""
    ang = np.arange(n) * 2 * np.pi / n + 0.1
    rim = np.stack([15.5 / 64 * np.cos(ang), 15.5 / 64 * np.sin(ang), np.ones(n)], 1)
    v = np.concatenate([[[0.0, 0.0, 1.0]], rim]).astype(np.float32)
    f = np.array([[0, 1 + i, 1 + (i + 1) % n] if i % 2 == 0 else [0, 1 + (i + 1) % n, 1 + i] for i in range(n)], np.int32)
    return v, f, np.array([64, 0, 24, 0, 64, 24], np.float32), 48, 48


def plane_case():
    """the plane through (-+0.25, -0.25, 1) and (-+0.5, 0.5, 2): it covers every pixel of a 64 x 64 image under K = [128 0 32;
    0 128 32] with half_pixel = 1, and its depth is z = (4/3) / (1 - y' / 0.75), y' = (py + 0.5 - 32) / 128
    -> (verts, faces, K, width, height, depth (64,) float64 per pixel row)"""
    v = np.array([[-0.25, -0.25, 1], [0.25, -0.25, 1], [0.5, 0.5, 2], [-0.5, 0.5, 2]], np.float32)
    yy = (np.arange(64) + 0.5 - 32) / 128
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([128, 0, 32, 0, 128, 32], np.float32), 64, 64, (4 / 3) / (1 - yy / 0.75)


def sphere_torus_case(width: int, height: int, fx: float):
    """icosphere(2) x 0.045 at (0.012, -0.007, 0.503) as the hand (320 faces), a turned torus x 0.06 at (-0.021, 0.013, 0.531) as the
    object (384 faces), a camera with skew and an off-centre principal point -> ((hand verts, faces), (obj verts, faces)), K"""
    from .mesh_sdf_oracle import icosphere, torus
    v1, f1 = icosphere(2)
    v2, f2 = torus()
    R = np.array([[0.8, 0, 0.6], [0.36, 0.8, -0.48], [-0.48, 0.6, 0.64]])
    hand = (np.asarray(v1) * 0.045 + [0.012, -0.007, 0.503]).astype(np.float32)
    obj = (np.asarray(v2) @ R.T * 0.06 + [-0.021, 0.013, 0.531]).astype(np.float32)
    K = np.array([fx, 7.0, width / 2 - 3.3, -5.0, fx * 1.1, height / 2 + 1.7], np.float32)
    return ((hand, np.asarray(f1, np.int32)), (obj, np.asarray(f2, np.int32))), K
