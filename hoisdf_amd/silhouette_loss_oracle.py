"""numpy restatement of csrc/silhouette_loss.hip (include/hoisdf.h "silhouette loss"): the exact squared Euclidean distance transform
of a mask and the two silhouette terms of one projected point set - its vertices pulled into the allowed region (the bilinear read
of the distance map) and the pixels of its own mask pulled under a projected vertex (nearest vertex per set pixel) - with the
gradient towards the vertices; the yardstick of tests/test_silhouette_loss_oracle.py and tests/test_gpu_silhouette_loss.py.
Integers and float64 throughout, the two sums in the kernels' order.  Not a fallback: nothing on the training path imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

EDT_NONE = 1 << 30                                             # HOISDF_EDT_NONE = (2^15)^2: no set pixel


def _set(mask, mask_or=None) -> np.ndarray:
    m = np.asarray(mask) > 0.5
    return m if mask_or is None else m | (np.asarray(mask_or) > 0.5)


def edt(mask, mask_or=None):
    """ONE sample: mask (h, w), a value > 0.5 is set, mask_or likewise (the set is their union) -> d2 (h, w) int32: the squared
    distance to the nearest set pixel (EDT_NONE everywhere without one), nearest (h, w) int32: y' w + x' of a nearest set pixel, the
    lowest index on an exact tie (-1 without one).  The kernel's two passes: per column the nearest set row (the upper one on a tie),
    then per row the minimum over the columns of the key (distance, y', x')."""
    m = _set(mask, mask_or)
    h, w = m.shape
    ys, xs = np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64)
    # pass 1: row[y][x] = the set row of column x nearest to y (-1: the column has none)
    dist = np.where(m[None, :, :], np.abs(ys[:, None, None] - ys[None, :, None]), 1 << 15)      # [y][y'][x]
    row = dist.argmin(1)                                       # the first minimum: the lower y' on a tie
    g = dist.min(1)
    row = np.where(g < (1 << 15), row, -1)
    # pass 2: per pixel the smallest key over the columns x'
    d = np.minimum(g[:, None, :] ** 2 + (xs[:, None] - xs[None, :]) ** 2, EDT_NONE)             # [y][x][x']
    key = (d << 32) | (np.maximum(row, 0)[:, None, :] << 16) | xs[None, None, :]
    key = np.where(row[:, None, :] >= 0, key, np.int64(EDT_NONE) << 32 | 0xFFFFFFFF)
    best = key.min(2)
    d2 = (best >> 32).astype(np.int32)
    nearest = np.where(d2 < EDT_NONE, ((best >> 16) & 0xFFFF) * w + (best & 0xFFFF), -1).astype(np.int32)
    return d2, nearest


def edt_brute(mask, mask_or=None):
    """the definition, all pairs: (d2, nearest) as ``edt`` returns them"""
    m = _set(mask, mask_or)
    h, w = m.shape
    sy, sx = np.nonzero(m)                                     # ascending y' w + x'
    if not len(sy):
        return np.full((h, w), EDT_NONE, np.int32), np.full((h, w), -1, np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    d = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2
    k = d.argmin(-1)                                           # the first minimum: the lowest index
    return d.min(-1).astype(np.int32), (sy[k] * w + sx[k]).astype(np.int32)


def ordered_sum(terms) -> float:
    """the kernels' sum: thread t of 256 adds elements t, t + 256, ... in ascending order, then s[t] += s[t + 128], s[t + 64], ..."""
    t = np.asarray(terms, np.float64).reshape(-1)
    pad = np.zeros((len(t) + 255) // 256 * 256)
    pad[:len(t)] = t
    s = np.zeros(256)
    for r in pad.reshape(-1, 256):
        s = s + r
    o = 128
    while o > 0:
        s[:o] = s[:o] + s[o:2 * o]
        o >>= 1
    return float(s[0])


def project(verts, n_verts, K, near: float):
    """-> u, v (V,) float64 and valid (V,) bool"""
    P = np.asarray(verts, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(6)
    n = len(P) if n_verts is None else min(max(int(n_verts), 0), len(P))
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    with np.errstate(all="ignore"):
        u = ((K[0] * x + K[1] * y) + K[2] * z) / z
        v = ((K[3] * x + K[4] * y) + K[5] * z) / z
        valid = np.isfinite(P).all(1) & ~(z < np.float64(np.float32(near))) &(np.arange(len(P)) < n) & np.isfinite(u) & np.isfinite(v)
    return u, v, valid, n


def silhouette_loss(verts, n_verts, K, d2, cover, w=None, near: float = 0.01, g_inside: float = 1.0, g_cover: float = 1.0) -> Dict[str, object]:
    """ONE sample: verts (V, 3) camera frame, metres (rows from n_verts on are padding), K (6,) for the mask grid, d2 (h, w) of
    ``edt`` (the allowed region), cover (h, w) (the point set's own mask), w (V,) weights or None = ones ->
      inside, cover (float64), nearest (h, w) int32: the nearest valid vertex of every set pixel of cover (-1: unset, or no valid
      vertex), cell (V, 2) int32 = (x0, y0) of the bilinear read (-1, -1: an invalid vertex), valid (V,), u, v (V,),
      d_verts (V, 3) = the gradient of g_inside inside + g_cover cover, abs_terms (V, 3): per coordinate the sum of the absolute
      values of the terms added into it (the scale of its rounding and of a finite difference's curvature)."""
    P = np.asarray(verts, np.float64).reshape(-1, 3)
    K = np.asarray(K, np.float64).reshape(6)
    d2 = np.asarray(d2, np.int64)
    cov = np.asarray(cover) > 0.5
    h, wd = d2.shape
    V = len(P)
    wt = np.ones(V) if w is None else np.asarray(w, np.float64).reshape(-1)
    assert wt.shape == (V,) and cov.shape == (h, wd)
    u, v, valid, n = project(P, n_verts, K, near)
    us, vs = np.where(valid, u, 0.0), np.where(valid, v, 0.0)
    # ---- inside: the bilinear read of sqrt(d2) at the clamped projection, plus the distance back onto the map
    uc, vc = np.clip(us, 0, wd - 1), np.clip(vs, 0, h - 1)
    x0 = np.minimum(np.floor(uc), max(wd - 2, 0)).astype(np.int64)
    y0 = np.minimum(np.floor(vc), max(h - 2, 0)).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, wd - 1), np.minimum(y0 + 1, h - 1)
    fx = uc - x0 if wd > 1 else np.zeros(V)
    fy = vc - y0 if h > 1 else np.zeros(V)
    c00, c10, c01, c11 = d2[y0, x0], d2[y0, x1], d2[y1, x0], d2[y1, x1]
    d00, d10, d01, d11 = (np.sqrt(c.astype(np.float64)) for c in (c00, c10, c01, c11))
    val = ((1 - fx) * (1 - fy) * d00 + fx * (1 - fy) * d10) + ((1 - fx) * fy * d01 + fx * fy * d11)
    ou, ov = us - uc, vs - vc
    out = np.sqrt(ou * ou + ov * ov)
    use = valid & (c00 < EDT_NONE) & (c10 < EDT_NONE) & (c01 < EDT_NONE) & (c11 < EDT_NONE)
    den = ordered_sum(np.where(np.arange(V) < n, wt, 0.0))
    inside = ordered_sum(np.where(use, wt * (val + out), 0.0)) / den if den > 0 else 0.0
    coef = np.where(use & (den > 0), g_inside * wt / (den if den > 0 else 1.0), 0.0)
    with np.errstate(all="ignore"):
        tu = np.where(ou == 0, (1 - fy) * (d10 - d00) + fy * (d11 - d01), 0.0) + np.where(out > 0, ou / np.where(out > 0, out, 1), 0.0)
        tv = np.where(ov == 0, (1 - fx) * (d01 - d00) + fx * (d11 - d10), 0.0) + np.where(out > 0, ov / np.where(out > 0, out, 1), 0.0)
    if wd == 1:
        tu = np.where(out > 0, ou / np.where(out > 0, out, 1), 0.0)
    if h == 1:
        tv = np.where(out > 0, ov / np.where(out > 0, out, 1), 0.0)
    acc_u, acc_v = coef * tu, coef * tv
    abs_u, abs_v = np.abs(acc_u), np.abs(acc_v)
    # ---- cover: every set pixel to its nearest valid vertex
    nearest = np.full((h, wd), -1, np.int32)
    cover_val = 0.0
    idx = np.nonzero(valid)[0]
    py, px = np.nonzero(cov)                                   # ascending pixel index
    if len(idx) and len(py):
        du = px[:, None].astype(np.float64) - u[idx][None, :]
        dv = py[:, None].astype(np.float64) - v[idx][None, :]
        dd = du * du + dv * dv
        k = dd.argmin(1)                                       # the first minimum: the lowest vertex index
        nearest[py, px] = idx[k]
        ddp = dd[np.arange(len(py)), k]
        dist = np.zeros((h, wd))
        dist[py, px] = np.sqrt(ddp)
        cover_val = ordered_sum(dist) / len(py)
        c = g_cover / len(py)
        nz = ddp > 0                                           # a pixel on its vertex has no direction
        i, s = idx[k[nz]], np.sqrt(ddp[nz])
        gu, gv = c * (u[i] - px[nz]) / s, c * (v[i] - py[nz]) / s
        for acc, g in ((acc_u, gu), (acc_v, gv), (abs_u, np.abs(gu)), (abs_v, np.abs(gv))):
            np.add.at(acc, i, g)                               # unbuffered: ascending pixel index, as the owning lane adds them
    # ---- the chain rule: du/dx = K0 / z, du/dy = K1 / z, du/dz = (K2 - u) / z, likewise v
    z = np.where(valid, P[:, 2], 1.0)
    Ju = np.stack([K[0] / z, K[1] / z, (K[2] - us) / z], 1)
    Jv = np.stack([K[3] / z, K[4] / z, (K[5] - vs) / z], 1)
    d_verts = np.where(valid[:, None], acc_u[:, None] * Ju + acc_v[:, None] * Jv, 0.0)
    abs_terms = np.where(valid[:, None], abs_u[:, None] * np.abs(Ju) + abs_v[:, None] * np.abs(Jv), 0.0)
    cell = np.where(valid[:, None], np.stack([x0, y0], 1), -1).astype(np.int32)
    return {"inside": float(inside), "cover": float(cover_val), "nearest": nearest, "cell": cell, "valid": valid, "u": u, "v": v,
            "d_verts": d_verts, "abs_terms": abs_terms, "use": use}
