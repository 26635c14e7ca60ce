"""numpy restatement of csrc/mesh_sdf.hip (include/hoisdf.h "mesh SDF"), in float64 or float32 on request: the yardstick of
tests/test_mesh_sdf_oracle.py and tests/test_gpu_mesh_sdf.py.  Same steps as the kernels - re-centre on the bounding-box centre of
the vertices, skip a face whose (unfused) normal is exactly zero or that names a vertex outside the mesh, the exact closest point
by Voronoi region, the Van Oosterom-Strackee solid angle, sign from the winding number, lowest face index / earliest corner on
ties - evaluated for all point x face pairs at once.  Not a fallback: nothing on the training path imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

PART_OF_JOINT = (0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)      # MANO joint -> palm + five fingers (num_class 6)


def vertex_part_labels(skin_weights) -> np.ndarray:
    """(V, 16) skinning weights -> (V,) int32 hand part of each vertex: the part of the joint that moves it most"""
    w = np.asarray(skin_weights)
    return np.asarray(PART_OF_JOINT, np.int32)[np.argmax(w, axis=1)]


def point_kind(i, uniform_every: int) -> np.ndarray:
    """kind of sample point i: 2 = uniform in the padded box (the last of every `uniform_every`; never for uniform_every <= 0),
    0 = near-surface with sigma1 (even place in its group), 1 = near-surface with sigma2 (odd place)"""
    i = np.asarray(i, np.int64)
    k = i % uniform_every if uniform_every > 0 else i
    return np.where((uniform_every > 0) & (k == uniform_every - 1), 2, k & 1).astype(np.int32)


def prepare(verts, faces, dtype=np.float64, recentre: bool = True) -> Dict[str, np.ndarray]:
    """one mesh: verts (V, 3), faces (F, 3) ints -> centre (3,), half (3,), tri (F, 3, 3) corners minus the centre, skipped (F,)
    bool, area (F,), cdf (F,)"""
    v = np.asarray(verts, dtype)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    lo, hi = (v.min(0), v.max(0)) if len(v) else (np.zeros(3, dtype), np.zeros(3, dtype))
    half_ = dtype(0.5)
    centre = (half_ * (lo + hi)).astype(dtype) if recentre else np.zeros(3, dtype)
    inside = np.all((f >= 0) & (f < len(v)), axis=1)
    tri = np.zeros((len(f), 3, 3), dtype)
    tri[inside] = v[f[inside]] - centre
    u, w = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
    skipped = ~inside | np.all(n == 0, axis=1)
    area = np.where(skipped, 0, half_ * np.sqrt((n * n).sum(1))).astype(dtype)
    return {"centre": centre, "half": (half_ * (hi - lo)).astype(dtype), "tri": tri, "skipped": skipped, "area": area,
            "cdf": np.cumsum(area, dtype=dtype), "faces": f}


def closest_point(p, a, b, c):
    """points p against triangles (a, b, c), broadcasting over leading axes (last axis = xyz) -> (v, w, d2): the closest point is
    (1 - v - w) a + v b + w c.  Regions in the kernel's order: the three corners, the three edges, the face."""
    dot = lambda x, y: (x * y).sum(-1)
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    ec, eb, ea = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    with np.errstate(divide="ignore", invalid="ignore"):
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        inv = 1 / (ea + eb + ec)
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6), (ec <= 0) & (d1 >= 0) & (d3 <= 0),
                 (eb <= 0) & (d2 >= 0) & (d6 <= 0), (ea <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        v = np.select(conds, [zero, one, zero, d1 / (d1 - d3), zero, 1 - w_bc], eb * inv)
        w = np.select(conds, [zero, zero, one, zero, d2 / (d2 - d6), w_bc], ec * inv)
    r = ap - v[..., None] * ab - w[..., None] * ac
    return v, w, dot(r, r)


def half_solid_angle(p, a, b, c):
    """atan2(det[a-p b-p c-p], ...): HALF the solid angle of the triangle seen from p (their sum / 2 pi = the winding number)"""
    dot = lambda x, y: (x * y).sum(-1)
    a, b, c = a - p, b - p, c - p
    la, lb, lc = np.sqrt(dot(a, a)), np.sqrt(dot(b, b)), np.sqrt(dot(c, c))
    det = dot(a, np.cross(b, c))
    return np.arctan2(det, la * lb * lc + dot(a, b) * lc + dot(b, c) * la + dot(c, a) * lb)


def mesh_sdf(points, verts, faces, vert_label=None, dtype=np.float64, recentre: bool = True, chunk: int = 512,
             label_sets: bool = False, face_tol: float = 1e-6, corner_tol: float = 1e-3) -> Dict[str, np.ndarray]:
    """points (N, 3) against one mesh -> dist (N,) unsigned, winding (N,), sdf (N,), face (N,) (-1: no usable face), bary (N, 3);
    with vert_label: label (N,), and with label_sets a list of N sets: the labels of every corner within corner_tol of the largest
    weight, over every face within face_tol of the minimum distance (the labels a correct fp32 evaluation may return).
    All point x face pairs of `chunk` points at a time."""
    m = prepare(verts, faces, dtype, recentre)
    use = np.flatnonzero(~m["skipped"])
    tri = m["tri"][use]
    P = np.asarray(points, dtype).reshape(-1, 3) - m["centre"]
    N = len(P)
    out = {"dist": np.full(N, 3.0e38, dtype), "winding": np.zeros(N, dtype), "face": np.full(N, -1, np.int64), "bary": np.zeros((N, 3), dtype)}
    sets = [set() for _ in range(N)] if label_sets else None
    lab = None if vert_label is None else np.asarray(vert_label, np.int64)
    for s in range(0, N, chunk):
        if not len(use):
            break
        p = P[s:s + chunk, None, :]
        v, w, d2 = closest_point(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        d2 = np.where(np.isnan(d2), np.inf, d2)
        j = np.argmin(d2, axis=1)                                    # the first minimum = the lowest face index
        r = np.arange(len(j))
        out["dist"][s:s + chunk] = np.sqrt(d2[r, j])
        out["face"][s:s + chunk] = use[j]
        out["bary"][s:s + chunk] = np.stack([1 - v[r, j] - w[r, j], v[r, j], w[r, j]], 1)
        out["winding"][s:s + chunk] = half_solid_angle(p, tri[None, :, 0], tri[None, :, 1], tri[None, :, 2]).sum(1, dtype=dtype) / (2 * np.pi)
        if sets is not None and lab is not None:
            d = np.sqrt(d2)
            near = d <= d[r, j][:, None] + face_tol
            bary = np.stack([1 - v - w, v, w], -1)
            top = bary >= bary.max(-1, keepdims=True) - corner_tol
            for pi, fi in zip(*np.nonzero(near)):
                sets[s + pi].update(lab[m["faces"][use[fi]][top[pi, fi]]].tolist())
    out["sdf"] = np.where(out["winding"] > 0.5, -out["dist"], out["dist"])
    if lab is not None:
        corner = np.argmax(out["bary"], axis=1)                      # the earliest corner on equal weights
        out["label"] = np.where(out["face"] >= 0, lab[m["faces"][np.maximum(out["face"], 0), corner]], -1)
        if sets is not None:
            out["label_sets"] = sets
    return out


def distance_to_face(points, verts, faces, face_ids, dtype=np.float64) -> np.ndarray:
    """(N,) distance of point i to the ONE triangle face_ids[i]"""
    v = np.asarray(verts, dtype)
    f = np.asarray(faces, np.int64).reshape(-1, 3)[np.asarray(face_ids, np.int64)]
    _, _, d2 = closest_point(np.asarray(points, dtype).reshape(-1, 3), v[f[:, 0]], v[f[:, 1]], v[f[:, 2]])
    return np.sqrt(d2)


def sdf_rows(hand_points, obj_points, hand_verts, hand_faces, obj_verts, obj_faces, hand_vert_label, clamp: float,
             dtype=np.float64) -> np.ndarray:
    """the row block of ONE sample as hoisdf_mesh_sdf_rows lays it out, for given points: (n_hand + n_obj, 6)"""
    pts = np.concatenate([np.asarray(hand_points, dtype).reshape(-1, 3), np.asarray(obj_points, dtype).reshape(-1, 3)], 0)
    nh = len(np.asarray(hand_points).reshape(-1, 3))
    h = mesh_sdf(pts, hand_verts, hand_faces, hand_vert_label, dtype)
    o = mesh_sdf(pts, obj_verts, obj_faces, None, dtype)
    label = np.where((np.arange(len(pts)) < nh) & (np.abs(h["sdf"]) <= clamp), h["label"], -1)
    return np.concatenate([pts, h["sdf"][:, None], o["sdf"][:, None], label[:, None].astype(dtype)], 1)


# ---- procedural meshes (outward winding) ------------------------------------------------------------------------------------------
def icosphere(subdivisions: int = 2):
    """unit icosphere: 12 / 42 / 162 vertices and 20 / 80 / 320 faces at 0 / 1 / 2 subdivisions -> verts (V, 3) f64, faces (F, 3) i32"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.stack(v), np.asarray(f, np.int32)


def torus(nu: int = 16, nv: int = 12, R: float = 0.7, r: float = 0.3):
    """torus around the z axis: nu x nv quads split in two -> verts (nu nv, 3) f64, faces (2 nu nv, 3) i32"""
    u = np.arange(nu) * 2 * np.pi / nu
    w = np.arange(nv) * 2 * np.pi / nv
    uu, ww = np.meshgrid(u, w, indexing="ij")
    verts = np.stack([(R + r * np.cos(ww)) * np.cos(uu), (R + r * np.cos(ww)) * np.sin(uu), r * np.sin(ww)], -1).reshape(-1, 3)
    faces = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            faces += [(a, b, c), (a, c, d)]
    return verts, np.asarray(faces, np.int32)


def box(hx: float = 1.0, hy: float = 0.7, hz: float = 0.5, n: int = 4):
    """closed box with n x n quads per side, every quad split in two (12 n^2 faces); vertices are not shared between sides"""
    verts, faces = [], []
    g = np.linspace(-1, 1, n + 1)
    for axis in range(3):
        for sgn in (-1.0, 1.0):
            a1, a2 = (axis + 1) % 3, (axis + 2) % 3
            base = len(verts)
            for i in range(n + 1):
                for j in range(n + 1):
                    p = np.zeros(3)
                    p[axis], p[a1], p[a2] = sgn, g[i], g[j]
                    verts.append(p * (hx, hy, hz))
            for i in range(n):
                for j in range(n):
                    a, b = base + i * (n + 1) + j, base + (i + 1) * (n + 1) + j
                    c, d = base + (i + 1) * (n + 1) + j + 1, base + i * (n + 1) + j + 1
                    faces += [(a, b, c), (a, c, d)] if sgn > 0 else [(a, c, b), (a, d, c)]
    return np.stack(verts), np.asarray(faces, np.int32)
