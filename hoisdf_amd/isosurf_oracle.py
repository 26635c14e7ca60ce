"""numpy restatement of the iso-surface rules of include/hoisdf.h ("iso-surface") and of hoisdf_eval_surface: the yardstick of
tests/test_isosurf_oracle.py and tests/test_gpu_isosurf.py.  It follows the rules as the header states them - the grid, the refined
grid, marching tetrahedra on the Kuhn subdivision with edge-owned vertices - with whole-array numpy instead of scans.  In float32
every operation whose order the header fixes is one float32 operation in that order, so indices, counts and vertex bits can be
compared exactly with csrc/isosurf.hip; float64 is the same text at higher precision, the ground truth of the float32 mode.  Not a
fallback: nothing on the model's path imports it."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np

MAX_GRID = 128
# the 7 edges a node owns, p -> p + d, as (dx, dy, dz), in the header's order
EDGE_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
# tetrahedron k of a cell: corners 000, e_a, e_a + e_b, 111 for the k-th permutation (a, b, c) of the axes in lexicographic order
TET_PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
TET_ODD = (False, True, True, False, False, True)                    # an odd permutation mirrors the tetrahedron
TET_EDGES = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))        # edge e of a tetrahedron joins these two of its corners
# case = sum of 2^k over the inside corners k -> triangles as tetrahedron edges, wound for an EVEN tetrahedron (an odd one swaps the
# last two).  Two inside corners i < j, outside k < l: the quad ik, il, jl, jk cut along ik - jl.
CASE_TRIS = ((), ((0, 1, 2),), ((0, 4, 3),), ((1, 2, 4), (1, 4, 3)), ((1, 3, 5),), ((0, 5, 2), (0, 3, 5)), ((0, 4, 5), (0, 5, 1)),
             ((2, 4, 5),), ((2, 5, 4),), ((0, 1, 5), (0, 5, 4)), ((0, 5, 3), (0, 2, 5)), ((1, 5, 3),), ((1, 3, 4), (1, 4, 2)),
             ((0, 3, 4),), ((0, 2, 1),), ())


def _tet_corners() -> np.ndarray:
    """(6, 4, 3) corner offsets (dx, dy, dz) of the six tetrahedra"""
    out = np.zeros((6, 4, 3), np.int64)
    for k, (a, b, _c) in enumerate(TET_PERMS):
        out[k, 1, a] = 1
        out[k, 2, a] = out[k, 2, b] = 1
        out[k, 3] = 1
    return out


def grid_points(grid, n: int, dtype=np.float32) -> np.ndarray:
    """grid (8,) = lo xyz, cell xyz, 0, 0 -> (n^3, 3): node i = ix + n (iy + n iz) at lo + ix cell (product, then sum)"""
    g = np.asarray(grid, np.float32).astype(dtype)
    idx = np.arange(n, dtype=dtype)
    ax = [(g[k] + (idx * g[3 + k]).astype(dtype)).astype(dtype) for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def refine_grid(values, grid, n: int, iso: float, pad_cells: int, n_out: int, dtype=np.float32) -> np.ndarray:
    """the n_out-node grid over the index box of the nodes with value < iso, grown by pad_cells and clipped; no such node: the whole
    coarse grid.  -> (8,)"""
    g = np.asarray(grid, np.float32).astype(dtype)
    v = np.asarray(values, np.float32).reshape(n, n, n)
    inside = v < np.float32(iso)
    out = np.zeros(8, dtype)
    for k in range(3):                                               # axis k of xyz is axis 2 - k of the [iz][iy][ix] array
        hit = np.flatnonzero(inside.any(axis=tuple(a for a in range(3) if a != 2 - k)))
        i0, i1 = (max(int(hit[0]) - pad_cells, 0), min(int(hit[-1]) + pad_cells, n - 1)) if len(hit) else (0, n - 1)
        lo = dtype(g[k] + dtype(dtype(i0) * g[3 + k]))
        hi = dtype(g[k] + dtype(dtype(i1) * g[3 + k]))
        out[k] = lo
        out[3 + k] = dtype(dtype(hi - lo) / dtype(n_out - 1))
    return out


def extract(values, grid, n: int, iso: float = 0.0, dtype=np.float32, out_scale: Optional[float] = None,
            out_shift=None) -> Tuple[np.ndarray, np.ndarray]:
    """one sample: values (n^3,) float32, grid (8,) -> verts (V, 3) dtype, faces (F, 3) int32, in the header's order"""
    val32 = np.asarray(values, np.float32).reshape(n, n, n)          # [iz][iy][ix]
    iso32 = np.float32(iso)
    inside = val32 < iso32                                           # strict; NaN is outside
    finite = np.isfinite(val32)
    val = val32.astype(dtype)
    N = n * n * n
    node = np.arange(N).reshape(n, n, n)
    iz, iy, ix = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")

    def shifted(a, d, fill):
        """a at p + d where that node exists, else fill"""
        out = np.full(a.shape, fill, a.dtype)
        out[:n - d[2], :n - d[1], :n - d[0]] = a[d[2]:, d[1]:, d[0]:]
        return out

    exists = [shifted(np.ones((n, n, n), bool), d, False) for d in EDGE_DIRS]
    active = np.stack([exists[e] & finite & shifted(finite, d, False) & (inside != shifted(inside, d, False))
                       for e, d in enumerate(EDGE_DIRS)], -1).reshape(N, 7)
    count = active.sum(1)
    prefix = np.cumsum(count) - count
    vid = prefix[:, None] + np.cumsum(active, 1) - active             # id of edge e of node p where active
    # ---- vertices: ascending node, then ascending edge = the row-major order of `active`
    p_idx, e_idx = np.nonzero(active)
    d = np.asarray(EDGE_DIRS, np.int64)[e_idx]
    pc = np.stack([ix.ravel()[p_idx], iy.ravel()[p_idx], iz.ravel()[p_idx]], 1)
    qc = pc + d
    vp = val.ravel()[p_idx]
    vq = val[qc[:, 2], qc[:, 1], qc[:, 0]]
    p_in = inside.ravel()[p_idx]
    va, vb = np.where(p_in, vp, vq), np.where(p_in, vq, vp)           # a = the inside end, b = the outside end
    ca, cb = np.where(p_in[:, None], pc, qc), np.where(p_in[:, None], qc, pc)
    g = np.asarray(grid, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        t = ((dtype(iso32) - va).astype(dtype) / (vb - va).astype(dtype)).astype(dtype)
        xa = (g[:3] + (ca.astype(dtype) * g[3:6]).astype(dtype)).astype(dtype)
        xb = (g[:3] + (cb.astype(dtype) * g[3:6]).astype(dtype)).astype(dtype)
        verts = (xa + (t[:, None] * (xb - xa).astype(dtype)).astype(dtype)).astype(dtype)
        if out_shift is not None:
            s = dtype(np.float32(1.0 if out_scale is None else out_scale))
            verts = ((verts * s).astype(dtype) + np.asarray(out_shift, np.float32).astype(dtype)).astype(dtype)
    # ---- faces: ascending cell, tetrahedron 0..5, the table's triangles
    m = n - 1
    if m < 1:
        return verts, np.zeros((0, 3), np.int32)
    tc = _tet_corners()
    cell_ok = np.ones((m, m, m), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cell_ok &= finite[dz:dz + m, dy:dy + m, dx:dx + m]
    base = node[:m, :m, :m]
    edge_no = {dd: e for e, dd in enumerate(EDGE_DIRS)}
    case = np.zeros((m, m, m, 6), np.int64)
    tet_vid = np.zeros((m, m, m, 6, 6), np.int64)
    for k in range(6):
        for c in range(4):
            o = tc[k, c]
            case[..., k] |= inside[o[2]:o[2] + m, o[1]:o[1] + m, o[0]:o[0] + m].astype(np.int64) << c
        for e, (i, j) in enumerate(TET_EDGES):
            o = tc[k, i]
            en = edge_no[tuple(int(x) for x in tc[k, j] - o)]
            tet_vid[..., k, e] = vid[base + (o[0] + n * (o[1] + n * o[2])), en]
    case[~cell_ok] = 0
    tri = np.zeros((16, 2, 3), np.int64)
    ntri = np.zeros(16, np.int64)
    for c, ts in enumerate(CASE_TRIS):
        ntri[c] = len(ts)
        for s, tr in enumerate(ts):
            tri[c, s] = tr
    te = tri[case]                                                   # (m, m, m, 6, 2, 3) tetrahedron edges
    odd = np.asarray(TET_ODD)[None, None, None, :, None]
    te = np.where(odd[..., None], te[..., [0, 2, 1]], te)
    fv = np.take_along_axis(tet_vid[..., None, :].repeat(2, axis=-2), te, axis=-1)
    keep = np.arange(2)[None, None, None, None, :] < ntri[case][..., None]
    return verts, fv[keep].astype(np.int32)


def mesh_report(verts, faces) -> Dict[str, object]:
    """topology and volume of an indexed triangle mesh (float64): V, E, F, euler, closed (every undirected edge in exactly two faces),
    oriented (every directed edge once), boundary (the undirected edges in one face only, (k, 2)), volume (divergence theorem)"""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    de = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0)
    ue, cnt = np.unique(np.sort(de, 1), axis=0, return_counts=True) if len(de) else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    _, dcnt = np.unique(de, axis=0, return_counts=True) if len(de) else (None, np.zeros(0, np.int64))
    used = len(np.unique(f))
    a, b, c = (v[f[:, k]] for k in range(3)) if len(f) else (np.zeros((0, 3)),) * 3
    return {"V": used, "E": len(ue), "F": len(f), "euler": used - len(ue) + len(f), "closed": bool(np.all(cnt == 2)),
            "oriented": bool(np.all(dcnt == 1)), "boundary": ue[cnt == 1],
            "volume": float((a * np.cross(b, c)).sum() / 6.0)}


def point_triangle_d2(p, a, b, c) -> np.ndarray:
    """squared distance of points p (N, 1, 3) to triangles (1, F, 3) each, float64, by projecting on the plane and clamping to the
    three edges - a different route from the kernel's Voronoi regions"""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))

    def seg(p, u, w):
        d = w - u
        t = np.clip(((p - u) * d).sum(-1) / np.maximum((d * d).sum(-1), 1e-300), 0, 1)
        r = p - (u + t[..., None] * d)
        return (r * r).sum(-1)

    nrm = np.cross(b - a, c - a)
    nn = np.maximum((nrm * nrm).sum(-1), 1e-300)
    dist = ((p - a) * nrm).sum(-1)
    q = p - (dist / nn)[..., None] * nrm
    inside = ((np.cross(b - a, q - a) * nrm).sum(-1) >= 0) & ((np.cross(c - b, q - b) * nrm).sum(-1) >= 0) & \
             ((np.cross(a - c, q - c) * nrm).sum(-1) >= 0)
    edge = np.minimum(np.minimum(seg(p, a, b), seg(p, b, c)), seg(p, c, a))
    return np.where(inside, dist * dist / nn, edge)


def eval_surface(pred_verts, gt_verts, gt_faces, samples) -> Dict[str, float]:
    """one sample, float64 brute force: pred_verts (k, 3) (the sample's own count), the ground-truth mesh, the points drawn on its
    surface (n_samples, 3) -> pred_to_gt, gt_to_pred, chamfer, n_used.  Faces whose normal is exactly zero take no part."""
    pv = np.asarray(pred_verts, np.float64).reshape(-1, 3)
    gv = np.asarray(gt_verts, np.float64)
    f = np.asarray(gt_faces, np.int64).reshape(-1, 3)
    a, b, c = gv[f[:, 0]], gv[f[:, 1]], gv[f[:, 2]]
    use = np.any(np.cross(b - a, c - a) != 0, axis=1) if len(f) else np.zeros(0, bool)
    if len(pv) == 0 or not use.any():
        return {"pred_to_gt": 0.0, "gt_to_pred": 0.0, "chamfer": 0.0, "n_used": 0}
    d2 = point_triangle_d2(pv[:, None, :], a[None, use], b[None, use], c[None, use]).min(1)
    s = np.asarray(samples, np.float64).reshape(-1, 3)
    nn = ((s[:, None, :] - pv[None, :, :]) ** 2).sum(-1).min(1)
    p2g, g2p = float(d2.mean()), float(nn.mean())
    return {"pred_to_gt": p2g, "gt_to_pred": g2p, "chamfer": p2g + g2p, "n_used": len(pv)}


# ---- analytic fields of the tests ------------------------------------------------------------------------------------------------
def cube_grid(lo: float, hi: float, n: int) -> np.ndarray:
    """the (8,) grid of n nodes per axis over [lo, hi]^3"""
    c = (np.float32(hi) - np.float32(lo)) / np.float32(n - 1)
    return np.array([lo, lo, lo, c, c, c, 0, 0], np.float32)


def sphere_field(points, centre=(0.0, 0.0, 0.0), r: float = 0.3) -> np.ndarray:
    p = np.asarray(points, np.float64) - np.asarray(centre, np.float64)
    return (np.sqrt((p * p).sum(1)) - r).astype(np.float32)


def torus_field(points, R: float = 0.29, r: float = 0.117) -> np.ndarray:
    """around the z axis; the defaults keep every node of the 9- and 17-node grids over [-0.5, 0.5]^3 more than 3e-3 from the level"""
    p = np.asarray(points, np.float64)
    q = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2) - R
    return (np.sqrt(q * q + p[:, 2] ** 2) - r).astype(np.float32)
