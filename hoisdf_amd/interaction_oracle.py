"""numpy restatement of csrc/interact.hip (include/hoisdf.h "interaction"): penetration depth, contact and intersection volume of a
posed hand mesh and a posed object mesh; the yardstick of tests/test_interaction_oracle.py and tests/test_gpu_interaction.py.
Distance, sign and winding number are mesh_sdf_oracle.mesh_sdf's, in float64.  The GRID is taken in float32, operation by operation
in the kernel's order (``grid``), so that oracle and kernel evaluate the very same cell centres; what is decided at a centre or at
a vertex is decided in float64, and the float64 distances and winding numbers are returned with the answers, for the tests' rules
on what lies too close to a surface to be compared.  Not a fallback: nothing on the evaluation path imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from .mesh_sdf_oracle import mesh_sdf

MAX_GRID = 64                                                  # HOISDF_INTERACT_MAX_GRID
_F = np.float32


def _box(verts):
    """centre and half extent as mesh_prepare_kernel leaves them in box[]: fp32, from the fp32 vertices"""
    v = np.asarray(verts, _F).reshape(-1, 3)
    m, M = v.min(0), v.max(0)
    return _F(0.5) * (m + M), _F(0.5) * (M - m)


def grid(hand_verts, obj_verts, voxel: float, max_grid: int = MAX_GRID) -> Dict[str, np.ndarray]:
    """the cells of one sample -> lo (3,) f32, cell (3,) f32, n (3,) int.  The header's grid rule, every operation in fp32 and in
    its order: lo = max(c_h - h_h, c_o - h_o), hi = min(c_h + h_h, c_o + h_o), extent = hi - lo, n = min(ceil(extent / voxel),
    max_grid) (at least 1), cell = extent / n; an extent <= 0 on any axis: n = 0 everywhere.  Every row of both vertex arrays counts
    for the boxes, padding rows too."""
    ch, hh = _box(hand_verts)
    co, ho = _box(obj_verts)
    lo, hi = np.maximum(ch - hh, co - ho), np.minimum(ch + hh, co + ho)
    ext = hi - lo
    if not np.all(ext > 0):
        return {"lo": lo, "cell": np.zeros(3, _F), "n": np.zeros(3, np.int64)}
    n = np.maximum(1, np.minimum(np.ceil(ext / _F(voxel)), _F(max_grid))).astype(np.int64)
    return {"lo": lo, "cell": ext / n.astype(_F), "n": n}


def centres(g) -> np.ndarray:
    """(n_x n_y n_z, 3) f32 cell centres, ix fastest: lo + (ix + 0.5) cell, the product rounded before the sum"""
    nx, ny, nz = (int(k) for k in g["n"])
    i = np.arange(nx * ny * nz)
    if not len(i):
        return np.zeros((0, 3), _F)
    idx = np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], 1).astype(_F)
    return (g["lo"] + ((idx + _F(0.5)) * g["cell"]).astype(_F)).astype(_F)


def pack_n(n) -> int:
    """grid_out[6]: n_x | n_y << 8 | n_z << 16"""
    return int(n[0]) | int(n[1]) << 8 | int(n[2]) << 16


def eval_interaction(hand_verts, hand_faces, obj_verts, obj_faces, obj_n_verts: Optional[int] = None, contact_dist: float = 0.005,
                     voxel: float = 0.005) -> Dict[str, object]:
    """ONE sample: hand_verts (Vh, 3), hand_faces (Fh, 3), obj_verts (Vo, 3) (rows from obj_n_verts on are padding), obj_faces
    (Fo, 3): only the faces that count ->
      pen_hand, pen_obj, min_dist (float64), contact_verts, in_contact, inside_count (int), volume (float32: ((count cell_x)
      cell_y) cell_z), inside (n cells,) bool, grid (``grid``), centres (n cells, 3) f32,
      hand_vert / obj_vert: mesh_sdf of the hand vertices against the object / of the object vertices that count against the hand,
      vox_obj / vox_hand: mesh_sdf of the cell centres against each mesh (dist, winding, sdf in float64)."""
    hv, ov = np.asarray(hand_verts, _F).reshape(-1, 3), np.asarray(obj_verts, _F).reshape(-1, 3)
    nvo = len(ov) if obj_n_verts is None else min(max(int(obj_n_verts), 0), len(ov))
    hand_vert = mesh_sdf(hv, ov, obj_faces)
    obj_vert = mesh_sdf(ov[:nvo], hv, hand_faces)
    g = grid(hv, ov, voxel)
    c = centres(g)
    vox_obj, vox_hand = mesh_sdf(c, ov, obj_faces), mesh_sdf(c, hv, hand_faces)
    inside = (vox_obj["winding"] > 0.5) & (vox_hand["winding"] > 0.5)
    count = int(inside.sum())
    pen_obj = float(np.maximum(0, -obj_vert["sdf"]).max()) if nvo else 0.0
    contact_verts = int((hand_vert["sdf"] <= contact_dist).sum())
    return {"pen_hand": float(np.maximum(0, -hand_vert["sdf"]).max()), "pen_obj": pen_obj, "min_dist": float(hand_vert["dist"].min()),
            "contact_verts": contact_verts, "in_contact": int(contact_verts > 0 or pen_obj > 0), "inside_count": count,
            "volume": _F(count) * g["cell"][0] * g["cell"][1] * g["cell"][2], "inside": inside, "grid": g, "centres": c,
            "hand_vert": hand_vert, "obj_vert": obj_vert, "vox_obj": vox_obj, "vox_hand": vox_hand}
