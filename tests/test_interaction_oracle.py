"""CPU: hoisdf_amd/interaction_oracle.py - the float64 restatement that tests/test_gpu_interaction.py holds csrc/interact.hip to -
against closed forms on axis-aligned boxes (mesh_sdf_oracle.box), where every number of the interaction metrics can be written down:
the grid box is the overlap of the two boxes, every cell centre is inside both, a vertex's depth is its distance to the nearest
side.  The boxes sit at camera depth, so their coordinates carry fp32 rounding (6e-8 m at 0.7 m); the analytic values are taken
from the rounded vertices, in float64."""
import numpy as np

from hoisdf_amd import interaction_oracle as I
from hoisdf_amd import mesh_sdf_oracle as O

CENTRE = np.array([0.03, -0.02, 0.7])
A_LO, A_HI = np.array([-0.04, -0.03, -0.05]), np.array([0.04, 0.03, 0.05])          # the "hand" box, 4 x 4 quads per side


def box(lo, hi):
    """a closed box mesh spanning lo .. hi (metres, about CENTRE) -> float32 verts, faces"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v, f = O.box(*(0.5 * (hi - lo)), n=4)
    return (v + 0.5 * (lo + hi) + CENTRE).astype(np.float32), f


def depth_inside(points, verts):
    """analytic: how deep each point lies inside the axis-aligned box spanned by verts (0 outside or on it)"""
    p, v = points.astype(np.float64), verts.astype(np.float64)
    return np.maximum(0, np.minimum(p - v.min(0), v.max(0) - p).min(1))


def distance_outside(points, verts):
    """analytic: distance of each point to the axis-aligned box spanned by verts (0 inside)"""
    p, v = points.astype(np.float64), verts.astype(np.float64)
    return np.linalg.norm(np.maximum(0, np.maximum(v.min(0) - p, p - v.max(0))), axis=1)


def test_two_overlapping_boxes_volume_count_and_depths():
    """overlap (19, 23, 15) mm at 4 mm voxels: 5 x 6 x 4 cells; hand vertex (40, 0, 0) mm sits 5 mm inside the object"""
    hv, hf = box(A_LO, A_HI)
    ov, of = box([0.021, -0.008, -0.005], [0.081, 0.015, 0.010])
    r = I.eval_interaction(hv, hf, ov, of, contact_dist=0.005, voxel=0.004)
    g = r["grid"]
    assert g["n"].tolist() == [5, 6, 4] and g["cell"].dtype == np.float32 and g["lo"].dtype == np.float32
    lo64 = np.maximum(hv.min(0), ov.min(0)).astype(np.float64)
    ext64 = np.minimum(hv.max(0), ov.max(0)).astype(np.float64) - lo64
    # fp32 box centres and half extents at 0.7 m: a few ulps of 6e-8 m
    assert np.abs(g["lo"] - lo64).max() < 3e-7 and np.abs(g["cell"] * g["n"] - ext64).max() < 3e-7
    assert r["inside_count"] == 5 * 6 * 4 and r["inside"].all() and len(r["centres"]) == 120
    assert np.abs(r["vox_obj"]["winding"] - 1).max() < 1e-9 and np.abs(r["vox_hand"]["winding"] - 1).max() < 1e-9
    # volume = the overlap, to fp32 rounding: each extent (>= 15 mm) is a difference of fp32 coordinates (ulp 6e-8 m at 0.7 m):
    # <= 4e-6 relative per axis, 1.2e-5 for the product, plus a few ulps of the fp32 products
    want = 0.019 * 0.023 * 0.015
    assert isinstance(r["volume"], np.float32) and abs(float(r["volume"]) - want) <= 2e-5 * want, (r["volume"], want)
    assert r["volume"] == np.float32(120) * g["cell"][0] * g["cell"][1] * g["cell"][2]
    # first cell centre, last cell centre, ix fastest
    c = r["centres"]
    assert np.abs(c[0] - (lo64 + 0.5 * ext64 / g["n"])).max() < 3e-7 and np.abs(c[-1] - (lo64 + ext64 - 0.5 * ext64 / g["n"])).max() < 3e-7
    assert c[1, 0] > c[0, 0] and c[1, 1] == c[0, 1] and c[5, 1] > c[0, 1] and c[5, 0] == c[0, 0] and c[30, 2] > c[0, 2]
    # the deepest vertices
    dh, do = depth_inside(hv, ov), depth_inside(ov, hv)
    assert abs(dh.max() - 0.005) < 1e-6 and do.max() > 0.005
    assert abs(r["pen_hand"] - dh.max()) < 1e-12 and abs(r["pen_obj"] - do.max()) < 1e-12
    assert r["min_dist"] < 1e-6                                # hand vertex (40, 15, 0) mm lies on the object's side y = 15 mm
    assert r["in_contact"] == 1 and r["contact_verts"] == int((r["hand_vert"]["sdf"] <= 0.005).sum()) >= 1
    assert I.pack_n(g["n"]) == 5 | 6 << 8 | 4 << 16


def test_disjoint_boxes_no_volume_no_contact_and_the_gap():
    hv, hf = box(A_LO, A_HI)
    ov, of = box([0.050, -0.008, -0.005], [0.110, 0.015, 0.010])                  # 10 mm beyond the hand's +x side
    r = I.eval_interaction(hv, hf, ov, of, contact_dist=0.005, voxel=0.004)
    assert r["grid"]["n"].tolist() == [0, 0, 0] and r["inside_count"] == 0 and r["volume"] == 0 and len(r["inside"]) == 0
    assert r["pen_hand"] == 0 and r["pen_obj"] == 0 and r["contact_verts"] == 0 and r["in_contact"] == 0
    gap = distance_outside(hv, ov).min()
    assert abs(gap - 0.010) < 1e-6 and abs(r["min_dist"] - gap) < 1e-12
    # the same pair with the contact distance beyond the gap: in contact without any penetration
    r = I.eval_interaction(hv, hf, ov, of, contact_dist=0.012, voxel=0.004)
    assert r["in_contact"] == 1 and r["contact_verts"] >= 1 and r["pen_hand"] == 0 and r["pen_obj"] == 0


def test_an_extent_of_100_voxels_is_cut_into_64_cells():
    hv, hf = box(A_LO, A_HI)
    ov, of = box([-0.010, -0.0011, -0.0006], [0.100, 0.0011, 0.0006])             # overlap 50 x 2.2 x 1.2 mm at 0.5 mm voxels
    r = I.eval_interaction(hv, hf, ov, of, voxel=0.0005)
    g = r["grid"]
    assert g["n"].tolist() == [64, 5, 3] and I.MAX_GRID == 64
    ext_x = np.float32(hv[:, 0].max()) - np.float32(ov[:, 0].min())
    assert abs(float(ext_x) - 0.05) < 2e-7 and abs(float(g["cell"][0]) - 0.05 / 64) < 1e-8
    assert abs(float(g["cell"][0]) * 64 - float(ext_x)) < 1e-7                    # the cells tile the extent
    assert r["inside_count"] == 64 * 5 * 3
    want = 0.05 * 0.0022 * 0.0012
    # extents of 2.2 and 1.2 mm from fp32 coordinates at 0.7 m: 1.2e-7 / 1.2e-3 = 1e-4 relative on the thinnest axis
    assert abs(float(r["volume"]) - want) <= 3e-4 * want


def test_padding_rows_count_for_the_box_and_not_for_the_penetration():
    hv, hf = box(A_LO, A_HI)
    ov, of = box([0.021, -0.008, -0.005], [0.081, 0.015, 0.010])
    base = I.eval_interaction(hv, hf, ov, of, voxel=0.004)
    deep = (CENTRE + [0.0, 0.0, 0.0]).astype(np.float32)                          # the middle of the hand box: 30 mm deep
    padded = np.concatenate([ov, np.repeat(deep[None], 7, 0)])
    r = I.eval_interaction(hv, hf, padded, of, obj_n_verts=len(ov), voxel=0.004)
    assert r["pen_obj"] == base["pen_obj"] and r["pen_hand"] == base["pen_hand"] and len(r["obj_vert"]["sdf"]) == len(ov)
    assert r["grid"]["n"][0] > base["grid"]["n"][0]                               # ... but the object's bounding box has grown
    assert r["grid"]["n"].tolist() == [10, 6, 4] and r["inside_count"] == 5 * 6 * 4   # x cells of 4 mm from 0: centres beyond 21 mm
    full = I.eval_interaction(hv, hf, padded, of, voxel=0.004)
    assert abs(full["pen_obj"] - 0.03) < 1e-6
