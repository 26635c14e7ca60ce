"""CPU: hoisdf_amd/isosurf_oracle.py - the numpy restatement of the iso-surface rules of include/hoisdf.h - against properties that
do not share its case table: closed and consistently oriented surfaces, Euler characteristics, positive volumes that converge to
the analytic one, open surfaces whose boundary lies on the grid's border, the strict inside rule, silent cells around a NaN, and
the float32 mode against the float64 mode.  Every input is an analytic field."""
import numpy as np
import pytest

from hoisdf_amd import isosurf_oracle as iso

EPS32 = float(np.finfo(np.float32).eps)
SPHERE_R = 0.3
SPHERE_VOLUME = 4.0 / 3.0 * np.pi * SPHERE_R ** 3
# |volume of the float64 oracle's sphere - SPHERE_VOLUME| as measured on the CPU, by nodes per axis (the surface is inscribed: all
# three volumes are too small)
SPHERE_VOLUME_ERROR = {9: 9.960441e-3, 17: 2.431168e-3, 33: 6.121674e-4}


def _fields(n):
    g = iso.cube_grid(-0.5, 0.5, n)
    p = iso.grid_points(g, n, np.float64)
    two = np.minimum(iso.sphere_field(p, (-0.25, 0.0, 0.0), 0.15), iso.sphere_field(p, (0.25, 0.0, 0.0), 0.15))
    return g, p, {"sphere": (iso.sphere_field(p, r=SPHERE_R), 2), "torus": (iso.torus_field(p), 0), "two spheres": (two, 4)}


@pytest.mark.parametrize("n", [9, 17])
def test_closed_surfaces_are_closed_oriented_and_have_the_right_euler_characteristic(n):
    g, _, fields = _fields(n)
    for name, (f, chi) in fields.items():
        v, faces = iso.extract(f, g, n, 0.0, np.float64)
        r = iso.mesh_report(v, faces)
        assert r["F"] > 0 and r["V"] == len(v), (name, "every vertex is used by a face")
        assert r["closed"], (name, "every undirected edge belongs to exactly two faces")
        assert r["oriented"], (name, "the two faces of an edge traverse it in opposite directions")
        assert r["euler"] == chi, (name, r["euler"])
        assert r["volume"] > 0, (name, "outward winding: the divergence theorem gives a positive volume")
        assert np.all((v >= -0.5) & (v <= 0.5))


def test_sphere_volume_converges_at_second_order():
    """Measured here with the float64 oracle (r = 0.3 in [-0.5, 0.5]^3, analytic volume 0.113097336): n = 9: 0.103136894 (error
    9.960441e-3), n = 17: 0.110666167 (2.431168e-3), n = 33: 0.112485168 (6.121674e-4) - ratios 4.10 and 3.97 per halving of the
    cell.  Each volume must stay within twice its own measured error, and the error must fall about fourfold per halving."""
    err = {}
    for n in (9, 17, 33):
        g, _, fields = _fields(n)
        v, faces = iso.extract(fields["sphere"][0], g, n, 0.0, np.float64)
        err[n] = abs(iso.mesh_report(v, faces)["volume"] - SPHERE_VOLUME)
        print(f"n={n}: volume error {err[n]:.6e}")
        assert err[n] <= 2.0 * SPHERE_VOLUME_ERROR[n], (n, err[n])
    assert 3.0 <= err[9] / err[17] <= 5.0 and 3.0 <= err[17] / err[33] <= 5.0, err


def test_a_plane_gives_an_open_surface_whose_boundary_is_on_the_border():
    n = 9
    g = iso.cube_grid(-0.5, 0.5, n)
    p = iso.grid_points(g, n, np.float64)
    f = (0.3 * p[:, 0] + 0.5 * p[:, 1] + p[:, 2] - 0.043).astype(np.float32)
    v, faces = iso.extract(f, g, n, 0.0, np.float64)
    r = iso.mesh_report(v, faces)
    assert r["F"] > 0 and r["oriented"] and len(r["boundary"]) > 0 and r["euler"] == 1          # a disc
    a, b = v[r["boundary"][:, 0]], v[r["boundary"][:, 1]]
    on_lo, on_hi = (a == -0.5) & (b == -0.5), (a == 0.5) & (b == 0.5)
    assert np.all((on_lo | on_hi).any(1)), "a boundary edge lies in one face of the grid's cube"
    # the normals point to the outside (value > 0): along the field's gradient
    nrm = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    assert np.all(nrm @ np.array([0.3, 0.5, 1.0]) > 0)


def test_degenerate_fields():
    for n in (2, 5):
        g = iso.cube_grid(0.0, 1.0, n)
        for value in (1.0, -1.0):
            v, faces = iso.extract(np.full(n ** 3, value, np.float32), g, n, 0.0)
            assert v.shape == (0, 3) and faces.shape == (0, 3)
    # a single cell with corner 000 inside: its 7 owned edges are cut in the middle, each tetrahedron has one inside corner and
    # gives one triangle (edge to e_a, edge to e_a + e_b, the diagonal), reversed in the odd tetrahedra - checked by hand
    f = np.ones(8, np.float32)
    f[0] = -1.0
    v, faces = iso.extract(f, iso.cube_grid(0.0, 1.0, 2), 2, 0.0)
    assert np.array_equal(v, 0.5 * np.array(iso.EDGE_DIRS, np.float32))
    assert faces.tolist() == [[0, 3, 6], [0, 6, 4], [1, 6, 3], [1, 5, 6], [2, 4, 6], [2, 6, 5]]
    nrm = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
    assert np.all(nrm @ np.ones(3) > 0), "away from the inside corner"


def test_a_node_equal_to_iso_is_outside():
    n, iso_level = 3, 0.25
    g = iso.cube_grid(0.0, 2.0, n)
    f = np.full(27, 1.0, np.float32)
    f[13] = iso_level                                   # the centre, exactly at the level: not inside, nothing to extract
    v, faces = iso.extract(f, g, n, iso_level)
    assert len(v) == 0 and len(faces) == 0
    f[13] = -1.0
    f[14] = iso_level                                   # its +x neighbour at the level: outside, and the vertex sits ON that node (t = 1)
    v, faces = iso.extract(f, g, n, iso_level)
    r = iso.mesh_report(v, faces)
    assert r["closed"] and r["oriented"] and r["euler"] == 2 and r["volume"] > 0
    assert np.any(np.all(v == np.array([2.0, 1.0, 1.0], np.float32), axis=1))


def test_one_nan_node_silences_exactly_the_cells_that_touch_it():
    n = 9
    g, _, fields = _fields(n)
    f = fields["sphere"][0].copy()
    bad = (6, 4, 4)                                     # ix, iy, iz: next to the surface at x = 0.3
    v0, f0 = iso.extract(f, g, n, 0.0, np.float64)
    f[bad[0] + n * (bad[1] + n * bad[2])] = np.nan
    v1, f1 = iso.extract(f, g, n, 0.0, np.float64)
    assert np.all(np.isfinite(v1))

    def by_cell(v, faces):
        tri = v[faces]                                  # (F, 3, 3); the centroid of a triangle lies inside its cell
        cell = np.floor((tri.mean(1) + 0.5) / 0.125).astype(int)
        return tri, cell

    t0, c0 = by_cell(v0, f0)
    t1, _ = by_cell(v1, f1)
    touches = np.all((c0 >= np.array(bad) - 1) & (c0 <= np.array(bad)), axis=1)
    assert touches.any() and len(f1) == len(f0) - touches.sum()
    assert np.array_equal(t1, t0[~touches]), "the other cells' triangles, in the same order, at the same positions"


@pytest.mark.parametrize("n", [9, 17])
def test_float32_mode_against_float64_mode(n):
    """Faces and counts are identical when no node is within 1e-3 of the level (rounding cannot flip a node); vertices within
    8 eps32 (max |coordinate| + max cell): t carries about 3 roundings (two differences, a quotient), each worth at most one cell x
    eps32 of position, the node coordinates and the final product and sum at most 2 eps32 of the coordinate each."""
    g, _, fields = _fields(n)
    for name, (f, _chi) in fields.items():
        assert np.abs(f).min() > 1e-3, (name, "a node too close to the level for this test")
        v64, f64 = iso.extract(f, g, n, 0.0, np.float64)
        v32, f32 = iso.extract(f, g, n, 0.0, np.float32)
        assert v32.dtype == np.float32 and f32.dtype == np.int32
        assert np.array_equal(f32, f64) and len(v32) == len(v64), name
        err = np.abs(v32.astype(np.float64) - v64).max()
        print(f"{name} n={n}: max vertex error {err:.3e}")
        assert err <= 8 * EPS32 * (0.5 + float(g[3:6].max())), (name, err)


def test_grid_points_and_refine_grid():
    n = 5
    g = np.array([-1.0, 0.5, 2.0, 0.1, 0.2, 0.3, 0, 0], np.float32)
    p = iso.grid_points(g, n)
    assert p.dtype == np.float32 and p.shape == (125, 3)
    assert np.array_equal(p[1 + n * (2 + n * 3)], np.float32([-1.0 + np.float32(0.1), 0.5 + np.float32(2) * np.float32(0.2),
                                                              2.0 + np.float32(3) * np.float32(0.3)]))
    f = np.ones((n, n, n), np.float32)                  # [iz][iy][ix]
    f[2, 1:3, 3] = -1.0                                 # inside: ix = 3, iy = 1..2, iz = 2
    out = iso.refine_grid(f.ravel(), g, n, 0.0, 1, 9)
    lo = np.float32([-1.0 + np.float32(2) * np.float32(0.1), 0.5, 2.0 + np.float32(0.3)])        # ix 2..4, iy 0..3, iz 1..3
    hi = np.float32([-1.0 + np.float32(4) * np.float32(0.1), 0.5 + np.float32(3) * np.float32(0.2), 2.0 + np.float32(3) * np.float32(0.3)])
    assert np.array_equal(out[:3], lo) and np.array_equal(out[3:6], (hi - lo) / np.float32(8)) and np.all(out[6:] == 0)
    # the last node of the refined grid is the box's upper corner up to the rounding of the cell
    assert np.allclose(iso.grid_points(out, 9)[-1], hi, rtol=0, atol=4 * EPS32 * 3)
    whole = iso.refine_grid(np.ones(n ** 3, np.float32), g, n, 0.0, 1, 9)
    assert np.array_equal(whole[:3], g[:3]) and np.allclose(whole[3:6], g[3:6] * 4 / 8, rtol=8 * EPS32)


def test_eval_surface_oracle_on_a_case_done_by_hand():
    gv = np.array([[0, 0, 0.6], [1, 0, 0.6], [1, 1, 0.6], [0, 1, 0.6]], np.float64)
    gf = np.array([[0, 1, 2], [0, 2, 3], [1, 1, 2]])                  # the last face has no area and takes no part
    pred = np.array([[0.25, 0.25, 0.61], [0.75, 0.5, 0.58], [1.5, 0.5, 0.6]])          # 0.01 above, 0.02 below, 0.5 beside
    samples = np.array([[0.25, 0.25, 0.6], [1.0, 0.5, 0.6]])
    r = iso.eval_surface(pred, gv, gf, samples)
    assert r["n_used"] == 3
    assert r["pred_to_gt"] == pytest.approx((1e-4 + 4e-4 + 0.25) / 3, rel=1e-12)
    assert r["gt_to_pred"] == pytest.approx((1e-4 + (0.0625 + 4e-4)) / 2, rel=1e-12)
    assert r["chamfer"] == pytest.approx(r["pred_to_gt"] + r["gt_to_pred"])
    assert iso.eval_surface(pred[:0], gv, gf, samples) == {"pred_to_gt": 0.0, "gt_to_pred": 0.0, "chamfer": 0.0, "n_used": 0}
    assert iso.eval_surface(pred, gv, gf[2:], samples)["n_used"] == 0
