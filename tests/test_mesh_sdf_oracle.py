"""CPU: hoisdf_amd/mesh_sdf_oracle.py, the numpy restatement of csrc/mesh_sdf.hip that tests/test_gpu_mesh_sdf.py holds the kernels to,
checked in fp64 against what is known in closed form: the unit sphere, the winding number of closed meshes, the skipped-face rule,
the sampler's index -> kind rule and the vertex -> hand-part rule."""
import numpy as np
import pytest

from hoisdf_amd import mesh_sdf_oracle as O


@pytest.fixture(scope="module")
def points():
    r = np.random.default_rng(11)
    return r.uniform(-1.4, 1.4, (1500, 3))


def test_icosphere_against_the_sphere(points):
    v, f = O.icosphere(2)
    assert v.shape == (162, 3) and f.shape == (320, 3)
    o = O.mesh_sdf(points, v, f)
    # the mesh is inscribed: its faces lie between radius 1 - delta and 1, delta from the face planes themselves; the unsigned
    # distance to a set is 1-Lipschitz in the Hausdorff distance of the set, which is delta here
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    delta = 1 - np.abs((n * v[f[:, 0]]).sum(1) / np.linalg.norm(n, axis=1)).min()
    rad = np.linalg.norm(points, axis=1)
    err = np.abs(np.abs(o["sdf"]) - np.abs(rad - 1)).max()
    print(f"icosphere: faceting bound {delta:.5f}, worst | |sdf| - | |p| - 1 | | = {err:.5f}")
    assert 0.01 < delta < 0.03 and err <= delta + 1e-12
    clear = np.abs(rad - 1) > 0.02
    assert clear.mean() > 0.9 and np.array_equal(o["sdf"][clear] < 0, rad[clear] < 1)
    assert (o["sdf"] < 0).any() and (o["sdf"] > 0).any()


@pytest.mark.parametrize("mesh", ["icosphere", "torus", "box"])
def test_winding_number_of_closed_meshes(points, mesh):
    v, f = {"icosphere": O.icosphere(2), "torus": O.torus(), "box": O.box()}[mesh]
    w = O.mesh_sdf(points, v, f)["winding"]
    dev = np.abs(w - np.round(w)).max()
    print(f"{mesh}: {len(f)} faces, winding within {dev:.2e} of an integer, inside share {np.mean(w > 0.5):.3f}")
    assert dev < 1e-12 and set(np.round(w).astype(int)) == {0, 1}


def test_torus_has_the_faces_and_areas_the_gpu_tests_count_on():
    v, f = O.torus(16, 12)
    a = O.prepare(v, f)["area"]
    assert f.shape == (384, 3) and 1.9 < a.max() / a.min() < 3.0


def test_an_exactly_degenerate_face_changes_nothing(points):
    v, f = O.icosphere(1)
    v = np.concatenate([v, v[3:4]])                                   # vertex 42 = a copy of vertex 3: coincident points
    bad = np.asarray([[5, 5, 9], [7, 2, 2], [3, 42, 3], [3, 42, 42], [1, 2, 99]], np.int32)   # the last names a vertex outside the mesh
    g = np.concatenate([f[:7], bad, f[7:]])
    m = O.prepare(v, g)
    assert m["skipped"].sum() == 5 and np.all(m["area"][7:12] == 0) and np.all(np.diff(m["cdf"])[6:11] == 0)
    a, b = O.mesh_sdf(points[:600], v[:42], f), O.mesh_sdf(points[:600], v, g, recentre=False)
    a0 = O.mesh_sdf(points[:600], v[:42], f, recentre=False)
    for k in ("sdf", "winding", "bary"):
        assert np.array_equal(a0[k], b[k]), k
    assert np.array_equal(np.where(a0["face"] >= 7, a0["face"] + 5, a0["face"]), b["face"])
    assert np.abs(a["sdf"] - a0["sdf"]).max() < 1e-14                 # re-centring moves nothing in fp64
    # fp32 skips the same faces: u x u is exactly zero when every product is rounded on its own
    assert np.array_equal(O.prepare(v, g, np.float32)["skipped"], m["skipped"])


def test_fp32_mode_is_fp32_and_close():
    v, f = O.torus()
    r = np.random.default_rng(3)
    v32 = (v * 0.08 + [0.03, -0.02, 0.7]).astype(np.float32)
    p32 = (r.uniform(-0.15, 0.15, (800, 3)) + [0.03, -0.02, 0.7]).astype(np.float32)
    a, b = O.mesh_sdf(p32, v32, f, dtype=np.float32), O.mesh_sdf(p32, v32, f)
    assert a["sdf"].dtype == np.float32 and b["sdf"].dtype == np.float64
    err = np.abs(np.abs(a["sdf"]) - np.abs(b["sdf"])).max()
    print(f"fp32 oracle vs fp64 at 0.7 m, re-centred: {err:.2e} m")
    assert err < 5e-7 and np.array_equal(a["sdf"] < 0, b["sdf"] < 0)


def test_closest_point_regions():
    a, b, c = np.array([0.0, 0, 0]), np.array([1.0, 0, 0]), np.array([0.0, 1, 0])
    cases = {(-1, -1, 2): (0, 0), (2, -0.5, 0): (1, 0), (-0.5, 2, 1): (0, 1), (0.5, -1, 0): (0.5, 0), (-1, 0.25, 0): (0, 0.25),
             (1, 1, 0): (0.5, 0.5), (0.25, 0.25, 3): (0.25, 0.25)}
    for p, (v, w) in cases.items():
        gv, gw, d2 = O.closest_point(np.asarray(p, float), a, b, c)
        q = (1 - v - w) * a + v * b + w * c
        assert (gv, gw) == (v, w) and d2 == pytest.approx(((np.asarray(p) - q) ** 2).sum(), abs=1e-15), p
    d = O.distance_to_face(np.asarray([[0.25, 0.25, 3.0]]), np.stack([a, b, c]), [[0, 1, 2]], [0])
    assert d[0] == 3.0


def test_labels_take_the_corner_with_the_largest_weight():
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.0]])
    f = np.array([[0, 1, 2], [1, 3, 2]])
    lab = np.array([10, 11, 12, 13])
    p = np.array([[0.1, 0.1, 0.5], [0.8, 0.1, -0.5], [0.9, 0.9, 0.2], [0.5, 0.5, 0.1], [0.375, 0.25, 1.0]])
    o = O.mesh_sdf(p, v, f, lab, label_sets=True)
    assert o["label"].tolist() == [10, 11, 13, 11, 10]                 # ties: lowest face, earliest corner
    assert o["label_sets"][0] == {10} and o["label_sets"][3] == {11, 12} and o["label_sets"][4] == {10, 11}


def test_index_to_kind_rule():
    k = O.point_kind(np.arange(64), 16)
    assert k[:16].tolist() == [0, 1] * 7 + [0, 2] and np.array_equal(k[:16], k[48:])
    assert (k == 2).sum() == 4 and (k == 0).sum() == 32 and (k == 1).sum() == 28
    assert (O.point_kind(np.arange(1000), 16) == 2).sum() == 1000 // 16
    assert O.point_kind(np.arange(6), 0).tolist() == [0, 1, 0, 1, 0, 1]
    assert O.point_kind(np.arange(3), 1).tolist() == [2, 2, 2]


def test_vertex_part_labels():
    w = np.zeros((5, 16))
    w[0, 0], w[1, 3], w[2, 4], w[3, 15], w[4, 9] = 1, 1, 1, 1, 1
    w[4, 10] = 0.5
    assert O.vertex_part_labels(w).tolist() == [0, 1, 2, 5, 3] and O.vertex_part_labels(w).dtype == np.int32
    assert len(O.PART_OF_JOINT) == 16 and set(O.PART_OF_JOINT) == set(range(6))
