"""CPU: hoisdf_amd/field_fit_oracle.py - the rules of the rigid fit of a point set to a sampled signed-distance field, in numpy
float64.  The inputs: the tanh of a rounded box's exact distance (half sides 0.5, 0.3, 0.2, radius 0.02) on 24 nodes over
[-0.9, 0.9] x [-0.8, 0.8] x [-0.7, 0.7], and 300 points of the box's faces moved by a known rotation of 10 / 20 / 30 / 45 degrees about
seeded axes and a translation of 0.05 / 0.1 / 0.15 / 0.2.  The fit must bring the points back; and every run must keep clear of
rounding-level branches, so that a comparison with another implementation of the same rules cannot hinge on one (a seed that does
not is replaced, the condition stays)."""
import numpy as np
import pytest

from hoisdf_amd import field_fit_oracle as F

STEP_TOL = 1e-7


@pytest.fixture(scope="module")
def runs():
    field = F.box_field()
    out = []
    for k in range(len(F.CASE_MOVES)):
        case = F.box_case(k)
        out.append((case, F.fit(field, F.BOX_GRID, F.BOX_N, case["points"], step_tol=STEP_TOL),
                    F.fit(field, F.BOX_GRID, F.BOX_N, case["points"], step_tol=STEP_TOL, order="plain")))
    return field, out


def _rms(a, b):
    return float(np.sqrt(((np.asarray(a, np.float64) - b) ** 2).sum(1).mean()))


def test_the_field_and_the_cases_are_what_the_tests_say():
    assert F.BOX_N == 24 and np.allclose(F.BOX_GRID[:3], [-0.9, -0.8, -0.7])
    nodes = F.grid_nodes(F.BOX_GRID, F.BOX_N)
    assert np.allclose(nodes[-1], [0.9, 0.8, 0.7], atol=1e-6) and len(nodes) == 24 ** 3
    # the exact distance: 0 on a face, -0.2 at the centre (the smallest half side), radius-rounded at a corner
    assert abs(F.rounded_box_sdf(np.array([0.5, 0.1, 0.05]))) < 1e-15 and abs(F.rounded_box_sdf(np.zeros(3)) + 0.2) < 1e-15
    corner = np.array(F.BOX_HALF)
    assert abs(F.rounded_box_sdf(corner) - (np.sqrt(3.0) - 1.0) * F.BOX_RADIUS) < 1e-15
    field = F.box_field()
    assert field.dtype == np.float32 and field.shape == (24 ** 3,) and field.min() < -0.15 and field.max() > 0.4
    for k, (deg, dist) in enumerate(F.CASE_MOVES):
        case = F.box_case(k)
        assert case["points"].shape == (300, 3) and case["points"].dtype == np.float32
        assert np.abs(F.rounded_box_sdf(case["truth"])).max() < 1e-12, "the true positions lie on the box"
        c = case["truth"].mean(0)
        moved = case["points"].astype(np.float64)
        assert abs(np.linalg.norm(moved.mean(0) - c) - dist) < 1e-6, "rotated about the mean, then moved by the distance"
        A, Bm = case["truth"] - c, moved - moved.mean(0)
        U, _, Vt = np.linalg.svd(A.T @ Bm)
        R = (U @ Vt).T
        assert abs(np.degrees(np.arccos((np.trace(R) - 1) / 2)) - deg) < 1e-3


def test_the_trilinear_read_and_its_gradient():
    field = F.box_field()
    rng = np.random.default_rng(0)
    x = rng.uniform(-0.6, 0.6, (50, 3))
    ok, f, g = F.field_read(field, F.BOX_GRID, F.BOX_N, x)
    assert ok.all()
    assert np.abs(f - np.tanh(F.rounded_box_sdf(x))).max() < 0.02, "the interpolant follows the field to the grid's resolution"
    h = 1e-6                                                         # inside one cell the interpolant is smooth: central differences
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        num = (F.field_read(field, F.BOX_GRID, F.BOX_N, x + e)[1] - F.field_read(field, F.BOX_GRID, F.BOX_N, x - e)[1]) / (2 * h)
        same_cell = np.floor((x + e - F.BOX_GRID[:3]) / F.BOX_GRID[3:6]).astype(int) == np.floor((x - e - F.BOX_GRID[:3]) / F.BOX_GRID[3:6]).astype(int)
        keep = same_cell.all(1)
        assert keep.sum() > 40 and np.abs(num - g[:, k])[keep].max() < 1e-8
    # the nodes themselves, the upper border included (the cell index is clamped to n - 2); outside and NaN take no part
    nodes = F.grid_nodes(F.BOX_GRID, F.BOX_N)
    pick = np.array([0, 23, 24 ** 3 - 1, 24 * 24 * 5 + 24 * 7 + 11])
    ok, f, _ = F.field_read(field, F.BOX_GRID, F.BOX_N, nodes[pick] - np.array([0.0, 0.0, 0.0]))
    inner = pick[[0, 3]]
    assert ok[[0, 3]].all() and np.abs(f[[0, 3]] - field[inner]).max() < 1e-6
    ok, _, _ = F.field_read(field, F.BOX_GRID, F.BOX_N, np.array([[2.0, 0, 0], [np.nan, 0, 0], [0, -0.81, 0]]))
    assert not ok.any()
    holed = field.copy()
    holed[24 * 24 * 12 + 24 * 12 + 12] = np.inf
    cell = F.BOX_GRID[3:6].astype(np.float64)
    at = F.BOX_GRID[:3] + cell * 12
    ok, _, _ = F.field_read(holed, F.BOX_GRID, F.BOX_N, np.stack([at + 0.3 * cell, at - 0.3 * cell, at + 1.3 * cell]))
    assert ok.tolist() == [False, False, True], "the eight cells around a node that is not finite are skipped"


def test_the_fit_brings_the_points_back(runs):
    _, out = runs
    for k, (case, res, _) in enumerate(out):
        start, end = _rms(case["points"], case["truth"]), _rms(res["points_out"], case["truth"])
        print(f"case {k}: rms {start:.4f} -> {end:.5f}, cost {res['cost'][0]:.3e} -> {res['cost'][1]:.3e}, info {res['info'].tolist()}, "
              f"stopped by {res['stopped_by']}, tested steps {['%.1e' % s for s in res['steps']]}")
        assert end <= start / 20.0, (k, start, end)
        assert all(b <= a for a, b in zip(res["costs"], res["costs"][1:])) and res["cost"][1] <= res["cost"][0], "the cost never rises"
        assert res["stopped_by"] == "step" and res["info"][2] <= 16, (k, res["stopped_by"], res["info"])
        assert res["info"][0] == 300 and res["info"][1] == 300 and res["info"][3] <= res["info"][2]
        R = res["rot"]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0
        # the pose reproduces the posed points: x = R (p - c) + c + t
        p = case["points"].astype(np.float64)
        c = p.mean(0)
        assert np.abs((p - c) @ R.T + c + res["trans"] - res["points_out"]).max() < 1e-12


def test_every_run_keeps_clear_of_rounding_level_branches(runs):
    _, out = runs
    for k, (_, res, plain) in enumerate(out):
        margins = [abs(t - c) / c for t, c, _ in res["decisions"]]
        print(f"case {k}: smallest decision margin {min(margins):.2e}, last tested steps {res['steps'][-2:]}")
        assert min(margins) > 1e-9, (k, min(margins))
        assert not any(0.5 * STEP_TOL <= s <= 2.0 * STEP_TOL for s in res["steps"]), (k, res["steps"])
        assert F.clear_of_rounding(res, STEP_TOL) and res["steps"][-1] < STEP_TOL
        # the two summation orders: the same decisions, the same result to rounding
        assert np.array_equal(plain["info"], res["info"]) and [d[2] for d in plain["decisions"]] == [d[2] for d in res["decisions"]]
        diff = max(np.abs(plain["points_out"] - res["points_out"]).max(), np.abs(plain["rot"] - res["rot"]).max())
        print(f"case {k}: lane order against ascending order {diff:.1e}")
        assert diff < 1e-12


def test_normal_equations_are_what_the_rules_say(runs):
    field, out = runs
    case = out[1][0]
    p = case["points"].astype(np.float64)
    c = p.mean(0)
    ne = F.normal_equations(field, F.BOX_GRID, F.BOX_N, p, c, np.eye(3), np.zeros(3), 0.1)
    ok, f, g = F.field_read(field, F.BOX_GRID, F.BOX_N, p)
    a = np.abs(f)
    w = np.where(a <= 0.1, 1.0, 0.1 / np.maximum(a, 1e-300))
    J = np.concatenate([g, np.cross(p - c, g)], 1)
    H = (w[:, None, None] * J[:, :, None] * J[:, None, :]).mean(0)
    assert (a > 0.1).any() and (a <= 0.1).any(), "both branches of the Huber cost are used"
    assert np.allclose([H[i, j] for i, j in F.TRI], ne["H"], rtol=0, atol=1e-14)
    assert np.allclose(((w * f)[:, None] * J).mean(0), ne["b"], rtol=0, atol=1e-14)
    rho = np.where(a <= 0.1, 0.5 * f * f, 0.1 * (a - 0.05))
    assert abs(rho.mean() - ne["cost"]) < 1e-15 and np.all(ne["abs"] >= np.abs(ne["normal"]) - 1e-18)
    # the run itself takes the threshold as a float32
    ne32 = F.normal_equations(field, F.BOX_GRID, F.BOX_N, p, c, np.eye(3), np.zeros(3), float(np.float32(0.1)))
    assert np.array_equal(out[1][1]["normal"], ne32["normal"])
    # the step: solve_step solves the damped system
    d = F.solve_step(ne["H"], ne["b"], 1e-3)
    A = H + 1e-3 * np.diag(np.diag(H)) + 1e-12 * np.eye(6)
    assert np.abs(A @ d + ne["b"]).max() < 1e-12
    assert F.solve_step(np.zeros(21) - 1.0, np.zeros(6), 1e-3) is None, "a pivot that is not positive"
    E = F.rodrigues(np.array([0.3, -0.2, 0.5]))
    assert np.abs(E @ E.T - np.eye(3)).max() < 1e-15 and np.abs(F.rodrigues(np.zeros(3)) - np.eye(3)).max() == 0
    tiny = F.rodrigues(np.array([1e-9, 0, 0]))
    assert abs(tiny[2, 1] - 1e-9) < 1e-24 and abs(tiny[1, 1] - 1.0) < 1e-16


def test_edges_of_the_rules():
    field = F.box_field()
    case = F.box_case(0)
    none = F.fit(field, F.BOX_GRID, F.BOX_N, case["points"] + np.float32(5.0))
    assert none["info"].tolist() == [0, 0, 0, 0] and np.array_equal(none["rot"], np.eye(3)) and not none["trans"].any()
    assert not none["cost"].any() and not none["normal"].any()
    zero = F.fit(field, F.BOX_GRID, F.BOX_N, case["points"], iters=0)
    assert zero["info"].tolist() == [300, 300, 0, 0] and zero["cost"][0] == zero["cost"][1] > 0 and zero["stopped_by"] == "iters"
    assert np.array_equal(zero["rot"], np.eye(3))
    three = F.fit(field, F.BOX_GRID, F.BOX_N, case["points"], iters=3)
    assert three["info"][2] == 3 and three["stopped_by"] == "iters"
    tail = np.concatenate([case["points"], np.full((20, 3), np.nan, np.float32)])
    cut = F.fit(field, F.BOX_GRID, F.BOX_N, tail, n_points=300)
    full = F.fit(field, F.BOX_GRID, F.BOX_N, case["points"])
    assert np.array_equal(cut["points_out"], full["points_out"]) and np.array_equal(cut["info"], full["info"])
    given = F.fit(field, F.BOX_GRID, F.BOX_N, case["points"], pivot=np.float32([0.1, -0.2, 0.05]))
    assert given["stopped_by"] == "step" and np.abs(given["points_out"] - full["points_out"]).max() < 1e-5, "the pivot moves R, t - not the points"
    # a sphere: the rotation is unobservable, the damped system still factors and the cost falls
    ball = F.sphere_field()
    d = np.random.default_rng(2).normal(size=(300, 3))
    pts = (0.3 * d / np.linalg.norm(d, axis=1, keepdims=True) + [0.06, -0.04, 0.05]).astype(np.float32)
    res = F.fit(ball, F.BOX_GRID, F.BOX_N, pts)
    assert np.isfinite(res["points_out"]).all() and np.abs(res["rot"] @ res["rot"].T - np.eye(3)).max() < 1e-12
    assert res["cost"][1] < 0.01 * res["cost"][0] and np.abs(res["trans"] + [0.06, -0.04, 0.05]).max() < 5e-3
