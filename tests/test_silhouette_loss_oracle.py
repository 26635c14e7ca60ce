"""CPU: the numpy restatement of the silhouette loss (hoisdf_amd/silhouette_loss_oracle.py) is itself held to something.
Its distance transform equals the definition (a brute-force minimum over all pairs) and, where scipy imports, scipy's; its
gradient equals central differences of its own fp64 values, step 1e-6 m per coordinate, to 1e-6 (abs_terms + 1) with abs_terms
the sum of the absolute values of the terms that meet in that coordinate.  The loss has kinks: where a vertex changes its
bilinear cell, and where a pixel changes its nearest vertex.  A vertex is left out of the comparison only when one of its six
+-1e-6 m moves changes its own cell or changes the nearest vertex of a pixel it owns or gains; at most 5 % of a sample's vertices
may be left out (asserted, the count printed).

The scenes (also those of tests/test_gpu_silhouette_loss.py): a procedural mesh of 40 mm around (0.03, -0.02, 0.7) m, jittered by
0.2 mm, seen by a camera whose principal point puts that base point on the centre of the map; cover = a disk of about the projected
radius shifted by a few pixels minus a second, smaller disk; allow = the union of the two disks.  The box at focal length 420 is
wider than its 48-pixel map: its off-map vertices exercise the `out` term and the clamped axes."""
import numpy as np
import pytest

from hoisdf_amd import mesh_sdf_oracle as O
from hoisdf_amd import silhouette_loss_oracle as S

BASE = np.array([0.03, -0.02, 0.7])
NEAR, STEP = 0.01, 1e-6
G_IN, G_COV = 0.7, 1.3
SCENES = {"icosphere": (lambda: O.icosphere(2)[0], 250.0, 40, 48), "torus": (lambda: O.torus()[0], 300.0, 33, 70),
          "box": (lambda: O.box()[0], 420.0, 40, 48), "torus250": (lambda: O.torus()[0], 250.0, 40, 48)}


def disk(h, w, cx, cy, r):
    yy, xx = np.mgrid[0:h, 0:w]
    return (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r


def scene(name, seed=5):
    """-> dict: verts (V, 3) float32, K (6,) float32, cover, allow (h, w) float32, d2 (h, w) int32, w (V,) float32 weights"""
    make, focal, h, w = SCENES[name]
    r = np.random.default_rng(seed)
    v = make() * 0.04 + BASE
    verts = (v + r.normal(0, 0.0002, v.shape)).astype(np.float32)
    cx, cy = w / 2, h / 2
    K = np.array([focal, 0, cx - focal * BASE[0] / BASE[2], 0, focal, cy - focal * BASE[1] / BASE[2]], np.float32)
    rad = focal * 0.04 / BASE[2]
    second = disk(h, w, cx - 0.4 * rad, cy + 0.3 * rad, 0.35 * rad)
    cover = disk(h, w, cx + 3, cy - 2, rad) & ~second
    allow = cover | second
    d2, _ = S.edt(allow)
    return {"verts": verts, "K": K, "cover": cover.astype(np.float32), "allow": allow.astype(np.float32), "d2": d2,
            "w": r.uniform(0.5, 1.5, len(verts)).astype(np.float32), "h": h, "wd": w}


def run(sc, verts, n_verts=None, w="w", g_inside=G_IN, g_cover=G_COV):
    return S.silhouette_loss(verts, n_verts, sc["K"], sc["d2"], sc["cover"], None if w is None else sc[w], NEAR, g_inside, g_cover)


def differences(sc, n_verts=None, extrapolate=True):
    """central differences of g_inside inside + g_cover cover over every coordinate of every vertex that counts, step STEP, with
    the step's h^2 error taken out by the same difference at STEP / 2 ((4 D(h/2) - D(h)) / 3: every move stays within +-STEP) ->
    (the oracle's result, numeric (V, 3), plain (V, 3): the difference at STEP alone, kink (V,) bool: a move changed the
    vertex's cell or the nearest vertex of a pixel it owns or gains).  extrapolate = False: the moves of +-STEP alone (enough for kink)"""
    P = sc["verts"].astype(np.float64)
    base = run(sc, P, n_verts)
    n = len(P) if n_verts is None else n_verts
    num, plain, kink = np.zeros((len(P), 3)), np.zeros((len(P), 3)), np.zeros(len(P), bool)
    for i in range(n):
        for c in range(3):
            d = []
            for step in (STEP, STEP / 2) if extrapolate else (STEP,):
                val = []
                for sgn in (1.0, -1.0):
                    Q = P.copy()
                    Q[i, c] += sgn * step
                    r = run(sc, Q, n_verts)
                    val.append(G_IN * r["inside"] + G_COV * r["cover"])
                    moved = r["nearest"] != base["nearest"]
                    if (r["cell"][i] != base["cell"][i]).any() or (moved & ((r["nearest"] == i) | (base["nearest"] == i))).any():
                        kink[i] = True
                d.append((val[0] - val[1]) / (2 * step))
            plain[i, c], num[i, c] = d[0], (4 * d[1] - d[0]) / 3 if extrapolate else d[0]
    return base, num, plain, kink


def assert_gradient(sc, n_verts=None, what=""):
    base, num, plain, kink = differences(sc, n_verts)
    n = len(num) if n_verts is None else n_verts
    print(f"{what}: inside {base['inside']:.4f} px, cover {base['cover']:.4f} px, {int(kink.sum())} of {n} vertices left out (a kink within 1e-6 m), "
          f"{int((~base['use'][:n]).sum())} without an inside term, largest gradient {np.abs(base['d_verts']).max():.3f}")
    assert kink.sum() <= 0.05 * n, (what, int(kink.sum()))
    err = np.abs(num - base["d_verts"])
    bar = 1e-6 * (base["abs_terms"] + 1)
    keep = ~kink
    print(f"{what}: worst error / bar {float((err[keep] / bar[keep]).max()):.3g}; of the difference at {STEP} m alone "
          f"{float((np.abs(plain - base['d_verts'])[keep] / bar[keep]).max()):.3g}")
    assert (err[keep] <= bar[keep]).all(), (what, float((err[keep] / bar[keep]).max()))
    assert np.abs(base["d_verts"]).max() > 1.0                 # pixels per metre: a bar of about 1e-6 means something
    return base


# ---- the distance transform ----------------------------------------------------------------------------------------------------------
def masks():
    r = np.random.default_rng(3)
    corner = np.zeros((9, 13), bool)
    corner[8, 12] = True
    return {"disks 40x48": disk(40, 48, 20, 17, 9) | disk(40, 48, 39, 30, 5) & ~disk(40, 48, 22, 18, 3),
            "33x70": disk(33, 70, 50, 10, 12) | (r.uniform(size=(33, 70)) < 0.01),
            "1x1 set": np.ones((1, 1), bool), "1x1 unset": np.zeros((1, 1), bool), "corner": corner,
            "all": np.ones((7, 5), bool), "none": np.zeros((6, 11), bool), "one row": r.uniform(size=(1, 37)) < 0.1,
            "one column": r.uniform(size=(29, 1)) < 0.1}


@pytest.mark.parametrize("name", list(masks()))
def test_edt_is_the_definition(name):
    m = masks()[name]
    d2, nearest = S.edt(m.astype(np.float32))
    bd, bn = S.edt_brute(m)
    assert d2.dtype == np.int32 and nearest.dtype == np.int32 and d2.shape == m.shape
    assert np.array_equal(d2, bd) and np.array_equal(nearest, bn), name
    if not m.any():
        assert (d2 == S.EDT_NONE).all() and (nearest == -1).all() and S.EDT_NONE == 1 << 30
    else:
        assert (d2[m] == 0).all() and np.array_equal(nearest[m], np.flatnonzero(m))
        try:
            from scipy import ndimage
        except ImportError:
            return
        assert np.array_equal(d2, np.rint(ndimage.distance_transform_edt(~m) ** 2).astype(np.int32)), name


def test_edt_of_a_union():
    a, b = disk(40, 48, 12, 12, 6), disk(40, 48, 30, 25, 8)
    d2, nearest = S.edt(a.astype(np.float32), b.astype(np.float32) * 0.75)
    bd, bn = S.edt_brute(a | b)
    assert np.array_equal(d2, bd) and np.array_equal(nearest, bn)
    assert not np.array_equal(d2, S.edt(a)[0])
    assert np.array_equal(S.edt(a, 0.5 * b)[0], S.edt(a)[0])      # 0.5 is not set


def test_the_sum_has_the_kernels_order():
    r = np.random.default_rng(0)
    t = r.uniform(size=700) * 10.0 ** r.integers(-8, 8, 700)
    s = np.zeros(256)
    for i, x in enumerate(t):
        s[i % 256] += x
    for o in (128, 64, 32, 16, 8, 4, 2, 1):
        for k in range(o):
            s[k] += s[k + o]
    assert S.ordered_sum(t) == s[0] and S.ordered_sum([]) == 0.0


# ---- the gradient ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["icosphere", "torus", "box"])
def test_gradient_against_central_differences(name):
    sc = scene(name)
    base = assert_gradient(sc, what=name)
    assert 0.3 <= base["inside"] <= 3.5 and 0.3 <= base["cover"] <= 3.5     # pixels: the scene is neither solved nor far off
    u, v = base["u"], base["v"]
    off = (u < 0) | (u > sc["wd"] - 1) | (v < 0) | (v > sc["h"] - 1)
    assert (off.sum() >= 20) == (name == "box"), int(off.sum())


def test_values_by_hand():
    """two vertices and a 3 x 4 map whose numbers can be followed on paper"""
    allow = np.zeros((3, 4), np.float32)
    allow[1, 1] = 1
    d2, _ = S.edt(allow)
    cover = np.zeros((3, 4), np.float32)
    cover[0, 0] = cover[2, 3] = 1
    K = np.array([2.0, 0, 0, 0, 2.0, 0], np.float32)
    verts = np.array([[0.25, 0.5, 1.0], [1.25, 1.0, 1.0]])     # project to (0.5, 1) and (2.5, 2)
    r = S.silhouette_loss(verts, None, K, d2, cover, None, NEAR)
    assert r["cell"].tolist() == [[0, 1], [2, 1]] and r["nearest"][0, 0] == 0 and r["nearest"][2, 3] == 1 and (r["nearest"] >= 0).sum() == 2
    # vertex 0: halfway between d = 1 (0, 1) and d = 0 (1, 1); vertex 1: fy = 1 -> halfway between d = sqrt 2 (2, 2) and d = sqrt 5 (3, 2)
    assert abs(r["inside"] - (0.5 + 0.5 * (2 ** 0.5 + 5 ** 0.5)) / 2) < 1e-15
    assert abs(r["cover"] - (1.25 ** 0.5 + 0.5) / 2) < 1e-15
    # padding, a vertex behind the camera plane and a NaN take no part
    more = np.array([[0.25, 0.5, 1.0], [1.25, 1.0, 1.0], [0.3, 0.3, 0.005], [np.nan, 0, 1], [0.5, 0.5, 1.0]])
    r2 = S.silhouette_loss(more, 4, K, d2, cover, None, NEAR)
    assert r2["valid"].tolist() == [True, True, False, False, False] and not r2["d_verts"][2:].any() and (r2["cell"][2:] == -1).all()
    assert abs(r2["inside"] - r["inside"] * 2 / 4) < 1e-15 and r2["cover"] == r["cover"]


def test_empty_maps_and_off_map_vertices():
    sc = scene("icosphere")
    none = dict(sc, d2=np.full_like(sc["d2"], S.EDT_NONE))
    r = run(none, sc["verts"], g_cover=0.0)
    assert r["inside"] == 0 and not r["d_verts"].any() and not r["use"].any()
    r = run(dict(sc, cover=np.zeros_like(sc["cover"])), sc["verts"], g_inside=0.0)
    assert r["cover"] == 0 and not r["d_verts"].any() and (r["nearest"] == -1).all()
    # a vertex off the map is pulled back along the axis it left by
    far = sc["verts"].astype(np.float64).copy()
    far[0] = BASE + [0.2, 0, 0]
    r = run(sc, far, g_cover=0.0)
    assert r["u"][0] > sc["wd"] - 1 and 0 <= r["v"][0] <= sc["h"] - 1
    assert r["d_verts"][0, 0] > 0 and r["abs_terms"][0, 0] >= r["d_verts"][0, 0]
