"""CPU: the numpy restatement of the interaction loss (hoisdf_amd/interaction_loss_oracle.py) is itself held to something - its
gradient to central differences in float64, its three values to cases whose answers are known, its weights to what they mean.

The gradient rule (include/hoisdf.h "interaction loss") holds the sign and the winning face constant, so it is the derivative
wherever neither changes within the step: asserted - no query point within 0.1 mm of the other surface, no winding number within
0.05 of 0.5 - for a step of 1 um.  The bar of a central difference along a unit direction u of the stacked vertex coordinates, from
its own error terms: h^2 / 6 times a bound on the third directional derivative - every point's sdf moves by at most |u| = 1, the
third derivative of a distance is at most 3 / d^2 (a corner region; less in the others) and that of alpha tanh(x / alpha) at most
2 / alpha^2, each weighted by the point's |coef| - plus the rounding of the two evaluations, 4 eps |L| / h."""
import numpy as np
import pytest

from hoisdf_amd import interaction_loss_oracle as L
from hoisdf_amd import mesh_sdf_oracle as O

H = 1e-6
G = (0.7, 1.3, 0.9)                                            # upstream gradients: three different numbers
ALPHA = 0.01


def pair(name, seed):
    """two meshes at hand size and camera depth, jittered by 0.2 mm, overlapping by about 10 mm"""
    r = np.random.default_rng(seed)
    centre = np.array([0.03, -0.02, 0.7])
    hv, hf = O.icosphere(2)
    ov, of = O.icosphere(2) if name == "spheres" else O.torus()
    hv = hv * 0.04 + centre + r.normal(0, 0.0002, hv.shape)
    ov = ov * (0.03 if name == "spheres" else 0.04) + centre + np.array([0.06 if name == "spheres" else 0.07, 0.004, -0.003])
    return hv, hf, ov + r.normal(0, 0.0002, ov.shape), of


def total(res):
    return G[0] * res["rep_hand"] + G[1] * res["att"] + G[2] * res["rep_obj"]


@pytest.mark.parametrize("name", ["spheres", "torus"])
def test_gradient_against_central_differences(name):
    hv, hf, ov, of = pair(name, 5)
    r = np.random.default_rng(5)
    wr, wa, wo = r.uniform(0.5, 1.5, len(hv)), r.uniform(0.5, 1.5, len(hv)), r.uniform(0.5, 1.5, len(ov))
    run = lambda a, b: L.interaction_loss(a, hf, b, of, None, wr, wa, wo, ALPHA, *G)
    res = run(hv, ov)
    for q in (res["hand_q"], res["obj_q"]):
        assert q["dist"].min() > 1e-4 and np.abs(q["winding"] - 0.5).min() > 0.05
        assert (q["sdf"] < 0).sum() >= 5 and (q["sdf"] > 0).sum() >= 5     # both kinds of term are there
    assert res["rep_hand"] > 1e-4 and res["rep_obj"] > 1e-4 and res["att"] > 1e-3
    bound = sum((np.abs(q["coef"]) * 3 / np.maximum(q["d"], 1e-4) ** 2).sum() for q in (res["hand_q"], res["obj_q"]))
    bound += G[1] * 2 / ALPHA ** 2
    tol = H * H / 6 * bound + 4 * np.finfo(np.float64).eps * abs(total(res)) / H
    grad = np.concatenate([res["d_hand"].ravel(), res["d_obj"].ravel()])
    assert np.abs(grad).max() > 1e-3
    # directions: six random unit vectors over all coordinates, and the single coordinates with the largest and some random gradients
    dirs = [u / np.linalg.norm(u) for u in r.normal(size=(6, len(grad)))]
    for i in list(np.argsort(-np.abs(grad))[:6]) + list(r.integers(0, len(grad), 6)):
        e = np.zeros(len(grad))
        e[i] = 1.0
        dirs.append(e)
    worst = 0.0
    for u in dirs:
        dh, do = (H * u[:hv.size]).reshape(hv.shape), (H * u[hv.size:]).reshape(ov.shape)
        fd = (total(run(hv + dh, ov + do)) - total(run(hv - dh, ov - do))) / (2 * H)
        err = abs(fd - grad @ u)
        worst = max(worst, err)
        assert err <= tol, (name, err, tol, fd)
    print(f"{name}: largest gradient component {np.abs(grad).max():.3e}, worst central-difference error {worst:.2e}, bar {tol:.2e}")
    assert tol < 1e-4 * np.abs(grad).max()                    # the bar means something


def test_concentric_spheres_have_known_answers():
    v, f = O.icosphere(2)
    inradius = np.abs((np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]) * v[f[:, 0]]).sum(1)
                      / np.linalg.norm(np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]), axis=1)).min()
    assert 0.97 < inradius < 1
    c = np.array([0.03, -0.02, 0.7])
    # the hand (3 cm) inside the object (5 cm): every hand vertex is between 5 inradius - 3 and 2 cm deep, nothing else is non-zero
    res = L.interaction_loss(0.03 * v + c, f, 0.05 * v + c, f, alpha=ALPHA)
    assert 0.05 * inradius - 0.03 - 1e-12 <= res["rep_hand"] <= 0.02 + 1e-12
    assert res["att"] == 0 and res["rep_obj"] == 0 and not res["d_obj"][res["obj_q"]["coef"] != 0].size
    assert (res["hand_q"]["coef"] < 0).all() and (res["obj_q"]["coef"] == 0).all()
    # repulsion pushes the hand's vertices OUT of the object along -gradient: towards the nearest surface, away from the centre
    assert ((-res["d_hand"]) * v).sum(1).min() > 0
    # the other way round: the object inside the hand
    res = L.interaction_loss(0.05 * v + c, f, 0.03 * v + c, f, alpha=ALPHA)
    assert res["rep_hand"] == 0 and 0.05 * inradius - 0.03 - 1e-12 <= res["rep_obj"] <= 0.02 + 1e-12
    lo, hi = ALPHA * np.tanh((0.05 - 0.03) / ALPHA), ALPHA * np.tanh((0.05 - 0.03 * inradius) / ALPHA)
    assert lo - 1e-12 <= res["att"] <= hi + 1e-12
    # a sphere in a cube, the one case in closed form: a vertex p is a - max |p_k| deep
    bv, bf = O.box(1.0, 1.0, 1.0)
    res = L.interaction_loss(0.03 * v + c, f, 0.05 * bv + c, bf, alpha=ALPHA)
    want = (0.05 - np.abs(0.03 * v).max(1)).mean()
    assert abs(res["rep_hand"] - want) < 1e-15 and res["att"] == 0 and res["rep_obj"] == 0


def test_disjoint_spheres_do_not_repel():
    v, f = O.icosphere(2)
    c = np.array([0.03, -0.02, 0.7])
    res = L.interaction_loss(0.04 * v + c, f, 0.03 * v + c + [0.1, 0, 0], f, alpha=ALPHA, g_att=0.0)
    assert res["rep_hand"] == 0 and res["rep_obj"] == 0 and not res["d_hand"].any() and not res["d_obj"].any()
    # 3 cm apart at the nearest, 17 at the farthest: the attraction is saturated, between alpha tanh(3) and alpha
    assert ALPHA * np.tanh(0.03 / ALPHA) - 1e-9 < res["att"] < ALPHA
    res = L.interaction_loss(0.04 * v + c, f, 0.03 * v + c + [0.1, 0, 0], f, alpha=ALPHA)
    assert np.abs(res["d_hand"]).max() > 0 and np.abs(res["d_obj"]).max() > 0       # the attraction does pull
    assert res["d_hand"][:, 0].sum() < 0 < res["d_obj"][:, 0].sum()                  # descent moves the hand towards +x, the object to -x


def test_a_weight_of_zero_removes_the_vertex():
    hv, hf, ov, of = pair("torus", 5)
    full = L.interaction_loss(hv, hf, ov, of, alpha=ALPHA)
    inside, outside = int(np.argmin(full["hand_q"]["sdf"])), int(np.argmax(full["hand_q"]["sdf"]))
    obj_in = int(np.argmin(full["obj_q"]["sdf"]))
    wr, wa, wo = np.ones(len(hv)), np.ones(len(hv)), np.ones(len(ov))
    wr[inside] = wa[outside] = wo[obj_in] = 0
    res = L.interaction_loss(hv, hf, ov, of, None, wr, wa, wo, ALPHA)
    s = full["hand_q"]["sdf"]
    keep = np.arange(len(hv)) != inside
    assert abs(res["rep_hand"] - np.maximum(0, -s[keep]).mean()) < 1e-15 and res["rep_hand"] < full["rep_hand"]
    keep = np.arange(len(hv)) != outside
    assert abs(res["att"] - (ALPHA * np.tanh(np.maximum(0, s[keep]) / ALPHA)).mean()) < 1e-15
    so = full["obj_q"]["sdf"]
    assert abs(res["rep_obj"] - np.maximum(0, -so[np.arange(len(ov)) != obj_in]).mean()) < 1e-15
    assert res["hand_q"]["coef"][inside] == 0 and res["hand_q"]["coef"][outside] == 0 and res["obj_q"]["coef"][obj_in] == 0
    assert full["hand_q"]["coef"][inside] != 0 and full["hand_q"]["coef"][outside] != 0 and full["obj_q"]["coef"][obj_in] != 0
    # all weights of a term zero: the term is 0, not 0 / 0
    res = L.interaction_loss(hv, hf, ov, of, None, np.zeros(len(hv)), wa, wo, ALPHA)
    assert res["rep_hand"] == 0 and np.isfinite(res["d_hand"]).all() and np.isfinite(res["d_obj"]).all()


def test_padding_and_a_mesh_without_faces():
    hv, hf, ov, of = pair("torus", 5)
    full = L.interaction_loss(hv, hf, ov, of, alpha=ALPHA)
    padded = np.concatenate([ov, np.repeat(hv.mean(0)[None], 7, 0)])           # seven padding rows in the middle of the hand
    res = L.interaction_loss(hv, hf, padded, of, len(ov), alpha=ALPHA)
    # (the padding rows move the box the object is centred on: the last bits may differ, nothing else)
    for k in ("rep_hand", "att", "rep_obj"):
        assert abs(res[k] - full[k]) < 1e-15
    close = lambda a, b: np.abs(a - b).max() < 1e-14
    assert close(res["d_hand"], full["d_hand"]) and close(res["d_obj"][:len(ov)], full["d_obj"]) and not res["d_obj"][len(ov):].any()
    none = L.interaction_loss(hv, hf, ov, np.zeros((0, 3), np.int32), alpha=ALPHA)
    assert none["rep_hand"] == 0 and none["att"] == 0 and none["rep_obj"] == 0 and not none["d_hand"].any() and not none["d_obj"].any()
    assert (none["hand_q"]["dist"] == L.NO_FACE).all() and not len(none["obj_q"]["sdf"])
    tol_h, tol_o = L.grad_tolerance(full)
    assert tol_h.shape == (len(hv),) and tol_o.shape == (len(ov),) and tol_h.min() >= 1e-9 and tol_h.max() > 1e-9
    assert not L.near_surface(full["hand_q"]).any()
