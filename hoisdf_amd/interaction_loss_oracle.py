"""numpy restatement of csrc/interact_loss.hip (include/hoisdf.h "interaction loss"): ObMan's repulsion and attraction terms of a posed
hand mesh and a posed object mesh with their gradients towards both vertex arrays; the yardstick of
tests/test_interaction_loss_oracle.py and tests/test_gpu_interaction_loss.py.  Distance, closest face, barycentric weights and sign
are mesh_sdf_oracle.mesh_sdf's, everything in float64.  The derivative is the envelope rule: with c = sum_k beta_k x_k the closest
point on the winning face, d = |p - c|, n = (p - c) / d and the sign s held piecewise constant, d sdf / d p = s n and
d sdf / d x_k = -beta_k s n.  Per query point the float64 sdf, dist, winding and coef (the derivative of its terms by sdf, weights,
denominators and upstream gradients included) are returned with the answers, for the tests' tolerances and their rule on what lies
too close to a surface to be compared.  Not a fallback: nothing on the training path imports it."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from .mesh_sdf_oracle import mesh_sdf

NO_FACE = 3.0e38                                               # the distance of a mesh without a usable face


def _weights(w, n: int) -> np.ndarray:
    w = np.ones(n) if w is None else np.asarray(w, np.float64).reshape(-1)
    assert w.shape == (n,), (w.shape, n)
    return w


def _direction(points, live: int, verts, faces, w_rep, w_att, alpha: float, g_rep: float, g_att: float) -> Dict[str, np.ndarray]:
    """points[:live] as query points against the mesh (verts, faces) -> the two weighted means, the gradient towards the points
    (len(points), 3) and towards the mesh's vertices (len(verts), 3), and the per-query record"""
    P, V = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(verts, np.float64).reshape(-1, 3)
    F = np.asarray(faces, np.int64).reshape(-1, 3)
    q = mesh_sdf(P[:live], V, F)
    sdf, ok = q["sdf"], q["face"] >= 0
    w_rep = _weights(w_rep, len(P))[:live]
    den_rep = w_rep.sum()
    rep_term = np.where(ok, np.maximum(0, -sdf), 0)
    rep = float((w_rep * rep_term).sum() / den_rep) if den_rep > 0 else 0.0
    coef = np.where(ok & (sdf < 0) & (den_rep > 0), -g_rep * w_rep / (den_rep if den_rep > 0 else 1), 0.0)
    att = 0.0
    if w_att is not False:
        w_att = _weights(w_att, len(P))[:live]
        den_att = w_att.sum()
        x = np.where(ok, np.maximum(0, sdf), 0) / alpha
        att = float((w_att * alpha * np.tanh(x)).sum() / den_att) if den_att > 0 else 0.0
        coef = coef + np.where(ok & (sdf > 0) & (den_att > 0), g_att * w_att / (den_att if den_att > 0 else 1) * (1 - np.tanh(x) ** 2), 0.0)
    corners = F[np.maximum(q["face"], 0)] if len(F) else np.zeros((live, 3), np.int64)   # vertex indices of the winning face
    c = (q["bary"][:, :, None] * V[corners]).sum(1)                  # the closest point
    r = P[:live] - c
    d = np.sqrt((r * r).sum(1))
    use = ok & (d > 0) & (coef != 0)
    sign = np.where(sdf < 0, -1.0, 1.0)
    g = np.where(use[:, None], (coef * sign / np.where(d > 0, d, 1))[:, None] * r, 0.0)
    d_points, d_verts = np.zeros_like(P), np.zeros_like(V)
    d_points[:live] = g
    for k in range(3):
        np.add.at(d_verts, corners[use, k], -q["bary"][use, k, None] * g[use])
    return {"rep": rep, "att": att, "d_points": d_points, "d_verts": d_verts, "sdf": sdf, "dist": q["dist"], "winding": q["winding"],
            "face": q["face"], "bary": q["bary"], "corners": corners, "coef": np.where(use, coef, 0.0), "d": d}


def interaction_loss(hand_verts, hand_faces, obj_verts, obj_faces, obj_n_verts: Optional[int] = None, rep_w_hand=None,
                     att_w_hand=None, rep_w_obj=None, alpha: float = 0.01, g_rep_hand: float = 1.0, g_att: float = 1.0,
                     g_rep_obj: float = 1.0) -> Dict[str, object]:
    """ONE sample: hand_verts (Vh, 3), hand_faces (Fh, 3), obj_verts (Vo, 3) (rows from obj_n_verts on are padding), obj_faces
    (Fo, 3): only the faces that count; weights (V,) or None = ones; g_*: the upstream gradients ->
      rep_hand, att, rep_obj (float64), d_hand (Vh, 3), d_obj (Vo, 3) = the gradient of g_rep_hand rep_hand + g_att att + g_rep_obj
      rep_obj, hand_q / obj_q: per query point of the hand against the object / of the object's vertices that count against the
      hand: sdf, dist, winding, face, bary, corners (the winning face's vertex indices), coef, d (the distance to the closest point
      as the gradient used it)."""
    hv, ov = np.asarray(hand_verts, np.float64).reshape(-1, 3), np.asarray(obj_verts, np.float64).reshape(-1, 3)
    nvo = len(ov) if obj_n_verts is None else min(max(int(obj_n_verts), 0), len(ov))
    if not len(np.asarray(obj_faces).reshape(-1, 3)):                # a mesh without faces is absent: its vertices are no query points
        nvo = 0
    ho = _direction(hv, len(hv) if len(np.asarray(hand_faces).reshape(-1, 3)) else 0, ov, obj_faces, rep_w_hand, att_w_hand, alpha, g_rep_hand, g_att)
    oh = _direction(ov, nvo, hv, hand_faces, rep_w_obj, False, alpha, g_rep_obj, 0.0)
    keep = ("sdf", "dist", "winding", "face", "bary", "corners", "coef", "d")
    return {"rep_hand": ho["rep"], "att": ho["att"], "rep_obj": oh["rep"], "d_hand": ho["d_points"] + oh["d_verts"],
            "d_obj": oh["d_points"] + ho["d_verts"], "hand_q": {k: ho[k] for k in keep}, "obj_q": {k: oh[k] for k in keep}}


def grad_tolerance(res, delta: float = 5e-7, floor: float = 1e-9):
    """the bar of a gradient computed from closest points that are off by at most `delta`: such a point turns n by at most
    2 delta / d, so destination vertex u may be off by sum_i |coef_i| beta_ik 2 delta / d_i over the query points i that contribute
    to it (its own term, beta = 1, included), plus `floor` -> (tol_hand (Vh,), tol_obj (Vo,))"""
    tol = [np.full(len(res["d_hand"]), floor), np.full(len(res["d_obj"]), floor)]
    for own, q in ((0, res["hand_q"]), (1, res["obj_q"])):
        use = q["coef"] != 0
        t = np.where(use, np.abs(q["coef"]) * 2 * delta / np.where(q["d"] > 0, q["d"], 1), 0.0)
        tol[own][:len(t)] += t
        for k in range(3):
            np.add.at(tol[1 - own], q["corners"][use, k], (q["bary"][:, k] * t)[use])
    return tol[0], tol[1]


def near_surface(q, dist: float = 1e-4, wind: float = 0.05) -> np.ndarray:
    """the query points whose float64 answer does not bind an fp32 evaluation: |sdf| < dist or winding within `wind` of 0.5"""
    return (q["dist"] < dist) | (np.abs(q["winding"] - 0.5) <= wind)
