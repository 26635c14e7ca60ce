"""Rigid pose refinement of the predicted pair against the two learned signed-distance fields (include/hoisdf.h "field fit",
csrc/field_fit.hip; the rules: hoisdf_amd/field_fit_oracle.py).  The test-time step of the SDF line this model descends from
(Grasping Field, AlignSDF, gSDF): the predicted hand mesh and the predicted object move, each as a rigid body, onto the zero level
set of the field the same network predicts.  Not in the reference; opt-in (cfg.eval_refine / HOISDF_REFINE=1 /
Evaluator(refine=True) / test.py --refine), off by default.  Limits: the field is the trilinear interpolant of the grid values,
not the network; rigid only - the hand's articulation stays as predicted; no gradient.  No weights are trained here: that the
step improves a metric is not claimed."""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import ops


def enabled(cfg=None) -> bool:
    """cfg.eval_refine (default False) or HOISDF_REFINE=1"""
    return bool(getattr(cfg, "eval_refine", False)) or os.environ.get("HOISDF_REFINE", "") == "1"


@torch.no_grad()
def fit_in_camera_frame(values, grid, n: int, points_cam, centre, scale: float, n_points=None, **fit) -> Dict[str, torch.Tensor]:
    """ops.field_fit on points given in the camera frame (metres) against a field whose frame is x_field = (x_cam - centre) * scale
    (Model.field_values: centre (B, 3), scale a float): the points go into the field's frame in float32, the posed points come back
    as x / scale + centre evaluated in float64 and rounded once.  ``fit``: the keywords of ops.field_fit.
    -> what ops.field_fit returns with points_out in the camera frame, trans in metres (trans / scale; rot needs no change: the
    frame change is a similarity) and trans_field = the translation in the field's frame."""
    points_cam, centre = points_cam.float(), centre.reshape(-1, 1, 3).float()
    res = dict(ops.field_fit(values, grid, n, (points_cam - centre) * float(scale), n_points=n_points, **fit))
    res["points_out"] = (res["points_out"].double() / float(scale) + centre.double()).float()
    res["trans_field"] = res["trans"]
    res["trans"] = (res["trans"].double() / float(scale)).float()
    return res


@torch.no_grad()
def fit_pair(model, feature_pyramid, meta, pair, iters: Optional[int] = None, huber: Optional[float] = None, **fit) -> Dict:
    """``pair``: what render.predicted_pair returns (hand (B, 778, 3), hand faces, obj (B, V, 3), obj faces, obj face counts, used),
    camera frame, metres.  For hand and object: the field on its refined grid (Model.field_values with cfg.refine_grid nodes -
    None: cfg.field_grid - and cfg.refine_pad_cells coarse cells around the inside nodes), the predicted vertices into the field's
    frame as (x - centre) * scale, hoisdf_field_fit (cfg.refine_iters, cfg.refine_huber unless given), the posed points back.
    -> {"pair": the refined pair (the same tuple with the two vertex arrays replaced), "hand": {rot (B, 3, 3), trans (B, 3) in
    metres, cost (B, 2), info (B, 4), ...}, "obj": the same}.  A sample whose object is not ``used`` is fitted like any other (it
    borrows template 0, as in the pair) and is for the caller to leave out.  Nothing synchronises."""
    c = model.cfg
    n = int(getattr(c, "refine_grid", None) or c.field_grid)
    fit.setdefault("iters", int(getattr(c, "refine_iters", 32)) if iters is None else int(iters))
    fit.setdefault("huber", float(getattr(c, "refine_huber", 0.1)) if huber is None else float(huber))
    hand, hf, obj, of, on, used = pair
    res = {}
    for kind, verts in (("hand", hand), ("obj", obj)):
        fv = model.field_values(feature_pyramid, meta, kind, n, max(n // 2, 2), pad_cells=int(getattr(c, "refine_pad_cells", 4)))
        res[kind] = fit_in_camera_frame(fv["values"], fv["grid"], n, verts.to(fv["values"].device), fv["centre"], fv["scale"], **fit)
    res["pair"] = (res["hand"]["points_out"], hf, res["obj"]["points_out"], of, on, used)
    return res
