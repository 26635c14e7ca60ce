"""Evaluation metrics of the reference's test driver, batched on the device.

  hand:    MJE / PA-MJE                         common/metrics.py:188-232 (rigid_transform_3D, rigid_align, eval_hand_joint)
  object:  ADD-S, MCE (bbox-corner error), OCE (centre error), MME (mean mesh error)
                                                 common/metrics.py:62-185 (compute_obj_metrics_*, eval_batched_obj_direct)
  mesh:    per-vertex EPE mean / AUC over thresholds (EvalUtil.get_measures) and F-scores at 5 / 15 mm
                                                 common/eval_util.py:11-136, main/test.py:204-261
  results.txt / pred_mano.json writers           main/test.py:229-265, data/ho3d_util.py:123-134

The reference loops over samples on the host (numpy SVD per sample, open3d nearest neighbours per mesh); here every
metric is one batched torch expression on the GPU (the N x N distance matrices of ADD-S / F-score are 778^2 ... 2000^2
per sample).  Object templates are dataset assets (YCB models) - callers pass ``templates[obj_id] = (V, 3)`` tensors.

The ``*_native`` functions and ``MeshEvalNative`` are the same metrics through the hoisdf_eval_* entries of the C ABI (csrc/eval.hip,
ops.eval_*): no distance matrix, an fp64 Jacobi SVD in the kernel, integer threshold counts, running mesh sums on the device.
Opt-in (``cfg.native_metrics`` / ``HOISDF_METRICS=native`` / ``test.py --native-metrics``); GPU only, no fallback.  ``Evaluator`` is
the per-batch bookkeeping of test.py over either backend.

Not in the reference: ``Evaluator(interaction=True)`` (``cfg.eval_interaction`` / ``HOISDF_INTERACTION=1`` / ``test.py --interaction``)
also asks whether the PREDICTED hand and the PREDICTED object are compatible with each other - penetration depth, contact ratio and
intersection volume, the numbers of ObMan and its successors - through hoisdf_eval_interaction (csrc/interact.hip, ops.eval_interaction)
and appends them to results.txt.  Off by default: the file is then what the reference writes.
``Evaluator(field=True)`` (``cfg.eval_field`` / ``HOISDF_FIELD=1`` / ``test.py --field-surface``) measures the zero level sets of the two
learned fields (Model.field_surface: hoisdf_iso_extract, csrc/isosurf.hip) against the ground-truth meshes - the Chamfer distance of
AlignSDF and gSDF, through hoisdf_eval_surface (ops.eval_surface) - and appends a ``Field:`` block after everything else.  Off by default.
``Evaluator(silhouette=True)`` (``cfg.eval_silhouette`` / ``HOISDF_SILHOUETTE=1`` / ``test.py --silhouette``) renders the predicted pair
with mutual occlusion (hoisdf_raster_meshes, csrc/raster.hip) and appends a ``Silhouette:`` block - the IoU of its two modal masks against
the mask targets - after everything else.  Off by default.
``Evaluator(refine=True)`` (``cfg.eval_refine`` / ``HOISDF_REFINE=1`` / ``test.py --refine``) measures the predicted pair before and after
its rigid fit to the two learned fields (refine.fit_pair: hoisdf_field_fit, csrc/field_fit.hip, run by the eval forward) against the
ground-truth meshes and appends a ``Refined:`` block after everything else.  Off by default.
"""
from __future__ import annotations

import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

_trapz = getattr(np, "trapezoid", None) or np.trapz


# ---- rotations -------------------------------------------------------------------------------------------------
def batch_rodrigues(aa: torch.Tensor) -> torch.Tensor:
    """axis-angle (B,3) -> (B,3,3), the quaternion form of manopth/rodrigues_layer.py:38-89 (|aa| + 1e-8)."""
    ang = (aa + 1e-8).norm(dim=1, keepdim=True)
    n = aa / ang
    h = 0.5 * ang
    w, xyz = torch.cos(h), torch.sin(h) * n
    q = torch.cat([w, xyz], 1)
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z,
                     2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x,
                     2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z], 1)
    return R.view(-1, 3, 3)


# ---- hand ------------------------------------------------------------------------------------------------------
def rigid_align(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """similarity (scale + rotation + translation) alignment of A (N,P,3) onto B (N,P,3), batched
    (common/metrics.py:188-211: H = (A-ca)^T (B-cb) / n, SVD, reflection fix on the last singular vector)."""
    A64, B64 = A.double(), B.double()
    ca, cb = A64.mean(1, keepdim=True), B64.mean(1, keepdim=True)
    H = (A64 - ca).transpose(1, 2) @ (B64 - cb) / A.shape[1]
    U, s, Vh = torch.linalg.svd(H)
    R = Vh.transpose(1, 2) @ U.transpose(1, 2)
    neg = torch.linalg.det(R) < 0
    s = s.clone()
    s[neg, -1] = -s[neg, -1]
    Vh = Vh.clone()
    Vh[neg, 2] = -Vh[neg, 2]
    R = Vh.transpose(1, 2) @ U.transpose(1, 2)
    varP = A64.var(dim=1, unbiased=False).sum(1)
    c = s.sum(1) / varP
    t = -(c[:, None, None] * R @ ca.transpose(1, 2)).transpose(1, 2) + cb
    return ((c[:, None, None] * R @ A64.transpose(1, 2)).transpose(1, 2) + t).to(A.dtype)


def eval_hand_joint(pred: torch.Tensor, gt: torch.Tensor) -> Tuple[float, float]:
    """(MJE, PA-MJE): mean over samples of the mean per-joint error (common/metrics.py:214-232)."""
    mje = (pred - gt).norm(dim=-1).mean(1)
    pa = (rigid_align(pred, gt) - gt).norm(dim=-1).mean(1)
    return float(mje.mean()), float(pa.mean())


# ---- object ----------------------------------------------------------------------------------------------------
_CORNERS = torch.tensor([[0, 1, 0, 0, 1, 0, 1, 1], [0, 0, 1, 0, 1, 1, 0, 1], [0, 0, 0, 1, 0, 1, 1, 1]])


def _adds(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """ADD-S per sample: mean over PREDICTED vertices of the distance to the closest target vertex."""
    return torch.cdist(pred, target).min(dim=2)[0].mean(1)


def _bbox_corners(m: torch.Tensor) -> torch.Tensor:
    mm = torch.stack([m.min(1)[0], m.max(1)[0]], 2)                       # (B,3,2)
    idx = _CORNERS.to(m.device)
    return torch.stack([mm[:, 0, idx[0]], mm[:, 1, idx[1]], mm[:, 2, idx[2]]], 2)   # (B,8,3)


def obj_metrics(obj_rot, obj_trans, obj_rot_gt, obj_trans_gt, template_verts, ho3d: bool):
    """common/metrics.py:118-185.  obj_rot / obj_trans: per-point predictions (B,P,3) -> averaged over points;
    template_verts (B,V,3).  Returns dict of per-batch means: ADDS + (MCE, OCE | MME)."""
    rot, trans = obj_rot.detach().mean(1), obj_trans.detach().mean(1)
    tgt = template_verts @ batch_rodrigues(obj_rot_gt).transpose(1, 2) + obj_trans_gt[:, None]
    prd = template_verts @ batch_rodrigues(rot).transpose(1, 2) + trans[:, None]
    out = {"ADDS": float(_adds(prd, tgt).mean())}
    if ho3d:
        out["MME"] = float((tgt - prd).norm(dim=-1).mean(-1).mean())
    else:
        out["MCE"] = float((_bbox_corners(prd) - _bbox_corners(tgt)).norm(dim=-1).mean(-1).mean())
        out["OCE"] = float((trans - obj_trans_gt).norm(dim=-1).mean())
    return out


# ---- mesh ------------------------------------------------------------------------------------------------------
def fscore(gt: torch.Tensor, pr: torch.Tensor, th: float) -> torch.Tensor:
    """per-sample F-score at threshold th (common/eval_util.py:117-136; nearest-neighbour distances both ways)."""
    d = torch.cdist(gt, pr)
    d1, d2 = d.min(2)[0], d.min(1)[0]                 # gt -> closest pred, pred -> closest gt
    recall = (d2 < th).float().mean(1)
    precision = (d1 < th).float().mean(1)
    s = recall + precision
    return torch.where(s > 0, 2 * recall * precision / s.clamp_min(1e-30), torch.zeros_like(s))


class MeshEval:
    """EvalUtil(num_kp=778).feed / get_measures (common/eval_util.py:11-103) for fully visible meshes."""

    def __init__(self):
        self.dist: List[torch.Tensor] = []

    def feed(self, gt: torch.Tensor, pred: torch.Tensor):
        self.dist.append((gt - pred).norm(dim=-1).double().cpu())          # (B,V)

    def get_measures(self, val_min: float, val_max: float, steps: int):
        d = torch.cat(self.dist, 0).numpy()                                   # (N,V)
        th = np.linspace(val_min, val_max, steps)
        norm = _trapz(np.ones_like(th), th)
        epe_mean = d.mean(0).mean()
        pck = (d[None] <= th[:, None, None]).mean(1)                          # (steps,V)
        auc = (_trapz(pck, th, axis=0) / norm).mean()
        return float(epe_mean), float(np.median(d, 0).mean()), float(auc), pck.mean(1), th


# ---- writers ---------------------------------------------------------------------------------------------------
def write_results(path: str, results: Dict[str, float], total_samples: int, mesh: Optional[Tuple[MeshEval, MeshEval]] = None,
                  fscores: Optional[Tuple[np.ndarray, np.ndarray, Sequence[float]]] = None) -> None:
    """results.txt in the reference's layout (main/test.py:229-261): ``key :  value`` lines, then the mesh block."""
    with open(path, "w+") as f:
        for k, v in results.items():
            print(k, ": ", v / total_samples, file=f)
        if mesh is not None:
            m3d, _, auc, _, _ = mesh[0].get_measures(0.0, 0.05, 100)
            print("Evaluation 3D MESH results:", file=f)
            print("auc=%.3f, mean_vert3d_avg=%.2f cm" % (auc, m3d * 100.0), file=f)
            m3d, _, auc, _, _ = mesh[1].get_measures(0.0, 0.05, 100)
            print("Evaluation 3D MESH ALIGNED results:", file=f)
            print("auc=%.3f, mean_vert3d_avg=%.2f cm\n" % (auc, m3d * 100.0), file=f)
        if fscores is not None:
            print("F-scores", file=f)
            fs, fa, ths = fscores
            for a, b, t in zip(fs, fa, ths):
                print("F@%.1fmm = %.3f" % (t * 1000, a.mean()), "\tF_aligned@%.1fmm = %.3f" % (t * 1000, b.mean()), file=f)


def dump_pred_mano(path: str, xyz_pred_list, verts_pred_list) -> None:
    """pred_mano.json of the HO3D submission format (data/ho3d_util.py:123-134): [[joints...], [verts...]]."""
    with open(path, "w") as fo:
        json.dump([[np.asarray(x).tolist() for x in xyz_pred_list], [np.asarray(v).tolist() for v in verts_pred_list]], fo)


# ---- the same metrics through the C ABI (csrc/eval.hip) ----------------------------------------------------------------
def native_metrics_enabled(cfg=None) -> bool:
    """cfg.native_metrics (default False) or HOISDF_METRICS=native: the Evaluator runs the hoisdf_eval_* entries"""
    return bool(getattr(cfg, "native_metrics", False)) or os.environ.get("HOISDF_METRICS", "") == "native"


def obj_metrics_native(obj_rot, obj_trans, obj_rot_gt, obj_trans_gt, templates, obj_ids, ho3d: bool):
    """``obj_metrics`` through hoisdf_eval_object.  The template of each sample is named, not gathered: templates (T,V,3) and
    obj_ids (B,) (``obj_metrics`` takes templates[obj_ids]).  Same dict of per-batch means (one read-back)."""
    from . import ops
    adds, mce, oce, mme, _ = ops.eval_object(obj_rot, obj_trans, obj_rot_gt, obj_trans_gt, templates, obj_ids)
    m = torch.stack([adds.mean(), mce.mean(), oce.mean(), mme.mean()]).tolist()
    return {"ADDS": m[0], "MME": m[3]} if ho3d else {"ADDS": m[0], "MCE": m[1], "OCE": m[2]}


def rigid_align_native(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """``rigid_align`` through hoisdf_eval_hand_joints (any number of points)"""
    from . import ops
    return ops.eval_hand_joints(A, B, want_aligned=True)[2]


def eval_hand_joint_native(pred: torch.Tensor, gt: torch.Tensor) -> Tuple[float, float]:
    """``eval_hand_joint`` through hoisdf_eval_hand_joints: (MJE, PA-MJE) batch means (one read-back)"""
    from . import ops
    mje, pa = ops.eval_hand_joints(pred, gt)[:2]
    m = torch.stack([mje.mean(), pa.mean()]).tolist()
    return m[0], m[1]


def fscore_native(gt: torch.Tensor, pr: torch.Tensor, th: float) -> torch.Tensor:
    """``fscore`` through hoisdf_eval_mesh: per-sample F-score of pr against gt at threshold th, no alignment.  (The Evaluator
    asks for every threshold, raw and aligned, in one call: ops.eval_mesh.)"""
    from . import ops
    return ops.eval_mesh(pr, gt, [float(th)])[2][:, 0]


def interaction_enabled(cfg=None) -> bool:
    """cfg.eval_interaction (default False) or HOISDF_INTERACTION=1: the Evaluator appends the interaction block"""
    return bool(getattr(cfg, "eval_interaction", False)) or os.environ.get("HOISDF_INTERACTION", "") == "1"


def silhouette_enabled(cfg=None) -> bool:
    """cfg.eval_silhouette (default False) or HOISDF_SILHOUETTE=1: the Evaluator appends the silhouette block"""
    return bool(getattr(cfg, "eval_silhouette", False)) or os.environ.get("HOISDF_SILHOUETTE", "") == "1"


def field_enabled(cfg=None) -> bool:
    """cfg.eval_field (default False) or HOISDF_FIELD=1: the eval forward extracts the two field surfaces and the Evaluator appends
    the Field block"""
    return bool(getattr(cfg, "eval_field", False)) or os.environ.get("HOISDF_FIELD", "") == "1"


class MeshEvalNative:
    """``MeshEval`` on the device (hoisdf_eval_accum_*): one fp64 sum per vertex and one count per (threshold, vertex) instead of
    every distance of the test set on the host.  The thresholds are fixed when the object is made, since the counts are taken as
    the samples arrive; ``get_measures`` must be asked for the same ones.  The MEDIAN error needs every distance and is not
    provided: ``get_measures`` returns NaN in its place (results.txt does not print it)."""

    def __init__(self, val_min: float = 0.0, val_max: float = 0.05, steps: int = 100):
        self.range = (float(val_min), float(val_max), int(steps))
        self.th = np.linspace(val_min, val_max, steps)
        self.state = self.th_dev = None
        self.V = 0

    def feed_dist(self, dist: torch.Tensor):
        """per-vertex distances (B,V) float32 on the device, as ops.eval_mesh returns them"""
        from . import ops
        if self.state is None:
            self.V = dist.shape[1]
            self.th_dev = ops.eval_thresholds(self.th, dist.device)
            self.state = ops.eval_accum_init(self.V, len(self.th), dist.device)
        assert dist.shape[1] == self.V, (tuple(dist.shape), self.V)
        ops.eval_accumulate(self.state, dist, self.th_dev)

    def feed(self, gt: torch.Tensor, pred: torch.Tensor):
        from . import ops
        self.feed_dist(ops.eval_hand_joints(pred, gt, want_dist=True)[4])

    def measures_device(self) -> torch.Tensor:
        """(2 + steps,) float64 on the device: mean EPE, AUC, PCK curve; nothing is read back"""
        from . import ops
        assert self.state is not None, "MeshEvalNative: nothing was fed"
        return ops.eval_accum_finish(self.state, self.V, self.th_dev)

    def get_measures(self, val_min: float, val_max: float, steps: int):
        assert (float(val_min), float(val_max), int(steps)) == self.range, ((val_min, val_max, steps), self.range)
        m = self.measures_device().cpu().numpy()
        return float(m[0]), float("nan"), float(m[1]), m[2:].copy(), self.th


# ---- the per-batch bookkeeping of the test driver (main/test.py:100-265) -----------------------------------------------
# data/ho3d.py:47-70: jointsMapSimpleToMano = argsort(jointsMapManoToSimple) - the order of the HO3D submission file
JOINTS_SIMPLE_TO_MANO = [0, 5, 6, 7, 9, 10, 11, 17, 18, 19, 13, 14, 15, 1, 2, 3, 4, 8, 12, 16, 20]
F_THRESHS = [0.005, 0.015]


class Evaluator:
    """Running evaluation of a test set: ``feed`` one batch of model outputs, ``write`` results.txt (and pred_mano.json for ho3d).
    templates (T,V,3) on the evaluation device; obj_cls (B,) = the template of each sample.  ``native=False`` is the batched torch
    path (every ``feed`` reads its batch means back); ``native=True`` runs the hoisdf_eval_* entries, keeps the running sums, the
    F-scores and the mesh accumulators on the device and reads them once in ``write``.  Only the native path knows samples that are not
    evaluated (obj_cls < 0): they count for the hand keys and not for the object keys (*_error).
    ``interaction=True`` (or cfg.eval_interaction / HOISDF_INTERACTION=1; either backend - there is one implementation): every
    ``feed`` also poses the PREDICTED pair in the camera frame - hand = the predicted MANO mesh + mano_root, object = the template
    turned and moved by the mean predicted rotation and translation + obj_center_cam - runs ops.eval_interaction on it (cfg.contact_dist,
    cfg.interaction_voxel) and keeps running sums on the device; ``write`` appends one block after everything else.  It needs the
    templates as meshes: ``template_faces`` = the ``faces`` (T,F,3) / ``n_faces`` (T,) of sdf_data.pack_templates (whose ``verts`` are
    ``templates``), and ``hand_faces`` (Fh,3) = the MANO layer's ``th_faces``.  Samples with obj_cls < 0 are not evaluated.
    ``field=True`` (or cfg.eval_field / HOISDF_FIELD=1; either backend): where a batch carries the ground-truth MANO mesh (the
    condition of the mesh block) and the field surfaces of the eval forward (``field_{hand,obj}_verts`` / ``_n_verts`` / ``_n_faces``,
    Model.field_surface), every ``feed`` runs ops.eval_surface of the hand surface against the ground-truth MANO mesh + mano_root and
    of the object surface against the template posed by the GROUND-TRUTH rotation and translation + obj_center_cam
    (cfg.field_samples points), keeps running sums on the device, and ``write`` appends one ``Field:`` block after everything else:
    the mean Chamfer distances in cm^2 over the samples that took part and the share of samples left out - a surface without a
    vertex, one that overflowed its capacity, a ground-truth mesh without area, for the object also obj_cls < 0.  It needs the same
    ``template_faces`` / ``hand_faces``.
    ``silhouette=True`` (or cfg.eval_silhouette / HOISDF_SILHOUETTE=1; either backend): every ``feed`` renders the predicted pair
    (render.predicted_pair, the pair of the interaction block) with mutual occlusion through meta["cam_intr"] at cfg.input_img_shape
    (ops.raster_meshes), folds the two modal masks to the shape of targets["hand_seg"] / ["obj_seg"] and counts intersection and
    union against them on the device (ops.eval_silhouette); ``write`` reads the integer counts once, divides in float64 on the host
    and appends one ``Silhouette:`` block after everything else: the mean IoU of the hand and of the object over the samples that
    took part and the share of samples left out - an empty union, or obj_cls < 0.  It needs the same ``template_faces`` /
    ``hand_faces``.
    ``refine=True`` (or cfg.eval_refine / HOISDF_REFINE=1; either backend; in the signature it stands before ``field``, which stays
    last: pass the switches by keyword): where a batch carries the ground-truth MANO mesh and the refined pair of the eval forward
    (``refined_{hand,obj}_verts``, ``refine_{hand,obj}_{cost,info}``: refine.fit_pair, hoisdf_field_fit), every ``feed`` measures the
    mean vertex error of the hand against the ground-truth MANO mesh + mano_root and of the object against the template posed by the
    ground-truth pose, before and after the fit, keeps running sums on the device, and ``write`` appends one ``Refined:`` block
    after everything else: both errors in cm, the mean start and end cost and the mean tried steps per field over the samples that
    took part, and the share left out - a fit without a point on the grid (info[0] == 0), for the object also obj_cls < 0.  It
    needs the same ``template_faces`` / ``hand_faces`` (render.predicted_pair poses the pair from them)."""

    def __init__(self, cfg, templates: torch.Tensor, native: bool = False, interaction: bool = False,
                 template_faces: Optional[Dict[str, torch.Tensor]] = None, hand_faces: Optional[torch.Tensor] = None,
                 silhouette: bool = False, refine: bool = False, field: bool = False):
        from .refine import enabled as refine_enabled
        self.cfg, self.templates, self.native = cfg, templates, bool(native)
        self.dev = templates.device
        self.interaction = bool(interaction) or interaction_enabled(cfg)
        self.field = bool(field) or field_enabled(cfg)
        self.silhouette = bool(silhouette) or silhouette_enabled(cfg)
        self.refine = bool(refine) or refine_enabled(cfg)
        self._hfaces = None
        if self.refine:
            # per field (hand, obj): the sums of the mean vertex error before and after [m], of the start and the end cost and of the
            # tried steps over the samples that took part, their number, the samples seen
            self._racc = torch.zeros(2, 7, device=self.dev, dtype=torch.float64)
        if self.silhouette:
            self._scounts = []          # per feed: int32 (B, 5) on the device = the four counts of ops.eval_silhouette, obj_cls >= 0
        if self.field:
            # per field (hand, obj): the sum of the Chamfer distances [m^2] over the samples that took part, their number, the samples seen
            self._facc = torch.zeros(2, 3, device=self.dev, dtype=torch.float64)
        have_faces = template_faces is not None and hand_faces is not None and "faces" in template_faces
        if (self.interaction or self.field or self.silhouette or self.refine) and not have_faces:
            raise ValueError("Evaluator(interaction=True) / Evaluator(field=True) / Evaluator(silhouette=True) / Evaluator(refine=True) needs "
                             "template_faces (faces, n_faces of sdf_data.pack_templates) and hand_faces")
        if have_faces:                                            # (also without a block: render.predicted_pair poses from them)
            self._tfaces = torch.as_tensor(template_faces["faces"]).to(self.dev, torch.int32)
            n = template_faces.get("n_faces")
            self._tn = torch.full((self._tfaces.shape[0],), self._tfaces.shape[1], dtype=torch.int32) if n is None else torch.as_tensor(n)
            self._tn = self._tn.to(self.dev, torch.int32)
            self._hfaces = torch.as_tensor(hand_faces).to(self.dev, torch.int32)
            if self._tfaces.dim() != 3 or self._tfaces.shape[0] != templates.shape[0] or self._tn.shape != (templates.shape[0],):
                raise ValueError(f"template_faces {tuple(self._tfaces.shape)} for {templates.shape[0]} templates")
        if self.interaction:
            # the sums of max(pen_hand, pen_obj) [m], in_contact, volume [m^3], contact_verts over the evaluated samples, their number
            self._iacc = torch.zeros(5, device=self.dev, dtype=torch.float64)
        self.ho3d = cfg.dataset == "ho3d"
        keys = ["ADDS_error"] + (["MME_error"] if self.ho3d else ["mano_mje", "mano_pamje", "OCE_error", "MCE_error"])
        self.results = {k: 0.0 for k in keys}                 # torch path: running sums on the host, in cm
        # native path: one device vector - the sum of every key's per-sample values [m], then the number of samples whose object was
        # evaluated (hoisdf_eval_object's used flag); one stacked reduction per batch, read once in write()
        self._acc = torch.zeros(len(keys) + 1, device=self.dev, dtype=torch.float64) if self.native else None
        self.total = 0
        if self.ho3d:
            self.coord_change = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]], device=self.dev)
            self.joint_list, self.mesh_list = [], []
        else:
            cls = MeshEvalNative if self.native else MeshEval
            self.mesh_err, self.mesh_err_al = cls(), cls()
            self.f_score, self.f_score_al, self.f_threshs = [], [], list(F_THRESHS)
            self._fth = None

    def _add(self, vals, B, used=None):
        """vals: key -> the batch mean on the host (torch path) or the per-sample device values (native path)"""
        if self.native:
            self._acc += torch.stack([vals[k] for k in self.results] + [used.float()]).sum(1, dtype=torch.float64)
        else:
            for k, v in vals.items():
                self.results[k] += v * B * 100

    def feed(self, out, targets, meta, obj_cls) -> None:
        from . import ops
        cfg, dev, ho3d = self.cfg, self.dev, self.ho3d
        B = meta["mano_root"].shape[0]
        tg = {k: v.to(dev) for k, v in targets.items()}
        root = meta["mano_root"].to(dev)
        if self.native:
            adds, mce, oce, mme, used = ops.eval_object(out["obj_rot_out"], out["obj_trans_out"], tg["obj_rot"], tg["rel_obj_trans"],
                                                        self.templates, obj_cls)
            om = {"ADDS": adds, "MCE": mce, "OCE": oce, "MME": mme}
        else:
            used = None
            om = obj_metrics(out["obj_rot_out"], out["obj_trans_out"], tg["obj_rot"], tg["rel_obj_trans"],
                             self.templates[obj_cls], ho3d)
        self.total += B
        if self.interaction:
            self._feed_interaction(out, meta, obj_cls)
        if self.silhouette:
            self._feed_silhouette(out, tg, meta, obj_cls)
        if ho3d:                                                                  # main/test.py:133-176
            if cfg.use_inverse_kinematics:
                joints, mesh = out["ik_joints_out"], out["ik_verts_out"]
            else:
                joints, mesh = out["mano_joints_out"], out["mano_mesh_out"]
            joints = (joints + root[:, None]) @ self.coord_change
            mesh = (mesh + root[:, None]) @ self.coord_change
            self._add({"ADDS_error": om["ADDS"], "MME_error": om["MME"]}, B, used)
            if self.native:                                                       # read back in write()
                self.joint_list.append(joints[:, JOINTS_SIMPLE_TO_MANO])
                self.mesh_list.append(mesh)
            else:
                self.joint_list += [j[JOINTS_SIMPLE_TO_MANO] for j in joints.cpu().numpy()]
                self.mesh_list += list(mesh.cpu().numpy())
            return
        if cfg.use_inverse_kinematics:                                            # main/test.py:178-225
            pj, gj = out["ik_joints_out"] - out["ik_joints_out"][:, :1], tg["joint_cam_no_trans"] / 1000
        else:
            pj, gj = out["mano_joints_out"], out["mano_joints_gt_out"]
        mje, pamje = ops.eval_hand_joints(pj, gj)[:2] if self.native else eval_hand_joint(pj, gj)
        self._add({"ADDS_error": om["ADDS"], "mano_mje": mje, "mano_pamje": pamje, "OCE_error": om["OCE"], "MCE_error": om["MCE"]}, B, used)
        if self.field and cfg.eval_mesh and "mano_mesh_gt_out" in out and "field_hand_verts" in out:
            self._feed_field(out, tg, meta, obj_cls)
        if self.refine and "mano_mesh_gt_out" in out and "refined_hand_verts" in out:
            self._feed_refine(out, tg, meta, obj_cls)
        if cfg.eval_mesh and "mano_mesh_out" in out:
            pv, gv = out["mano_mesh_out"], out["mano_mesh_gt_out"]
            if self.native:
                if self._fth is None:
                    self._fth = ops.eval_thresholds(self.f_threshs, dev)
                d0, d1, f0, f1, _ = ops.eval_mesh(pv, gv, self._fth)
                self.mesh_err.feed_dist(d0)
                self.mesh_err_al.feed_dist(d1)
                self.f_score.append(f0)
                self.f_score_al.append(f1)
            else:
                al = rigid_align(pv, gv)
                self.mesh_err.feed(gv, pv)
                self.mesh_err_al.feed(gv, al)
                self.f_score.append(torch.stack([fscore(gv, pv, t) for t in self.f_threshs], 1).cpu().numpy())
                self.f_score_al.append(torch.stack([fscore(gv, al, t) for t in self.f_threshs], 1).cpu().numpy())

    def interaction_per_sample(self, out, meta, obj_cls):
        """ops.eval_interaction on the predicted pair of every sample -> (its dict, used (B,) bool: obj_cls >= 0)"""
        from . import ops
        from .render import predicted_pair
        hand, hf, obj, of, on, used = predicted_pair(out, meta, obj_cls, self)
        return ops.eval_interaction(hand, hf, obj, of, on, None, self.cfg.contact_dist, self.cfg.interaction_voxel), used

    def silhouette_per_sample(self, out, targets, meta, obj_cls):
        """the predicted pair rendered and counted against the mask targets -> (counts int32 (B, 4) = hand intersection, hand union,
        object intersection, object union, used (B,) bool: obj_cls >= 0), on the device"""
        from . import ops
        from .render import predicted_pair, render_pair
        pair = predicted_pair(out, meta, obj_cls, self)
        masks = render_pair(pair, meta["cam_intr"], self.cfg, want=(), masks=True)
        gh, go = targets["hand_seg"].to(self.dev), targets["obj_seg"].to(self.dev)
        if gh.shape != masks["hand_seg"].shape or go.shape != masks["obj_seg"].shape:
            raise ValueError(f"silhouette: mask targets {tuple(gh.shape)} / {tuple(go.shape)}, rendered {tuple(masks['hand_seg'].shape)}")
        return ops.eval_silhouette(masks["hand_seg"], masks["obj_seg"], gh, go), pair[5]

    def _feed_silhouette(self, out, targets, meta, obj_cls) -> None:
        counts, used = self.silhouette_per_sample(out, targets, meta, obj_cls)
        self._scounts.append(torch.cat([counts, used.to(torch.int32)[:, None]], 1))

    def _feed_interaction(self, out, meta, obj_cls) -> None:
        r, used = self.interaction_per_sample(out, meta, obj_cls)
        vals = torch.stack([torch.maximum(r["pen_hand"], r["pen_obj"]).double(), r["in_contact"].double(), r["volume"].double(),
                            r["contact_verts"].double(), torch.ones_like(r["volume"]).double()])
        self._iacc += (vals * used.double()[None]).sum(1)

    def field_per_sample(self, out, targets, meta, obj_cls):
        """ops.eval_surface of the two field surfaces of every sample -> {"hand": (its dict, used (B,) bool), "obj": ...}; used: the
        sample took part (n_used > 0, no overflowed capacity, for the object obj_cls >= 0)"""
        from . import ops
        dev = self.dev
        root = meta["mano_root"].to(dev)
        cls = torch.as_tensor(obj_cls).to(dev).long()
        known = cls >= 0
        cls = cls.clamp_min(0)
        gt_hand = out["mano_mesh_gt_out"].detach() + root[:, None]
        R = batch_rodrigues(targets["obj_rot"].to(dev).reshape(-1, 3))
        gt_obj = self.templates[cls] @ R.transpose(1, 2) + (targets["rel_obj_trans"].to(dev).reshape(-1, 3) + meta["obj_center_cam"].to(dev))[:, None]
        res = {}
        for kind, gv, gf, gn, ok in (("hand", gt_hand, self._hfaces, None, torch.ones_like(known)),
                                     ("obj", gt_obj, self._tfaces[cls], self._tn[cls], known)):
            v, nv, nf = out[f"field_{kind}_verts"], out[f"field_{kind}_n_verts"], out[f"field_{kind}_n_faces"]
            r = ops.eval_surface(v, nv, gv, gf, gn, int(getattr(self.cfg, "field_samples", 4096)), seed=self.total)
            fits = (nv <= v.shape[1]) & (nf <= out[f"field_{kind}_faces"].shape[1])
            res[kind] = (r, ok & fits & (r["n_used"] > 0))
        return res

    def _feed_field(self, out, targets, meta, obj_cls) -> None:
        res = self.field_per_sample(out, targets, meta, obj_cls)
        self._facc += torch.stack([torch.stack([(r["chamfer"].double() * used.double()).sum(), used.double().sum(),
                                                torch.tensor(float(used.numel()), device=self.dev, dtype=torch.float64)])
                                   for r, used in (res["hand"], res["obj"])])

    def refine_per_sample(self, out, targets, meta, obj_cls):
        """the refined pair of the eval forward (refine.fit_pair) against the ground truth -> {"hand": (before (B,), after (B,): the
        mean vertex error in metres against the ground-truth MANO mesh + mano_root, cost (B, 2), info (B, 4), used (B,) bool),
        "obj": the same against the template posed by the ground-truth rotation and translation + obj_center_cam}; used: the fit had
        a point to work with (info[0] > 0), for the object also obj_cls >= 0"""
        from .render import predicted_pair
        dev = self.dev
        root = meta["mano_root"].to(dev)
        hand, _, obj, _, _, known = predicted_pair(out, meta, obj_cls, self)
        cls = torch.as_tensor(obj_cls).to(dev).long().clamp_min(0)
        gt_hand = out["mano_mesh_gt_out"].detach() + root[:, None]
        R = batch_rodrigues(targets["obj_rot"].to(dev).reshape(-1, 3))
        gt_obj = self.templates[cls] @ R.transpose(1, 2) + (targets["rel_obj_trans"].to(dev).reshape(-1, 3) + meta["obj_center_cam"].to(dev))[:, None]
        res = {}
        for kind, before, gt, ok in (("hand", hand, gt_hand, torch.ones_like(known)), ("obj", obj, gt_obj, known)):
            after, info = out[f"refined_{kind}_verts"].to(dev), out[f"refine_{kind}_info"].to(dev)
            err = lambda v: (v.double() - gt.double()).norm(dim=2).mean(1)
            res[kind] = (err(before), err(after), out[f"refine_{kind}_cost"].to(dev), info, ok & (info[:, 0] > 0))
        return res

    def _feed_refine(self, out, targets, meta, obj_cls) -> None:
        res = self.refine_per_sample(out, targets, meta, obj_cls)
        rows = []
        for before, after, cost, info, used in (res["hand"], res["obj"]):
            u = used.double()
            rows.append(torch.stack([(before * u).sum(), (after * u).sum(), (cost[:, 0] * u).sum(), (cost[:, 1] * u).sum(),
                                     (info[:, 2].double() * u).sum(), u.sum(),
                                     torch.tensor(float(used.numel()), device=self.dev, dtype=torch.float64)]))
        self._racc += torch.stack(rows)

    def write(self, out_dir: str) -> str:
        """results.txt (and, for ho3d, pred_mano.json) under out_dir -> the path of results.txt"""
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, "results.txt")
        results = self.results
        if self.native:                                        # the one read-back of the running sums
            *vals, n_used = self._acc.tolist()
            # a sample whose object was not evaluated (obj_cls < 0: HO3D's 019_pitcher_base, common/metrics.py:131-149) added zeros:
            # the object keys are means over the evaluated samples, as the reference takes them; write_results divides by self.total
            obj_scale = self.total / n_used if n_used > 0 else 0.0
            results = {k: v * 100 * (obj_scale if k.endswith("_error") else 1.0) for k, v in zip(results, vals)}
        if not self.ho3d and self.cfg.eval_mesh and self.f_score:
            if self.native:
                fs, fa = torch.cat(self.f_score).cpu().numpy(), torch.cat(self.f_score_al).cpu().numpy()
            else:
                fs, fa = np.concatenate(self.f_score), np.concatenate(self.f_score_al)
            write_results(path, results, self.total, mesh=(self.mesh_err, self.mesh_err_al), fscores=(fs.T, fa.T, self.f_threshs))
        else:
            write_results(path, results, self.total)
        if self.interaction:                                   # appended after everything results.txt has without the option
            pen, con, vol, nv, n = self._iacc.tolist()
            n = max(n, 1.0)
            with open(path, "a") as f:
                print("Interaction:", file=f)
                print("penetration_depth=%.3f cm, contact_ratio=%.3f, intersection_volume=%.3f cm^3, contact_verts=%.1f"
                      % (pen / n * 100.0, con / n, vol / n * 1.0e6, nv / n), file=f)
        if self.field:                                         # after everything else, the interaction block included
            (hs, hn, ht), (os_, on, ot) = self._facc.tolist()
            with open(path, "a") as f:
                print("Field:", file=f)
                print("hand_chamfer=%.4f cm^2, obj_chamfer=%.4f cm^2, hand_left_out=%.3f, obj_left_out=%.3f"
                      % (hs / max(hn, 1.0) * 1.0e4, os_ / max(on, 1.0) * 1.0e4, 1.0 - hn / max(ht, 1.0), 1.0 - on / max(ot, 1.0)), file=f)
        if self.silhouette:                                    # after everything else; integer counts from the device, fp64 division here
            c = torch.cat(self._scounts).cpu().numpy().astype(np.float64) if self._scounts else np.zeros((0, 5))
            line = []
            for name, k in (("hand", 0), ("obj", 2)):
                took = (c[:, 4] > 0) & (c[:, k + 1] > 0)
                iou = float((c[took, k] / c[took, k + 1]).mean()) if took.any() else 0.0
                line.append((name, iou, 1.0 - took.sum() / max(len(c), 1)))
            with open(path, "a") as f:
                print("Silhouette:", file=f)
                print("hand_iou=%.6f, obj_iou=%.6f, hand_left_out=%.3f, obj_left_out=%.3f"
                      % (line[0][1], line[1][1], line[0][2], line[1][2]), file=f)
        if self.refine:                                        # after everything else
            with open(path, "a") as f:
                print("Refined:", file=f)
                for name, (eb, ea, c0, c1, tried, n, seen) in zip(("hand", "obj"), self._racc.tolist()):
                    d = max(n, 1.0)
                    print("%s_vertex_error=%.4f cm -> %.4f cm, %s_cost=%.6f -> %.6f, %s_steps=%.2f, %s_left_out=%.3f"
                          % (name, eb / d * 100.0, ea / d * 100.0, name, c0 / d, c1 / d, name, tried / d, name, 1.0 - n / max(seen, 1.0)),
                          file=f)
        if self.ho3d:
            if self.native:
                joints = list(torch.cat(self.joint_list).cpu().numpy()) if self.joint_list else []
                meshes = list(torch.cat(self.mesh_list).cpu().numpy()) if self.mesh_list else []
            else:
                joints, meshes = self.joint_list, self.mesh_list
            dump_pred_mano(os.path.join(out_dir, "pred_mano.json"), joints, meshes)
            self.n_dumped = (len(joints), len(meshes))
        return path
