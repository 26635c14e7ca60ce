"""Evaluation metrics (csrc/eval.hip, the hoisdf_eval_* entries of include/hoisdf.h).  Stateless: marshal, size, allocate, one C call."""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call
from ._marshal import _chk, _p, _st, _workspace


# ---------------------------------------------------------------------------------------------
# (f5) evaluation metrics (csrc/eval.hip, the hoisdf_eval_* entries).  Device tensors in, device tensors out; nothing here
# synchronises or reads a value back.
# ---------------------------------------------------------------------------------------------
def _eval_workspace(B: int, V: int, dev) -> torch.Tensor:
    return _workspace("hoisdf_eval_workspace_bytes", B, V, dev, least=0)[0]


def eval_thresholds(ths, dev) -> torch.Tensor:
    """thresholds as the device fp64 array the evaluation entries read (a tensor on the device is passed through)"""
    if torch.is_tensor(ths) and ths.is_cuda and ths.dtype == torch.float64:
        return ths.contiguous()
    return torch.as_tensor(np.asarray(ths, dtype=np.float64)).to(dev)


@torch.no_grad()
def eval_object(obj_rot, obj_trans, obj_rot_gt, obj_trans_gt, templates, obj_ids):
    """hoisdf_eval_object: obj_rot / obj_trans (B,P,3) per-point predictions, obj_rot_gt / obj_trans_gt (B,3), templates (T,V,3),
    obj_ids (B,) integer template of each sample (negative: not evaluated) -> per-sample (adds, mce, oce, mme) float32 (B,) and
    used int32 (B,)."""
    obj_rot, obj_trans = obj_rot.detach().contiguous().float(), obj_trans.detach().contiguous().float()
    obj_rot_gt, obj_trans_gt = obj_rot_gt.contiguous().float(), obj_trans_gt.contiguous().float()
    templates = templates.contiguous().float()
    _chk(obj_rot, obj_trans, obj_rot_gt, obj_trans_gt, templates)
    B, P = obj_rot.shape[0], obj_rot.shape[1]
    T, V = templates.shape[0], templates.shape[1]
    assert obj_rot.shape == (B, P, 3) and obj_trans.shape == (B, P, 3) and obj_rot_gt.shape == (B, 3) and obj_trans_gt.shape == (B, 3)
    assert templates.dim() == 3 and templates.shape[2] == 3 and obj_ids.shape == (B,), (tuple(templates.shape), tuple(obj_ids.shape))
    dev = obj_rot.device
    ids = obj_ids.to(device=dev, dtype=torch.int32).contiguous()
    adds, mce, oce, mme = (torch.empty(B, device=dev, dtype=torch.float32) for _ in range(4))
    used = torch.empty(B, device=dev, dtype=torch.int32)
    ws = _eval_workspace(B, V, dev)
    call("hoisdf_eval_object", _p(obj_rot), _p(obj_trans), P, _p(obj_rot_gt), _p(obj_trans_gt), _p(templates), T, V, _p(ids), B, _p(adds),
         _p(mce), _p(oce), _p(mme), _p(used), _p(ws), ws.numel(), _st())
    return adds, mce, oce, mme, used


@torch.no_grad()
def eval_hand_joints(pred, gt, want_aligned: bool = False, want_transform: bool = False, want_dist: bool = False):
    """hoisdf_eval_hand_joints: pred / gt (B,J,3) -> per-sample (mje, pamje) float32 (B,), the aligned points (B,J,3) or None, and
    the fitted similarity (B,13) float64 = c, R row-major, t or None; with want_dist also the per-point distances before and
    after the alignment, (B,J) each."""
    pred, gt = pred.detach().contiguous().float(), gt.detach().contiguous().float()
    _chk(pred, gt)
    B, J = pred.shape[0], pred.shape[1]
    assert pred.shape == (B, J, 3) and gt.shape == (B, J, 3), (tuple(pred.shape), tuple(gt.shape))
    dev = pred.device
    mje, pamje = torch.empty(B, device=dev, dtype=torch.float32), torch.empty(B, device=dev, dtype=torch.float32)
    aligned = torch.empty(B, J, 3, device=dev, dtype=torch.float32) if want_aligned else None
    xf = torch.empty(B, 13, device=dev, dtype=torch.float64) if want_transform else None
    d0 = torch.empty(B, J, device=dev, dtype=torch.float32) if want_dist else None
    d1 = torch.empty(B, J, device=dev, dtype=torch.float32) if want_dist else None
    call("hoisdf_eval_hand_joints", _p(pred), _p(gt), B, J, _p(mje), _p(pamje), _p(aligned), _p(xf), _p(d0), _p(d1), _st())
    return (mje, pamje, aligned, xf, d0, d1) if want_dist else (mje, pamje, aligned, xf)


@torch.no_grad()
def eval_mesh(pred, gt, thresholds, want_aligned: bool = False):
    """hoisdf_eval_mesh: pred / gt (B,V,3), thresholds = F-score thresholds (a sequence, or eval_thresholds of one) ->
    dist_raw, dist_aligned (B,V), fscore, fscore_aligned (B,n_thresh), aligned (B,V,3) or None."""
    pred, gt = pred.detach().contiguous().float(), gt.detach().contiguous().float()
    _chk(pred, gt)
    B, V = pred.shape[0], pred.shape[1]
    assert pred.shape == (B, V, 3) and gt.shape == (B, V, 3), (tuple(pred.shape), tuple(gt.shape))
    dev = pred.device
    th = eval_thresholds(thresholds, dev)
    nt = th.numel()
    d0, d1 = torch.empty(B, V, device=dev, dtype=torch.float32), torch.empty(B, V, device=dev, dtype=torch.float32)
    f0, f1 = torch.empty(B, nt, device=dev, dtype=torch.float32), torch.empty(B, nt, device=dev, dtype=torch.float32)
    aligned = torch.empty(B, V, 3, device=dev, dtype=torch.float32) if want_aligned else None
    ws = _eval_workspace(B, V, dev)
    call("hoisdf_eval_mesh", _p(pred), _p(gt), B, V, _p(th), nt, _p(d0), _p(d1), _p(f0), _p(f1), _p(aligned), _p(ws), ws.numel(), _st())
    return d0, d1, f0, f1, aligned


def eval_accum_init(V: int, steps: int, dev) -> torch.Tensor:
    """a zeroed accumulator state (hoisdf_eval_accum_init) for V vertices and `steps` thresholds"""
    state = _workspace("hoisdf_eval_accum_state_bytes", V, steps, dev, least=0)[0]
    call("hoisdf_eval_accum_init", _p(state), V, steps, _st())
    return state


@torch.no_grad()
def eval_accumulate(state, dist, thresholds) -> None:
    """hoisdf_eval_accum_feed: add dist (B,V) float32 to the state; thresholds = the state's device fp64 array (steps,)"""
    dist = dist.contiguous()
    _chk(dist)
    assert thresholds.is_cuda and thresholds.dtype == torch.float64 and thresholds.is_contiguous()
    B, V = dist.shape
    call("hoisdf_eval_accum_feed", _p(state), _p(dist), B, V, _p(thresholds), thresholds.numel(), _st())


@torch.no_grad()
def eval_accum_finish(state, V: int, thresholds) -> torch.Tensor:
    """hoisdf_eval_accum_finish -> (2 + steps,) float64 on the device: mean EPE, AUC, the PCK curve"""
    out = torch.empty(2 + thresholds.numel(), device=state.device, dtype=torch.float64)
    call("hoisdf_eval_accum_finish", _p(state), V, _p(thresholds), thresholds.numel(), _p(out), _st())
    return out
