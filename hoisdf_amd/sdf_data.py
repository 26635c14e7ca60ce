"""(f2) dataset-side SDF sample selection on the device.

The reference's dataset object loads one ``sdf_processed/<frame>.npy`` per sample ((N_h + N_o, 6) float32 rows
``[x y z sdf_hand sdf_obj label]``, written by tool/pre_process_sdf.py:140-148 together with ``sdf_index.npy`` =
``[[N_h, N_o], ...]``) and draws the query points with ``np.random.choice(..., replace=False)``
(data/dexycb.py:514-546).  At > 200 samples/s per GPU that CPU path is the bottleneck, so here the rows of all frames
of a shard live in HBM (288 GB per MI355X: ~10^10 rows) and a batch is drawn by three kernels:
uniform keys (``hoisdf_sdf_sample_keys``) -> k smallest keys per segment (``hoisdf_select_smallest_abs``) -> row fetch.
Same distribution as the reference (uniform without replacement, optional |sdf| < dist pre-filter), different random
stream.  Output layout = what the reference's ``__getitem__`` produces before augmentation: rows ordered
[hand_sdf | obj_sdf | hand_pre | obj_pre], ``sdf_points`` = columns 0-4, ``sdf_raw_label`` = column 5.
``MeshSdfSource`` (cfg.sdf_source = "mesh") needs no precomputed rows at all: it computes candidate rows from the batch's own hand
and object meshes on the device (csrc/mesh_sdf.hip) and draws from them with the same three kernels."""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import ops
from ._lib import call
from ._marshal import _p, _st


def load_frame(path: str) -> np.ndarray:
    """one ``sdf_processed/<frame>.npy`` file"""
    a = np.load(path)
    if a.ndim != 2 or a.shape[1] != 6 or a.dtype != np.float32:
        raise ValueError(f"{path}: expected float32 (N, 6) rows [x y z sdf_hand sdf_obj label], got {a.dtype} {a.shape}")
    return a


class SdfStore:
    """HBM-resident rows of many frames + per-frame [first_row, n_hand, n_obj]."""

    def __init__(self, frames: Sequence[np.ndarray], index: np.ndarray, device="cuda"):
        index = np.asarray(index, dtype=np.int64).reshape(-1, 2)
        if len(frames) != len(index):
            raise ValueError("one sdf_index row per frame")
        for f, (nh, no) in zip(frames, index):
            if f.shape[0] != nh + no:             # data/dexycb.py:517
                raise ValueError(f"frame has {f.shape[0]} rows but sdf_index says {nh} + {no}")
        self.n_frames = len(frames)
        self.index = torch.from_numpy(index)                                         # host copy
        self.row0 = torch.from_numpy(np.concatenate([[0], np.cumsum(index.sum(1))]).astype(np.int64))
        rows = np.concatenate(frames, 0).astype(np.float32) if frames else np.zeros((0, 6), np.float32)
        self.rows = torch.from_numpy(rows).to(device)
        self.device = self.rows.device

    @classmethod
    def from_directory(cls, sdf_dir: str, frame_names: Optional[Sequence[str]] = None, device="cuda"):
        """``sdf_dir`` holds ``sdf_index.npy`` and ``sdf_processed/*.npy`` (tool/pre_process_sdf.py layout); the index
        rows follow the sorted file list unless ``frame_names`` gives the order."""
        proc = os.path.join(sdf_dir, "sdf_processed")
        names = list(frame_names) if frame_names is not None else sorted(
            f[:-4] for f in os.listdir(proc) if f.endswith(".npy"))
        index = np.load(os.path.join(sdf_dir, "sdf_index.npy"))
        return cls([load_frame(os.path.join(proc, n + ".npy")) for n in names], index[:len(names)], device)

    def sample(self, frame_ids, num_hand: int, num_obj: int, dist: float, train: bool, seed: int,
               validate: bool = True) -> Dict[str, torch.Tensor]:
        """frame_ids (B,) ints -> ``sdf_points`` (B, n, 5), ``sdf_raw_label`` (B, n), ``rows`` (B, n) store row ids;
        n = num_hand + num_obj (+ the same again in training: the |sdf| < dist "pre" points)."""
        fid = torch.as_tensor(frame_ids, dtype=torch.int64).reshape(-1)
        rows = draw_rows(self.rows, self.row0[fid], self.index[fid, 0], self.index[fid, 1], num_hand, num_obj, dist, train, seed,
                         validate)
        data = self.rows[rows.reshape(-1)].view(fid.numel(), rows.shape[1], 6)
        return {"sdf_points": data[..., :5], "sdf_raw_label": data[..., 5], "rows": rows}

    def make_inputs(self, frame_ids, hand_root: torch.Tensor, obj_center: torch.Tensor, num_hand: int, num_obj: int,
                    dist: float, hand_scale: float, obj_scale: float, train: bool, seed: int,
                    do_flip: Optional[torch.Tensor] = None, rot_mat: Optional[torch.Tensor] = None,
                    validate: bool = True, rows: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """The point entries of one batch exactly as the reference's ``__getitem__`` hands them to the model
        (data/dexycb.py:514-549 draw, :548-549 flip ``x *= -1``, data_aug :288 in-plane rotation ``p . rot_mat^T``,
        :593-620 centre + scale), all on the device:
          inputs : hand_sdf_points (B,N_h,3), obj_sdf_points (B,N_o,3) [, hand_pre_points, obj_pre_points]
          targets: hand_sdf (B,N_h) = column 3 * hand_scale, obj_sdf (B,N_o) = column 4 * obj_scale
        ``hand_root`` / ``obj_center`` (B,3) are the centres AFTER the same flip / rotation (the dataset object computes
        them from the augmented joints / bbox); ``do_flip`` (B,) bool, ``rot_mat`` (B,3,3).
        ``rows`` (B, n) store row ids in the reference's order [hand_sdf | obj_sdf | hand_pre | obj_pre]: hand off THESE rows
        instead of drawing (tests/golden/g14_sampler.npz feeds numpy's own draws through the device hand-off)."""
        if rows is None:
            smp = self.sample(frame_ids, num_hand, num_obj, dist, train, seed, validate)
        else:
            rows = torch.as_tensor(rows, dtype=torch.int64, device=self.device)
            smp = {"sdf_points": self.rows[rows.reshape(-1)].view(rows.shape[0], rows.shape[1], 6)[..., :5], "rows": rows}
        return assemble_inputs(smp["sdf_points"], smp["rows"], hand_root, obj_center, num_hand, num_obj, hand_scale, obj_scale, train,
                               do_flip, rot_mat)


def draw_rows(rows: torch.Tensor, base: torch.Tensor, nh: torch.Tensor, no: torch.Tensor, num_hand: int, num_obj: int, dist: float,
              train: bool, seed: int, validate: bool = True) -> torch.Tensor:
    """The draw both sources share.  ``rows`` (R, 6) on the device; sample b owns rows base[b] .. base[b] + nh[b] + no[b], hand rows
    first (host int64 (B,) each).  Uniform without replacement per segment: keys (hoisdf_sdf_sample_keys) -> the k smallest
    (hoisdf_select_smallest_abs).  -> (B, n) row ids in the reference's order [hand | obj | hand_pre | obj_pre]."""
    dev, B = rows.device, base.numel()
    # segments per sample: hand, obj, [hand_pre, obj_pre]; all segments of a kind share k
    kinds = [(base, nh, -1, num_hand), (base + nh, no, -1, num_obj)]
    if train:
        kinds += [(base, nh, 3, num_hand), (base + nh, no, 4, num_obj)]
    out_rows = []
    for gi, (r0, ln, col, k) in enumerate(kinds):
        off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(ln, 0)])
        n_keys = int(off[-1])
        if n_keys >= 2 ** 31:
            raise ValueError("batch too large for int32 key offsets")
        d_r0 = r0.to(dev)
        d_len = ln.to(dev, torch.int32)
        d_off = off[:-1].to(dev, torch.int32)
        d_col = torch.full((B,), col, dtype=torch.int32, device=dev)
        keys = torch.empty(max(n_keys, 1), device=dev, dtype=torch.float32)
        elig = torch.empty(B, device=dev, dtype=torch.int32)
        call("hoisdf_sdf_sample_keys", _p(rows), 6, _p(d_r0), _p(d_len), _p(d_off), _p(d_col), B,
             int(ln.max()) if B else 0, float(dist), int(seed) * 4 + gi, _p(keys), _p(elig), _st())
        if validate and B and int(elig.min()) < k:                     # np.random.choice would raise ValueError
            raise ValueError(f"a frame has only {int(elig.min())} eligible rows for {k} draws (segment kind {gi})")
        sel = ops.select_smallest_abs(keys, d_off, d_len, k)          # (B, k) indices into keys
        out_rows.append(sel.long() - d_off.long()[:, None] + d_r0[:, None])
    return torch.cat(out_rows, 1)                                     # (B, n) rows, reference order


def assemble_inputs(sdf_points: torch.Tensor, rows: torch.Tensor, hand_root: torch.Tensor, obj_center: torch.Tensor, num_hand: int,
                    num_obj: int, hand_scale: float, obj_scale: float, train: bool, do_flip: Optional[torch.Tensor] = None,
                    rot_mat: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """drawn rows (B, n, >= 5) [x y z sdf_hand sdf_obj] in the order [hand | obj | hand_pre | obj_pre] -> the model's point entries:
    flip, in-plane rotation, centre and scale (data/dexycb.py:548-549, :288, :593-620)"""
    dev = sdf_points.device
    pts = sdf_points[..., :5].clone()                                 # (B, n, 5): xyz, sdf_hand, sdf_obj
    B = pts.shape[0]
    if do_flip is not None:
        sgn = torch.where(do_flip.to(dev).bool(), -1.0, 1.0).view(B, 1)
        pts[..., 0] = pts[..., 0] * sgn
    if rot_mat is not None:
        pts[..., :3] = pts[..., :3] @ rot_mat.to(dev).transpose(1, 2)
    hr, oc = hand_root.to(dev)[:, None], obj_center.to(dev)[:, None]
    a, b = num_hand, num_hand + num_obj
    hand, obj = pts[:, :a].clone(), pts[:, a:b].clone()
    hand[..., :3] -= hr
    obj[..., :3] -= oc
    hand, obj = hand * hand_scale, obj * obj_scale
    out = {"hand_sdf_points": hand[..., :3].contiguous(), "obj_sdf_points": obj[..., :3].contiguous(),
           "hand_sdf": hand[..., 3].contiguous(), "obj_sdf": obj[..., 4].contiguous(), "rows": rows}
    if train:
        c = b + num_hand
        out["hand_pre_points"] = ((pts[:, b:c, :3] - hr) * hand_scale).contiguous()
        out["obj_pre_points"] = ((pts[:, c:, :3] - oc) * obj_scale).contiguous()
    return out


def synthetic_store(n_frames: int, rows_hand: int = 6000, rows_obj: int = 4000, seed: int = 0, device="cuda") -> "SdfStore":
    """A store shaped like tool/pre_process_sdf.py's output (points in a ~0.3 m box around the hand at z ~ 0.7 m,
    |sdf| small for ~half of the rows) for smoke runs without the licence-gated datasets."""
    r = np.random.default_rng(seed)
    frames, index = [], []
    for _ in range(n_frames):
        nh, no = rows_hand + int(r.integers(0, 200)), rows_obj + int(r.integers(0, 200))
        a = np.zeros((nh + no, 6), np.float32)
        a[:, :3] = r.uniform(-0.1, 0.1, (nh + no, 3)) + np.array([0.0, 0.0, 0.7], np.float32)
        a[:, 3] = r.uniform(-0.02, 0.1, nh + no)
        a[:, 4] = r.uniform(-0.02, 0.1, nh + no)
        a[:, 5] = r.integers(0, 6, nh + no)
        frames.append(a)
        index.append([nh, no])
    return SdfStore(frames, np.asarray(index), device)


def mesh_sdf_enabled(cfg) -> bool:
    """cfg.sdf_source == "mesh" (default "": off) or HOISDF_SDF=mesh"""
    return getattr(cfg, "sdf_source", "") == "mesh" or os.environ.get("HOISDF_SDF", "") == "mesh"


def procedural_templates(scale: float = 0.04, device="cpu") -> Dict[str, torch.Tensor]:
    """Three closed, outward-wound object templates (icosphere 320 faces, torus 384, box 192) about `scale` metres in radius, padded
    to one shape: verts (T, V, 3) (padding repeats vertex 0), faces (T, F, 3) int32 (padding rows are -1), n_faces (T,) int32.
    For smoke runs without the licence-gated object models; real templates (metrics.prepare_model_template) go in the same dict."""
    from .mesh_sdf_oracle import box, icosphere, torus
    return pack_templates([icosphere(2), torus(), box()], scale, device)


def pack_templates(meshes, scale: float = 1.0, device="cpu") -> Dict[str, torch.Tensor]:
    """[(verts (V_i, 3), faces (F_i, 3)), ...] -> the padded dict MeshSdfSource takes"""
    V, F = max(len(v) for v, _ in meshes), max(len(f) for _, f in meshes)
    verts, faces = np.zeros((len(meshes), V, 3), np.float32), np.full((len(meshes), F, 3), -1, np.int32)
    for t, (v, f) in enumerate(meshes):
        verts[t, :len(v)], verts[t, len(v):], faces[t, :len(f)] = np.asarray(v) * scale, np.asarray(v)[0] * scale, f
    n = np.asarray([len(f) for _, f in meshes], np.int32)
    return {"verts": torch.from_numpy(verts).to(device), "faces": torch.from_numpy(faces).to(device), "n_faces": torch.from_numpy(n).to(device)}


DISTAL_JOINTS = (3, 6, 9, 12, 15)                              # of MANO's 16: the last joint of each of the five fingers


def contact_zone_weights(skin_weights: torch.Tensor) -> torch.Tensor:
    """(V, 16) skinning weights -> (V,) float32: 1 on the vertices that a distal finger joint moves most (the finger tips and pads),
    else 0.  The attraction zones of the interaction loss; ObMan's own zone files are not redistributable, this is derived from the
    layer alone."""
    top = skin_weights.detach().argmax(1)
    return torch.isin(top, torch.tensor(DISTAL_JOINTS, device=top.device)).float()


class MeshSdfSource:
    """The SDF query points of a training batch computed on the device from the batch's own meshes (hoisdf_mesh_sdf_rows) instead of
    read from precomputed ``sdf_processed`` rows: per sample ``cfg.mesh_sdf_candidates`` x (num_samp_hand + num_samp_obj) candidate
    rows [x y z sdf_hand sdf_obj label] in camera metres - sampled around the hand mesh (``targets["mano_param"]`` through
    ops.mano_gt, moved to ``meta["mano_root"]``) and around the object template ``meta["obj_cls"]`` placed by ``targets["obj_rot"]``
    and ``targets["rel_obj_trans"]`` + ``meta["obj_center_cam"]`` - from which ``make_inputs`` draws with SdfStore's own code.
    The 3D labels are those of the augmented (flipped, rotated) frame already, so the points get neither flip nor rotation.
    ``templates``: the dict of ``pack_templates``.  ``vert_label`` (778,) hand part per vertex; default: the part of the joint
    with the largest skinning weight.  Sampling follows cfg.mesh_sdf_* (DeepSDF's near-surface recipe at hand size, not fitted to
    the precomputed files)."""

    def __init__(self, mano_layer, templates: Dict[str, torch.Tensor], cfg, vert_label: Optional[torch.Tensor] = None):
        from .mesh_sdf_oracle import vertex_part_labels
        self.layer, self.cfg = mano_layer, cfg
        self.templates = {k: torch.as_tensor(v) for k, v in templates.items()}
        if vert_label is None:
            vert_label = torch.from_numpy(vertex_part_labels(mano_layer.th_weights.detach().cpu().numpy()))
        self.vert_label = torch.as_tensor(vert_label).to(torch.int32)
        self.n_templates = self.templates["verts"].shape[0]
        # the vertex rows of a template that its faces name (the rows behind them repeat vertex 0: padding)
        f, n = self.templates["faces"].long(), self.templates["n_faces"].long()
        named = torch.where(torch.arange(f.shape[1], device=f.device)[None, :, None] < n[:, None, None], f, torch.zeros_like(f))
        self.templates["n_verts"] = (named.flatten(1).max(1).values + 1).to(torch.int32) * (n > 0).to(torch.int32)

    def to(self, dev):
        """the layer, the templates and the labels on ``dev`` (moved once)"""
        if next(self.layer.buffers()).device != dev:
            self.layer.to(dev)
        if self.templates["verts"].device != dev:
            self.templates = {k: v.to(dev) for k, v in self.templates.items()}
            self.vert_label = self.vert_label.to(dev)
        return self

    def meshes(self, targets, meta):
        """-> hand verts (B, 778, 3), hand faces (F, 3), object verts (B, V, 3), object faces (B, F, 3), object face counts (B,):
        camera metres, on the device of ``targets["mano_param"]``"""
        from .metrics import batch_rodrigues
        dev = targets["mano_param"].device
        self.to(dev)
        assets = self.layer.kernel_assets()
        if assets is None:
            raise RuntimeError("MeshSdfSource needs the MANO layer the HIP head takes (on the GPU, wrist-centred, flat hand mean)")
        hand = ops.mano_gt(targets["mano_param"], assets)[0] + meta["mano_root"].to(dev)[:, None]
        cls = meta["obj_cls"].to(dev).long()
        R = batch_rodrigues(targets["obj_rot"].to(dev).float())
        trans = (targets["rel_obj_trans"].to(dev) + meta["obj_center_cam"].to(dev))[:, None]
        obj = self.templates["verts"][cls] @ R.transpose(1, 2) + trans
        return hand, self.layer.th_faces.to(torch.int32), obj, self.templates["faces"][cls], self.templates["n_faces"][cls]

    def candidate_rows(self, targets, meta, num_hand: int, num_obj: int, seed: int) -> torch.Tensor:
        """(B, candidates x (num_hand + num_obj), 6)"""
        c = self.cfg
        k = int(c.mesh_sdf_candidates)
        if k < 1:
            raise ValueError(f"cfg.mesh_sdf_candidates = {k}: at least one candidate row per drawn point")
        hand, hf, obj, of, on = self.meshes(targets, meta)
        mixed = (int(seed) * 0x9E3779B97F4A7C15 + 0x7F4A7C15) & 0x3FFFFFFFFFFFFFFF      # unrelated to the draw's own streams
        return ops.mesh_sdf_rows(hand, hf, obj, of, on, self.vert_label, k * num_hand, k * num_obj, c.mesh_sdf_sigma,
                                 c.mesh_sdf_uniform_every, c.mesh_sdf_pad, c.mesh_sdf_label_clamp, mixed)

    def make_inputs(self, targets, meta, num_hand: int, num_obj: int, dist: float, hand_scale: float, obj_scale: float, train: bool,
                    seed: int, validate: bool = True) -> Dict[str, torch.Tensor]:
        """what ``SdfStore.make_inputs`` returns, same keys and shapes; ``rows`` indexes the candidate block of this call, kept as
        ``self.last_candidates`` (B n, 6) so that a caller can look the drawn rows up"""
        cand = self.candidate_rows(targets, meta, num_hand, num_obj, seed)
        B, n = cand.shape[0], cand.shape[1]
        k = int(self.cfg.mesh_sdf_candidates)
        flat = cand.view(B * n, 6)
        full = lambda x: torch.full((B,), x, dtype=torch.int64)
        rows = draw_rows(flat, torch.arange(B, dtype=torch.int64) * n, full(k * num_hand), full(k * num_obj), num_hand, num_obj, dist,
                         train, seed, validate)
        data = flat[rows.reshape(-1)].view(B, rows.shape[1], 6)
        self.last_candidates = flat
        return assemble_inputs(data, rows, meta["mano_root"], meta["obj_center_cam"], num_hand, num_obj, hand_scale, obj_scale, train)
