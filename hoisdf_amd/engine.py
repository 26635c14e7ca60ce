"""Runtime harness with the reference's driver surface:

  * ``Trainer`` / ``Tester``: same roles as common/base.py:59-193 - AdamW(lr=cfg.lr) +
    StepLR(cfg.lr_drop, cfg.lr_decay_gamma), the 1e-5 learning-rate floor (base.py:30-32), the loss
    weighting of main/train.py:113-127;
  * checkpoints in the reference's on-disk format: ``snapshot_{epoch}_{iter}.pth.tar`` holding
    {"epoch", "network", "optimizer", "lr_scheduler"} with every network key prefixed ``module.``
    (the DataParallel prefix, common/base.py:113-150), resumed from the highest (epoch, iter);
  * released reference checkpoints load with ``strict=True`` (state-dict schema checked against the
    reference in tests/test_checkpoint_schema.py).
Redesigned for MI355X: one process per GPU (torchrun), gradients reduced by
``hoisdf_amd.ddp.GradReducer`` over RCCL instead of single-process ``nn.DataParallel``.
Datasets are licence-gated and absent offline: ``SyntheticDataset`` yields DexYCB / HO3D shaped
samples with the schema of data/dexycb.py:627-655; a real dataset object with the same
``__getitem__`` contract can be passed instead.
"""
from __future__ import annotations

import glob
import os
import os.path as osp
import re
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.distributed as dist

from . import testing as T
from .config import Config
from .ddp import GradReducer, reducible_parameters
from .model import get_model

LOSS_WEIGHTS = {  # main/train.py:115-127 <- cfg attribute
    "sdfhand_loss": "sdf_hand_weight", "sdfobj_loss": "sdf_obj_weight", "joint_heatmap": "hm_weight",
    "obj_seg": "obj_hm_weight", "hand_seg": "obj_hm_weight", "obj_rot": "obj_rot_weight",
    "obj_trans": "obj_trans_weight", "loss_joint_3d": "joint_weight", "loss_joint_cls": "cls_weight",
    "loss_all_joint_3d": "joint_weight",
    # not in the reference: the hand-object interaction loss (cfg.interaction_loss)
    "interaction_rep": "interaction_rep_weight", "interaction_att": "interaction_att_weight",
    # not in the reference: the silhouette loss of the predicted pair against the mask targets (cfg.silhouette_loss)
    "silhouette_in": "silhouette_in_weight", "silhouette_cover": "silhouette_cover_weight"}


def _mix_seed(epoch_seed: int, draw: int) -> int:
    """splitmix64 of (per-epoch per-rank seed, draw index within the epoch): streams of different ranks / epochs / resumed
    runs are unrelated instead of shifted copies of each other"""
    x = (epoch_seed * 0x9E3779B97F4A7C15 + draw * 0xBF58476D1CE4E5B9 + 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 31
    return x >> 3            # 61 bits: SdfStore.sample derives 4 sub-streams as seed * 4 + i in 64 bits


def weighted_total(model_out: Dict[str, torch.Tensor], cfg: Config):
    """main/train.py:111-138: split on the ``_out`` suffix, mean every loss, apply cfg weights, sum."""
    out = {k[:-4]: v for k, v in model_out.items() if "_out" in k}
    loss = {k: v.mean() for k, v in model_out.items() if "_out" not in k}
    for k, attr in LOSS_WEIGHTS.items():
        if k in loss:
            loss[k] = loss[k] * getattr(cfg, attr)
    return sum(loss.values()), loss, out


def adjust_learning_rate(lr_scheduler, optimizer, floor: float = 1e-5):
    """common/base.py:30-32."""
    if lr_scheduler.get_last_lr()[-1] < floor:
        for g in optimizer.param_groups:
            g["lr"] = floor


class SyntheticSdfDataset(torch.utils.data.Dataset):
    """(f2) the dataset contract when the SDF rows live in HBM (``hoisdf_amd.sdf_data.SdfStore``): ``__getitem__`` yields
    everything the reference's does EXCEPT the four point sets and the two SDF targets; in their place meta_info carries
    ``sdf_frame`` (row of the store), ``do_flip`` and ``aug_rot`` (the 3x3 in-plane augmentation rotation) and
    ``Trainer(sdf_store=...)`` draws the points on the device (data/dexycb.py:514-549 + :288, :593-620)."""

    def __init__(self, cfg: Config, n_frames: int, length: int = 64, seed: int = 0):
        self.cfg, self.n_frames, self.length, self.seed = cfg, n_frames, length, seed

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        import math
        ins, tg, mt = T.synthetic_batch(1, 1, 1, seed=self.seed * 100003 + i)
        sq = lambda d: {k: v[0] for k, v in d.items()}
        ins, tg, mt = sq(ins), sq(tg), sq(mt)
        for k in ("hand_sdf_points", "obj_sdf_points", "hand_pre_points", "obj_pre_points"):
            ins.pop(k)
        tg.pop("hand_sdf"), tg.pop("obj_sdf")
        g = torch.Generator().manual_seed(self.seed * 7919 + i)
        ang = float((torch.rand(1, generator=g) - 0.5) * math.pi / 3)             # +-30 degrees, like cfg.max_rot
        c, s_ = math.cos(ang), math.sin(ang)
        mt["sdf_frame"] = torch.tensor(i % self.n_frames)
        mt["do_flip"] = torch.rand(1, generator=g)[0] < 0.5
        mt["aug_rot"] = torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]])
        return ins, tg, mt


class SyntheticMeshSdfDataset(torch.utils.data.Dataset):
    """the dataset contract of ``Trainer(sdf_source=...)`` (``hoisdf_amd.sdf_data.MeshSdfSource``): no point sets and no SDF targets
    at all - ``mano_param``, ``obj_rot``, ``rel_obj_trans`` (targets), ``mano_root``, ``obj_center_cam`` and ``obj_cls`` = the
    object's template (meta_info) are what the points and their distances are computed from on the device, every step anew"""

    def __init__(self, cfg: Config, n_templates: int, length: int = 64, seed: int = 0, keep_points: bool = False):
        self.cfg, self.n_templates, self.length, self.seed = cfg, n_templates, length, seed
        self.keep_points = keep_points      # for Trainer(seg_source=...) without an SDF source: the point sets and SDF targets stay

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        n = (self.cfg.num_samp_hand, self.cfg.num_samp_obj) if self.keep_points else (1, 1)
        ins, tg, mt = T.synthetic_batch(1, n[0], n[1], seed=self.seed * 100003 + i)
        sq = lambda d: {k: v[0] for k, v in d.items()}
        ins, tg, mt = sq(ins), sq(tg), sq(mt)
        if not self.keep_points:
            for k in ("hand_sdf_points", "obj_sdf_points", "hand_pre_points", "obj_pre_points"):
                ins.pop(k)
            tg.pop("hand_sdf"), tg.pop("obj_sdf")
        mt["obj_cls"] = torch.tensor((self.seed + i) % self.n_templates)
        return ins, tg, mt


RAW_FRAME_SHAPE = (480, 640)          # the reference's camera frames (H, W)


class SyntheticDataset(torch.utils.data.Dataset):
    """``raw_frames=True``: a sample shaped like the reference's BEFORE its crop - inputs carry ``frame`` (uint8 [480][640][3]),
    ``hand_mask`` / ``obj_mask`` (uint8 [480][640]) instead of ``img``; meta_info carries the raw frame's ``joints_uv_raw`` (21, 2)
    float32, ``p2d_raw`` (21, 2) float64, ``cam_intr_raw`` and ``do_flip`` instead of ``cam_intr`` / ``bbox_hand`` / ``bbox_obj``;
    targets lack ``hand_seg`` / ``obj_seg`` / ``joint_coord``.  ``ImagePipeline`` (cfg.native_image) produces what is missing."""

    def __init__(self, cfg: Config, length: int = 64, seed: int = 0, raw_frames: bool = False):
        self.cfg, self.length, self.seed, self.raw_frames = cfg, length, seed, raw_frames

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        ins, tg, mt = T.synthetic_batch(1, self.cfg.num_samp_hand, self.cfg.num_samp_obj, seed=self.seed * 100003 + i)
        sq = lambda d: {k: v[0] for k, v in d.items()}
        ins, tg, mt = sq(ins), sq(tg), sq(mt)
        if self.raw_frames:
            H, W = RAW_FRAME_SHAPE
            g = torch.Generator().manual_seed(self.seed * 104729 + i)
            ins.pop("img")
            for k in ("hand_seg", "obj_seg", "joint_coord"):
                tg.pop(k)
            for k in ("cam_intr", "bbox_hand", "bbox_obj"):
                mt.pop(k)
            ins["frame"] = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
            c = torch.tensor([W / 2.0, H / 2.0]) + 60 * (torch.rand(2, generator=g) - 0.5)
            mt["joints_uv_raw"] = c + 70 * (torch.rand(21, 2, generator=g) - 0.5)
            mt["p2d_raw"] = (c + torch.tensor([30.0, 10.0]) + 60 * (torch.rand(21, 2, generator=g) - 0.5)).double()
            yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
            ins["hand_mask"] = (((xx - c[0]) ** 2 + (yy - c[1]) ** 2) < 45 ** 2).to(torch.uint8)
            ins["obj_mask"] = (((xx - c[0] - 30).abs() < 35) & ((yy - c[1] - 10).abs() < 30)).to(torch.uint8)
            mt["cam_intr_raw"] = torch.tensor([[600.0, 0, W / 2.0 - 8], [0, 600.0, H / 2.0 + 1], [0, 0, 1]])
            mt["do_flip"] = torch.rand(1, generator=g)[0] < 0.5
        return ins, tg, mt


def native_image_enabled(cfg: Config) -> bool:
    """cfg.native_image (default False) or HOISDF_IMAGE=native"""
    return bool(getattr(cfg, "native_image", False)) or os.environ.get("HOISDF_IMAGE", "") == "native"


def apply_image_pipeline(pipe, inputs, targets, meta, rng=None, draws=None):
    """A raw-frame batch (SyntheticDataset(raw_frames=True)) through ``ImagePipeline``: the dicts gain, in place, what the reference's
    loader would have delivered - ``img`` (a channels_last view of the NHWC crop, no copy), ``hand_seg`` / ``obj_seg`` /
    ``joint_coord``, ``cam_intr`` / ``bbox_hand`` / ``bbox_obj`` / ``p2d`` - and, for a training batch (``rng`` given), the 3D labels
    turned by the augmentation and ``aug_rot`` / ``do_flip`` for ``SdfStore.make_inputs``.  Returns the pipeline's output."""
    B = inputs["frame"].shape[0]
    labels = []
    for b in range(B):
        lab = dict(joints_uv=meta["joints_uv_raw"][b].cpu().numpy(), p2d=meta["p2d_raw"][b].cpu().numpy(),
                   K=meta["cam_intr_raw"][b].double().cpu().numpy(), flip=bool(meta["do_flip"][b]))
        if rng is not None:                 # (the synthetic 3D labels are already those of the mirrored frame: only the rotation applies)
            lab.update(flip_3d=False, joints_3d=targets["joint_cam_no_trans"][b], mano_param=targets["mano_param"][b], obj_rot=targets["obj_rot"][b],
                       obj_trans=targets["rel_obj_trans"][b])
        labels.append(lab)
    frames, masks = inputs.pop("frame"), (inputs.pop("hand_mask"), inputs.pop("obj_mask"))
    if rng is None:
        out = pipe.eval_batch(frames, masks, labels)
    else:
        out = pipe.train_batch(frames, masks, labels, rng, draws)
        targets.update(joint_cam_no_trans=out["joints_3d"], mano_param=out["mano_param"], obj_rot=out["obj_rot"],
                       rel_obj_trans=out["obj_trans"])
        meta["aug_rot"] = out["rot_mat"]
    inputs["img"] = out["img"].permute(0, 3, 1, 2)
    targets.update(hand_seg=out["hand_seg"], obj_seg=out["obj_seg"], joint_coord=out["joint_coord"])
    meta.update(cam_intr=out["cam_intr"], bbox_hand=out["bbox_hand"], bbox_obj=out["bbox_obj"], p2d=out["p2d"])
    return out


def reserve_hbm_pool(model: torch.nn.Module, fraction: float = 0.5, device=None) -> int:
    """After the first steps: hand PyTorch's caching allocator `fraction` of the peak it has seen so far as FREE cached blocks, one per
    stream the model launches on (blocks are owned by the stream they were freed on).  The step's allocation pattern is not exactly
    repeatable - two streams race, a training step after `cfg.point_sampling_epoch` draws its point branch - and a request the cache
    cannot serve costs a hipMalloc: synchronous, 50-250 ms for the multi-GB workspaces of `sdf_infer` (measured: the first branch-B
    step of a run took 383 ms instead of 90).  288 GB of HBM per GPU is there to be laid out once.  Returns the bytes reserved."""
    if not torch.cuda.is_available():
        return 0
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    if dev.type != "cuda":
        return 0
    peak = torch.cuda.max_memory_allocated(dev)
    free, _ = torch.cuda.mem_get_info(dev)
    extra = min(int(fraction * peak), int(0.25 * free))
    streams = [torch.cuda.current_stream(dev)]
    side = getattr(model, "_side_stream", None)
    if side is None:                    # (a wrapper around the Model)
        side = getattr(getattr(model, "module", None), "_side_stream", None)
    if side is not None:
        streams.append(side)
    per = extra // len(streams) // (1 << 20) * (1 << 20)
    if per <= 0:
        return 0
    for st in streams:
        with torch.cuda.stream(st):
            t = torch.empty(per, dtype=torch.uint8, device=dev)
            del t
    return per * len(streams)


def snapshot_path(model_dir: str, epoch: int, itr: int) -> str:
    return osp.join(model_dir, f"snapshot_{epoch}_{itr}.pth.tar")


def latest_snapshot(model_dir: str) -> Optional[Tuple[str, int, int]]:
    """highest epoch, then highest iteration (common/base.py:121-142)."""
    best = None
    for f in glob.glob(osp.join(model_dir, "snapshot_*.pth.tar")):
        m = re.search(r"snapshot_(\d+)_(\d+)\.pth\.tar$", f)
        if m:
            key = (int(m.group(1)), int(m.group(2)))
            if best is None or key > best[1:]:
                best = (f, *key)
    return best


def to_reference_state_dict(model: torch.nn.Module) -> Dict[str, torch.Tensor]:
    return {"module." + k: v for k, v in model.state_dict().items()}


def load_reference_state_dict(model: torch.nn.Module, network: Dict[str, torch.Tensor], strict: bool = True):
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in network.items()}
    return model.load_state_dict(sd, strict=strict)


class Trainer:
    def __init__(self, cfg: Config, device: torch.device, dataset=None, batch_size: Optional[int] = None,
                 channels_last: bool = True, tune_encoder: bool = True, sdf_store=None, sdf_source=None, seg_source=None):
        self.cfg, self.device = cfg, device
        self.seg_source = seg_source        # the two mask targets rendered from the batch's meshes (render.MeshSegSource)
        self.sdf_store = sdf_store          # (f2) HBM-resident sdf_processed rows: the query points are drawn on the device
        self.sdf_source = sdf_source        # no rows at all: points and distances computed from the batch's meshes (MeshSdfSource)
        self._sdf_draws = 0
        self.rank = dist.get_rank() if dist.is_initialized() else 0
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.base_seed = int(getattr(cfg, "seed", 0))
        torch.manual_seed(self.base_seed)                        # identical initial weights on every rank
        self.model = get_model("train", cfg=cfg).to(device).train()
        if channels_last:
            if device.type == "cuda" and tune_encoder:
                from . import miopen_tuning
                miopen_tuning.enable()       # tuned fp32 NHWC conv solvers for the encoder (shipped find-db)
            self.model.backbone_net.to(memory_format=torch.channels_last)
            self.model.decoder_net.to(memory_format=torch.channels_last)
        self.channels_last = channels_last
        on_gpu = device.type == "cuda"
        self.reducer = GradReducer(reducible_parameters(self.model), average=not on_gpu)
        # reference: AdamW over ALL named parameters in one group, frozen BN affine included (common/base.py:64-73):
        # the optimizer state_dict's ``params`` index list must have that length/order for snapshots to be
        # interchangeable.  Parameters without a gradient are skipped by the update either way.
        params = list(self.model.parameters())
        if on_gpu:
            from .optim import FusedAdamW                       # same rule / state layout, one launch, 1/world folded in
            self.optimizer = FusedAdamW(params, lr=cfg.lr, grad_scale=1.0 / self.world)
        else:
            self.optimizer = torch.optim.AdamW(params, lr=cfg.lr)
        self.lr_scheduler = torch.optim.lr_scheduler.StepLR(self.optimizer, step_size=cfg.lr_drop,
                                                            gamma=cfg.lr_decay_gamma)
        self.start_epoch = 0
        if self.sdf_source is None and sdf_store is None:
            from .sdf_data import MeshSdfSource, mesh_sdf_enabled, procedural_templates
            if mesh_sdf_enabled(cfg):       # cfg.sdf_source = "mesh" / HOISDF_SDF=mesh without a source: the model's own MANO layer, procedural objects
                head = getattr(self.model, "mano_head", None)
                layer = head.mano_layer if head is not None else self.model.ik_mano_layer
                self.sdf_source = MeshSdfSource(layer, procedural_templates(), cfg)
        if self.seg_source is None:
            from .render import MeshSegSource, seg_from_mesh
            if seg_from_mesh(cfg):          # cfg.seg_source = "mesh" / HOISDF_SEG=mesh without a source: the SDF source's meshes, else the same stand-ins
                src = self.sdf_source
                if src is None:
                    from .sdf_data import MeshSdfSource, procedural_templates
                    head = getattr(self.model, "mano_head", None)
                    src = MeshSdfSource(head.mano_layer if head is not None else self.model.ik_mano_layer, procedural_templates(), cfg)
                self.seg_source = MeshSegSource(src, cfg)
        self.interaction_source = None
        # cfg.interaction_loss / HOISDF_INTERACTION_LOSS=1, cfg.silhouette_loss / HOISDF_SILHOUETTE_LOSS=1 (both pose the predicted
        # pair from the same templates): the meshes of the existing source, else the same stand-ins
        if self.model.interaction_loss_enabled() or self.model.silhouette_loss_enabled():
            src = self.sdf_source if self.sdf_source is not None else getattr(self.seg_source, "source", None)
            if src is None:
                from .sdf_data import MeshSdfSource, procedural_templates
                src = MeshSdfSource(self.model.mano_head.mano_layer, procedural_templates(), cfg)
            self.interaction_source = src
            self.model.set_interaction_source(src)
        if dataset is None and sdf_store is not None:
            dataset = SyntheticSdfDataset(cfg, sdf_store.n_frames, seed=self.rank)
        elif dataset is None and self.sdf_source is not None:
            dataset = SyntheticMeshSdfDataset(cfg, self.sdf_source.n_templates, seed=self.rank)
        elif dataset is None and self.seg_source is not None:      # the full synthetic sample + the template its masks are rendered from
            dataset = SyntheticMeshSdfDataset(cfg, self.seg_source.n_templates, seed=self.rank, keep_points=True)
        elif dataset is None and self.interaction_source is not None:   # likewise: the template the predicted object is posed from
            dataset = SyntheticMeshSdfDataset(cfg, self.interaction_source.n_templates, seed=self.rank, keep_points=True)
        ds = dataset if dataset is not None else SyntheticDataset(cfg, seed=self.rank)
        bs = batch_size or cfg.train_batch_size
        sampler = torch.utils.data.distributed.DistributedSampler(ds, self.world, self.rank, shuffle=True) \
            if self.world > 1 else None
        self.batch_generator = torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=sampler is None, sampler=sampler,
                                                           num_workers=0, drop_last=True, pin_memory=True)
        self.sampler = sampler
        self.itr_per_epoch = len(self.batch_generator)
        self.begin_epoch(self.start_epoch)

    def begin_epoch(self, epoch: int):
        """Per-epoch, per-rank random streams: a new DistributedSampler shuffle every epoch, and distinct dropout masks /
        point jitter on every rank (the weights were initialised from the shared seed above).  Also what --continue
        resumes with, so a resumed epoch does not replay the streams of epoch 0."""
        if self.sampler is not None:
            self.sampler.set_epoch(epoch)
        from . import ops
        s = self.base_seed + 1000003 * (epoch + 1) + 7919 * self.rank
        torch.manual_seed(s)
        ops.manual_seed(s)
        self.model._py_random.seed(s)                            # the branch A / B draw (main/model.py:426)
        self._epoch_seed, self._sdf_draws = s, 0                 # the device-side SDF point draw restarts per epoch too

    def train_step(self, inputs, targets, meta, epoch: int, batch_ratio: float):
        dev = self.device
        if "frame" in inputs and native_image_enabled(self.cfg):
            from .image_data import ImagePipeline
            if getattr(self, "_image_pipeline", None) is None:
                self._image_pipeline = ImagePipeline(self.cfg, dev, nchw=False)
            self._image_draws = getattr(self, "_image_draws", 0) + 1
            rng = np.random.default_rng(_mix_seed(getattr(self, "_epoch_seed", self.base_seed), (1 << 20) + self._image_draws))
            apply_image_pipeline(self._image_pipeline, inputs, targets, meta, rng)
        inputs, targets, meta = (T.to_device(x, dev) for x in (inputs, targets, meta))
        pts = None
        if self.sdf_store is not None and "sdf_frame" in meta:
            c = self.cfg
            self._sdf_draws += 1
            pts = self.sdf_store.make_inputs(
                meta["sdf_frame"].cpu(), meta["mano_root"], meta["obj_center_cam"], c.num_samp_hand, c.num_samp_obj,
                c.points_filter_dist, c.hand_sdf_scale, c.obj_sdf_scale, train=True,
                seed=_mix_seed(self._epoch_seed, self._sdf_draws),
                do_flip=meta.get("do_flip"), rot_mat=meta.get("aug_rot"))
        elif self.sdf_source is not None and "obj_cls" in meta and "hand_sdf_points" not in inputs:
            c = self.cfg
            self._sdf_draws += 1
            pts = self.sdf_source.make_inputs(targets, meta, c.num_samp_hand, c.num_samp_obj, c.points_filter_dist, c.hand_sdf_scale,
                                              c.obj_sdf_scale, train=True, seed=_mix_seed(self._epoch_seed, self._sdf_draws))
        if pts is not None:
            for k in ("hand_sdf_points", "obj_sdf_points", "hand_pre_points", "obj_pre_points"):
                inputs[k] = pts[k]
            targets["hand_sdf"], targets["obj_sdf"] = pts["hand_sdf"], pts["obj_sdf"]
        if self.seg_source is not None:
            self.seg_source.fill(targets, meta)                   # hand_seg / obj_seg: the silhouettes of the step's own label meshes
        if self.channels_last:
            inputs["img"] = inputs["img"].contiguous(memory_format=torch.channels_last)
        self.reducer.zero_grad()
        out = self.model(inputs, targets, meta, "train", epoch, batch_ratio)
        total, loss, _ = weighted_total(out, self.cfg)
        total.backward()
        self.reducer.finish()
        self.optimizer.step()
        self._steps_done = getattr(self, "_steps_done", 0) + 1
        if self._steps_done == 3 and dev.type == "cuda":
            # the allocator has seen the step's pattern: leave it free cached blocks on both streams, so that a later step that
            # allocates differently (the other point branch, the two streams racing) does not stall in a hipMalloc
            self.hbm_pool_bytes = reserve_hbm_pool(self.model, float(getattr(self.cfg, "hbm_pool_fraction", 0.5)), dev)
        return total.detach(), {k: v.detach() for k, v in loss.items()}

    def save_model(self, epoch: int, itr: int) -> Optional[str]:
        if self.rank != 0:
            return None
        os.makedirs(self.cfg.model_dir, exist_ok=True)
        path = snapshot_path(self.cfg.model_dir, epoch, itr)
        torch.save({"epoch": epoch, "network": to_reference_state_dict(self.model),
                    "optimizer": self.optimizer.state_dict(), "lr_scheduler": self.lr_scheduler.state_dict()}, path)
        return path

    def load_model(self) -> int:
        found = latest_snapshot(self.cfg.model_dir)
        if found is None:
            return 0
        ckpt = torch.load(found[0], map_location=self.device)
        load_reference_state_dict(self.model, ckpt["network"], strict=True)
        self.optimizer.load_state_dict(ckpt["optimizer"])
        self.lr_scheduler.load_state_dict(ckpt["lr_scheduler"])
        self.start_epoch = ckpt["epoch"] + 1
        return self.start_epoch


class Tester:
    def __init__(self, cfg: Config, device: torch.device, ckpt_path: Optional[str] = None):
        self.cfg, self.device = cfg, device
        self.model = get_model("test", cfg=cfg).to(device).eval()
        if ckpt_path:
            ckpt = torch.load(ckpt_path, map_location=device)
            load_reference_state_dict(self.model, ckpt["network"], strict=True)

    @torch.no_grad()
    def predict(self, inputs, targets, meta, mano_layer=None):
        """eval forward; for the IK variant (``cfg.use_inverse_kinematics``) the closed-form IK post-process of
        main/test.py:139-160 runs on the device as well when a MANO layer is given: adds ``ik_joints_out`` /
        ``ik_verts_out`` (root-relative metres, before the caller's mano_root shift) and ``ik_pose_out``.  With
        ``cfg.native_ik`` / ``HOISDF_IK=native`` the post-process is one HIP launch (hoisdf_ik_mano_fwd) - the last launch of
        hoisdf_pose_infer itself when native inference is on as well."""
        from .ik import ik_solver_mano, ik_solver_mano_native, native_ik_enabled
        if "frame" in inputs and native_image_enabled(self.cfg):
            from .image_data import ImagePipeline
            if getattr(self, "_image_pipeline", None) is None:
                self._image_pipeline = ImagePipeline(self.cfg, self.device, nchw=False)      # NHWC: what hoisdf_encoder_infer reads
            apply_image_pipeline(self._image_pipeline, inputs, targets, meta)
        inputs, targets, meta = (T.to_device(x, self.device) for x in (inputs, targets, meta))
        ik = self.cfg.use_inverse_kinematics and mano_layer is not None
        native = ik and native_ik_enabled(self.cfg)
        if native and self.model.ik_mano_layer is not mano_layer:
            self.model.set_ik_mano_layer(mano_layer)             # (moved to the device by the first native call that reads it)
        out = self.model(inputs, targets, meta, "eval")
        if native and "ik_pose_out" not in out:          # (there already: hoisdf_pose_infer ran the solve)
            if next(mano_layer.buffers()).device != out["hand_joints_out"].device:
                mano_layer.to(self.device)
            r = ik_solver_mano_native(mano_layer, out.get("mano_shape_out"), out["hand_joints_out"])
            out["ik_joints_out"], out["ik_verts_out"], out["ik_pose_out"] = r["joints"], r["verts"], r["pose"]
        elif ik and not native:
            hj = torch.cat([torch.zeros_like(out["hand_joints_out"][:, :1]), out["hand_joints_out"]], 1)
            r = ik_solver_mano(mano_layer.to(self.device), out.get("mano_shape_out"), hj)
            out["ik_joints_out"], out["ik_verts_out"], out["ik_pose_out"] = r["joints"], r["verts"], r["pose"]
        return out


def mpjpe(pred: torch.Tensor, gt: torch.Tensor) -> float:
    """mean per-joint position error (common/metrics.py:213-232), inputs (N,J,3)."""
    return float((pred - gt).norm(dim=-1).mean())


def pa_mpjpe(pred: torch.Tensor, gt: torch.Tensor) -> float:
    """MPJPE after a per-sample similarity (Procrustes) alignment (common/metrics.py:188-232)."""
    errs = []
    for p, g in zip(pred.double().cpu(), gt.double().cpu()):
        mp, mg = p.mean(0), g.mean(0)
        p0, g0 = p - mp, g - mg
        U, S, Vt = torch.linalg.svd(p0.T @ g0)
        d = torch.sign(torch.linalg.det(U @ Vt))
        D = torch.diag(torch.tensor([1.0, 1.0, float(d)], dtype=torch.float64))
        R = U @ D @ Vt
        s = (S * torch.diag(D)).sum() / (p0 ** 2).sum()
        errs.append(float(((s * p0 @ R + mg) - g).norm(dim=-1).mean()))
    return sum(errs) / max(len(errs), 1)
