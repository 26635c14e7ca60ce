"""What the mesh rasteriser (csrc/raster.hip, ops.raster_meshes) is used for, all three off by default:
  * ``MeshSegSource`` - the mask targets of a training step rendered from the step's own label meshes (cfg.seg_source = "mesh");
  * ``predicted_pair`` - the predicted hand and object of a batch posed in the camera frame, the one place where that posing
    happens: the interaction block, the silhouette block (metrics.Evaluator) and the overlays all take it from here;
  * ``overlay_batch`` / ``write_overlays`` - the predicted pair blended over the input crop (test.py --overlay DIR).
Nothing here renders on the host: hoisdf_amd/raster_oracle.py is the tests' yardstick, not a fallback."""
from __future__ import annotations

import os
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops

HAND_COLOUR, OBJ_COLOUR = (70, 130, 255), (255, 160, 40)


def seg_from_mesh(cfg=None) -> bool:
    """cfg.seg_source == "mesh" (default "": off) or HOISDF_SEG=mesh"""
    return getattr(cfg, "seg_source", "") == "mesh" or os.environ.get("HOISDF_SEG", "") == "mesh"


def camera_rows(cam_intr: torch.Tensor) -> torch.Tensor:
    """meta["cam_intr"] (B, 3, 3) (or its top two rows already) -> K (B, 6) as hoisdf_raster_meshes takes it"""
    K = cam_intr.float()
    return (K[:, :2, :] if K.dim() == 3 else K).reshape(K.shape[0], 6).contiguous()


def mask_camera_rows(cam_intr: torch.Tensor, cfg) -> torch.Tensor:
    """meta["cam_intr"] -> K (B, 6) for the MASK grid of cfg.output_hm_shape, as ops.silhouette_loss takes it: a point that
    projects onto the sample point of the raster pixel a mask pixel reads lands on that mask pixel.  The masks are the NEAREST fold of
    a cfg.input_img_shape raster: mask pixel i reads raster pixel floor((i + .5) s) = s i + floor(s / 2), s = W / hm_w a whole
    number, and that raster pixel is sampled at its index (cfg.raster_half_pixel: + 0.5).  So i = (u - floor(s / 2) - 0.5 half) / s:
    the first row of K is divided by s after the offset left its third entry, the second row likewise with H / hm_h."""
    K = camera_rows(cam_intr).clone()
    hm_h, hm_w = _hm_shape(cfg)
    H, W = int(cfg.input_img_shape[0]), int(cfg.input_img_shape[1])
    if W % hm_w or H % hm_h:
        raise ValueError(f"mask_camera_rows: the raster {W} x {H} must be a whole multiple of the mask grid {hm_w} x {hm_h}")
    half = 0.5 if bool(cfg.raster_half_pixel) else 0.0
    for row, s in ((0, W // hm_w), (1, H // hm_h)):
        K[:, 3 * row + 2] -= s // 2 + half
        K[:, 3 * row:3 * row + 3] /= s
    return K


def _hm_shape(cfg) -> Tuple[int, int]:
    return int(cfg.output_hm_shape[-2]), int(cfg.output_hm_shape[-1])


class MeshSegSource:
    """targets["hand_seg"] / ["obj_seg"] of a batch rendered on the device from the batch's own label meshes: the modal silhouettes
    of the ground-truth hand and object (``MeshSdfSource.meshes``: MANO through targets["mano_param"] at meta["mano_root"], the
    template meta["obj_cls"] placed by targets["obj_rot"] / ["rel_obj_trans"] + meta["obj_center_cam"]) seen through the crop's
    meta["cam_intr"], rendered with mutual occlusion at cfg.input_img_shape and folded to cfg.output_hm_shape like image_crop folds
    a mask file.  ``mesh_source``: a ``MeshSdfSource`` (shared with cfg.sdf_source = "mesh"), or a MANO layer with ``templates`` =
    the dict of ``sdf_data.pack_templates``."""

    def __init__(self, mesh_source, cfg, templates: Optional[Dict[str, torch.Tensor]] = None):
        if templates is not None:
            from .sdf_data import MeshSdfSource
            mesh_source = MeshSdfSource(mesh_source, templates, cfg)
        if not hasattr(mesh_source, "meshes"):
            raise ValueError("MeshSegSource: a MeshSdfSource, or a MANO layer together with templates")
        self.source, self.cfg = mesh_source, cfg
        self.n_templates = mesh_source.n_templates

    def meshes(self, targets, meta):
        return self.source.meshes(targets, meta)

    def render(self, targets, meta, want=()) -> Dict[str, torch.Tensor]:
        """-> hand_seg, obj_seg float32 (B, hm_h, hm_w) and what ``want`` names of ops.raster_meshes' ids / depth / counts"""
        c = self.cfg
        hand, hf, obj, of, on = self.source.meshes(targets, meta)
        H, W = int(c.input_img_shape[0]), int(c.input_img_shape[1])
        return ops.raster_meshes(hand, hf, obj, of, camera_rows(meta["cam_intr"].to(hand.device)), W, H, obj_n_faces=on,
                                 half_pixel=bool(c.raster_half_pixel), near=float(c.raster_near), hm_shape=_hm_shape(c), want=want)

    def fill(self, targets, meta) -> None:
        """the two mask targets, filled or replaced in place"""
        if "obj_cls" not in meta:
            raise ValueError("seg_source = \"mesh\": the batch's meta_info must name each sample's object template (obj_cls)")
        res = self.render(targets, meta)
        targets["hand_seg"], targets["obj_seg"] = res["hand_seg"], res["obj_seg"]


class PairSource:
    """What ``predicted_pair`` needs to pose the pair, and nothing else: the object templates as meshes and the hand's faces on one
    device.  templates (T, V, 3); template_faces = the ``faces`` (T, F, 3) / ``n_faces`` (T,) of sdf_data.pack_templates (whose
    ``verts`` are ``templates``); hand_faces (Fh, 3) = the MANO layer's ``th_faces``.  For a caller without an Evaluator: the
    refinement of the eval forward (Model.set_refine_source)."""

    def __init__(self, cfg, templates: torch.Tensor, template_faces: Dict[str, torch.Tensor], hand_faces: torch.Tensor):
        self.cfg, self.templates, self.dev = cfg, templates, templates.device
        self._tfaces = torch.as_tensor(template_faces["faces"]).to(self.dev, torch.int32)
        n = template_faces.get("n_faces")
        self._tn = (torch.full((self._tfaces.shape[0],), self._tfaces.shape[1], dtype=torch.int32) if n is None else torch.as_tensor(n))
        self._tn = self._tn.to(self.dev, torch.int32)
        self._hfaces = torch.as_tensor(hand_faces).to(self.dev, torch.int32)
        if self._tfaces.dim() != 3 or self._tfaces.shape[0] != templates.shape[0] or self._tn.shape != (templates.shape[0],):
            raise ValueError(f"template_faces {tuple(self._tfaces.shape)} for {templates.shape[0]} templates")


def predicted_pair(out, meta, obj_cls, evaluator):
    """The PREDICTED pair of every sample in the camera frame: hand = the predicted MANO mesh (the IK variant: its solved mesh) +
    mano_root, object = the template obj_cls turned and moved by the mean predicted rotation and translation + obj_center_cam.
    ``evaluator``: a metrics.Evaluator built with template_faces / hand_faces, or a ``PairSource``.
    -> hand (B, 778, 3), hand faces (Fh, 3), obj (B, V, 3), obj faces (B, F, 3), obj face counts (B,), used (B,) bool: obj_cls >= 0
    (a sample that is not used borrows template 0)"""
    from .metrics import batch_rodrigues
    ev = evaluator
    if getattr(ev, "_hfaces", None) is None:
        raise ValueError("predicted_pair: the Evaluator needs template_faces and hand_faces")
    dev = ev.dev
    root = meta["mano_root"].to(dev)
    hand = (out["ik_verts_out"] if ev.cfg.use_inverse_kinematics else out["mano_mesh_out"]).detach() + root[:, None]
    cls = torch.as_tensor(obj_cls).to(dev).long()
    used = cls >= 0
    cls = cls.clamp_min(0)
    rot, trans = out["obj_rot_out"].detach().mean(1), out["obj_trans_out"].detach().mean(1)
    obj = ev.templates[cls] @ batch_rodrigues(rot).transpose(1, 2) + (trans + meta["obj_center_cam"].to(dev))[:, None]
    return hand, ev._hfaces, obj, ev._tfaces[cls], ev._tn[cls], used


def render_pair(pair, cam_intr, cfg, want=("ids",), masks: bool = False) -> Dict[str, torch.Tensor]:
    """a pair as ``predicted_pair`` returns it through the crop's camera at cfg.input_img_shape; a sample that is not ``used`` has
    no object (face count 0) instead of the borrowed template"""
    hand, hf, obj, of, on, used = pair
    on = torch.where(used, on, torch.zeros_like(on))
    H, W = int(cfg.input_img_shape[0]), int(cfg.input_img_shape[1])
    return ops.raster_meshes(hand, hf, obj, of, camera_rows(cam_intr.to(hand.device)), W, H, obj_n_faces=on,
                             half_pixel=bool(cfg.raster_half_pixel), near=float(cfg.raster_near),
                             hm_shape=_hm_shape(cfg) if masks else None, want=want)


def image_u8(img: torch.Tensor) -> torch.Tensor:
    """the model's input crop, float (B, 3, H, W) in 0 .. 1 (any memory format) or uint8 (B, H, W, 3) -> uint8 (B, H, W, 3)"""
    if img.dtype == torch.uint8:
        return img.contiguous()
    return (img.detach().float().permute(0, 2, 3, 1) * 255.0 + 0.5).floor().clamp(0, 255).to(torch.uint8).contiguous()


def overlay_batch(img, ids, colour=(HAND_COLOUR, OBJ_COLOUR), alpha: int = 160) -> torch.Tensor:
    """img as ``image_u8`` takes it, ids int32 (B, H, W) of ops.raster_meshes -> uint8 (B, H, W, 3) on the device: flat colours, a
    covered pixel is (alpha colour[mesh] + (256 - alpha) image + 128) >> 8"""
    return ops.raster_overlay(ids, image_u8(img).to(ids.device), colour, int(alpha))


def write_image(path_stem: str, rgb: np.ndarray) -> str:
    """uint8 (H, W, 3) -> path_stem + ".png" through PIL where it imports, otherwise a binary PPM (P6) -> the path written"""
    rgb = np.ascontiguousarray(rgb, np.uint8)
    try:
        from PIL import Image
    except ImportError:
        path = path_stem + ".ppm"
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]))
            f.write(rgb.tobytes())
        return path
    path = path_stem + ".png"
    Image.fromarray(rgb, "RGB").save(path)
    return path


def write_overlays(out_dir: str, first: int, inputs, out, meta, obj_cls, evaluator, cfg):
    """one image per sample of the batch, ``overlay_<index>`` counted from ``first``: the predicted pair over inputs["img"]"""
    os.makedirs(out_dir, exist_ok=True)
    pair = predicted_pair(out, meta, obj_cls, evaluator)
    ids = render_pair(pair, meta["cam_intr"], cfg)["ids"]
    over = overlay_batch(inputs["img"], ids, alpha=int(cfg.overlay_alpha)).cpu().numpy()
    return [write_image(os.path.join(out_dir, "overlay_%05d" % (first + b)), over[b]) for b in range(over.shape[0])]
