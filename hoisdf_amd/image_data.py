"""The image half of the dataset's work on the device (csrc/imgprep.hip, csrc/imgprep_params.c): crop parameters, the affine warp of
the frame and its two masks, the photometric augmentation, and the labels that move with them - what the reference's ``__getitem__``
does per sample with PIL and numpy (data/dexycb.py:219-404).  Opt-in (``cfg.native_image`` / HOISDF_IMAGE=native); there is no CPU
fallback: the kernels are the path.  hoisdf_amd/image_oracle.py states the same arithmetic in numpy for the tests.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import image_oracle as IO

OPS = IO.OPS


def _labels(joints_uv, p2d, K):
    j = np.ascontiguousarray(joints_uv, np.float32).reshape(-1, 2)
    p = np.ascontiguousarray(p2d, np.float64).reshape(-1, 2)
    k = np.ascontiguousarray(K, np.float64).reshape(9)
    return j, p, k


def crop_params(joints_uv, p2d, K, frame_w: int, frame_h: int, flip: bool, res: int, hm: int) -> _lib.Crop:
    """hoisdf_crop_params_dexycb: the evaluation crop of the RAW frame's labels (float32 joints, float64 corners, 3 x 3 K)"""
    j, p, k = _labels(joints_uv, p2d, K)
    out = _lib.Crop()
    _lib.call("hoisdf_crop_params_dexycb", j.ctypes.data, len(j), p.ctypes.data, len(p), k.ctypes.data, int(frame_w), int(frame_h),
              int(bool(flip)), int(res), int(hm), C.addressof(out))
    return out


def crop_params_ho3d(bbox_hand, p2d, K, frame_w: int, frame_h: int, res: int, hm: int) -> _lib.Crop:
    """hoisdf_crop_params_ho3d: the hand is a box (x0, y0, x1, y1)"""
    b = np.ascontiguousarray(bbox_hand, np.float64).reshape(4)
    _, p, k = _labels(np.zeros((1, 2)), p2d, K)
    out = _lib.Crop()
    _lib.call("hoisdf_crop_params_ho3d", b.ctypes.data, p.ctypes.data, len(p), k.ctypes.data, int(frame_w), int(frame_h), int(res), int(hm),
              C.addressof(out))
    return out


def aug_params(joints_uv, p2d, K, frame_w: int, frame_h: int, flip: bool, res: int, hm: int, center_u, scale_jitter: float, rot: float,
               center_jittering: float = 0.1) -> _lib.Crop:
    """hoisdf_aug_params_dexycb: the training crop with its random numbers given (``draw_aug`` draws them)"""
    j, p, k = _labels(joints_uv, p2d, K)
    cu = np.ascontiguousarray(center_u, np.float64).reshape(2)
    out = _lib.Crop()
    _lib.call("hoisdf_aug_params_dexycb", j.ctypes.data, len(j), p.ctypes.data, len(p), k.ctypes.data, int(frame_w), int(frame_h),
              int(bool(flip)), int(res), int(hm), float(center_jittering), cu.ctypes.data, float(scale_jitter), float(rot), C.addressof(out))
    return out


def crop_to_dict(c: _lib.Crop) -> Dict[str, np.ndarray]:
    f = lambda a, shape, dt: np.ctypeslib.as_array(a).astype(dt).reshape(shape).copy()
    return dict(affine=f(c.affine, (3, 3), np.float32), post_rot_trans=f(c.post_rot_trans, (3, 3), np.float32),
                rot_mat=f(c.rot_mat, (3, 3), np.float32), inverse=f(c.inverse, (2, 3), np.float64), K=f(c.K, (3, 3), np.float64),
                bbox_hand=f(c.bbox_hand, (4,), np.float64), bbox_obj=f(c.bbox_obj, (4,), np.float64), flip=int(c.flip),
                joints_uv=f(c.joints_uv, (-1, 2), np.float64)[:c.n_joints], p2d=f(c.p2d, (-1, 2), np.float64)[:c.n_corners])


def crop_from_inverse(inverse, flip: bool = False) -> _lib.Crop:
    """a hoisdf_crop that carries only what the warp reads (tests, callers with their own affine)"""
    c = _lib.Crop()
    c.inverse[:] = [float(v) for v in np.asarray(inverse, np.float64).reshape(6)]
    c.flip = int(bool(flip))
    return c


def make_photo(blur_sigma: float, factors: Sequence[Optional[float]], order: Sequence[int]) -> _lib.Photo:
    """``factors`` in OPS order (brightness, contrast, saturation, hue), None = the op is absent; ``order``: a permutation of 0..3"""
    p = _lib.Photo()
    p.blur_sigma = float(blur_sigma)
    p.enabled = 0
    for i, v in enumerate(factors):
        if v is not None:
            p.factor[i] = float(v)
            p.enabled |= 1 << i
    p.order[:] = [int(o) for o in order]
    return p


def draw_aug(rng: np.random.Generator, n: int, max_rot=np.pi, scale_jittering=0.2, center_jittering=0.1, hue=0.15, saturation=0.5,
             contrast=0.5, brightness=0.5, blur_radius=0.5) -> List[dict]:
    """The DISTRIBUTION of data/dexycb.py:253-273, :312 and dataset_util.get_color_params / color_jitter on a numpy Generator (same
    distribution, another stream; defaults = the class defaults of data/dexycb.py:32-39)."""
    out = []
    for _ in range(n):
        center_u = rng.uniform(-1, 1, 2)
        sj = float(np.clip(scale_jittering * rng.standard_normal() + 1, 1 - scale_jittering, 1 + scale_jittering))
        rot = float(np.clip(rng.standard_normal(), -2.0, 2.0) * 30) if rng.random() <= 0.6 else 0.0
        rot = rot * max_rot / 180
        blur = rng.random() * blur_radius
        fac = [rng.uniform(max(0, 1 - brightness), 1 + brightness) if brightness > 0 else None,
               rng.uniform(max(0, 1 - contrast), 1 + contrast) if contrast > 0 else None,
               rng.uniform(max(0, 1 - saturation), 1 + saturation) if saturation > 0 else None,
               rng.uniform(-hue, hue) if hue > 0 else None]
        out.append(dict(center_u=center_u, center_jittering=center_jittering, scale_jitter=sj, rot=rot, blur=blur, factors=fac,
                        order=[int(o) for o in rng.permutation(4)]))
    return out


# ---------------------------------------------------------------------------------------------- device calls
def _frames_array(frames, hand_masks, obj_masks, packed: bool):
    B = len(frames)
    arr = (_lib.Frame * max(B, 1))()
    for b in range(B):
        f, h, o = frames[b], hand_masks[b], obj_masks[b]
        for t in (f, h, o):
            if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous()):
                raise ValueError("frames and masks must be contiguous uint8 CUDA tensors")
        H, W = int(f.shape[0]), int(f.shape[1])
        need = (H * W + 7) // 8 if packed else H * W
        if f.shape[2] != 3 or h.numel() < need or o.numel() < need:
            raise ValueError(f"sample {b}: frame {tuple(f.shape)} with masks of {h.numel()} / {o.numel()} bytes")
        arr[b].frame, arr[b].hand_mask, arr[b].obj_mask = f.data_ptr(), h.data_ptr(), o.data_ptr()
        arr[b].H, arr[b].W, arr[b].mask_packed = H, W, int(packed)
    return arr


def _crops_array(crops: Sequence[_lib.Crop]):
    arr = (_lib.Crop * max(len(crops), 1))()
    for b, c in enumerate(crops):
        arr[b] = c
    return arr


def _outputs(B, res, hm, nchw, dev, want_u8):
    img = torch.empty((B, 3, res, res) if nchw else (B, res, res, 3), dtype=torch.float32, device=dev)
    u8 = torch.empty((B, res, res, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    return img, u8, torch.empty((B, hm, hm), dtype=torch.float32, device=dev), torch.empty((B, hm, hm), dtype=torch.float32, device=dev)


def image_crop(frames, hand_masks, obj_masks, crops: Sequence[_lib.Crop], res: int, hm: int, nchw: bool = False, packed: bool = False,
               want_u8: bool = False) -> Dict[str, torch.Tensor]:
    """hoisdf_image_crop on the current stream.  frames: [B][H][W][3] uint8 tensor or a list of [H][W][3] tensors (sizes may differ)."""
    B = len(frames)
    dev = frames[0].device if B else torch.device("cuda")
    img, u8, hs, os_ = _outputs(B, res, hm, nchw, dev, want_u8)
    fr, cr = _frames_array(frames, hand_masks, obj_masks, packed), _crops_array(crops)
    _lib.call("hoisdf_image_crop", C.addressof(fr), C.addressof(cr), B, int(res), int(hm), int(nchw), img.data_ptr(),
              u8.data_ptr() if want_u8 else None, hs.data_ptr(), os_.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return dict(img=img, crop_u8=u8, hand_seg=hs, obj_seg=os_)


def image_augment(frames, hand_masks, obj_masks, crops: Sequence[_lib.Crop], photo: Sequence[_lib.Photo], res: int, hm: int,
                  nchw: bool = False, packed: bool = False) -> Dict[str, torch.Tensor]:
    """hoisdf_image_augment on the current stream; ``crop_u8`` is the warped crop before the chain, ``lsum`` the contrast's luma sums"""
    B = len(frames)
    dev = frames[0].device if B else torch.device("cuda")
    img, u8, hs, os_ = _outputs(B, res, hm, nchw, dev, True)
    lsum = torch.empty((max(B, 1),), dtype=torch.int32, device=dev)
    fr, cr = _frames_array(frames, hand_masks, obj_masks, packed), _crops_array(crops)
    ph = (_lib.Photo * max(B, 1))()
    for b, p in enumerate(photo):
        ph[b] = p
    _lib.call("hoisdf_image_augment", C.addressof(fr), C.addressof(cr), C.addressof(ph), B, int(res), int(hm), int(nchw), img.data_ptr(),
              u8.data_ptr(), lsum.data_ptr(), hs.data_ptr(), os_.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return dict(img=img, crop_u8=u8, hand_seg=hs, obj_seg=os_, lsum=lsum[:B])


# ---------------------------------------------------------------------------------------------- the pipeline
def flip_labels_3d(lab: dict) -> dict:
    """the left-hand mirror of the 3D labels (data/dexycb.py:459-462, :502-503): x -> -x, axis-angle (x, y, z) -> (x, -y, -z)"""
    out = dict(lab)
    for k in ("joints_3d", "p3d"):
        if k in out:
            v = np.array(out[k], np.float64)
            v[:, 0] *= -1
            out[k] = v
    if "obj_trans" in out:
        v = np.array(out["obj_trans"], np.float64)
        v[0] *= -1
        out["obj_trans"] = v
    if "obj_rot" in out:
        v = np.array(out["obj_rot"], np.float64)
        v[1:] *= -1
        out["obj_rot"] = v
    if "mano_param" in out:
        v = np.array(out["mano_param"], np.float64)
        pose = v[:48].reshape(-1, 3)
        pose[:, 1:] *= -1
        out["mano_param"] = v
    return out


class ImagePipeline:
    """Raw frames -> the image entries of the reference's ``inputs`` / ``targets`` / ``meta_info`` on ``device``.

    ``frames`` / ``masks``: per sample a uint8 [H][W][3] frame and a (hand, object) pair of [H][W] byte masks (or packed bits with
    ``packed_masks=True``), numpy or tensors; ``labels``: per sample a dict with ``joints_uv`` (21, 2), ``p2d`` (21, 2), ``K`` (3, 3),
    ``flip`` and optionally the 3D labels ``joints_3d``, ``p3d``, ``mano_param``, ``obj_rot``, ``obj_trans`` of the RAW frame."""

    def __init__(self, cfg, device, nchw: bool = True, packed_masks: bool = False):
        self.res, self.hm = int(cfg.input_img_shape[0]), int(cfg.output_hm_shape[0])
        self.device, self.nchw, self.packed = torch.device(device), bool(nchw), bool(packed_masks)

    def _dev(self, a):
        t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, np.uint8))
        return t.to(self.device, non_blocking=True).contiguous()

    def _upload(self, frames, masks):
        """-> per-sample device tensors; a whole [B][H][W][3] batch (and a (hand, object) pair of [B][H][W] batches) moves in one copy"""
        if torch.is_tensor(frames) and isinstance(masks, tuple) and torch.is_tensor(masks[0]) and masks[0].dim() == frames.dim() - 1:
            return list(self._dev(frames)), list(self._dev(masks[0])), list(self._dev(masks[1]))
        return [self._dev(f) for f in frames], [self._dev(m[0]) for m in masks], [self._dev(m[1]) for m in masks]

    def _pack(self, dev_out, crops, labels3d):
        cd = [crop_to_dict(c) for c in crops]
        t = lambda key, dt=np.float32: torch.from_numpy(np.stack([np.asarray(d[key], dt) for d in cd])).to(self.device)
        out = dict(img=dev_out["img"], hand_seg=dev_out["hand_seg"], obj_seg=dev_out["obj_seg"], cam_intr=t("K"), bbox_hand=t("bbox_hand"),
                   bbox_obj=t("bbox_obj"), joint_coord=t("joints_uv"), p2d=t("p2d"), rot_mat=t("rot_mat"),
                   do_flip=torch.tensor([bool(d["flip"]) for d in cd], device=self.device))
        if labels3d and all(l is not None for l in labels3d):
            for k in labels3d[0]:
                out[k] = torch.from_numpy(np.stack([np.asarray(l[k], np.float32) for l in labels3d])).to(self.device)
        for k in ("crop_u8", "lsum"):
            if dev_out.get(k) is not None:
                out[k] = dev_out[k]
        return out

    @staticmethod
    def _labels_3d(lab, rot_mat):
        """whichever 3D labels the sample carries, mirrored (left hand) and turned by the crop's in-plane rotation, host float64"""
        keys = [k for k in ("joints_3d", "p3d", "mano_param", "obj_rot", "obj_trans") if k in lab]
        if not keys:
            return None
        l = {k: np.asarray(torch.as_tensor(lab[k]).cpu().numpy() if torch.is_tensor(lab[k]) else lab[k], np.float64) for k in keys}
        if lab.get("flip_3d", lab.get("flip")):          # flip_3d = False: the labels are those of the mirrored frame already
            l = flip_labels_3d(l)
        R = np.asarray(rot_mat, np.float64)
        out = {}
        for k in keys:
            if k in ("joints_3d", "p3d"):
                out[k] = l[k] @ R.T
            elif k == "obj_trans":
                out[k] = R @ l[k]
            elif k == "obj_rot":
                out[k] = IO.rodrigues_inv(R @ IO.rodrigues(l[k]))
            else:
                out[k] = l[k].copy()
                out[k][:3] = IO.rodrigues_inv(R @ IO.rodrigues(l[k][:3]))
        return out

    def eval_batch(self, frames, masks, labels) -> Dict[str, torch.Tensor]:
        f, h, o = self._upload(frames, masks)
        crops = [crop_params(l["joints_uv"], l["p2d"], l["K"], f[b].shape[1], f[b].shape[0], l.get("flip", False), self.res, self.hm)
                 for b, l in enumerate(labels)]
        dev_out = image_crop(f, h, o, crops, self.res, self.hm, nchw=self.nchw, packed=self.packed)
        return self._pack(dev_out, crops, [self._labels_3d(l, np.eye(3)) for l in labels])

    def train_batch(self, frames, masks, labels, rng: np.random.Generator, draws: Optional[List[dict]] = None) -> Dict[str, torch.Tensor]:
        f, h, o = self._upload(frames, masks)
        draws = draw_aug(rng, len(labels)) if draws is None else draws
        crops = [aug_params(l["joints_uv"], l["p2d"], l["K"], f[b].shape[1], f[b].shape[0], l.get("flip", False), self.res, self.hm,
                            d["center_u"], d["scale_jitter"], d["rot"], d.get("center_jittering", 0.1))
                 for b, (l, d) in enumerate(zip(labels, draws))]
        photo = [make_photo(d["blur"], d["factors"], d["order"]) for d in draws]
        dev_out = image_augment(f, h, o, crops, photo, self.res, self.hm, nchw=self.nchw, packed=self.packed)
        return self._pack(dev_out, crops, [self._labels_3d(l, crop_to_dict(c)["rot_mat"]) for l, c in zip(labels, crops)])
