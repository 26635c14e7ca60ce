"""Generator of tests/golden/g16_image_crop.npz and g17_image_aug.npz: the image half of the reference's ``__getitem__``.

    python tests/golden/make_golden_image.py REFERENCE_ROOT          (or HOISDF_REFERENCE=REFERENCE_ROOT)

Like make_golden.py's sampler fixture, the reference's own source is read at generation time and executed; none of it is copied
here.  data/dataset_util.py is imported whole; ``data_crop`` / ``data_aug`` of data/dexycb.py and ``data_crop`` of data/ho3d.py are
cut out of their class by line search, dedented and exec'ed with a stand-in ``self``.  Harness stubs: ``cv2.Rodrigues`` through
scipy, ``libyana`` and ``pytorch3d`` as empty modules, ``torchvision.transforms.functional`` as the four PIL enhancers its PIL
backend calls.  The random numbers ``data_aug`` and ``color_jitter`` draw are scripted (a stand-in ``random`` / ``np.random``), so the
fixture can pin rotations, blur radii, factors and op orders; the same numbers are recorded as the inputs of the native path.
Frames are synthetic 160 x 120, inp_res 64, heat map 16: noise for g16 (a one-pixel warp difference shows), smooth for g17.
"""
import importlib.util
import os
import sys
import textwrap
import types

import numpy as np
from PIL import Image, ImageEnhance, ImageFilter

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("HOISDF_REFERENCE", "")          # a checkout of the reference code base
OUT = os.path.dirname(os.path.abspath(__file__))
W, H, RES, HM, B = 160, 120, 64, 16, 6


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def _rodrigues(x):
    from scipy.spatial.transform import Rotation
    x = np.asarray(x, np.float64)
    if x.shape == (3, 3):
        return Rotation.from_matrix(x).as_rotvec().reshape(3, 1), None
    return Rotation.from_rotvec(x.reshape(3)).as_matrix(), None


class Script:
    """stands in for ``random`` and ``np.random``: every draw pops the next scripted number"""

    def __init__(self):
        self.q = {}
        self.log = {}

    def load(self, **kw):
        self.q = {k: list(v) for k, v in kw.items()}

    def _pop(self, k):
        return self.q[k].pop(0)

    def uniform(self, *a, low=None, high=None, size=None):
        if size is not None:                                   # np.random.uniform(low=-1, high=1, size=2)
            return np.asarray(self._pop("center_u"), np.float64)
        lo, hi = a                                             # random.uniform(lo, hi) of get_color_params
        v = self._pop("factor")
        assert lo <= v <= hi, (lo, v, hi)
        return v

    def randn(self):
        return np.float64(self._pop("randn"))

    def random(self):
        return self._pop("random")

    def shuffle(self, lst):
        perm = self._pop("perm")
        assert sorted(perm) == list(range(len(lst))), (perm, len(lst))
        lst[:] = [lst[i] for i in perm]


class NumpyWith:
    def __init__(self, rnd):
        self.random = rnd

    def __getattr__(self, k):
        return getattr(np, k)


def load_reference():
    _stub("cv2", Rodrigues=_rodrigues, IMREAD_COLOR=1, IMREAD_IGNORE_ORIENTATION=128)
    _stub("libyana")
    _stub("libyana.meshutils", meshio=None)
    _stub("pytorch3d")
    _stub("pytorch3d.io", load_obj=None)
    F = _stub("torchvision.transforms.functional",
              adjust_brightness=lambda im, f: ImageEnhance.Brightness(im).enhance(f),
              adjust_contrast=lambda im, f: ImageEnhance.Contrast(im).enhance(f),
              adjust_saturation=lambda im, f: ImageEnhance.Color(im).enhance(f),
              adjust_hue=_adjust_hue)
    _stub("torchvision.transforms", functional=F)
    _stub("torchvision", transforms=sys.modules["torchvision.transforms"])
    spec = importlib.util.spec_from_file_location("ref_dataset_util", os.path.join(REF, "data", "dataset_util.py"))
    du = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(du)
    return du


def _adjust_hue(im, hue_factor):
    """torchvision's PIL backend: H of the HSV image += uint8(hue_factor * 255), modulo 256"""
    h, s, v = im.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over="ignore"):
        np_h += np.uint8(int(hue_factor * 255) & 255)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def method(path, name, ns):
    """the source of method ``name`` in ``path`` (from its def to the next def of the class), dedented and exec'ed in ``ns``"""
    src = open(path).read().split("\n")
    a = next(i for i, l in enumerate(src) if l.startswith("    def %s(" % name))
    b = next(i for i in range(a + 1, len(src)) if src[i].startswith("    def "))
    exec(textwrap.dedent("\n".join(src[a:b])), ns)
    return ns[name]


def labels(r, n, spread, centre):
    """21 hand joints (float32) and 21 projected object corners (float64) around ``centre``"""
    j = (centre + spread * r.uniform(-1, 1, (21, 2))).astype(np.float32)
    p = centre + np.array([0.6, 0.3]) * spread + 0.8 * spread * r.uniform(-1, 1, (21, 2))
    return j, p.astype(np.float64)


def noise_frame(r):
    return r.integers(0, 256, (H, W, 3), dtype=np.uint8)


def smooth_frame(r):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    ph = r.uniform(0, 6.28, (3, 3))
    ch = [127 + 70 * np.sin(x / 23.0 + ph[c, 0]) * np.cos(y / 17.0 + ph[c, 1]) + 45 * np.sin((x + y) / 31.0 + ph[c, 2]) for c in range(3)]
    return np.clip(np.stack(ch, -1) + r.normal(0, 2.0, (H, W, 3)), 0, 255).astype(np.uint8)


def masks(r, j, p):
    y, x = np.mgrid[0:H, 0:W]
    hand = ((x - j[:, 0].mean()) ** 2 + (y - j[:, 1].mean()) ** 2 < (0.6 * np.ptp(j[:, 0])) ** 2).astype(np.uint8)
    obj = ((np.abs(x - p[:, 0].mean()) < 0.5 * np.ptp(p[:, 0])) & (np.abs(y - p[:, 1].mean()) < 0.5 * np.ptp(p[:, 1]))).astype(np.uint8)
    return hand, obj


def reference_flip(du, frame, hand, obj, j, p, K):
    """data/dexycb.py:427-430, :462-465, :479-481, :501 on the 2D inputs (the corners: the mirrored projection)"""
    j, p, K = j.copy(), p.copy(), K.copy()
    j[:, 0] = np.array(W, dtype=np.float32) - j[:, 0] - 1
    p[:, 0] = W - p[:, 0] - 1
    K[0, 2] = W - K[0, 2] - 1
    return frame[:, ::-1, :].copy(), hand[:, ::-1].copy(), obj[:, ::-1].copy(), j, p, K


# centre / spread of the six samples: 0 right hand, 1 left hand, 2 leaves the frame top-left, 3 an integer scale (set below),
# 4 leaves bottom-right and is a left hand, 5 small
LAYOUT = [((80, 60), 14, 0), ((95, 55), 17, 1), ((12, 9), 15, 0), ((14, 40), 8, 0), ((150, 112), 16, 1), ((60, 40), 7, 0)]


def make_inputs(seed, frame_fn):
    r = np.random.default_rng(seed)
    S = []
    for i, (c, spread, flip) in enumerate(LAYOUT):
        j, p = labels(r, 21, spread, np.array(c, np.float64))
        if i == 3:                                             # hand box [14 - 18, 14 + 18] clamped to [0, 32]: crop scale 64 / 32 = 2
            j = np.clip(j, [3, 32], [25, 48]).astype(np.float32)
            p = np.clip(p, [6, 34], [22, 46])
            j[0], j[1] = (2.0, 36.0), (26.0, 44.0)
        K = np.array([[180.0 + 3 * i, 0, 81.3 + i], [0, 181.5 + 2 * i, 58.7 - i], [0, 0, 1]])
        frame = frame_fn(r)
        hand, obj = masks(r, j, p)
        S.append(dict(frame=frame, hand=hand, obj=obj, j=j, p=p, K=K, flip=flip))
    return r, S


def g16(du):
    ns = dict(dataset_util=du, np=np, Image=Image)
    data_crop = method(os.path.join(REF, "data", "dexycb.py"), "data_crop", ns)
    ho3d_crop = method(os.path.join(REF, "data", "ho3d.py"), "data_crop", dict(ns))
    me = types.SimpleNamespace(inp_res=RES, heatmap_res=HM)
    r, S = make_inputs(16, noise_frame)
    out = {k: [] for k in ("img", "bbox_hand", "bbox_obj", "K_out", "joints_uv_out", "p2d_out", "hand_seg", "obj_seg", "ho3d_img", "ho3d_K",
                           "ho3d_bbox_hand", "ho3d_bbox_obj", "ho3d_box_in")}
    for s in S:
        f, hm_, om_, j, p, K = (reference_flip(du, s["frame"], s["hand"], s["obj"], s["j"], s["p"], s["K"]) if s["flip"]
                                else (s["frame"], s["hand"], s["obj"], s["j"], s["p"], s["K"]))
        img, bh, bo, Ko, juv, p2, hs, os_ = data_crop(me, Image.fromarray(f), K, j, p, Image.fromarray(hm_), Image.fromarray(om_))
        for k, v in zip(("img", "bbox_hand", "bbox_obj", "K_out", "joints_uv_out", "p2d_out", "hand_seg", "obj_seg"),
                        (np.asarray(img), bh, bo, Ko, juv, p2, hs, os_)):
            out[k].append(np.asarray(v))
        box = np.array([s["j"][:, 0].min(), s["j"][:, 1].min(), s["j"][:, 0].max(), s["j"][:, 1].max()], np.float64)   # HO3D: the raw frame
        img, Ko, bh, bo = ho3d_crop(me, Image.fromarray(s["frame"]), s["K"], box, s["p"])
        for k, v in zip(("ho3d_img", "ho3d_K", "ho3d_bbox_hand", "ho3d_bbox_obj", "ho3d_box_in"), (np.asarray(img), Ko, bh, bo, box)):
            out[k].append(np.asarray(v))
    save("g16_image_crop", S, out)


def g17(du):
    rnd = Script()
    du.random = rnd
    ns = dict(dataset_util=du, np=NumpyWith(rnd), random=rnd, Image=Image, ImageFilter=ImageFilter, cv2=sys.modules["cv2"])
    data_aug = method(os.path.join(REF, "data", "dexycb.py"), "data_aug", ns)
    captured = {}
    real_affine, real_warp = du.get_affine_transform, du.transform_img
    du.get_affine_transform = lambda *a, **k: captured.setdefault("affine", real_affine(*a, **k))
    du.transform_img = lambda im, *a: captured.setdefault("warp", []).append(real_warp(im, *a)) or captured["warp"][-1]
    r, S = make_inputs(17, smooth_frame)
    #            randn (scale, [rot])   random (rot?, blur)   factors b, c, s, h (None: absent)      order of the present ones [b, s, h, c]
    plan = [dict(randn=[0.0], random=[0.9, 0.04], fac=(1.3, 0.7, 1.4, 0.08), perm=[0, 1, 2, 3]),          # no rotation, blur 0.02
            dict(randn=[0.6, 0.5], random=[0.3, 0.4], fac=(0.6, 1.35, 0.55, -0.12), perm=[3, 2, 1, 0]),   # +15 deg, blur 0.2, left hand
            dict(randn=[-0.8, -1.2], random=[0.1, 1.0], fac=(1.2, None, 1.25, None), perm=[1, 0]),        # -36 deg, blur 0.5, no contrast / hue
            dict(randn=[0.0], random=[0.7, 0.4], fac=(None, 1.45, None, 0.1), perm=[1, 0]),               # integer scale, no brightness / saturation
            dict(randn=[3.0, 2.5], random=[0.6, 1.0], fac=(0.85, 0.6, None, -0.05), perm=[2, 0, 1]),      # clipped jitter, +60 deg, left hand
            dict(randn=[-0.3], random=[0.61, 0.04], fac=(None, None, 0.7, None), perm=[0])]
    keys = ("img", "mano_param", "K_out", "hand_seg", "obj_seg", "p2d_out", "joints_uv_out", "bbox_hand", "bbox_obj", "sdf_points",
            "joints_3d", "p3d", "obj_rot", "obj_trans")
    out = {k: [] for k in keys + ("affine", "post_rot_trans", "rot_mat", "pil_crop", "center_u", "scale_jitter", "rot", "blur", "factors",
                                  "enabled", "order", "alone", "in_mano_param", "in_sdf_points", "in_joints_3d", "in_p3d", "in_obj_rot",
                                  "in_obj_trans")}
    for i, (s, pl) in enumerate(zip(S, plan)):
        f, hm_, om_, j, p, K = (reference_flip(du, s["frame"], s["hand"], s["obj"], s["j"], s["p"], s["K"]) if s["flip"]
                                else (s["frame"], s["hand"], s["obj"], s["j"], s["p"], s["K"]))
        cu = r.uniform(-1, 1, 2) if i != 3 else np.zeros(2)
        me = types.SimpleNamespace(inp_res=RES, heatmap_res=HM, center_jittering=0.1, scale_jittering=0.2, max_rot=np.pi, blur_radius=0.5,
                                   **{k: (0.5 if v is not None else 0) for k, v in zip(("brightness", "contrast", "saturation"), pl["fac"][:3])},
                                   hue=0.15 if pl["fac"][3] is not None else 0)
        rnd.load(center_u=[cu], randn=pl["randn"], random=pl["random"], factor=[v for v in pl["fac"] if v is not None], perm=[pl["perm"]])
        mano = np.concatenate([r.normal(0, 0.8, 3), r.normal(0, 0.2, 45), r.normal(0, 1, 10)]).astype(np.float32)
        sdf = r.normal(0, 0.1, (4, 5)).astype(np.float32)
        j3 = (r.normal(0, 0.05, (21, 3)) + [0.02, -0.03, 0.6]).astype(np.float32)
        p3 = r.normal(0, 0.06, (21, 3)) + [0.05, 0.01, 0.65]
        orot, otr = r.normal(0, 1.0, 3), np.array([0.05, 0.01, 0.65]) + r.normal(0, 0.01, 3)
        captured.clear()
        res = data_aug(me, Image.fromarray(f), mano, j, K, Image.fromarray(hm_), Image.fromarray(om_), p, sdf, j3, p3, orot, otr)
        assert not any(rnd.q.values()), rnd.q
        for k, v in zip(keys, res):
            out[k].append(np.asarray(v))
        for k, v in zip(("affine", "post_rot_trans", "rot_mat"), captured["affine"]):
            out[k].append(v)
        crop = captured["warp"][0].crop((0, 0, RES, RES))
        out["pil_crop"].append(np.asarray(crop))
        # the given numbers of the native path, formed as data_aug forms them
        sj = np.clip(0.2 * np.float64(pl["randn"][0]) + 1, 1 - 0.2, 1 + 0.2)
        rot = (np.clip(np.float64(pl["randn"][1]), -2.0, 2.0) * 30 if pl["random"][0] <= 0.6 else 0)
        rot = rot * np.pi / 180
        blur = pl["random"][1] * 0.5
        present = [o for o, v in zip((0, 2, 3, 1), (pl["fac"][0], pl["fac"][2], pl["fac"][3], pl["fac"][1])) if v is not None]   # list order b, s, h, c
        order = [present[k] for k in pl["perm"]]
        order += [o for o in range(4) if o not in order]
        fac = [1.25, 0.75, 1.3, 0.1]                            # "alone" factors of an absent op
        fac = [v if v is not None else d for v, d in zip(pl["fac"], fac)]
        F = sys.modules["torchvision.transforms.functional"]
        out["alone"].append(np.stack([np.asarray(F.adjust_brightness(crop, fac[0])), np.asarray(F.adjust_contrast(crop, fac[1])),
                                      np.asarray(F.adjust_saturation(crop, fac[2])), np.asarray(F.adjust_hue(crop, fac[3])),
                                      np.asarray(crop.filter(ImageFilter.GaussianBlur(blur)))]))
        for k, v in zip(("center_u", "scale_jitter", "rot", "blur", "factors", "enabled", "order"),
                        (cu, sj, rot, blur, fac, sum(1 << o for o in present), order)):
            out[k].append(np.asarray(v))
        for k, v in zip(("in_mano_param", "in_sdf_points", "in_joints_3d", "in_p3d", "in_obj_rot", "in_obj_trans"), (mano, sdf, j3, p3, orot, otr)):
            out[k].append(v)
    du.get_affine_transform, du.transform_img = real_affine, real_warp
    save("g17_image_aug", S, out)


def save(name, S, out):
    d = {"frame": np.stack([s["frame"] for s in S]), "hand_mask_bits": np.stack([np.packbits(s["hand"]) for s in S]),
         "obj_mask_bits": np.stack([np.packbits(s["obj"]) for s in S]), "joints_uv": np.stack([s["j"] for s in S]),
         "p2d": np.stack([s["p"] for s in S]), "K": np.stack([s["K"] for s in S]), "flip": np.array([s["flip"] for s in S], np.int32),
         "res": np.int32(RES), "hm": np.int32(HM)}
    d.update({"ref." + k: np.stack(v) for k, v in out.items()})
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print(name, os.path.getsize(path), "bytes;", {k: (v.dtype.str, v.shape) for k, v in d.items() if k.startswith("ref.")})


if __name__ == "__main__":
    if not os.path.isfile(os.path.join(REF, "data", "dataset_util.py")):
        raise SystemExit(__doc__)
    du = load_reference()
    g16(du)
    g17(du)
