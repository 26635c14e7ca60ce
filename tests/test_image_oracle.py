"""CPU: the image pipeline's definition (hoisdf_amd/image_oracle.py) and the host entries of the C ABI (hoisdf_crop_params_dexycb /
_ho3d, hoisdf_aug_params_dexycb; csrc/imgprep_params.c) against what the reference's data_crop / data_aug produced with PIL
(tests/golden/g16_image_crop.npz, g17_image_aug.npz; generator tests/golden/make_golden_image.py).

Bars: parameters and labels 1e-5 absolute (float32 values of magnitude <= 1e3 computed in float64 with the reference's own casts
reproduced); the warp at most 0.5 % differing pixels per image, each the frame's value at one of the 8 neighbours of the
restatement's source pixel (PIL evaluates the same rule in 16.16 fixed point / an accumulated double); brightness, contrast and
saturation never more than one level from PIL and at most 0.5 % of the values differing."""
import os

import numpy as np
import pytest

from hoisdf_amd import image_oracle as IO

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5


@pytest.fixture(scope="module")
def g16():
    return dict(np.load(os.path.join(GOLD, "g16_image_crop.npz")))


@pytest.fixture(scope="module")
def g17():
    return dict(np.load(os.path.join(GOLD, "g17_image_aug.npz")))


@pytest.fixture(scope="module")
def capi():
    from hoisdf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    from hoisdf_amd import image_data
    return image_data


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max() if a.size else 0.0
    assert err <= TOL, (what, err)


def eval_params(g, i, impl):
    W, H = g["frame"].shape[2], g["frame"].shape[1]
    return impl(g["joints_uv"][i], g["p2d"][i], g["K"][i], W, H, bool(g["flip"][i]), int(g["res"]), int(g["hm"]))


def train_params(g, i, impl):
    W, H = g["frame"].shape[2], g["frame"].shape[1]
    return impl(g["joints_uv"][i], g["p2d"][i], g["K"][i], W, H, bool(g["flip"][i]), int(g["res"]), int(g["hm"]),
                g["ref.center_u"][i], float(g["ref.scale_jitter"][i]), float(g["ref.rot"][i]))


def impls(capi):
    o_eval = lambda *a: IO.crop_params_dexycb(*a)
    c_eval = lambda *a: capi.crop_to_dict(capi.crop_params(*a))
    o_ho3d = lambda *a: IO.crop_params_ho3d(*a)
    c_ho3d = lambda *a: capi.crop_to_dict(capi.crop_params_ho3d(*a))
    o_aug = lambda j, p, K, W, H, fl, res, hm, cu, sj, rot: IO.aug_params_dexycb(j, p, K, W, H, fl, res, hm, 0.1, cu, sj, rot)
    c_aug = lambda *a: capi.crop_to_dict(capi.aug_params(*a))
    return {"numpy": (o_eval, o_ho3d, o_aug), "C": (c_eval, c_ho3d, c_aug)}


@pytest.mark.parametrize("which", ["numpy", "C"])
def test_evaluation_crop_parameters_match_the_reference(g16, capi, which):
    ev, ho, _ = impls(capi)[which]
    for i in range(len(g16["frame"])):
        p = eval_params(g16, i, ev)
        close(p["K"], g16["ref.K_out"][i], f"K' {i}")
        close(p["bbox_hand"], g16["ref.bbox_hand"][i], f"bbox_hand {i}")
        close(p["bbox_obj"], g16["ref.bbox_obj"][i], f"bbox_obj {i}")
        close(p["joints_uv"].astype(np.float32), g16["ref.joints_uv_out"][i].astype(np.float32), f"joint_coord {i}")
        close(p["p2d"], g16["ref.p2d_out"][i], f"p2d {i}")
        W, H = g16["frame"].shape[2], g16["frame"].shape[1]
        q = ho(g16["ref.ho3d_box_in"][i], g16["p2d"][i], g16["K"][i], W, H, int(g16["res"]), int(g16["hm"]))
        close(q["K"], g16["ref.ho3d_K"][i], f"ho3d K' {i}")
        close(q["bbox_hand"], g16["ref.ho3d_bbox_hand"][i], f"ho3d bbox_hand {i}")
        close(q["bbox_obj"], g16["ref.ho3d_bbox_obj"][i], f"ho3d bbox_obj {i}")


@pytest.mark.parametrize("which", ["numpy", "C"])
def test_training_crop_parameters_match_the_reference(g17, capi, which):
    _, _, aug = impls(capi)[which]
    for i in range(len(g17["frame"])):
        p = train_params(g17, i, aug)
        for k in ("affine", "post_rot_trans", "rot_mat", "bbox_hand", "bbox_obj"):
            close(p[k], g17["ref." + k][i], f"{k} {i}")
        close(p["K"], g17["ref.K_out"][i], f"K' {i}")
        close(p["joints_uv"], g17["ref.joints_uv_out"][i], f"joint_coord {i}")
        close(p["p2d"], g17["ref.p2d_out"][i], f"p2d {i}")


def test_c_and_numpy_parameters_are_the_same_numbers(g16, g17, capi):
    """the inverse the kernel reads is the restatement's, bit for bit"""
    im = impls(capi)
    for i in range(len(g16["frame"])):
        a, b = eval_params(g16, i, im["numpy"][0]), eval_params(g16, i, im["C"][0])
        c, d = train_params(g17, i, im["numpy"][2]), train_params(g17, i, im["C"][2])
        for x, y in ((a, b), (c, d)):
            assert np.array_equal(x["affine"], y["affine"]) and np.array_equal(x["inverse"], y["inverse"]), i


def test_host_entries_refuse_malformed_calls(g16, capi):
    """null pointers, point counts outside 1 .. 32, sizes <= 0, an empty box: HOISDF_ERR_INVALID with a message, nothing written"""
    import ctypes as C
    from hoisdf_amd import _lib
    lib = _lib.lib()
    j = np.ascontiguousarray(g16["joints_uv"][0], np.float32)
    p, K = np.ascontiguousarray(g16["p2d"][0]), np.ascontiguousarray(g16["K"][0].reshape(9))
    out = _lib.Crop()
    out.K[0] = 42.0
    ok = dict(j=j.ctypes.data, nj=21, p=p.ctypes.data, nc=21, K=K.ctypes.data, W=160, H=120, res=64, hm=16, out=C.addressof(out))
    call = lambda **kw: (lambda a: lib.hoisdf_crop_params_dexycb(a["j"], a["nj"], a["p"], a["nc"], a["K"], a["W"], a["H"], 0, a["res"], a["hm"], a["out"]))({**ok, **kw})
    for kw in (dict(j=None), dict(p=None), dict(K=None), dict(out=None), dict(nj=0), dict(nj=33), dict(nc=0), dict(nc=33), dict(W=0), dict(H=-1),
               dict(res=0), dict(hm=0)):
        assert call(**kw) == -1 and len(lib.hoisdf_last_error()) > 0, kw
    same = np.ascontiguousarray(np.tile(j[:1], (21, 1))), np.ascontiguousarray(np.tile(j[:1].astype(np.float64), (21, 1)))
    assert call(j=same[0].ctypes.data, p=same[1].ctypes.data) == -1 and b"box" in lib.hoisdf_last_error()
    assert out.K[0] == 42.0
    cu = np.zeros(2)
    assert lib.hoisdf_aug_params_dexycb(j.ctypes.data, 21, p.ctypes.data, 21, K.ctypes.data, 160, 120, 0, 64, 16, 0.1, cu.ctypes.data, 0.0, 0.0,
                                        C.addressof(out)) == -1
    assert lib.hoisdf_aug_params_dexycb(j.ctypes.data, 21, p.ctypes.data, 21, K.ctypes.data, 160, 120, 0, 64, 16, 0.1, None, 1.0, 0.0,
                                        C.addressof(out)) == -1
    assert lib.hoisdf_crop_params_ho3d(None, p.ctypes.data, 21, K.ctypes.data, 160, 120, 64, 16, C.addressof(out)) == -1
    assert call() == 0 and out.K[0] != 42.0


def test_rotated_3d_labels_match_the_reference(g17):
    for i in range(len(g17["frame"])):
        r = IO.rotate_labels(g17["ref.rot_mat"][i], g17["ref.in_joints_3d"][i], g17["ref.in_p3d"][i], g17["ref.in_mano_param"][i][:3],
                             g17["ref.in_obj_rot"][i], g17["ref.in_obj_trans"][i])
        close(r["joints_3d"], g17["ref.joints_3d"][i], "joints_3d")
        close(r["p3d"], g17["ref.p3d"][i], "p3d")
        close(r["obj_trans"], g17["ref.obj_trans"][i], "obj_trans")
        close(IO.rodrigues(r["obj_rot"]), IO.rodrigues(g17["ref.obj_rot"][i]), "obj_rot as a matrix")
        close(IO.rodrigues(r["mano_root"]), IO.rodrigues(g17["ref.mano_param"][i][:3]), "mano_param[:3] as a matrix")
        close(g17["ref.sdf_points"][i][:, :3], g17["ref.in_sdf_points"][i][:, :3].astype(np.float64) @ g17["ref.rot_mat"][i].T.astype(np.float64),
              "sdf points")


def check_warp(mine, pil, frame, inverse, n, step, what):
    """<= 0.5 % differing pixels; each one is the (flipped) frame's value at a neighbour of the restatement's source, 0 outside"""
    mine, pil = mine.reshape(n, n, -1), pil.reshape(n, n, -1)
    diff = (mine != pil).any(-1)
    share = diff.mean()
    print(f"{what}: {diff.sum()} of {diff.size} pixels differ ({100 * share:.3f} %)")
    assert share <= 0.005, (what, share)
    sx, sy = IO.source_pixels(inverse, n, step)
    H, W = frame.shape[:2]
    fr = frame.reshape(H, W, -1)
    for y, x in zip(*np.nonzero(diff)):
        cands = []
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                u, v = int(sx[y, x]) + dx, int(sy[y, x]) + dy
                cands.append(fr[v, u] if 0 <= u < W and 0 <= v < H else np.zeros(fr.shape[-1], fr.dtype))
        assert any(np.array_equal(pil[y, x], c) for c in cands), (what, y, x)


def test_warp_restatement_against_pil_on_noise_frames(g16):
    res, hm = int(g16["res"]), int(g16["hm"])
    H, W = g16["frame"].shape[1:3]
    for i in range(len(g16["frame"])):
        flip = bool(g16["flip"][i])
        inv = eval_params(g16, i, IO.crop_params_dexycb)["inverse"]
        frame = g16["frame"][i]
        seen = frame[:, ::-1] if flip else frame
        check_warp(IO.warp(frame, inv, res, flip), g16["ref.img"][i], seen, inv, res, 1.0, f"crop {i}")
        for name in ("hand", "obj"):
            m = IO.unpack_mask(g16[name + "_mask_bits"][i], H, W)
            mine = IO.warp_mask(m, inv, res, hm, flip)
            diff = mine != g16["ref." + name + "_seg"][i]
            print(f"{name}_seg {i}: {diff.sum()} of {diff.size} differ")
            check_warp(mine.astype(np.uint8), g16["ref." + name + "_seg"][i], m[:, ::-1] if flip else m, inv, hm, res / hm, f"{name}_seg {i}")
    zero = IO.warp(g16["frame"][2], eval_params(g16, 2, IO.crop_params_dexycb)["inverse"], res) == 0
    assert zero.all(-1).mean() > 0.05, "sample 2 must leave the frame"


def check_blend(mine, pil, what):
    d = np.abs(mine.astype(np.int32) - pil.astype(np.int32))
    print(f"{what}: max {d.max()} level, {100 * (d > 0).mean():.3f} % differ")
    assert d.max() <= 1, (what, d.max())
    assert (d > 0).mean() <= 0.005, (what, (d > 0).mean())


def test_brightness_contrast_saturation_alone_against_pil(g17):
    for i in range(len(g17["frame"])):
        crop, f = g17["ref.pil_crop"][i], g17["ref.factors"][i]
        check_blend(IO.brightness(crop, f[0]), g17["ref.alone"][i][0], f"brightness {i}")
        check_blend(IO.contrast(crop, f[1]), g17["ref.alone"][i][1], f"contrast {i}")
        check_blend(IO.saturation(crop, f[2]), g17["ref.alone"][i][2], f"saturation {i}")


def test_hue_alone_is_pils_conversion(g17):
    """the integer RGB <-> HSV restatement reproduces PIL: the recorded hue outputs are equal, not close"""
    for i in range(len(g17["frame"])):
        assert np.array_equal(IO.hue(g17["ref.pil_crop"][i], g17["ref.factors"][i][3]), g17["ref.alone"][i][3]), i


def test_full_size_against_pil_directly():
    """the same checks at 256 x 256 from a 480 x 640 frame, PIL called here"""
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance
    r = np.random.default_rng(164)
    frame = r.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    j = (np.array([300.0, 250.0]) + 60 * r.uniform(-1, 1, (21, 2))).astype(np.float32)
    p = np.array([330.0, 260.0]) + 50 * r.uniform(-1, 1, (21, 2))
    K = np.array([[615.0, 0, 312.0], [0, 615.0, 241.0], [0, 0, 1]])
    for rot in (0.0, 0.4, -0.9):
        pr = IO.aug_params_dexycb(j, p, K, 640, 480, False, 256, 64, 0.1, r.uniform(-1, 1, 2), 1.07, rot)
        t = pr["inverse"]
        pil = Image.fromarray(frame).transform((256, 256), Image.AFFINE, tuple(float(v) for v in t.reshape(6)))
        check_warp(IO.warp(frame, t, 256), np.asarray(pil), frame, t, 256, 1.0, f"rot {rot}")
    y, x = np.mgrid[0:256, 0:256]
    smooth = np.clip(np.stack([128 + 90 * np.sin(x / 31.0), 128 + 80 * np.cos(y / 23.0), 100 + 0.5 * x], -1) + r.normal(0, 3, (256, 256, 3)),
                     0, 255).astype(np.uint8)
    im = Image.fromarray(smooth)
    for f in (0.55, 1.0, 1.45):
        check_blend(IO.brightness(smooth, f), np.asarray(ImageEnhance.Brightness(im).enhance(f)), f"brightness {f}")
        check_blend(IO.contrast(smooth, f), np.asarray(ImageEnhance.Contrast(im).enhance(f)), f"contrast {f}")
        check_blend(IO.saturation(smooth, f), np.asarray(ImageEnhance.Color(im).enhance(f)), f"saturation {f}")
    assert np.array_equal(IO.rgb_to_hsv(smooth), np.asarray(im.convert("HSV")))
    assert np.array_equal(IO.hsv_to_rgb(smooth), np.asarray(Image.fromarray(smooth, "HSV").convert("RGB")))
