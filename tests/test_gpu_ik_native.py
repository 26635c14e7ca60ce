"""-m gpu: the IK variant's closed-form post-process as ONE HIP launch (csrc/mano.hip ik_mano_fwd_kernel; hoisdf_ik_mano_fwd,
ops.ik_mano, ik.ik_solver_mano_native, and hoisdf_pose_infer with ik_solve = 1) against
  - g12_ik.npz = the REFERENCE's own ik_solver_mano on seeded joints, with the assertions and bars of tests/test_ik.py::_check_golden;
  - the torch restatement hoisdf_amd/ik.py (the yardstick) on the shapes the kernel can get wrong: one hand and more hands than fit
    one dispatch wave, a padded betas row, both joint layouts, a wrist away from the origin, mirrored (reflected) hands;
  - the algorithm's own guarantee (MANO(pose from IK) reproduces the joints MANO produced).
The 2e-5 bars are the project's own (tests/test_ik.py): the torch restatement holds them in fp32 on the same device."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from conftest import load_golden
from hoisdf_amd import ops
from hoisdf_amd.ik import PALM, ik_solver_mano, ik_solver_mano_native
from hoisdf_amd.nets import mano as MANO

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 2e-5
SEED, HANDS = 0, 33


@pytest.fixture(scope="module")
def layer():
    return MANO.ManoLayer(MANO.synthetic_assets(0)).to(DEV)


def _rot(pose):
    return MANO.axis_angle_to_matrix(pose.cpu().reshape(-1, 3))


def check_solution(out, ref, label):
    """the assertions of tests/test_ik.py::_check_golden, each figure printed before it is held to its bar; ref: a dict with the
    reference's vis / pose / joints / verts (verts optional)"""
    vis = torch.as_tensor(ref["vis"]).reshape(-1).bool().cpu()
    assert torch.equal(out["vis"].reshape(-1).bool().cpu(), vis), f"{label}: valid flags differ"
    pose, rpose = out["pose"].cpu(), torch.as_tensor(ref["pose"]).cpu()
    figs = {"pose as rotations": (_rot(pose) - _rot(rpose)).abs().max().item(),
            "pose as vectors (valid hands)": (pose - rpose)[vis].abs().max().item() if bool(vis.any()) else 0.0,
            "joints [m]": (out["joints"].cpu() - torch.as_tensor(ref["joints"]).cpu()).abs().max().item()}
    if "verts" in ref:
        figs["verts [m]"] = (out["verts"].cpu() - torch.as_tensor(ref["verts"]).cpu()).abs().max().item()
    for k, v in figs.items():
        print(f"{label}: {k}: max abs err {v:.3e}")
    for k, v in figs.items():
        assert v < BAR, f"{label}: {k}: {v:.3e} >= {BAR:.0e}"
    if not bool(vis.all()):
        assert pose[~vis].abs().max().item() == 0.0, f"{label}: a reflected hand left the zero pose"      # reference :66-71


def test_reference_fixture(layer):
    g = load_golden("g12_ik")
    out = ik_solver_mano_native(layer, g["betas"].to(DEV), g["joints_in"].to(DEV))
    vis = torch.from_numpy(g["vis"]).reshape(-1).bool()
    assert int(vis.sum()) >= 4 and not bool(vis.all())                    # proper fits and reflections both present
    assert out["verts"].shape == (8, 778, 3) and out["joints"].shape == (8, 21, 3) and out["pose"].shape == (8, 48)
    assert out["vis"].shape == (8, 1) and out["vis"].dtype == torch.int64 and torch.equal(out["shape"].cpu(), g["betas"])
    check_solution(out, g, "g12_ik")
    out0 = ik_solver_mano_native(layer, None, g["joints_in"].to(DEV))
    err = (out0["joints"].cpu() - g["joints_noshape"]).abs().max().item()
    print(f"g12_ik betas=None: joints: max abs err {err:.3e}")
    assert err < BAR
    assert (_rot(out0["pose"]) - _rot(g["pose_noshape"])).abs().max().item() < BAR
    assert torch.equal(out0["shape"].cpu(), torch.zeros(8, 10))


# ---- against the torch solver ---------------------------------------------------------------------------------------------------
def make_hands(n, seed):
    """MANO joints of random poses and shapes + 1e-3 noise, a third of the hands mirrored in x (a left hand: the palm fit is a
    reflection) -> wrist-centred joints (n,21,3), betas (n,10), wrist translations (n,1,3); CPU, seeded"""
    g = torch.Generator().manual_seed(seed)
    cpu = MANO.ManoLayer(MANO.synthetic_assets(0))
    pose = torch.randn(n, 48, generator=g) * 0.25
    betas = torch.randn(n, 10, generator=g) * 0.5
    with torch.no_grad():
        joints = cpu(pose, betas)[1] / 1000.0 + 1e-3 * torch.randn(n, 21, 3, generator=g)
    joints[2::3, :, 0] *= -1.0
    joints = joints - joints[:, :1]
    return joints, betas, 0.3 * torch.randn(n, 1, 3, generator=g)


def palm_fit_conditioning(joints, betas):
    """H = T0 P0^T of every hand in fp64 on the CPU -> (sigma3 / sigma1, | |det R| - 1 |) per hand"""
    cpu = MANO.ManoLayer(MANO.synthetic_assets(0)).double()
    with torch.no_grad():
        tpl = cpu(torch.zeros(len(joints), 48, dtype=torch.float64), betas.double())[1] / 1000.0
    tgt = joints.double()
    T0 = (tpl[:, PALM] - tpl[:, :1]).transpose(1, 2)
    P0 = (tgt[:, PALM] - tgt[:, :1]).transpose(1, 2)
    U, S, Vt = torch.linalg.svd(T0 @ P0.transpose(1, 2))
    R = Vt.transpose(1, 2) @ U.transpose(1, 2)
    return S[:, 2] / S[:, 0], (torch.linalg.det(R).abs() - 1).abs()


@pytest.fixture(scope="module")
def hands(layer):
    """the inputs of make_hands and the torch solver's answer on them (computed once): wrist-centred and translated"""
    joints, betas, root = make_hands(HANDS, SEED)
    ratio, det_err = palm_fit_conditioning(joints, betas)
    print(f"palm fits: sigma3/sigma1 in [{ratio.min().item():.3e}, {ratio.max().item():.3e}], | |det R| - 1 | <= {det_err.max().item():.1e}")
    assert bool((ratio > 1e-3).all()) and bool((det_err < 1e-6).all())              # every hand: none is left out of the comparison
    j, b, r = joints.to(DEV), betas.to(DEV), root.to(DEV)
    ref_c = ik_solver_mano(layer, b, j)
    ref_t = ik_solver_mano(layer, b, j + r)
    mirrored = torch.zeros(HANDS, dtype=torch.bool)
    mirrored[2::3] = True
    assert torch.equal(ref_c["vis"].reshape(-1).bool().cpu(), ~mirrored)             # the mirrored third is what the guard catches
    return {"joints": j, "betas": b, "root": r, "ref_centred": ref_c, "ref_translated": ref_t}


@pytest.mark.parametrize("n", [1, HANDS])
def test_both_joint_layouts_against_the_torch_solver(layer, hands, n):
    j, r = hands["joints"][:n], hands["root"][:n]
    wide = torch.zeros(n, 12, device=DEV)                                            # betas with a row stride of 12
    wide[:, :10] = hands["betas"][:n]
    wide[:, 10:] = 1e9                                                               # (the pad must never be read)
    betas = wide[:, :10]
    assert betas.stride() == (12, 1)
    cut = lambda ref: {k: v[:n] for k, v in ref.items()}
    assets = layer.kernel_assets()

    def solve(x):
        pose, verts, joints, valid = ops.ik_mano(x, betas, assets)
        return {"pose": pose, "verts": verts, "joints": joints, "vis": valid}

    o21 = solve(j)                                                                   # wrist-centred, 21 rows
    o20 = solve(j[:, 1:])                                                            # the layout of hand_joints_out
    o21t = solve(j + r)                                                              # wrist away from the origin
    torch.cuda.synchronize()
    check_solution(o21, cut(hands["ref_centred"]), f"{n} hands, 21 joints")
    check_solution(o20, cut(hands["ref_centred"]), f"{n} hands, 20 joints")
    check_solution(o21t, cut(hands["ref_translated"]), f"{n} hands, 21 joints translated")
    for k in o21:
        assert torch.equal(o20[k], o21[k]), f"{k}: the 20-joint form differs from the 21-joint form on wrist-centred input"
    # the translation moves the outputs, not the solution's validity
    assert torch.equal(o21t["vis"], o21["vis"])


def test_ik_reproduces_mano_joints(layer):
    """tests/test_ik.py::test_ik_reproduces_mano_joints through the kernel"""
    torch.manual_seed(0)
    cpu = MANO.ManoLayer(MANO.synthetic_assets(0))
    B = 6
    pose = torch.randn(B, 48) * 0.25
    betas = torch.randn(B, 10) * 0.5
    joints = cpu(pose, betas)[1] / 1000.0 + torch.randn(B, 1, 3) * 0.3               # arbitrary root translation
    out = ik_solver_mano_native(layer, betas.to(DEV), joints.to(DEV))
    assert out["verts"].shape == (B, 778, 3) and out["pose"].shape == (B, 48) and out["vis"].shape == (B, 1)
    assert bool(out["vis"].all())
    bones = [i for i in range(21) if i not in (4, 8, 12, 16, 20)]                     # (the tips are skinned vertices: test_ik.py)
    err = (out["joints"].cpu() - joints)[:, bones].norm(dim=-1).max().item()
    print(f"MANO(IK(joints)) - joints: {err:.3e} m")
    assert err < 5e-5, err
    rerr = (MANO.axis_angle_to_matrix(pose[:, :3]) - MANO.axis_angle_to_matrix(out["pose"][:, :3].cpu())).abs().max().item()
    print(f"wrist rotation: {rerr:.3e}")
    assert rerr < 1e-4


def test_two_calls_are_bit_identical(layer, hands):
    a = ops.ik_mano(hands["joints"] + hands["root"], hands["betas"], layer.kernel_assets())
    b = ops.ik_mano(hands["joints"] + hands["root"], hands["betas"], layer.kernel_assets())
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_whole_model_with_ik_solve():
    """hoisdf_pose_infer with ik_solve = 1 (Model.infer_native with cfg.native_ik): the solve is the call's last launch, on that
    call's own hand_joints_out / mano_shape_out; everything written before it is bit-identical to a call without it"""
    from hoisdf_amd.model import _POSE_CACHE
    from test_gpu_pose_infer import case_inputs
    model, c, pyr, inputs, targets, meta, g = case_inputs(("ho3d_render", False, 48, 16, 16, 2))
    assert model.ik_mano_layer is not None and not model.native_ik_enabled()
    off = model.infer_native(pyr, meta)
    assert not any(k.startswith("ik_") for k in off)
    c.native_ik = True
    on = model.infer_native(pyr, meta)
    builds = _POSE_CACHE[model]["builds"]
    on2 = model.infer_native(pyr, meta)                                              # a second frame
    assert _POSE_CACHE[model]["builds"] == builds == 2, "the blob is built once per setting of the switch"
    torch.cuda.synchronize()
    for k in ("hand_joints_out", "obj_rot_out", "obj_trans_out", "mano_shape_out"):
        assert torch.equal(on[k], off[k]), f"{k} depends on ik_solve"
    for k in on:
        assert torch.equal(on[k], on2[k]), k
    assert on["ik_pose_out"].shape == (2, 48) and on["ik_joints_out"].shape == (2, 21, 3) and on["ik_verts_out"].shape == (2, 778, 3)
    layer = model.ik_mano_layer
    assert next(layer.buffers()).is_cuda
    hj = torch.cat([torch.zeros_like(on["hand_joints_out"][:, :1]), on["hand_joints_out"]], 1)
    ref = ik_solver_mano(layer, on["mano_shape_out"], hj)
    ratio, det_err = palm_fit_conditioning(hj.cpu(), on["mano_shape_out"].cpu())
    print(f"whole model: palm fits sigma3/sigma1 {ratio.tolist()}, | |det R| - 1 | {det_err.tolist()}, vis {ref['vis'].reshape(-1).tolist()}")
    assert bool(ref["vis"].any()), "both palm fits are reflections: the pose comparison below would be 0 == 0"
    got = {"pose": on["ik_pose_out"], "joints": on["ik_joints_out"], "verts": on["ik_verts_out"], "vis": on["ik_valid_out"]}
    check_solution(got, ref, "whole model")
    # and the same outputs through the Python surface the tester uses
    sep = ik_solver_mano_native(layer, on["mano_shape_out"], on["hand_joints_out"])
    for a, b in (("pose", "ik_pose_out"), ("joints", "ik_joints_out"), ("verts", "ik_verts_out")):
        assert torch.equal(sep[a], on[b]), a


def test_tester_predict_with_the_switch():
    """engine.Tester.predict on the IK variant (image encoder included): off = the torch solver as before; cfg.native_ik = the
    kernel on that forward's own hand_joints_out / mano_shape_out; with cfg.native_infer as well the solve comes out of
    hoisdf_pose_infer itself.  Each native result is the bits of ik_solver_mano_native on the same call's outputs."""
    from hoisdf_amd import testing as T
    from hoisdf_amd.config import Config
    from hoisdf_amd.engine import Tester
    from hoisdf_amd.model import _POSE_CACHE
    nh, no, b = 96, 32, 2
    c = Config()
    c.resnet_type = 18
    c.apply_setting("ho3d_render")
    c.num_samp_hand, c.num_samp_obj = nh, no
    tester = Tester(c, torch.device("cuda", 0))
    ml = MANO.ManoLayer(MANO.synthetic_assets(0))                                    # on the CPU: predict moves it
    inputs, targets, meta = T.synthetic_batch(b, nh, no, seed=5)
    off = tester.predict(inputs, targets, meta, mano_layer=ml)
    assert tester.model.ik_mano_layer is not ml                                      # off: the model was not touched
    hj = torch.cat([torch.zeros_like(off["hand_joints_out"][:, :1]), off["hand_joints_out"]], 1)
    ref = ik_solver_mano(ml, off["mano_shape_out"], hj)
    assert torch.equal(off["ik_pose_out"], ref["pose"]) and torch.equal(off["ik_verts_out"], ref["verts"])
    c.native_ik = True
    on = tester.predict(inputs, targets, meta, mano_layer=ml)
    assert tester.model.ik_mano_layer is ml and tester.model not in _POSE_CACHE      # the Python hot path ran, then the kernel
    # (two forwards through the image encoder are not bit-reproducible outside deterministic mode: each solve is compared with
    # the solver on ITS call's outputs)
    sep = ik_solver_mano_native(ml, on["mano_shape_out"], on["hand_joints_out"])
    for a, k in (("pose", "ik_pose_out"), ("joints", "ik_joints_out"), ("verts", "ik_verts_out")):
        assert on[k].shape == off[k].shape and torch.equal(on[k], sep[a]), k
    c.native_infer = True
    nat = tester.predict(inputs, targets, meta, mano_layer=ml)
    torch.cuda.synchronize()
    assert _POSE_CACHE[tester.model]["prepared"].desc.ik_solve == 1 and "ik_valid_out" in nat
    sep = ik_solver_mano_native(ml, nat["mano_shape_out"], nat["hand_joints_out"])
    for a, k in (("pose", "ik_pose_out"), ("joints", "ik_joints_out"), ("verts", "ik_verts_out")):
        assert nat[k].shape == off[k].shape and torch.equal(nat[k], sep[a]), k
    assert torch.equal(nat["ik_valid_out"].long(), sep["vis"].reshape(-1))


def test_c_host_ik(layer, hands, tmp_path):
    """A plain C host (tests/c/test_ik_host.c: hoisdf_mano_prepare + hoisdf_ik_mano_fwd on dumped joints, betas and assets) gets
    the bits the Python call gets"""
    n, ld = 5, 12
    joints = (hands["joints"] + hands["root"])[:n].contiguous()
    wide = torch.zeros(n, ld, device=DEV)
    wide[:, :10] = hands["betas"][:n]
    pose, verts, out_joints, valid = ops.ik_mano(joints, wide[:, :10], layer.kernel_assets())
    torch.cuda.synchronize()

    def arr(f, t):
        t = t.detach().float().cpu().contiguous().reshape(-1)
        f.write(struct.pack("<q", t.numel()))
        f.write(t.numpy().astype("<f4").tobytes())

    src, dst = str(tmp_path / "ik_in.bin"), str(tmp_path / "ik_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<3i", n, 21, ld))
        for t in (joints, wide, layer.th_shapedirs, layer.th_posedirs, layer.th_weights, layer.th_v_template, layer.th_J_regressor):
            arr(f, t)
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_ik_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_ik_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "c host ik ok" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(dst, dtype="<f4", count=n * (48 + 63 + 2334))
    c_valid = np.fromfile(dst, dtype="<i4", offset=4 * n * (48 + 63 + 2334))
    c_pose, c_joints, c_verts = np.split(raw, [n * 48, n * (48 + 63)])
    assert np.array_equal(c_pose.view(np.uint32), pose.cpu().numpy().reshape(-1).view(np.uint32))
    assert np.array_equal(c_joints.view(np.uint32), out_joints.cpu().numpy().reshape(-1).view(np.uint32))
    assert np.array_equal(c_verts.view(np.uint32), verts.cpu().numpy().reshape(-1).view(np.uint32))
    assert np.array_equal(c_valid, valid.cpu().numpy())
