"""-m gpu: the whole stage after the image encoder through ONE C-ABI call (include/hoisdf.h hoisdf_pose_infer, Model.infer_native)
against the reference's own eval outputs (tests/golden/g7_e2e_*, the fixtures and inputs of
test_gpu_model.py::test_eval_forward_matches_reference_goldens) at the north-star bars: 1e-4 m on joints / mesh, 1e-4 on the
per-point object outputs compared as means over the points."""
import ctypes as C
import os
import struct
import subprocess

import pytest
import torch

from conftest import load_golden
from hoisdf_amd import testing as T
from test_gpu_model import E2E, build, nhwc_pyramid, _needs_the_emulated_attention

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-4
SKIPPED_BY_NAME = ("mano_joints_gt_out", "mano_mesh_gt_out")        # ground-truth MANO outputs: not produced by the entry


def case_inputs(case):
    """model, pyramid and meta of one E2E case, exactly as test_eval_forward_matches_reference_goldens sets them up"""
    setting, big, nh, no, bins, b = case[:6]
    sfx = case[6] if len(case) > 6 else ""
    model, c = build(setting, nh, no, bins)
    if sfx == "_smallbeta":
        _needs_the_emulated_attention()
        with torch.no_grad():
            for k_, v_ in T.SMALL_BETA.items():
                getattr(model, k_).fill_(v_)
    pyr, _ = nhwc_pyramid(T.synthetic_pyramid(b, big=big, seed=2, outliers=100.0 if sfx == "_smallbeta" else 1.0))
    inputs, targets, meta = T.synthetic_batch(b, nh, no, seed=21)
    if bins == 16:
        meta["bbox_hand"] = torch.tensor([0.0, 0, 256, 256]).repeat(b, 1)
        meta["bbox_obj"] = torch.tensor([0.0, 0, 256, 256]).repeat(b, 1)
    inputs, targets, meta = (T.to_device(x, DEV) for x in (inputs, targets, meta))
    return model, c, pyr, inputs, targets, meta, load_golden(f"g7_e2e_{setting}_n{nh + no}{sfx}")


def check_against_fixture(out, g, label=""):
    """every *_out key of the fixture (but the ground-truth MANO ones) must be there and within the bar -> how many were compared"""
    n = 0
    for k, ref in g.items():
        if not (k.endswith("_out") or k.endswith("_out_mean")) or k in SKIPPED_BY_NAME:
            continue                                          # scalar losses (obj_rot / obj_trans / *_loss ...): not produced
        name = k[:-5] if k.endswith("_mean") else k
        assert name in out, f"missing output {name}"
        got = out[name].float().cpu()
        if k.endswith("_mean"):
            got = got.mean(1)
        elif name in ("obj_rot_out", "obj_trans_out"):      # per-point rows follow the |sdf| order: compare means
            got, ref = got.mean(1), ref.mean(1)
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        assert not torch.isnan(got).any(), k
        err = (got - ref).abs().max().item()
        print(f"{label}{name}: max abs err vs the reference {err:.3e}")
        assert err <= BAR, f"{name}: max abs err {err:.3e} > {BAR:.1e}"
        n += 1
    return n


@pytest.mark.parametrize("case", E2E, ids=lambda c: "-".join(str(x) for x in c))
def test_infer_native_matches_reference_goldens(case):
    model, c, pyr, inputs, targets, meta, g = case_inputs(case)
    out = model.infer_native(pyr, meta)
    torch.cuda.synchronize()
    want = {"hand_joints_out": (case[5], 20, 3), "obj_rot_out": (case[5], case[3], 3), "obj_trans_out": (case[5], case[3], 3)}
    for k, sh in want.items():
        assert tuple(out[k].shape) == sh, (k, out[k].shape)
    assert check_against_fixture(out, g) >= 4


def test_side_stream_and_repeat_are_bit_identical_and_prepare_runs_once():
    model, c, pyr, inputs, targets, meta, g = case_inputs(E2E[3])
    from hoisdf_amd.model import _POSE_CACHE
    a = model.infer_native(pyr, meta)                         # two streams (cfg.overlap_streams default)
    ent = _POSE_CACHE[model]
    builds, ptr = ent["builds"], ent["prepared"].blob.data_ptr()
    assert builds == 1 and ent["prepared"].version == 1
    b = model.infer_native(pyr, meta)                         # the same call again
    assert ent["builds"] == builds and ent["prepared"].blob.data_ptr() == ptr, "a second frame prepared the weights again"
    c.overlap_streams = False
    s = model.infer_native(pyr, meta)                         # everything on one stream
    assert ent["builds"] == builds and ent["prepared"].blob.data_ptr() == ptr
    torch.cuda.synchronize()
    assert set(a) == set(b) == set(s)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: two calls on the same inputs differ"
        assert torch.equal(a[k], s[k]), f"{k}: the result depends on the side stream"
    # a changed weight is seen: the blob is rebuilt where the SDF-query folds are
    model.invalidate_sdf_query_weights()
    model.infer_native(pyr, meta)
    assert ent["builds"] == builds + 1
    with torch.no_grad():
        model.linear_obj_rot.layers[2].bias.add_(1.0)
    moved = model.infer_native(pyr, meta)
    assert ent["builds"] == builds + 2
    torch.cuda.synchronize()
    assert torch.allclose(moved["obj_rot_out"], a["obj_rot_out"] + 1.0, atol=1e-5)
    assert torch.equal(moved["hand_joints_out"], a["hand_joints_out"])


@pytest.mark.parametrize("case", [E2E[0], E2E[3], E2E[5], E2E[7]], ids=lambda c: "-".join(str(x) for x in c))
def test_infer_native_next_to_the_python_path(case):
    """the same inputs through Model.hot_path(..., "eval"): the largest difference per output goes to the log (bit-identity is
    expected where both hosts pick the same kernels; the fused head kernel sums in another order than the Python path's GEMM
    launches, so it is reported, not asserted); both are held to the reference bars"""
    model, c, pyr, inputs, targets, meta, g = case_inputs(case)
    with torch.no_grad():
        _, py = model.hot_path(pyr, inputs, targets, meta, "eval")
    nat = model.infer_native(pyr, meta, debug=True)
    torch.cuda.synchronize()
    for k in sorted(nat):
        if k in py:
            assert nat[k].shape == py[k].shape, (k, nat[k].shape, py[k].shape)
            d = (nat[k] - py[k]).abs().max().item()
            print(f"{'-'.join(str(x) for x in case)} {k}: max |native - python| = {d:.3e}{' (bit-identical)' if torch.equal(nat[k], py[k]) else ''}")
    assert check_against_fixture(nat, g, "native ") >= 4
    assert check_against_fixture(py, g, "python ") >= 4
    # the debug outputs are the points sdf_infer selects
    pts, sdf, _, _ = model.sdf_infer(pyr, meta["mano_root"], meta["cam_intr"], meta["bbox_hand"], c.hand_sdf_scale, c.num_samp_hand, "hand")
    assert torch.equal(nat["hand_points_out"], pts) and torch.equal(nat["hand_sdf_out"], sdf.squeeze(-1))


def test_a_short_sample_is_refused_before_anything_is_launched():
    """the tiny-bbox case of test_sdf_infer_selects_the_oracle_set"""
    nh, no, bins, b = 384, 128, 64, 2
    model, c = build("dexycb", nh, no, bins)
    pyr, _ = nhwc_pyramid(T.synthetic_pyramid(b, seed=8))
    _, _, meta = T.synthetic_batch(b, nh, no, seed=81)
    m = T.to_device(meta, DEV)
    m["bbox_hand"] = torch.tensor([100.0, 100, 101, 101], device=DEV).repeat(b, 1)
    with pytest.raises(ValueError, match=r"sdf_infer\(hand\): sample 0 has only"):
        model.infer_native(pyr, m)
    # and the C entry itself, given those counts, answers HOISDF_ERR_TOO_FEW from the host-side check
    from hoisdf_amd import _lib, ops
    from hoisdf_amd.model import _POSE_CACHE
    prepared = _POSE_CACHE[model]["prepared"]
    counts = ops.PoseInferCounts(prepared.desc, m["mano_root"], m["obj_center_cam"], m["cam_intr"], m["bbox_hand"], m["bbox_obj"])
    cl = counts.wait()
    assert min(cl[:b]) < nh
    ch = (C.c_int32 * (2 * b))(*cl)
    o = _lib.PoseOutputs(**{k: 0x100000 for k in ("hand_joints_out", "obj_rot_out", "obj_trans_out", "mano_mesh_out", "mano_joints_out")})
    s = pyr.struct()
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = _lib.lib().hoisdf_pose_infer(C.addressof(prepared.desc), p(prepared.blob), C.byref(s), p(m["mano_root"]), p(m["obj_center_cam"]),
                                      p(m["cam_intr"]), p(m["bbox_hand"]), p(m["bbox_obj"]), p(counts.counts), C.addressof(ch), C.addressof(o),
                                      C.c_void_p(0x100000), 1 << 40, None, None)
    assert rc == -3 and b"fewer than num_points" in _lib.lib().hoisdf_last_error()
    torch.cuda.synchronize()                                 # nothing faulted: the fake buffers were never touched


def test_forward_with_the_switch_on_runs_the_native_entry():
    """Model.forward in eval mode with cfg.native_infer: encoder in PyTorch, then infer_native; dexycb keeps its ground-truth MANO
    outputs and the encoder-side maps; with the switch off nothing changes"""
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import _POSE_CACHE, get_model
    from hoisdf_amd.nets import mano as MANO
    nh, no, b = 96, 32, 2
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = nh, no
    model = get_model("train", cfg=c, mano_layer=MANO.ManoLayer(MANO.synthetic_assets(0))).to(DEV).eval()
    inputs, targets, meta = (T.to_device(x, DEV) for x in T.synthetic_batch(b, nh, no, seed=5))
    with torch.no_grad():
        ref = model(inputs, targets, meta, "eval")
    assert model not in _POSE_CACHE                          # off by default: the native entry was not touched
    c.native_infer = True
    with torch.no_grad():
        nat = model(inputs, targets, meta, "eval")
    torch.cuda.synchronize()
    assert model in _POSE_CACHE and _POSE_CACHE[model]["builds"] == 1
    for k in ("hand_joints_out", "mano_mesh_out", "mano_joints_out", "mano_joints_gt_out", "mano_mesh_gt_out", "obj_rot_out", "obj_trans_out",
              "joint_heatmap_out", "hand_seg_pred_out", "obj_seg_pred_out"):
        assert k in nat and nat[k].shape == ref[k].shape, k
    for k in ("hand_joints_out", "mano_mesh_out", "mano_joints_out"):
        err = (nat[k] - ref[k]).abs().max().item()
        print(f"forward native vs python {k}: {err:.3e}")
        assert err <= BAR, (k, err)
    assert torch.equal(nat["mano_joints_gt_out"], ref["mano_joints_gt_out"])
    assert not any("loss" in k for k in nat)


def _flat_arrays(model, c):
    """the weights in the order tests/c/test_pose_infer_host.c reads them"""
    a = []
    lin = lambda m: [t for l in m.layers for t in (l.weight, l.bias)]
    a += lin(model.linear_sdfin)
    for dec in (model.hand_sdf_decoder, model.obj_sdf_decoder):
        for i in range(4):
            l = getattr(dec, f"linh{i}")
            a += [l.weight_v, l.weight_g, l.bias]
        a += [dec.linh4.weight, dec.linh4.bias]
    a += lin(model.linear_transformerin)
    a += [model.hand_sigmoid_beta, model.obj_sigmoid_beta]
    for stack in (model.hand_transformer.encoder, model.obj_transformer.encoder):
        for l in stack.layers:
            s = l.self_attn
            a += [s.in_proj_weight, s.in_proj_bias, s.out_proj.weight, s.out_proj.bias, l.norm1.weight, l.norm1.bias, l.linear1.weight,
                  l.linear1.bias, l.linear2.weight, l.linear2.bias, l.norm2.weight, l.norm2.bias]
        a += [stack.inter_norm.weight, stack.inter_norm.bias]
    dec = model.hand_transformer.decoder
    for l in dec.layers:
        s, m = l.self_attn, l.multihead_attn
        a += [s.in_proj_weight, s.in_proj_bias, s.out_proj.weight, s.out_proj.bias, m.in_proj_weight, m.in_proj_bias, m.out_proj.weight,
              m.out_proj.bias, l.linear1.weight, l.linear1.bias, l.linear2.weight, l.linear2.bias, l.norm1.weight, l.norm1.bias,
              l.norm2.weight, l.norm2.bias, l.norm3.weight, l.norm3.bias]
    a += [dec.norm.weight, dec.norm.bias, model.mano_query_embed.weight]
    for m in (model.linear_pose, model.linear_shape, model.linear_handvote, model.linear_handcls, model.linear_obj_rot,
              model.linear_obj_rel_trans):
        a += lin(m)
    ml = model.mano_head.mano_layer
    a += [ml.th_shapedirs, ml.th_posedirs, ml.th_weights, ml.th_v_template, ml.th_J_regressor, ml.th_hands_mean]
    return a


def test_c_host_pose_infer(tmp_path):
    """A plain C host (no Python, no torch) runs prepare -> infer_begin -> wait for the counts -> infer on one flat binary file
    (descriptor, every weight, the pyramid, the camera inputs, the g7_e2e_dexycb_n512 outputs of the reference) and checks
    the outputs at 1e-4 - tests/c/test_pose_infer_host.c, the call sequence of INTEGRATION.md."""
    case = E2E[3]
    assert case[:4] == ("dexycb", False, 384, 128)
    model, c, pyr, inputs, targets, meta, g = case_inputs(case)
    b = case[5]
    desc = model._pose_desc(b, pyr.C)

    def arr(f, t):
        t = t.detach().float().cpu().contiguous().reshape(-1)
        f.write(struct.pack("<q", t.numel()))
        f.write(t.numpy().astype("<f4").tobytes())

    path = str(tmp_path / "pose_infer.bin")
    with open(path, "wb") as f:
        f.write(bytes(desc))
        for t in _flat_arrays(model, c):
            arr(f, t)
        f.write(struct.pack("<i", len(pyr.levels)))
        for lv in pyr.levels:
            f.write(struct.pack("<3i", lv.shape[3], lv.shape[1], lv.shape[2]))
            arr(f, lv)
        for k in ("mano_root", "obj_center_cam", "cam_intr", "bbox_hand", "bbox_obj"):
            arr(f, meta[k])
        arr(f, g["hand_joints_out"])
        arr(f, g["obj_rot_out"].mean(1))
        arr(f, g["obj_trans_out"].mean(1))
        arr(f, g["mano_mesh_out"])
        arr(f, g["mano_joints_out"])
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_pose_infer_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_pose_infer_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "c host pose infer ok" in out.stdout, out.stdout + out.stderr
