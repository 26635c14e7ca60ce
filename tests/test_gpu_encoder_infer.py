"""-m gpu: the image encoder in evaluation mode through ONE C-ABI call (include/hoisdf.h hoisdf_encoder_infer, Model.encode_native) next
to the torch modules of hoisdf_amd/nets/encoder.py (f32 on the GPU = the path Model.forward takes without the switch, float64 = the
truth), the prepared-blob cache, the switch, image to pose against the torch encoder, and a C host that takes an image to a pose.

Encoder weights everywhere here: kaiming_normal_ on every convolution and transposed convolution (tests/test_gpu_bnact.py: the
reference's std = 0.001 init makes every activation vanish), BatchNorm gamma in [0.5, 1.5], beta ~ N(0, 0.1), running mean ~ N(0, 0.5),
running variance in [0.5, 2], from a fixed seed."""
import copy
import os
import struct
import subprocess

import pytest
import torch

from hoisdf_amd import testing as T
from test_gpu_bnact import rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 1e-4
LEVELS = ("stride2", "stride4", "stride8", "stride16", "stride32")


def init_encoder(nets, seed):
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    with torch.no_grad():
        for net in nets:
            for m in net.modules():
                if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
                    torch.nn.init.kaiming_normal_(m.weight)
                    if m.bias is not None:
                        m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                elif isinstance(m, torch.nn.BatchNorm2d):
                    n = m.weight.shape[0]
                    m.weight.copy_(torch.rand(n, generator=g) + 0.5)
                    m.bias.copy_(0.1 * torch.randn(n, generator=g))
                    m.running_mean.copy_(0.5 * torch.randn(n, generator=g))
                    m.running_var.copy_(1.5 * torch.rand(n, generator=g) + 0.5)


def torch_encoder(bb, dec, img, dtype):
    """the existing modules in evaluation mode -> ([level maps NCHW in pyramid order], aux NCHW)"""
    bb, dec = copy.deepcopy(bb).to(dtype).eval(), copy.deepcopy(dec).to(dtype).eval()
    bb.to(memory_format=torch.channels_last); dec.to(memory_format=torch.channels_last)
    with torch.no_grad():
        feat, skips = bb(img.to(dtype).contiguous(memory_format=torch.channels_last))
        pyr, aux = dec(feat, skips)
    return [pyr[k] for k in LEVELS], aux


def nchw(level_nhwc):
    return level_nhwc.permute(0, 3, 1, 2)


def state(bb, dec):
    sd = {"backbone_net." + k: v for k, v in bb.state_dict().items()}
    sd.update({"decoder_net." + k: v for k, v in dec.state_dict().items()})
    return sd


@pytest.mark.parametrize("resnet,big", [(18, False), (50, False), (50, True)], ids=["r18-small", "r50-small", "r50-big"])
def test_whole_encoder_next_to_torch(resnet, big):
    """B = 2 on 64 x 96 (not square: an H / W swap cannot pass), levels 32 x 48 ... 2 x 3.  Per level and for the three aux maps:
    rel(native, truth) <= max(3 rel(torch f32, truth), 1e-4), the form tests/test_gpu_bnact.py holds the encoder to."""
    from hoisdf_amd import _lib, ops
    from hoisdf_amd.nets import encoder as E
    bb, dec = E.BackboneNet(resnet), E.DecoderNet(resnet, big=big)
    init_encoder((bb, dec), 11)
    bb, dec = bb.to(DEV).eval(), dec.to(DEV).eval()
    img = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(12)).to(DEV)
    f32, aux32 = torch_encoder(bb, dec, img, torch.float32)
    truth, aux64 = torch_encoder(bb, dec, img, torch.float64)
    for k, t in zip(LEVELS, truth):
        assert torch.isfinite(t).all() and float(t.std()) > 1e-3 * float(t.abs().max()) > 0, f"{k}: the truth is constant or not finite"
    desc = _lib.EncoderDesc(B=2, img_h=64, img_w=96, resnet_type=resnet, big_decoder=int(big))
    prepared = ops.EncoderPrepared(desc, state(bb, dec), img.device)
    pyr, aux = ops.encoder_infer(prepared, img)
    torch.cuda.synchronize()
    shapes = [tuple(t.shape) for t in truth]
    assert [tuple(nchw(l).shape) for l in pyr.levels] == shapes and shapes[0][2:] == (32, 48) and shapes[4][2:] == (2, 3)
    worst = []
    for k, got, a, t in list(zip(LEVELS, map(nchw, pyr.levels), f32, truth)) + [
            (f"aux{c}", nchw(aux)[:, c], aux32[:, c], aux64[:, c]) for c in range(3)]:
        rn, rt = rel(got, t), rel(a, t)
        print(f"resnet{resnet}{' big' if big else ''} {k}: rel(native, truth) {rn:.3e}  rel(torch f32, truth) {rt:.3e}  max |truth| {float(t.abs().max()):.3e}")
        if not rn <= max(3 * rt, 1e-4):
            worst.append((k, rn, rt))
    assert not worst, worst


def test_aux_is_optional_and_two_calls_are_bit_identical():
    from hoisdf_amd import _lib, ops
    from hoisdf_amd.nets import encoder as E
    bb, dec = E.BackboneNet(18), E.DecoderNet(18)
    init_encoder((bb, dec), 13)
    bb, dec = bb.to(DEV).eval(), dec.to(DEV).eval()
    img = torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(14)).to(DEV)       # B = 1: the deep layers cut K
    desc = _lib.EncoderDesc(B=1, img_h=64, img_w=96, resnet_type=18, big_decoder=0)
    prepared = ops.EncoderPrepared(desc, state(bb, dec), img.device)
    a, aux_a = ops.encoder_infer(prepared, img)
    b, aux_b = ops.encoder_infer(prepared, img.contiguous(memory_format=torch.channels_last))      # passed without a copy
    c, none = ops.encoder_infer(prepared, img, want_aux=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(aux_a, aux_b)
    for la, lb, lc in zip(a.levels, b.levels, c.levels):
        assert torch.equal(la, lb), "two calls on the same image differ"
        assert torch.equal(la, lc), "the pyramid depends on aux_out"


# ---- through the model: ResNet-18, 96 + 32 points, B = 2, 256 x 256 (the set-up of test_forward_with_the_switch_on_runs_the_native_entry)
NH, NO, B_ = 96, 32, 2
# The seed of the encoder's weights.  Top-K by |sdf| can flip on a 1e-6 perturbation, so the input has to be well-conditioned by the
# EXISTING code alone (test_the_input_is_well_conditioned): the torch-f32 pyramid, the float64 pyramid and the float64 pyramid under
# 1e-5 relative noise (ten times the rounding level of an f32 encoder) must select identical hand and object point sets.  The first
# seed tried, 21, does not (torch f32 and float64 already disagree in two points); 22, 23 and 24 do, and 23 also holds under 1e-4 noise.
ENCODER_SEED = 23


@pytest.fixture(scope="module")
def setup():
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import get_model
    from hoisdf_amd.nets import mano as MANO
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = NH, NO
    torch.manual_seed(0)
    model = get_model("train", cfg=c, mano_layer=MANO.ManoLayer(MANO.synthetic_assets(0)))
    init_encoder((model.backbone_net, model.decoder_net), ENCODER_SEED)
    model = model.to(DEV).eval()
    inputs, targets, meta = (T.to_device(x, DEV) for x in T.synthetic_batch(B_, NH, NO, seed=5))
    return model, c, inputs, targets, meta


def test_blob_cache_follows_the_encoder_weights(setup):
    from hoisdf_amd.model import _ENCODER_CACHE
    model, c, inputs, targets, meta = setup
    img = inputs["img"]
    first, _ = model.encode_native(img)
    ent = _ENCODER_CACHE[model]
    builds, ptr = ent["builds"], ent["prepared"].blob.data_ptr()
    for _ in range(2):
        model.encode_native(img)
    assert ent["builds"] == builds and ent["prepared"].blob.data_ptr() == ptr, "an unchanged model prepared again"
    bn = model.backbone_net.resnet.layer2[0].bn1
    saved = bn.running_mean.clone()
    with torch.no_grad():
        bn.running_mean.add_(0.25)                            # a buffer changed in place
    moved, _ = model.encode_native(img)
    model.encode_native(img)
    assert ent["builds"] == builds + 1, "a changed BatchNorm buffer must rebuild the blob exactly once"
    torch.cuda.synchronize()
    assert torch.equal(moved.levels[0].isfinite(), torch.ones_like(moved.levels[0], dtype=torch.bool))
    assert not torch.equal(moved.levels[4], first.levels[4]), "the pyramid did not follow the changed statistics"
    with torch.no_grad():
        bn.running_mean.copy_(saved)                          # (bit-exactly what it was: the tests below share this model)
    back, _ = model.encode_native(img)
    torch.cuda.synchronize()
    assert ent["builds"] == builds + 2 and all(torch.equal(x, y) for x, y in zip(back.levels, first.levels))


def test_forward_with_both_switches_is_encode_native_then_infer_native(setup):
    from hoisdf_amd.model import _ENCODER_CACHE
    model, c, inputs, targets, meta = setup
    try:
        c.native_infer, c.native_encoder = True, False
        _ENCODER_CACHE.pop(model, None)
        with torch.no_grad():
            off = model(inputs, targets, meta, "eval")
        assert model not in _ENCODER_CACHE, "with native_encoder off the encoder blob must never be created"
        c.native_encoder = True
        with torch.no_grad():
            out = model(inputs, targets, meta, "eval")
        pyr, aux = model.encode_native(inputs["img"])
        hand = model.infer_native(pyr, meta)
        torch.cuda.synchronize()
        assert _ENCODER_CACHE[model]["builds"] == 1
        for k, v in hand.items():
            assert torch.equal(out[k], v), k
        dec = aux.permute(0, 3, 1, 2)
        for k, ch in (("joint_heatmap_out", 0), ("hand_seg_pred_out", 1), ("obj_seg_pred_out", 2)):
            assert out[k].shape == off[k].shape and torch.equal(out[k], dec[:, ch]), k
        assert set(out) == set(off)
        assert not any("loss" in k for k in out)
    finally:
        c.native_infer = c.native_encoder = False


def point_sets(out):
    """per sample the selected hand and object points as sorted unique rows (the order inside a sample follows |sdf|)"""
    return [torch.unique(out[k][b], dim=0) for k in ("hand_points_out", "obj_points_out") for b in range(out[k].shape[0])]


def same_sets(a, b):
    return all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(point_sets(a), point_sets(b)))


@pytest.fixture(scope="module")
def three_runs(setup):
    """infer_native on the torch-f32 pyramid, on the float64 pyramid cast to f32, on the float64 pyramid under 1e-5 relative noise, and on
    the native encoder's pyramid"""
    from hoisdf_amd import ops
    model, c, inputs, targets, meta = setup
    img = inputs["img"]
    f32, _ = torch_encoder(model.backbone_net, model.decoder_net, img, torch.float32)
    f64, _ = torch_encoder(model.backbone_net, model.decoder_net, img, torch.float64)
    run = lambda maps: model.infer_native(ops.PyramidNHWC.from_nchw([m.float() for m in maps]), meta, debug=True)
    a, t = run(f32), run(f64)
    g = torch.Generator(device=DEV).manual_seed(1)
    noisy = run([m * (1 + 1e-5 * torch.randn(m.shape, device=DEV, dtype=m.dtype, generator=g)) for m in f64])
    pyr, _ = model.encode_native(img)
    n = model.infer_native(pyr, meta, debug=True)
    torch.cuda.synchronize()
    return a, t, n, noisy


def test_the_input_is_well_conditioned(three_runs):
    """the existing code alone: Top-K by |sdf| can flip on a 1e-6 perturbation and a flipped point moves the votes, so the comparison
    below is only meaningful on an input where the f32 and the float64 pyramid select the same points"""
    a, t, _, noisy = three_runs
    assert same_sets(a, t), "pick another ENCODER_SEED: torch f32 and float64 pyramids select different points"
    assert same_sets(noisy, t), "pick another ENCODER_SEED: 1e-5 relative noise on the float64 pyramid changes the selected points"


def test_image_to_pose_next_to_the_torch_encoder(three_runs):
    a, t, n, _ = three_runs
    dist = lambda x, y, k: float((x[k] - y[k]).abs().max())
    mean = lambda x, y, k: float((x[k].mean(1) - y[k].mean(1)).abs().max())
    for k in ("hand_joints_out", "mano_mesh_out", "mano_joints_out"):
        print(f"{k}: |native - f64| {dist(n, t, k):.3e}  |torch f32 - f64| {dist(a, t, k):.3e}  |native - torch f32| {dist(n, a, k):.3e}")
    for k in ("obj_rot_out", "obj_trans_out"):
        print(f"{k} (means): |native - f64| {mean(n, t, k):.3e}  |torch f32 - f64| {mean(a, t, k):.3e}  |native - torch f32| {mean(n, a, k):.3e}")
    assert same_sets(n, t), "the native encoder's pyramid selects other points than the float64 pyramid"
    for k in ("hand_joints_out", "mano_mesh_out", "mano_joints_out"):
        assert torch.isfinite(n[k]).all() and dist(n, t, k) <= BAR, (k, dist(n, t, k))
    for k in ("obj_rot_out", "obj_trans_out"):              # per-point rows follow the |sdf| order: compared as means
        assert mean(n, t, k) <= BAR, (k, mean(n, t, k))


def test_c_host_image_to_pose(setup, tmp_path):
    """A plain C host (no Python, no torch): encoder_prepare + pose_prepare, infer_begin, encoder_infer on the same stream, wait for the
    counts, pose_infer - on one flat file, against what the Python native path produced from the same file (1e-6 m)."""
    from hoisdf_amd import ops
    from hoisdf_amd.model import _ENCODER_CACHE
    from test_gpu_pose_infer import _flat_arrays
    model, c, inputs, targets, meta = setup
    pyr, _ = model.encode_native(inputs["img"])
    want = model.infer_native(pyr, meta)
    torch.cuda.synchronize()
    enc = _ENCODER_CACHE[model]["prepared"]
    sd = state(model.backbone_net, model.decoder_net)

    def arr(f, t):
        t = t.detach().float().cpu().contiguous().reshape(-1)
        f.write(struct.pack("<q", t.numel()))
        f.write(t.numpy().astype("<f4").tobytes())

    path = str(tmp_path / "image_to_pose.bin")
    with open(path, "wb") as f:
        f.write(bytes(enc.desc))
        f.write(bytes(model._pose_desc(B_, pyr.C)))
        for name, _ in ops.encoder_tensor_table(enc.desc):
            arr(f, sd[name])
        for t in _flat_arrays(model, c):
            arr(f, t)
        arr(f, inputs["img"].permute(0, 2, 3, 1))
        for k in ("mano_root", "obj_center_cam", "cam_intr", "bbox_hand", "bbox_obj"):
            arr(f, meta[k])
        for k in ("hand_joints_out", "obj_rot_out", "obj_trans_out", "mano_mesh_out", "mano_joints_out"):
            arr(f, want[k])
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_image_to_pose_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_image_to_pose_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "c host image to pose ok" in out.stdout, out.stdout + out.stderr
