"""CPU: the image-encoder entries of the C ABI (include/hoisdf.h hoisdf_encoder_*, csrc/encoder_infer.hip).  The tensor table is the
checkpoint's: every floating-point backbone_net.* / decoder_net.* key of the REAL reference's state dict
(tests/golden/g10_state_dict_schema.json), in order, and encoder.py's own for the depths the schema does not hold.  Size queries are
pure host arithmetic, and every malformed call is refused with HOISDF_ERR_INVALID and a message before anything is launched (no GPU
here: a launch would fail loudly)."""
import ctypes as C
import json
import math
import os

import pytest

from hoisdf_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCHEMA = json.load(open(os.path.join(GOLDEN, "g10_state_dict_schema.json")))
INVALID = -1
ENC = ("backbone_net.", "decoder_net.")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def desc(**kw):
    d = dict(B=2, img_h=256, img_w=256, resnet_type=50, big_decoder=0)
    d.update(kw)
    return _lib.EncoderDesc(**d)


def table(lib, d):
    n = lib.hoisdf_encoder_tensor_count(C.addressof(d))
    assert n > 0, lib.hoisdf_last_error()
    return [(lib.hoisdf_encoder_tensor_name(C.addressof(d), i).decode(), lib.hoisdf_encoder_tensor_numel(C.addressof(d), i)) for i in range(n)]


@pytest.mark.parametrize("variant,rt,big", [("dexycb_resnet50", 50, 0), ("ho3d_resnet50", 50, 1), ("ho3d_render_resnet50", 50, 0),
                                            ("dexycb_resnet18", 18, 0)])
def test_tensor_table_is_the_released_checkpoints(lib, variant, rt, big):
    want = [(k, math.prod(shape)) for k, shape in SCHEMA[variant].items() if k.startswith(ENC) and not k.endswith("num_batches_tracked")]
    assert len(want) > 100
    assert table(lib, desc(resnet_type=rt, big_decoder=big)) == want


@pytest.mark.parametrize("rt,big", [(34, 0), (101, 0), (101, 1), (152, 0), (152, 1)])
def test_tensor_table_is_the_modules_state_dict(lib, rt, big):
    from hoisdf_amd.nets.encoder import BackboneNet, DecoderNet
    want = []
    for prefix, net in (("backbone_net.", BackboneNet(rt)), ("decoder_net.", DecoderNet(rt, big=bool(big)))):
        want += [(prefix + k, v.numel()) for k, v in net.state_dict().items() if v.is_floating_point()]
    assert table(lib, desc(resnet_type=rt, big_decoder=big)) == want


def test_size_queries_answer_without_a_device(lib):
    d = desc()
    nb = lib.hoisdf_encoder_prepared_bytes(C.addressof(d))
    assert nb >= 4 * sum(n for _, n in table(lib, d) if _.endswith("weight") and ".bn" not in _) // 2
    ws = lib.hoisdf_encoder_infer_workspace(C.addressof(d))
    assert ws > 4 * d.B * 128 * 128 * 64                                        # at least the stem's map
    assert 0 < lib.hoisdf_encoder_infer_workspace(C.addressof(desc(B=1))) < ws
    assert lib.hoisdf_encoder_prepared_bytes(C.addressof(desc(big_decoder=1))) > nb
    assert lib.hoisdf_encoder_launch_count(C.addressof(d)) > 60
    assert lib.hoisdf_conv_packed_floats(64, 3, 7, 7) == 147 * 64 and lib.hoisdf_conv_packed_floats(1, 32, 1, 1) == 32 * 4
    assert lib.hoisdf_conv_workspace_bytes(6, 512, 2048, 1) > 0 and lib.hoisdf_conv_workspace_bytes(1 << 18, 64, 576, 1) == 0
    tile, splitk = C.c_int(0), C.c_int(0)
    assert lib.hoisdf_conv_plan(6, 512, 2048, 1, C.addressof(tile), C.addressof(splitk)) == 0 and splitk.value > 1 and tile.value == 64
    assert lib.hoisdf_conv_plan(1 << 18, 256, 64, 1, C.addressof(tile), C.addressof(splitk)) == 0 and splitk.value == 1 and tile.value == 128


@pytest.mark.parametrize("rt,big,chans", [(50, 0, (32, 64, 128, 256, 512)), (18, 0, (32, 64, 128, 256, 512)),
                                          (50, 1, (128, 256, 512, 1024, 2048))])
def test_pyramid_shape(lib, rt, big, chans):
    d = desc(resnet_type=rt, big_decoder=big)
    p = _lib.Pyramid()
    assert lib.hoisdf_encoder_pyramid_shape(C.addressof(d), C.byref(p)) == 0
    assert p.n_levels == 5 and p.B == d.B
    assert tuple(p.C[i] for i in range(5)) == chans
    assert [p.H[i] for i in range(5)] == [128, 64, 32, 16, 8] and [p.W[i] for i in range(5)] == [128, 64, 32, 16, 8]
    d = desc(img_h=64, img_w=96)
    assert lib.hoisdf_encoder_pyramid_shape(C.addressof(d), C.byref(p)) == 0
    assert [(p.H[i], p.W[i]) for i in range(5)] == [(32, 48), (16, 24), (8, 12), (4, 6), (2, 3)]


@pytest.mark.parametrize("bad,word", [(dict(resnet_type=20), b"resnet_type=20"), (dict(resnet_type=18, big_decoder=1), b"big_decoder"),
                                      (dict(resnet_type=34, big_decoder=1), b"big_decoder"), (dict(img_h=250), b"multiples of 32"),
                                      (dict(img_w=100), b"multiples of 32"), (dict(B=0), b"B=0")])
def test_bad_descriptors_are_refused_with_a_message(lib, bad, word):
    d = desc(**bad)
    fake = C.c_void_p(0x100000)
    levels = (C.c_void_p * 5)(*([0x100000] * 5))
    assert lib.hoisdf_encoder_infer_workspace(C.addressof(d)) == -1 and word in lib.hoisdf_last_error()
    assert lib.hoisdf_encoder_infer(C.addressof(d), fake, fake, levels, None, fake, 1 << 40, None) == INVALID
    assert word in lib.hoisdf_last_error()
    p = _lib.Pyramid()
    assert lib.hoisdf_encoder_pyramid_shape(C.addressof(d), C.byref(p)) == INVALID
    if "resnet_type" in bad:                                  # the architecture itself is wrong: no table, no blob either
        assert lib.hoisdf_encoder_tensor_count(C.addressof(d)) == -1
        assert lib.hoisdf_encoder_prepared_bytes(C.addressof(d)) == -1
        assert lib.hoisdf_encoder_prepare(C.addressof(d), levels, 5, fake, 1 << 40, None) == INVALID


def test_null_pointers_short_buffers_and_a_wrong_count_are_refused_before_any_launch(lib):
    """every pointer non-null and aligned, none of them real: a call that got past its checks would fault"""
    d = desc()
    da = C.addressof(d)
    fake = C.c_void_p(0x100000)
    n = lib.hoisdf_encoder_tensor_count(da)
    tensors = (C.c_void_p * n)(*([0x100000] * n))
    nb, ws = lib.hoisdf_encoder_prepared_bytes(da), lib.hoisdf_encoder_infer_workspace(da)
    assert lib.hoisdf_encoder_prepare(da, tensors, n - 1, fake, nb, None) == INVALID
    assert f"{n - 1} tensors, the table has {n}".encode() in lib.hoisdf_last_error()
    assert lib.hoisdf_encoder_prepare(da, tensors, n, fake, nb - 1, None) == INVALID                  # a byte short
    assert f"blob of {nb - 1} bytes, need {nb}".encode() in lib.hoisdf_last_error()
    assert lib.hoisdf_encoder_prepare(da, None, n, fake, nb, None) == INVALID and b"null" in lib.hoisdf_last_error()
    assert lib.hoisdf_encoder_prepare(da, tensors, n, None, nb, None) == INVALID and b"null" in lib.hoisdf_last_error()
    tensors[7] = None
    assert lib.hoisdf_encoder_prepare(da, tensors, n, fake, nb, None) == INVALID
    assert b"tensor 7 (backbone_net.resnet.layer1.0.bn1.bias)" in lib.hoisdf_last_error()
    levels = (C.c_void_p * 5)(*([0x100000] * 5))
    assert lib.hoisdf_encoder_infer(da, fake, fake, levels, None, fake, ws - 1, None) == INVALID      # a byte short
    assert f"workspace of {ws - 1} bytes, need {ws}".encode() in lib.hoisdf_last_error()
    for args in ((None, fake, levels, fake), (fake, None, levels, fake), (fake, fake, None, fake), (fake, fake, levels, None)):
        assert lib.hoisdf_encoder_infer(da, args[0], args[1], args[2], None, args[3], ws, None) == INVALID
        assert b"null" in lib.hoisdf_last_error()
    levels[3] = None
    assert lib.hoisdf_encoder_infer(da, fake, fake, levels, None, fake, ws, None) == INVALID and b"level 3" in lib.hoisdf_last_error()
    assert lib.hoisdf_encoder_infer(None, fake, fake, levels, None, fake, ws, None) == INVALID
    assert lib.hoisdf_encoder_tensor_name(da, n) is None and lib.hoisdf_encoder_tensor_numel(da, -1) == -1


def test_conv_unit_entries_validate_before_any_launch(lib):
    fake = C.c_void_p(0x100000)
    ok = dict(x=fake, ldx=64, w=fake, bias=fake, res=None, ldr=0, y=fake, ldy=64, c_off=0, B=2, H=9, W=7, Ci=64, Co=64, KH=3, KW=3, s=1, p=1, act=1)

    def conv(**kw):
        a = dict(ok, **kw)
        return lib.hoisdf_conv2d_fwd(a["x"], a["ldx"], a["w"], a["bias"], a["res"], a["ldr"], a["y"], a["ldy"], a["c_off"], a["B"], a["H"], a["W"],
                                     a["Ci"], a["Co"], a["KH"], a["KW"], a["s"], a["p"], a["act"], None, 0, None)
    assert conv(x=None) == INVALID and b"null" in lib.hoisdf_last_error()
    assert conv(ldx=32) == INVALID and b"strides" in lib.hoisdf_last_error()
    assert conv(c_off=8) == INVALID and b"strides" in lib.hoisdf_last_error()
    assert conv(act=3) == INVALID and b"act=3" in lib.hoisdf_last_error()
    assert conv(s=0) == INVALID and conv(Co=0) == INVALID
    assert conv(res=fake, ldr=32) == INVALID
    assert lib.hoisdf_conv_transpose2d_fwd(fake, 16, fake, fake, fake, 8, 0, 2, 3, 2, 32, 16, 0, None, 0, None) == INVALID      # ldx < C_in
    assert lib.hoisdf_maxpool2d_fwd(None, 64, fake, 64, 2, 9, 7, 64, None) == INVALID
    assert lib.hoisdf_conv_pack_weight(fake, None, fake, None, None, None, 1e-5, 8, 8, 3, 3, 0, fake, fake, None) == INVALID    # half a BatchNorm
    assert lib.hoisdf_conv_pack_weight(fake, None, None, None, None, None, 0.0, 8, 8, 3, 3, 1, fake, fake, None) == INVALID     # transposed is 4x4
    assert lib.hoisdf_conv_workspace_bytes(0, 8, 8, 1) == -1


def test_python_surface_is_opt_in():
    from hoisdf_amd import ops
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import Model
    assert Config().native_encoder is False
    assert hasattr(Model, "encode_native") and hasattr(Model, "native_encoder_enabled")
    assert hasattr(ops, "EncoderPrepared") and hasattr(ops, "encoder_infer")
