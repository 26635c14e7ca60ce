"""CPU: the whole-model inference entries of the C ABI (include/hoisdf.h "whole-model inference", csrc/pose_infer.hip) are exported,
their size queries are pure host arithmetic, and malformed descriptors / buffers are refused with HOISDF_ERR_INVALID and a
message before anything is launched (no GPU here: a launch would fail loudly)."""
import ctypes as C
import os
import subprocess

import pytest

from hoisdf_amd import _lib

ENTRIES = ("hoisdf_pose_prepared_bytes", "hoisdf_pose_prepare", "hoisdf_pose_infer_begin", "hoisdf_pose_infer_workspace",
           "hoisdf_pose_infer")
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def desc(**kw):
    d = dict(B=2, num_samp_hand=384, num_samp_obj=128, bins_n=64, img_h=256, img_w=256, hand_sdf_scale=3.1, obj_sdf_scale=3.1,
             clamping_distance=0.15, hidden_dim=256, nheads=4, dim_feedforward=1024, enc_layers=6, dec_layers=4, C=992,
             use_inverse_kinematics=0, pre_norm=0, classifier_branch=0, attention=2)
    d.update(kw)
    return _lib.PoseDesc(**d)


def counts(d, n=5000):
    return (C.c_int32 * (2 * d.B))(*([n] * (2 * d.B)))


def test_the_five_entries_are_exported(lib):
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert f" T {name}\n" in syms, name
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES or name in _lib._OTHER


def test_size_queries_answer_without_a_device(lib):
    d = desc()
    nb = lib.hoisdf_pose_prepared_bytes(C.addressof(d))
    # at least one copy of the token MLP's first matrix and of the six hand encoder layers
    assert nb > 4 * (992 * 1024 + 6 * (4 * 256 * 256 + 2 * 256 * 1024))
    c = counts(d)
    ws = lib.hoisdf_pose_infer_workspace(C.addressof(d), C.addressof(c))
    assert ws > 4 * d.B * (d.num_samp_hand + d.num_samp_obj) * (992 + 2 * 256)          # the gathered rows and both token buffers
    big = counts(d, 20000)
    assert lib.hoisdf_pose_infer_workspace(C.addressof(d), C.addressof(big)) > ws        # sized by the survivor counts
    ik = desc(use_inverse_kinematics=1, C=3968)
    assert lib.hoisdf_pose_prepared_bytes(C.addressof(ik)) > nb                          # the wide pyramid's input matrices
    one = desc(B=1)
    assert 0 < lib.hoisdf_pose_infer_workspace(C.addressof(one), C.addressof(counts(one))) < ws


@pytest.mark.parametrize("bad,word", [(dict(nheads=8), b"heads of 64"), (dict(num_samp_hand=0), b"num_samp_hand=0"),
                                      (dict(hidden_dim=512, nheads=8), b"256"), (dict(pre_norm=1), b"pre_norm"),
                                      (dict(enc_layers=13), b"enc_layers"), (dict(attention=1), b"attention"), (dict(C=990), b"C=990")])
def test_bad_descriptors_are_refused_with_a_message(lib, bad, word):
    d = desc(**bad)
    assert lib.hoisdf_pose_prepared_bytes(C.addressof(d)) == -1
    assert word in lib.hoisdf_last_error()
    c = counts(d)
    assert lib.hoisdf_pose_infer_workspace(C.addressof(d), C.addressof(c)) == -1
    w = _lib.PoseWeights()
    fake = C.c_void_p(0x100000)
    assert lib.hoisdf_pose_prepare(C.addressof(d), C.addressof(w), fake, 1 << 40, None) == INVALID
    assert word in lib.hoisdf_last_error()
    assert lib.hoisdf_pose_infer_begin(C.addressof(d), fake, fake, fake, fake, fake, fake, C.addressof(c), None) == INVALID


def _infer_args(d, outputs, ws_bytes, c=None):
    """every pointer non-null and aligned, none of them real: a call that got past its argument checks would fault, so a clean
    INVALID shows that nothing was launched"""
    pyr = _lib.Pyramid()
    pyr.n_levels, pyr.B = 5, d.B
    for i, ch in enumerate((32, 64, 128, 256, 512)):
        pyr.data[i], pyr.C[i], pyr.H[i], pyr.W[i] = 0x100000, ch, 128 >> i, 128 >> i
    c = counts(d) if c is None else c
    fake = C.c_void_p(0x100000)
    keep = (pyr, c)
    return keep, (C.addressof(d), fake, C.byref(pyr), fake, fake, fake, fake, fake, fake, C.addressof(c),
                  None if outputs is None else C.addressof(outputs), fake, ws_bytes, None, None)


def test_null_outputs_and_a_short_workspace_are_refused_before_any_launch(lib):
    d = desc()
    c = counts(d)
    need = lib.hoisdf_pose_infer_workspace(C.addressof(d), C.addressof(c))
    full = _lib.PoseOutputs(**{k: 0x100000 for k in ("hand_joints_out", "obj_rot_out", "obj_trans_out", "mano_mesh_out", "mano_joints_out")})
    keep, args = _infer_args(d, None, need)
    assert lib.hoisdf_pose_infer(*args) == INVALID and b"null output" in lib.hoisdf_last_error()
    part = _lib.PoseOutputs(hand_joints_out=0x100000, obj_rot_out=0x100000, obj_trans_out=0x100000)         # no MANO outputs
    keep, args = _infer_args(d, part, need)
    assert lib.hoisdf_pose_infer(*args) == INVALID and b"null output" in lib.hoisdf_last_error()
    keep, args = _infer_args(d, full, need - 1)                                                              # one byte short
    assert lib.hoisdf_pose_infer(*args) == INVALID
    assert f"workspace of {need - 1} bytes, need {need}".encode() in lib.hoisdf_last_error()
    # the IK variant wants mano_shape_out instead
    ik = desc(use_inverse_kinematics=1)
    keep, args = _infer_args(ik, full, 1 << 40)
    assert lib.hoisdf_pose_infer(*args) == INVALID and b"mano_shape" in lib.hoisdf_last_error()
    # a pyramid that is not the descriptor's
    wide = desc(C=3968)
    keep, args = _infer_args(wide, full, 1 << 40)
    assert lib.hoisdf_pose_infer(*args) == INVALID and b"pyramid" in lib.hoisdf_last_error()


def test_a_short_sample_is_refused_on_the_host(lib):
    """fewer lattice survivors than requested points (the reference fails at main/model.py:348): HOISDF_ERR_TOO_FEW from the counts
    alone, before the workspace is even looked at"""
    d = desc()
    c = counts(d)
    c[d.B + 1] = d.num_samp_obj - 1
    full = _lib.PoseOutputs(**{k: 0x100000 for k in ("hand_joints_out", "obj_rot_out", "obj_trans_out", "mano_mesh_out", "mano_joints_out")})
    keep, args = _infer_args(d, full, 0, c)
    assert lib.hoisdf_pose_infer(*args) == -3
    assert b"sdf_infer(obj): sample 1 has only 127" in lib.hoisdf_last_error()


def test_python_surface_is_opt_in():
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import Model
    assert Config().native_infer is False
    assert hasattr(Model, "infer_native") and hasattr(Model, "native_infer_enabled")
