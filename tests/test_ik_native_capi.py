"""CPU: the IK entry of the C ABI (include/hoisdf.h hoisdf_ik_mano_fwd, csrc/mano.hip) and the ik_solve switch of the whole-model
entry (hoisdf_pose_desc.ik_solve, hoisdf_pose_outputs.mano_pose_out / ik_valid_out) refuse malformed calls with HOISDF_ERR_INVALID
and a message before anything is launched (no GPU here: a launch would fail loudly), and the size query counts the MANO tables."""
import ctypes as C
import os

import pytest

from hoisdf_amd import _lib
from test_pose_infer_capi import _infer_args, desc

INVALID = -1
FAKE = C.c_void_p(0x100000)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_ik_mano_fwd_checks_its_arguments_before_any_launch(lib):
    assert "hoisdf_ik_mano_fwd" in _lib.SIGNATURES
    none = (None,) * 4
    assert lib.hoisdf_ik_mano_fwd(None, 21, None, 10, 4, *none, None, None, None, None, None) == INVALID
    assert b"null" in lib.hoisdf_last_error()
    # betas and valid_out are optional, everything else is required: each one missing alone is refused
    full = [FAKE, 21, None, 0, 4, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None]
    for i in (0, 5, 6, 7, 8, 9, 10, 11):
        args = list(full)
        args[i] = None
        assert lib.hoisdf_ik_mano_fwd(*args) == INVALID and b"null" in lib.hoisdf_last_error(), i
    assert lib.hoisdf_ik_mano_fwd(None, 21, None, 10, 0, *none, None, None, None, None, None) == 0          # zero hands: nothing to do
    assert lib.hoisdf_ik_mano_fwd(None, 20, None, 10, 0, *none, None, None, None, None, None) == 0
    full[1] = 19
    assert lib.hoisdf_ik_mano_fwd(*full) == INVALID and b"n_joints=19" in lib.hoisdf_last_error()
    full[1], full[2], full[3] = 21, FAKE, 9                                                               # a betas row shorter than 10
    assert lib.hoisdf_ik_mano_fwd(*full) == INVALID and b"ldbetas=9" in lib.hoisdf_last_error()
    full[4] = -1
    assert lib.hoisdf_ik_mano_fwd(*full) == INVALID


def test_ik_solve_is_appended_and_needs_the_ik_variant(lib):
    assert _lib.PoseDesc._fields_[-1][0] == "ik_solve"
    assert [n for n, _ in _lib.PoseOutputs._fields_[-2:]] == ["mano_pose_out", "ik_valid_out"]
    assert desc().ik_solve == 0                                                     # a caller that never heard of the field
    plain, solve = desc(use_inverse_kinematics=1), desc(use_inverse_kinematics=1, ik_solve=1)
    nb0, nb1 = lib.hoisdf_pose_prepared_bytes(C.addressof(plain)), lib.hoisdf_pose_prepared_bytes(C.addressof(solve))
    # the blob gains the transposed table image, the template, the regressor and the skinning weights
    assert nb1 >= nb0 + 4 * (lib.hoisdf_mano_dirs_image_floats() + 778 * 3 + 2 * 16 * 778)
    bad = desc(use_inverse_kinematics=0, ik_solve=1)
    assert lib.hoisdf_pose_prepared_bytes(C.addressof(bad)) == INVALID
    assert b"ik_solve" in lib.hoisdf_last_error()
    w = _lib.PoseWeights()
    assert lib.hoisdf_pose_prepare(C.addressof(bad), C.addressof(w), FAKE, 1 << 40, None) == INVALID
    assert b"ik_solve" in lib.hoisdf_last_error()


def test_pose_infer_with_ik_solve_wants_its_three_outputs(lib):
    d = desc(use_inverse_kinematics=1, ik_solve=1)
    base = ("hand_joints_out", "obj_rot_out", "obj_trans_out", "mano_shape_out")
    o = _lib.PoseOutputs(**{k: 0x100000 for k in base + ("mano_mesh_out", "mano_joints_out")})            # no mano_pose_out
    keep, args = _infer_args(d, o, 1 << 40)
    assert lib.hoisdf_pose_infer(*args) == INVALID
    assert b"null output" in lib.hoisdf_last_error() and b"mano_pose_out" in lib.hoisdf_last_error()
    for missing in ("mano_mesh_out", "mano_joints_out"):                          # (one message names all three: the status says it)
        names = base + tuple(n for n in ("mano_pose_out", "mano_mesh_out", "mano_joints_out") if n != missing)
        o = _lib.PoseOutputs(**{k: 0x100000 for k in names})
        keep, args = _infer_args(d, o, 1 << 40)
        assert lib.hoisdf_pose_infer(*args) == INVALID
    # without the switch the IK variant asks for none of them, as before (it gets past the outputs check to the fake pyramid's
    # channel count, which is not the descriptor's)
    off = desc(use_inverse_kinematics=1, C=3968)
    o = _lib.PoseOutputs(**{k: 0x100000 for k in base})
    keep, args = _infer_args(off, o, 1 << 40)
    assert lib.hoisdf_pose_infer(*args) == INVALID and b"pyramid" in lib.hoisdf_last_error()


def test_python_surface_is_opt_in(monkeypatch):
    from hoisdf_amd import ik, ops
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import Model
    monkeypatch.delenv("HOISDF_IK", raising=False)
    assert Config().native_ik is False and not ik.native_ik_enabled(Config())
    monkeypatch.setenv("HOISDF_IK", "native")
    assert ik.native_ik_enabled(Config())
    assert hasattr(ops, "ik_mano") and hasattr(ik, "ik_solver_mano_native") and hasattr(Model, "native_ik_enabled")


def test_the_ik_model_keeps_its_layer_out_of_the_state_dict():
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import get_model
    from hoisdf_amd.nets import mano as MANO
    c = Config()
    c.resnet_type = 18
    c.apply_setting("ho3d_render")
    layer = MANO.ManoLayer(MANO.synthetic_assets(0))
    model = get_model("test", cfg=c, mano_layer=layer, with_encoder=False)
    assert model.ik_mano_layer is layer
    assert not any("mano_layer" in k or k.startswith("th_") or ".th_" in k for k in model.state_dict())
    assert all(m is not layer for m in model.modules())
    assert not model.native_ik_enabled()                                            # the switch is off
    c.native_ik = True
    assert model.native_ik_enabled() and model._pose_desc(2, 992).ik_solve == 1
    c.apply_setting("dexycb")
    assert not get_model("test", cfg=c, mano_layer=layer, with_encoder=False).native_ik_enabled()   # not the IK variant
