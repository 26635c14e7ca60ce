"""CPU: the interaction-loss entries of the C ABI (include/hoisdf.h hoisdf_interaction_loss_fwd / _bwd, csrc/interact_loss.hip)
refuse malformed calls with HOISDF_ERR_INVALID and a message that names the argument before anything is launched (no GPU here: a
launch would fail loudly), return 0 for an empty batch, their workspace query is arithmetic, and the Python surface is opt-in."""
import ctypes as C
import inspect
import os

import pytest

from hoisdf_amd import _lib

INVALID = -1
FAKE = C.c_void_p(0x100000)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _mesh(**kw):
    d = dict(verts=0x100000, faces=0x100000, n_faces=None, face_batch_stride=0, V=778, max_faces=1538)
    d.update(kw)
    return _lib.Mesh(**d)


def test_the_entries_and_their_tile_are_declared_and_exported(lib):
    fwd, bwd = _lib.SIGNATURES["hoisdf_interaction_loss_fwd"], _lib.SIGNATURES["hoisdf_interaction_loss_bwd"]
    assert len(fwd) == 17 and len(bwd) == 19 and fwd[:11] == bwd[:11] and fwd[10] is C.c_float and fwd[-1] is C.c_void_p
    assert _lib._OTHER["hoisdf_interaction_loss_workspace_bytes"] == ([C.c_int] * 5, C.c_long)
    assert _lib.CONSTANTS["INTERACT_LOSS_TILE"] == 64
    for name in ("hoisdf_interaction_loss_fwd", "hoisdf_interaction_loss_bwd", "hoisdf_interaction_loss_workspace_bytes"):
        assert hasattr(lib, name), name


def test_the_workspace_query_is_arithmetic(lib):
    q = lib.hoisdf_interaction_loss_workspace_bytes
    B, Vh, Fh, Vo, Fo = 4, 778, 1538, 1000, 2000
    need = q(B, Vh, Fh, Vo, Fo)
    # both prepared meshes, per query point of both directions sdf + face + three weights, four doubles per sample
    least = B * (Fh + Fo) * (48 + 4 + 4) + 2 * B * 32 + B * (Vh + Vo) * 20 + B * 32
    assert least <= need <= least + 20 * 256 and need % 256 == 0
    assert need >= lib.hoisdf_mesh_sdf_rows_workspace_bytes(B, Fh, Fo)
    assert q(2 * B, Vh, Fh, Vo, Fo) > need and q(B, Vh, Fh, Vo, Fo) == need
    assert q(0, 0, 0, 0, 0) == 0
    assert q(B, Vh, 4097, Vo, Fo) == INVALID and b"4097" in lib.hoisdf_last_error()
    assert q(B, Vh, Fh, Vo, 5000) == INVALID and b"5000" in lib.hoisdf_last_error()
    assert q(-1, Vh, Fh, Vo, Fo) == INVALID and q(65536, Vh, Fh, Vo, Fo) == INVALID and q(B, -1, Fh, Vo, Fo) == INVALID


@pytest.mark.parametrize("entry", ["fwd", "bwd"])
def test_both_entries_check_their_arguments_before_any_launch(lib, entry):
    hand, obj = _mesh(), _mesh(V=1000, max_faces=2000, face_batch_stride=6000)
    need = lib.hoisdf_interaction_loss_workspace_bytes(4, 778, 1538, 1000, 2000)
    outs = ("rep_hand", "att", "rep_obj") if entry == "fwd" else ("d_hand_verts", "d_obj_verts")

    def call(h=hand, o=obj, nv=None, B=4, wr=None, sr=0, wa=None, sa=0, wo=None, so=0, alpha=0.01, ws=FAKE, nws=need, **out):
        head = (None if h is None else C.addressof(h), None if o is None else C.addressof(o), nv, B, wr, sr, wa, sa, wo, so, alpha)
        ptrs = [out.get(k, FAKE) for k in outs]
        if entry == "fwd":
            return lib.hoisdf_interaction_loss_fwd(*head, *ptrs, ws, nws, None)
        return lib.hoisdf_interaction_loss_bwd(*head, None, None, None, *ptrs, ws, nws, None)

    for kw, what in ((dict(h=None), b"hand"), (dict(o=None), b"obj"), (dict(ws=None), b"workspace"), (dict(h=_mesh(verts=None)), b"verts"),
                     (dict(o=_mesh(V=1000, max_faces=2000, faces=None)), b"faces")) + tuple((dict([(k, None)]), k.encode()) for k in outs):
        assert call(**kw) == INVALID and b"null" in lib.hoisdf_last_error() and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    inf, nan = float("inf"), float("nan")
    for kw, what in ((dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"), (dict(h=_mesh(max_faces=4097)), b"max_faces=4097"),
                     (dict(o=_mesh(max_faces=5000)), b"max_faces=5000"), (dict(h=_mesh(V=0)), b"without vertices"),
                     (dict(o=_mesh(max_faces=2000, face_batch_stride=5999)), b"face_batch_stride=5999"),
                     (dict(wr=FAKE, sr=777), b"rep_w_hand_stride=777"), (dict(wa=FAKE, sa=-1), b"att_w_hand_stride=-1"),
                     (dict(wo=FAKE, so=778), b"rep_w_obj_stride=778"),
                     (dict(alpha=0.0), b"alpha=0"), (dict(alpha=-0.01), b"alpha=-0.01"), (dict(alpha=inf), b"alpha=inf"), (dict(alpha=nan), b"alpha="),
                     (dict(nws=need - 1), b"workspace"), (dict(nws=0), b"workspace")):
        assert call(**kw) == INVALID and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
        assert f"interaction_loss_{entry}".encode() in lib.hoisdf_last_error()
    # B = 0: nothing to do, whatever the pointers
    assert call(B=0, ws=None, nws=0, **{k: None for k in outs}) == 0
    assert call(B=0, wr=FAKE, sr=778, wo=FAKE, so=1000, ws=None, nws=0) == 0


def test_python_surface_is_opt_in(monkeypatch):
    from hoisdf_amd import engine, interaction_loss_oracle, ops
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import get_model
    monkeypatch.delenv("HOISDF_INTERACTION_LOSS", raising=False)
    c = Config()
    assert c.interaction_loss is False and c.interaction_alpha == 0.01
    assert engine.LOSS_WEIGHTS["interaction_rep"] == "interaction_rep_weight" and engine.LOSS_WEIGHTS["interaction_att"] == "interaction_att_weight"
    assert all(hasattr(c, a) for a in engine.LOSS_WEIGHTS.values())
    c.resnet_type = 18
    m = get_model("train", cfg=c, with_encoder=False)
    assert not m.interaction_loss_enabled() and m._interaction is None
    monkeypatch.setenv("HOISDF_INTERACTION_LOSS", "1")
    assert m.interaction_loss_enabled()
    monkeypatch.delenv("HOISDF_INTERACTION_LOSS")
    c.interaction_loss = True
    assert m.interaction_loss_enabled()
    ik = Config()
    ik.resnet_type = 18
    ik.apply_setting("ho3d_render")
    ik.interaction_loss = True
    with pytest.raises(ValueError, match="interaction_loss"):
        get_model("train", cfg=ik, with_encoder=False)
    sig = inspect.signature(ops.interaction_loss).parameters
    assert list(sig)[:10] == ["hand_verts", "hand_faces", "obj_verts", "obj_faces", "obj_n_faces", "obj_n_verts", "rep_w_hand", "att_w_hand",
                              "rep_w_obj", "alpha"]
    assert sig["alpha"].default == 0.01 and all(sig[k].default is None for k in list(sig)[4:9])
    assert interaction_loss_oracle.NO_FACE == 3.0e38
    # nothing on the product path imports the restatement
    import hoisdf_amd
    root = os.path.dirname(hoisdf_amd.__file__)
    for name in ("ops.py", "_marshal.py", "ops_eval.py", "ops_mesh.py", "ops_infer.py", "model.py", "engine.py", "sdf_data.py", "metrics.py"):
        assert "interaction_loss_oracle" not in open(os.path.join(root, name)).read(), name


def test_default_contact_zones_come_from_the_skinning_weights():
    import torch
    from hoisdf_amd.nets.mano import ManoLayer
    from hoisdf_amd.sdf_data import DISTAL_JOINTS, MeshSdfSource, contact_zone_weights, procedural_templates
    from hoisdf_amd.config import Config
    layer = ManoLayer()
    w = contact_zone_weights(layer.th_weights)
    top = layer.th_weights.argmax(1)
    assert w.shape == (778,) and w.dtype == torch.float32 and set(w.tolist()) == {0.0, 1.0}
    assert DISTAL_JOINTS == (3, 6, 9, 12, 15) and all((w[i] == 1) == (int(top[i]) in DISTAL_JOINTS) for i in range(778))
    src = MeshSdfSource(layer, procedural_templates(), Config())
    assert src.templates["n_verts"].tolist() == [162, 192, 150] and src.templates["n_faces"].tolist() == [320, 384, 192]


def test_the_header_states_the_rules_the_tests_and_the_oracle_rely_on():
    text = " ".join(open(_lib.HEADER_PATH).read().split())
    for phrase in ("rep_hand = sum_v rep_w_hand[v] max(0, -sdf_obj(v)) / sum_v rep_w_hand[v]", "alpha tanh(max(0, sdf_obj(v)) / alpha)",
                   "d sdf / d p = s n", "d sdf / d x_k = -beta_k s n", "ASCENDING query index", "no atomics", "5 launches", "2 launches",
                   "every row is written", "Two calls give the same bits", "a batch equals its samples run one by one",
                   "one that is not positive gives 0", "A point with d = 0", "tiles of HOISDF_INTERACT_LOSS_TILE records"):
        assert phrase in text, phrase
