"""CPU: the interaction entry of the C ABI (include/hoisdf.h hoisdf_eval_interaction, csrc/interact.hip) refuses malformed calls with
HOISDF_ERR_INVALID and a message that names the argument before anything is launched (no GPU here: a launch would fail loudly),
returns 0 for an empty batch, its workspace query is arithmetic, and the Python surface is opt-in."""
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


def test_the_entry_and_its_limit_are_declared_and_exported(lib):
    assert "hoisdf_eval_interaction" in _lib.SIGNATURES and _lib.SIGNATURES["hoisdf_eval_interaction"][-1] is C.c_void_p
    assert len(_lib.SIGNATURES["hoisdf_eval_interaction"]) == 18
    assert _lib._OTHER["hoisdf_eval_interaction_workspace_bytes"] == ([C.c_int] * 5, C.c_long)
    assert _lib.CONSTANTS["INTERACT_MAX_GRID"] == 64
    for name in ("hoisdf_eval_interaction", "hoisdf_eval_interaction_workspace_bytes"):
        assert hasattr(lib, name), name


def test_the_workspace_query_is_arithmetic(lib):
    q = lib.hoisdf_eval_interaction_workspace_bytes
    B, Vh, Fh, Vo, Fo = 4, 778, 1538, 1000, 2000
    need = q(B, Vh, Fh, Vo, Fo)
    # both prepared meshes (triangles, areas, prefix sums, boxes), the two vertex distance arrays, one count per block of 64 cells
    least = B * (Fh + Fo) * (48 + 4 + 4) + 2 * B * 32 + B * (Vh + Vo) * 4 + B * (64 ** 3 // 64) * 4
    assert least <= need <= least + 16 * 256 and need % 256 == 0
    assert need >= lib.hoisdf_mesh_sdf_rows_workspace_bytes(B, Fh, Fo)
    assert q(2 * B, Vh, Fh, Vo, Fo) > need and q(B, Vh, Fh, Vo, Fo) == need
    assert q(0, 0, 0, 0, 0) == 0
    assert q(B, Vh, 4097, Vo, Fo) == INVALID and b"4097" in lib.hoisdf_last_error()
    assert q(B, Vh, Fh, Vo, 5000) == INVALID and b"5000" in lib.hoisdf_last_error()
    assert q(-1, Vh, Fh, Vo, Fo) == INVALID and q(65536, Vh, Fh, Vo, Fo) == INVALID and q(B, -1, Fh, Vo, Fo) == INVALID
    assert q(B, Vh, Fh, -2, Fo) == INVALID and b"V=-2" in lib.hoisdf_last_error()


def test_eval_interaction_checks_its_arguments_before_any_launch(lib):
    hand, obj = _mesh(), _mesh(V=1000, max_faces=2000, face_batch_stride=6000)
    need = lib.hoisdf_eval_interaction_workspace_bytes(4, 778, 1538, 1000, 2000)
    outs = ("pen_hand", "pen_obj", "min_dist", "contact_verts", "in_contact", "volume", "inside_count")

    def call(h=hand, o=obj, nv=None, B=4, cd=0.005, voxel=0.005, mask=None, grid=None, ws=FAKE, nws=need, **out):
        ptrs = [out.get(k, FAKE) for k in outs]
        return lib.hoisdf_eval_interaction(None if h is None else C.addressof(h), None if o is None else C.addressof(o), nv, B, cd, voxel,
                                           *ptrs, mask, grid, ws, nws, None)

    for kw, what in ((dict(h=None), b"hand"), (dict(o=None), b"obj"), (dict(ws=None), b"workspace"), (dict(h=_mesh(verts=None)), b"verts"),
                     (dict(o=_mesh(V=1000, max_faces=2000, faces=None)), b"faces")) + tuple((dict([(k, None)]), k.encode()) for k in outs):
        assert call(**kw) == INVALID and b"null" in lib.hoisdf_last_error() and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    inf, nan = float("inf"), float("nan")
    for kw, what in ((dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"), (dict(h=_mesh(max_faces=4097)), b"max_faces=4097"),
                     (dict(o=_mesh(max_faces=5000)), b"max_faces=5000"), (dict(h=_mesh(V=0)), b"without vertices"),
                     (dict(o=_mesh(max_faces=2000, face_batch_stride=5999)), b"face_batch_stride=5999"),
                     (dict(cd=-0.001), b"contact_dist=-0.001"), (dict(cd=inf), b"contact_dist=inf"), (dict(cd=nan), b"contact_dist="),
                     (dict(voxel=0.0), b"voxel=0"), (dict(voxel=-0.005), b"voxel=-0.005"), (dict(voxel=inf), b"voxel=inf"),
                     (dict(voxel=nan), b"voxel="), (dict(nws=need - 1), b"workspace"), (dict(nws=0), b"workspace")):
        assert call(**kw) == INVALID and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    # B = 0: nothing to do, whatever the pointers
    assert call(B=0, ws=None, nws=0, **{k: None for k in outs}) == 0


def test_python_surface_is_opt_in(monkeypatch):
    from hoisdf_amd import interaction_oracle, metrics, ops
    from hoisdf_amd.config import Config
    monkeypatch.delenv("HOISDF_INTERACTION", raising=False)
    c = Config()
    assert c.eval_interaction is False and (c.contact_dist, c.interaction_voxel) == (0.005, 0.005)
    assert not metrics.interaction_enabled(c)
    monkeypatch.setenv("HOISDF_INTERACTION", "1")
    assert metrics.interaction_enabled(Config())
    monkeypatch.delenv("HOISDF_INTERACTION")
    c.eval_interaction = True
    assert metrics.interaction_enabled(c)
    sig = inspect.signature(ops.eval_interaction).parameters
    assert list(sig)[:9] == ["hand_verts", "hand_faces", "obj_verts", "obj_faces", "obj_n_faces", "obj_n_verts", "contact_dist", "voxel", "want_mask"]
    assert (sig["contact_dist"].default, sig["voxel"].default, sig["want_mask"].default) == (0.005, 0.005, False)
    ev = inspect.signature(metrics.Evaluator.__init__).parameters
    assert ev["interaction"].default is False and ev["template_faces"].default is None
    assert interaction_oracle.MAX_GRID == _lib.CONSTANTS["INTERACT_MAX_GRID"]
    with pytest.raises(ValueError, match="template_faces"):
        import torch
        metrics.Evaluator(c, torch.zeros(2, 8, 3))


def test_the_header_states_the_rules_the_tests_and_the_oracle_rely_on():
    text = " ".join(open(_lib.HEADER_PATH).read().split())
    for phrase in ("n = min(ceil(extent / voxel), HOISDF_INTERACT_MAX_GRID)", "cell = extent / n", "lo + (ix + 0.5) cell",
                   "winding_obj > 0.5 and winding_hand > 0.5", "6 launches", "ix fastest", "metres", "sdf_obj <= contact_dist",
                   "bytes from n_x n_y n_z on are not touched", "n_x | n_y << 8 | n_z << 16"):
        assert phrase in text, phrase
