"""CPU: the raster entries of the C ABI (include/hoisdf.h "raster", csrc/raster.hip) refuse malformed calls with HOISDF_ERR_INVALID
and a message that names the argument before anything is launched (no GPU here: a launch would fail loudly), return 0 for an empty
batch, their workspace query is arithmetic, the library exports what the header declares, and the Python surface is opt-in."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from hoisdf_amd import _lib

INVALID = -1
FAKE = C.c_void_p(0x100000)
ENTRIES = ("hoisdf_raster_meshes", "hoisdf_raster_overlay", "hoisdf_eval_silhouette")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def _mesh(**kw):
    d = dict(verts=0x100000, faces=0x100000, n_faces=None, face_batch_stride=0, V=12, max_faces=20)
    d.update(kw)
    return _lib.Mesh(**d)


def test_the_entries_are_declared_and_the_library_exports_what_the_header_declares(lib):
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][-1] is C.c_void_p, name
    assert _lib._OTHER["hoisdf_raster_workspace_bytes"] == ([C.c_int] * 3, C.c_long)
    assert len(_lib.SIGNATURES["hoisdf_raster_meshes"]) == 18 and len(_lib.SIGNATURES["hoisdf_raster_overlay"]) == 9
    assert len(_lib.SIGNATURES["hoisdf_eval_silhouette"]) == 8
    assert _lib.SIGNATURES["hoisdf_raster_meshes"][7] is C.c_float, "near"
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (hoisdf_\w+)", syms))
    assert set(_lib.exported_symbols()) <= exported, set(_lib.exported_symbols()) - exported
    assert set(ENTRIES + ("hoisdf_raster_workspace_bytes",)) <= exported


def test_the_constants_come_from_the_header_and_the_kernel_is_held_to_them():
    from hoisdf_amd import raster_oracle
    c = _lib.CONSTANTS
    assert c["RASTER_TILE"] >= 8 and c["RASTER_CHUNK"] >= 64 and c["RASTER_CHUNK"] % 64 == 0, "a wave rejects 64 records at a time"
    assert c["RASTER_MAX_SIZE"] == raster_oracle.MAX_SIZE == 4096
    src = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "raster.hip")).read()
    assert re.search(r"static_assert\(HOISDF_RASTER_TILE == \w+ && HOISDF_RASTER_CHUNK == \w+", src)
    text = " ".join(re.sub(r"^ \*", " ", open(_lib.HEADER_PATH).read(), flags=re.M).split())          # comment lines joined
    for phrase in ("2 launches", "u = ((K0 x + K1 y) + K2 z) / z", "X = rint(256 u)", "round half to even", "NO clipping",
                   "|u| or |v| >= 16384", "A2 = (X1-X0)(Y2-Y0) - (X2-X0)(Y1-Y0)", "No back-face culling", "corners 1 and 2 swapped",
                   "E = dx (py' - Ya) - dy (px' - Xa)", "left edge", "top edge", "l_i = (double)E_i / (double)A2",
                   "invz = (l0 (1/z0) + l1 (1/z1)) + l2 (1/z2)", "(z_pix as float32, mesh id, face row)", "mesh << 16 | face row",
                   "(alpha colour[mesh][c] + (256 - alpha) in + 128) >> 8", "image_out == image_in is allowed", "a value > 0.5 is set"):
        assert phrase in text, phrase


def test_the_workspace_query_is_arithmetic(lib):
    q = lib.hoisdf_raster_workspace_bytes
    need = q(22, 1538, 2000)
    assert need % 256 == 0 and 22 * 3538 * 32 <= need <= 22 * 3538 * 128, "tens of bytes per face row"
    assert q(0, 1538, 2000) == 0 and q(22, 0, 0) == 0 and q(44, 1538, 2000) > need and q(22, 1538, 2001) >= need
    assert q(22, 1538, 0) + q(22, 0, 2000) in range(need, need + 257)
    for bad, what in (((-1, 1, 1), b"B=-1"), ((65536, 1, 1), b"B=65536"), ((2, 4097, 1), b"max_faces=4097"), ((2, 1, 4097), b"max_faces=4097"),
                      ((2, -1, 1), b"max_faces=-1")):
        assert q(*bad) == INVALID and what in lib.hoisdf_last_error(), bad


def test_raster_meshes_checks_its_arguments_before_any_launch(lib):
    outs = ("id_out", "depth_out", "hand_seg", "obj_seg", "counts")
    need = lib.hoisdf_raster_workspace_bytes(2, 20, 20)

    def rm(hand=_mesh(), obj=_mesh(), K=FAKE, B=2, w=64, h=48, half=0, near=0.01, hm_w=32, hm_h=24, ws=FAKE, nws=need, **out):
        ptrs = [out.get(k, FAKE) for k in outs]
        return lib.hoisdf_raster_meshes(None if hand is None else C.addressof(hand), None if obj is None else C.addressof(obj), K, B, w, h,
                                        half, near, ptrs[0], ptrs[1], ptrs[2], ptrs[3], hm_w, hm_h, ptrs[4], ws, nws, None)

    err = lib.hoisdf_last_error
    for kw, what in ((dict(hand=None, obj=None), b"hand and obj"), (dict(K=None), b"(K)"), (dict(ws=None), b"workspace"),
                     (dict(hand=_mesh(verts=None)), b"verts"), (dict(obj=_mesh(faces=None)), b"faces"),
                     (dict({k: None for k in outs}), b"one output at least")):
        assert rm(**kw) == INVALID and b"null" in err() and what in err(), (kw, err())
    for kw, what in ((dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"), (dict(w=0), b"width=0"), (dict(w=4097), b"width=4097"),
                     (dict(h=0), b"height=0"), (dict(h=4097), b"height=4097"), (dict(half=2), b"half_pixel=2"), (dict(half=-1), b"half_pixel=-1"),
                     (dict(near=0.0), b"near=0"), (dict(near=-1.0), b"near=-1"), (dict(near=float("inf")), b"near=inf"),
                     (dict(near=float("nan")), b"near="), (dict(hand=_mesh(max_faces=4097)), b"max_faces=4097"),
                     (dict(obj=_mesh(V=0)), b"without vertices"), (dict(obj=_mesh(face_batch_stride=59)), b"face_batch_stride=59"),
                     (dict(hand=_mesh(face_batch_stride=59)), b"hand face_batch_stride=59"),
                     (dict(hm_w=0), b"hm_w=0"), (dict(hm_w=48), b"hm_w=48"), (dict(hm_h=7), b"hm_h=7"), (dict(hm_h=-2), b"hm_h=-2"),
                     (dict(nws=need - 1), b"workspace"), (dict(nws=0), b"workspace")):
        assert rm(**kw) == INVALID and what in err(), (kw, err())
    assert rm(hand=None, nws=need // 2 - 1) == INVALID and b"workspace" in err(), "one mesh: half the records"
    assert rm(B=0, K=None, ws=None, nws=0, **{k: None for k in outs[1:]}) == 0
    assert rm(B=0, K=None, ws=None, nws=0, **{k: None for k in outs}) == INVALID, "also an empty batch names its outputs"


def test_overlay_and_silhouette_check_their_arguments_before_any_launch(lib):
    colour = (C.c_uint8 * 6)(1, 2, 3, 4, 5, 6)

    def ov(ids=FAKE, src=FAKE, dst=FAKE, col=C.addressof(colour), alpha=160, B=2, w=64, h=48):
        return lib.hoisdf_raster_overlay(ids, src, dst, col, alpha, B, w, h, None)

    err = lib.hoisdf_last_error
    for kw, what in ((dict(ids=None), b"id"), (dict(src=None), b"image_in"), (dict(dst=None), b"image_out"), (dict(col=None), b"colour")):
        assert ov(**kw) == INVALID and b"null" in err() and what in err(), (kw, err())
    for kw, what in ((dict(alpha=-1), b"alpha=-1"), (dict(alpha=257), b"alpha=257"), (dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"),
                     (dict(w=0), b"width=0"), (dict(h=4097), b"height=4097")):
        assert ov(**kw) == INVALID and what in err(), (kw, err())
    assert ov(B=0, ids=None, src=None, dst=None) == 0

    def sil(ph=FAKE, po=FAKE, gh=FAKE, go=FAKE, B=2, n=100, counts=FAKE):
        return lib.hoisdf_eval_silhouette(ph, po, gh, go, B, n, counts, None)

    for k, what in (("ph", b"pred_hand"), ("po", b"pred_obj"), ("gh", b"gt_hand"), ("go", b"gt_obj"), ("counts", b"counts")):
        assert sil(**{k: None}) == INVALID and b"null" in err() and what in err(), (k, err())
    for kw, what in ((dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"), (dict(n=0), b"n=0"), (dict(n=(1 << 24) + 1), b"n=16777217")):
        assert sil(**kw) == INVALID and what in err(), (kw, err())
    assert sil(B=0, ph=None, po=None, gh=None, go=None, counts=None) == 0


def test_the_python_surface_is_opt_in(monkeypatch):
    from hoisdf_amd import engine, metrics, ops, render
    from hoisdf_amd.config import Config
    for name in ("raster_meshes", "raster_overlay", "eval_silhouette"):
        assert callable(getattr(ops, name))
    sig = inspect.signature(ops.raster_meshes).parameters
    assert list(sig)[:7] == ["hand_verts", "hand_faces", "obj_verts", "obj_faces", "K", "width", "height"]
    assert sig["half_pixel"].default is False and sig["near"].default == 0.01
    for var in ("HOISDF_SEG", "HOISDF_SILHOUETTE"):
        monkeypatch.delenv(var, raising=False)
    c = Config()
    assert c.seg_source != "mesh" and c.eval_silhouette is False and not c.overlay_dir
    assert c.raster_half_pixel is False and c.raster_near == 0.01 and c.overlay_alpha == 160
    assert not render.seg_from_mesh(c) and not metrics.silhouette_enabled(c)
    monkeypatch.setenv("HOISDF_SEG", "mesh")
    monkeypatch.setenv("HOISDF_SILHOUETTE", "1")
    assert render.seg_from_mesh(Config()) and metrics.silhouette_enabled(Config())
    monkeypatch.delenv("HOISDF_SEG")
    monkeypatch.delenv("HOISDF_SILHOUETTE")
    c.seg_source, c.eval_silhouette = "mesh", True
    assert render.seg_from_mesh(c) and metrics.silhouette_enabled(c)
    assert inspect.signature(engine.Trainer.__init__).parameters["seg_source"].default is None
    assert inspect.signature(metrics.Evaluator.__init__).parameters["silhouette"].default is False
    for name in ("MeshSegSource", "predicted_pair", "overlay_batch"):
        assert callable(getattr(render, name))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "test.py")).read()
    assert "--silhouette" in text and "--overlay" in text
