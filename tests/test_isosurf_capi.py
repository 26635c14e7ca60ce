"""CPU: the iso-surface entries of the C ABI (include/hoisdf.h "iso-surface", csrc/isosurf.hip) refuse malformed calls with
HOISDF_ERR_INVALID and a message that names the argument before anything is launched (no GPU here: a launch would fail loudly),
return 0 for an empty batch, their workspace queries are arithmetic, the library exports what the header declares, and the Python
surface is opt-in."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from hoisdf_amd import _lib

INVALID = -1
FAKE = C.c_void_p(0x100000)
ENTRIES = ("hoisdf_iso_grid_points", "hoisdf_iso_refine_grid", "hoisdf_iso_extract", "hoisdf_eval_surface")
QUERIES = ("hoisdf_iso_extract_workspace_bytes", "hoisdf_eval_surface_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_the_entries_are_declared_and_the_library_exports_what_the_header_declares(lib):
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][-1] is C.c_void_p, name
    assert _lib._OTHER["hoisdf_iso_extract_workspace_bytes"] == ([C.c_int] * 2, C.c_long)
    assert _lib._OTHER["hoisdf_eval_surface_workspace_bytes"] == ([C.c_int] * 4, C.c_long)
    assert _lib.CONSTANTS["ISO_MAX_GRID"] == 128
    assert len(_lib.SIGNATURES["hoisdf_iso_extract"]) == 17 and len(_lib.SIGNATURES["hoisdf_eval_surface"]) == 16
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (hoisdf_\w+)", syms))
    assert set(_lib.exported_symbols()) <= exported, set(_lib.exported_symbols()) - exported
    assert set(ENTRIES + QUERIES) <= exported


def test_the_workspace_queries_are_arithmetic(lib):
    q = lib.hoisdf_iso_extract_workspace_bytes
    B, n = 22, 64
    need = q(B, n)
    least = B * n ** 3 * 4 + 2 * B * (n ** 3 // 256) * 4          # one word per node, two counts per block of 256 nodes
    assert least <= need <= least + 3 * 256 and need % 256 == 0
    assert q(0, 2) == 0 and q(2 * B, n) > need and q(B, 128) > need
    for bad, what in (((B, 1), b"n=1"), ((B, 129), b"n=129"), ((-1, n), b"B=-1"), ((65536, n), b"B=65536")):
        assert q(*bad) == INVALID and what in lib.hoisdf_last_error(), bad
    s = lib.hoisdf_eval_surface_workspace_bytes
    need = s(4, 300, 20, 512)
    least = 4 * 20 * (48 + 4 + 4) + 4 * 32 + 4 * 300 * 4 + 4 * 512 * 16
    assert least <= need <= least + 8 * 256 and need % 256 == 0
    for bad, what in (((4, 300, 4097, 512), b"4097"), ((4, -1, 20, 512), b"max_verts=-1"), ((4, 300, 20, 0), b"n_samples=0"),
                      ((65536, 300, 20, 512), b"B=65536")):
        assert s(*bad) == INVALID and what in lib.hoisdf_last_error(), bad


def test_grid_points_and_refine_grid_check_their_arguments_before_any_launch(lib):
    gp = lambda grid=FAKE, n=8, B=2, pts=FAKE, idx=None: lib.hoisdf_iso_grid_points(grid, n, B, pts, idx, None)
    for kw, what in ((dict(grid=None), b"null"), (dict(pts=None), b"null"), (dict(n=1), b"n=1"), (dict(n=129), b"n=129"),
                     (dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536")):
        assert gp(**kw) == INVALID and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    assert gp(B=0, grid=None, pts=None) == 0

    def rf(values=FAKE, ld=1, grid=FAKE, n=8, B=2, iso=0.0, pad=1, n_out=16, out=FAKE):
        return lib.hoisdf_iso_refine_grid(values, ld, grid, n, B, iso, pad, n_out, out, None)

    for kw, what in ((dict(values=None), b"values"), (dict(grid=None), b"grid_in"), (dict(out=None), b"grid_out"), (dict(ld=0), b"ld=0"),
                     (dict(n=1), b"n=1"), (dict(n=129), b"n=129"), (dict(n_out=1), b"n_out=1"), (dict(n_out=129), b"n_out=129"),
                     (dict(pad=-1), b"pad_cells=-1"), (dict(B=65536), b"B=65536"), (dict(iso=float("nan")), b"iso")):
        assert rf(**kw) == INVALID and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    assert rf(B=0, values=None, grid=None, out=None) == 0


def test_iso_extract_checks_its_arguments_before_any_launch(lib):
    need = lib.hoisdf_iso_extract_workspace_bytes(2, 8)

    def ex(values=FAKE, ld=1, grid=FAKE, n=8, B=2, iso=0.0, scale=1.0, shift=None, verts=FAKE, mv=100, faces=FAKE, mf=200, nv=FAKE,
           nf=FAKE, ws=FAKE, nws=need):
        return lib.hoisdf_iso_extract(values, ld, grid, n, B, iso, scale, shift, verts, mv, faces, mf, nv, nf, ws, nws, None)

    for kw, what in ((dict(values=None), b"values"), (dict(grid=None), b"grid"), (dict(nv=None), b"n_verts"), (dict(nf=None), b"n_faces"),
                     (dict(ws=None), b"workspace")):
        assert ex(**kw) == INVALID and b"null" in lib.hoisdf_last_error() and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    for kw, what in ((dict(n=1), b"n=1"), (dict(n=129), b"n=129"), (dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"), (dict(ld=0), b"ld=0"),
                     (dict(mv=-1), b"max_verts=-1"), (dict(mf=-5), b"max_faces=-5"), (dict(nws=need - 1), b"workspace"),
                     (dict(nws=0), b"workspace"), (dict(iso=float("nan")), b"iso")):
        assert ex(**kw) == INVALID and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    assert ex(B=0, values=None, grid=None, nv=None, nf=None, ws=None, nws=0) == 0


def test_eval_surface_checks_its_arguments_before_any_launch(lib):
    outs = ("pred_to_gt", "gt_to_pred", "chamfer", "n_used")
    need = lib.hoisdf_eval_surface_workspace_bytes(2, 300, 20, 512)

    def mesh(**kw):
        d = dict(verts=0x100000, faces=0x100000, n_faces=None, face_batch_stride=0, V=12, max_faces=20)
        d.update(kw)
        return _lib.Mesh(**d)

    def ev(pred=FAKE, pn=FAKE, mv=300, gt=mesh(), B=2, ns=512, ws=FAKE, nws=need, **out):
        ptrs = [out.get(k, FAKE) for k in outs]
        return lib.hoisdf_eval_surface(pred, pn, mv, None if gt is None else C.addressof(gt), B, ns, 7, *ptrs, None, None, ws, nws, None)

    for kw, what in ((dict(gt=None), b"gt"), (dict(pred=None), b"pred_verts"), (dict(pn=None), b"pred_n_verts"), (dict(ws=None), b"workspace"),
                     (dict(gt=mesh(verts=None)), b"verts"), (dict(gt=mesh(faces=None)), b"faces")) + tuple(
                         (dict([(k, None)]), k.encode()) for k in outs):
        assert ev(**kw) == INVALID and b"null" in lib.hoisdf_last_error() and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    for kw, what in ((dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"), (dict(gt=mesh(max_faces=4097)), b"max_faces=4097"),
                     (dict(gt=mesh(V=0)), b"without vertices"), (dict(gt=mesh(face_batch_stride=59)), b"face_batch_stride=59"),
                     (dict(mv=-1), b"max_verts=-1"), (dict(ns=0), b"n_samples=0"), (dict(nws=need - 1), b"workspace")):
        assert ev(**kw) == INVALID and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    assert ev(B=0, pred=None, pn=None, ws=None, nws=0, **{k: None for k in outs}) == 0


def test_python_surface_and_the_oracle_agree_with_the_header():
    from hoisdf_amd import isosurf_oracle, ops
    assert isosurf_oracle.MAX_GRID == _lib.CONSTANTS["ISO_MAX_GRID"]
    sig = inspect.signature(ops.iso_surface).parameters
    assert list(sig) == ["values", "grid", "n", "iso", "max_verts", "max_faces", "out_scale", "out_shift"]
    assert [sig[k].default for k in list(sig)[3:]] == [0.0, None, None, None, None]
    for name in ("iso_grid_points", "iso_refine_grid", "eval_surface"):
        assert callable(getattr(ops, name))
    text = " ".join(re.sub(r"^ \*", " ", open(_lib.HEADER_PATH).read(), flags=re.M).split())      # comment lines joined
    for phrase in ("lo + ix cell", "value < iso", "100, 010, 001, 110, 101, 011, 111", "t = (iso - v_a) / (v_b - v_a)",
                   "ascending node index, then ascending edge number", "xyz, xzy, yxz, yzx, zxy, zyx", "cut along io - jp",
                   "counter-clockwise seen from the outside", "the counts NEEDED", "the lowest index wins an exact tie"):
        assert phrase in text, phrase


def test_field_evaluation_is_opt_in(monkeypatch):
    import torch
    from hoisdf_amd import metrics
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import Model
    monkeypatch.delenv("HOISDF_FIELD", raising=False)
    c = Config()
    assert c.eval_field is False and c.field_grid == 64 and c.field_max_verts > 0 and c.field_samples > 0
    assert not metrics.field_enabled(c)
    monkeypatch.setenv("HOISDF_FIELD", "1")
    assert metrics.field_enabled(Config())
    monkeypatch.delenv("HOISDF_FIELD")
    c.eval_field = True
    assert metrics.field_enabled(c)
    ev = inspect.signature(metrics.Evaluator.__init__).parameters
    assert ev["field"].default is False and list(ev)[-1] == "field", "appended: the positional order of the existing arguments stays"
    with pytest.raises(ValueError, match="template_faces"):
        metrics.Evaluator(c, torch.zeros(2, 8, 3))
    sig = inspect.signature(Model.field_surface).parameters
    assert list(sig)[:8] == ["self", "feature_pyramid", "meta_info", "kind", "n", "coarse_n", "box", "return_values"]
    assert [sig[k].default for k in ("kind", "n", "coarse_n", "box", "return_values")] == ["hand", 64, 32, None, False]
    assert Model.FIELD_CHUNK_ROWS == 64 ** 3 and "262144" in Model.field_surface.__doc__
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "--field-surface" in open(os.path.join(root, "test.py")).read()
