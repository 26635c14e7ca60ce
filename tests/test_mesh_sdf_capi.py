"""CPU: the mesh-SDF entries of the C ABI (include/hoisdf.h hoisdf_mesh_*, csrc/mesh_sdf.hip) refuse malformed calls with
HOISDF_ERR_INVALID and a message before anything is launched (no GPU here: a launch would fail loudly), return 0 for an empty batch,
and the Python surface is opt-in."""
import ctypes as C
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


def test_the_entries_and_limits_are_declared(lib):
    for name in ("hoisdf_mesh_prepare", "hoisdf_mesh_sample_points", "hoisdf_mesh_sdf", "hoisdf_mesh_sdf_rows"):
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][-1] is C.c_void_p, name      # status entries, stream last
    assert _lib._OTHER["hoisdf_mesh_sdf_rows_workspace_bytes"] == ([C.c_int] * 3, C.c_long)
    assert _lib.CONSTANTS["MESH_MAX_FACES"] == 4096 and _lib.CONSTANTS["MESH_TILE"] == 128
    assert [n for n, _ in _lib.Mesh._fields_] == ["verts", "faces", "n_faces", "face_batch_stride", "V", "max_faces"]


def test_mesh_prepare_checks_its_arguments_before_any_launch(lib):
    full = [FAKE, 2, 10, FAKE, 0, None, 8, FAKE, FAKE, FAKE, FAKE, None]        # n_faces is optional
    for i in (0, 3, 7, 8, 9, 10):
        args = list(full)
        args[i] = None
        assert lib.hoisdf_mesh_prepare(*args) == INVALID and b"null" in lib.hoisdf_last_error(), i
    for i, bad, what in ((1, -1, b"B=-1"), (1, 65536, b"B=65536"), (2, -3, b"V=-3"), (6, -1, b"max_faces=-1"),
                         (6, 4097, b"max_faces=4097"), (4, 23, b"face_batch_stride=23"), (4, -1, b"face_batch_stride=-1")):
        args = list(full)
        args[i] = bad
        assert lib.hoisdf_mesh_prepare(*args) == INVALID and what in lib.hoisdf_last_error(), (i, bad, lib.hoisdf_last_error())
    assert lib.hoisdf_mesh_prepare(None, 0, 10, None, 0, None, 8, None, None, None, None, None) == 0      # no sample: nothing to do


def test_mesh_sample_points_checks_its_arguments_before_any_launch(lib):
    full = [FAKE, FAKE, FAKE, None, 8, 2, 100, 0.01, 0.003, 16, 0.05, 7, FAKE, 3, None, None]   # n_faces and face_out are optional
    for i in (0, 1, 2, 12):
        args = list(full)
        args[i] = None
        assert lib.hoisdf_mesh_sample_points(*args) == INVALID and b"null" in lib.hoisdf_last_error(), i
    for i, bad, what in ((4, 4097, b"max_faces=4097"), (5, -1, b"B=-1"), (6, -5, b"N=-5"), (13, 2, b"ldp=2"), (7, -0.01, b"sigma1=-0.01"),
                         (8, -1.0, b"sigma2=-1"), (10, -0.5, b"pad=-0.5")):
        args = list(full)
        args[i] = bad
        assert lib.hoisdf_mesh_sample_points(*args) == INVALID and what in lib.hoisdf_last_error(), (i, bad, lib.hoisdf_last_error())
    for i in (5, 6):                                                             # B = 0, N = 0
        args = [None if isinstance(a, C.c_void_p) else a for a in full]
        args[i] = 0
        assert lib.hoisdf_mesh_sample_points(*args) == 0, i


def test_mesh_sdf_checks_its_arguments_before_any_launch(lib):
    full = [FAKE, 3, 2, 100, FAKE, FAKE, None, 8, None, 0, FAKE, 1, None, None, None, None, None]
    for i in (0, 4, 5, 10):
        args = list(full)
        args[i] = None
        assert lib.hoisdf_mesh_sdf(*args) == INVALID and b"null" in lib.hoisdf_last_error(), i
    args = list(full)
    args[15] = FAKE                                                              # labels wanted, no vertex labels given
    assert lib.hoisdf_mesh_sdf(*args) == INVALID and b"vert_label" in lib.hoisdf_last_error()
    for i, bad, what in ((1, 2, b"ldp=2"), (2, -1, b"B=-1"), (3, -1, b"N=-1"), (7, 4097, b"max_faces=4097"), (7, -1, b"max_faces=-1"),
                         (9, -1, b"label_batch_stride=-1"), (11, 0, b"ld=0")):
        args = list(full)
        args[i] = bad
        assert lib.hoisdf_mesh_sdf(*args) == INVALID and what in lib.hoisdf_last_error(), (i, bad, lib.hoisdf_last_error())
    for i in (2, 3):
        args = [None if isinstance(a, C.c_void_p) else a for a in full]
        args[i] = 0
        assert lib.hoisdf_mesh_sdf(*args) == 0, i


def _mesh(**kw):
    d = dict(verts=0x100000, faces=0x100000, n_faces=None, face_batch_stride=0, V=778, max_faces=1538)
    d.update(kw)
    return _lib.Mesh(**d)


def test_mesh_sdf_rows_checks_its_arguments_before_any_launch(lib):
    hand, obj = _mesh(), _mesh(V=1000, max_faces=2000, face_batch_stride=6000)
    need = lib.hoisdf_mesh_sdf_rows_workspace_bytes(4, 1538, 2000)
    assert need >= 4 * (1538 + 2000) * (48 + 4 + 4) + 2 * 4 * 32                 # triangles, areas, prefix sums, two boxes
    assert lib.hoisdf_mesh_sdf_rows_workspace_bytes(4, 4097, 2000) == INVALID and b"4097" in lib.hoisdf_last_error()
    assert lib.hoisdf_mesh_sdf_rows_workspace_bytes(-1, 10, 10) == INVALID
    assert lib.hoisdf_mesh_sdf_rows_workspace_bytes(0, 0, 0) == 0

    def call(h=hand, o=obj, label=FAKE, B=4, nh=2400, no=800, s1=0.01, s2=0.003, every=16, pad=0.05, clamp=0.05, rows=FAKE, ld=6,
             ws=FAKE, nws=need):
        return lib.hoisdf_mesh_sdf_rows(None if h is None else C.addressof(h), None if o is None else C.addressof(o), label, B, nh, no,
                                        s1, s2, every, pad, clamp, 3, rows, ld, ws, nws, None)

    for kw in (dict(h=None), dict(o=None), dict(label=None), dict(rows=None), dict(ws=None), dict(h=_mesh(verts=None)),
               dict(o=_mesh(V=1000, max_faces=2000, faces=None))):
        assert call(**kw) == INVALID and b"null" in lib.hoisdf_last_error(), kw
    for kw, what in ((dict(ld=5), b"ld=5"), (dict(B=-1), b"B=-1"), (dict(nh=-1), b"n_hand=-1"), (dict(no=-2), b"n_obj=-2"),
                     (dict(h=_mesh(max_faces=4097)), b"max_faces=4097"), (dict(o=_mesh(max_faces=5000)), b"max_faces=5000"),
                     (dict(o=_mesh(max_faces=2000, face_batch_stride=5999)), b"face_batch_stride=5999"), (dict(clamp=-1.0), b"clamp=-1"),
                     (dict(s1=-0.5), b"sigma1=-0.5"), (dict(nws=need - 1), b"workspace")):
        assert call(**kw) == INVALID and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    assert call(B=0, rows=None, ws=None, label=None) == 0
    assert call(nh=0, no=0, rows=None, ws=None, label=None) == 0


def test_python_surface_is_opt_in(monkeypatch):
    from hoisdf_amd import engine, ops, sdf_data
    from hoisdf_amd.config import Config
    monkeypatch.delenv("HOISDF_SDF", raising=False)
    c = Config()
    assert c.sdf_source == "" and not sdf_data.mesh_sdf_enabled(c)
    assert (tuple(c.mesh_sdf_sigma), c.mesh_sdf_uniform_every, c.mesh_sdf_pad, c.mesh_sdf_candidates) == ((0.01, 0.003), 16, 0.05, 4)
    monkeypatch.setenv("HOISDF_SDF", "mesh")
    assert sdf_data.mesh_sdf_enabled(Config())
    monkeypatch.delenv("HOISDF_SDF")
    c.sdf_source = "mesh"
    assert sdf_data.mesh_sdf_enabled(c)
    for name in ("mesh_sdf", "mesh_sample_points", "mesh_sdf_rows", "PreparedMesh"):
        assert hasattr(ops, name), name
    assert hasattr(sdf_data, "MeshSdfSource") and hasattr(engine, "SyntheticMeshSdfDataset")
    import inspect
    assert "sdf_source" in inspect.signature(engine.Trainer.__init__).parameters


def test_procedural_templates_are_padded_to_one_shape():
    from hoisdf_amd import sdf_data
    t = sdf_data.procedural_templates()
    assert t["verts"].shape == (3, 192, 3) and t["faces"].shape == (3, 384, 3) and t["n_faces"].tolist() == [320, 384, 192]
    for i, n in enumerate(t["n_faces"].tolist()):
        assert int(t["faces"][i, :n].min()) >= 0 and bool((t["faces"][i, n:] == -1).all())


def test_the_dataset_yields_labels_and_no_points():
    from hoisdf_amd.config import Config
    from hoisdf_amd.engine import SyntheticMeshSdfDataset
    ins, tg, mt = SyntheticMeshSdfDataset(Config(), 3)[4]
    assert not any("points" in k for k in ins) and "hand_sdf" not in tg and "obj_sdf" not in tg
    assert {"mano_param", "obj_rot", "rel_obj_trans"} <= set(tg) and {"mano_root", "obj_center_cam", "obj_cls"} <= set(mt)
    assert int(mt["obj_cls"]) == 1
