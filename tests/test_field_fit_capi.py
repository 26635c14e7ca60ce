"""CPU: the field-fit entries of the C ABI (include/hoisdf.h "field fit", csrc/field_fit.hip) exist with the header's signatures, agree
with the oracle on the iteration limit, answer their two queries by arithmetic, refuse every malformed call with HOISDF_ERR_INVALID and
a message that names the argument before anything is launched (no GPU here: a launch would fail loudly), return 0 for an empty batch,
and the Python surface is what the documents say and opt-in."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from hoisdf_amd import _lib

INVALID = -1
FAKE = C.c_void_p(0x100000)
ENTRIES = ("hoisdf_field_fit_workspace_bytes", "hoisdf_field_fit_launch_count", "hoisdf_field_fit")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.lib()


def test_the_entries_are_declared_and_exported(lib):
    P, I, F = C.c_void_p, C.c_int, C.c_float
    assert _lib.SIGNATURES["hoisdf_field_fit"] == [P, C.c_long, P, I, P, I, P, P, I, I, F, F, F, I, P, P, P, P, P, P, P, P, C.c_long, P]
    assert _lib._OTHER["hoisdf_field_fit_workspace_bytes"] == ([I], C.c_long)
    assert _lib._OTHER["hoisdf_field_fit_launch_count"] == ([I], I)
    syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(ENTRIES) <= set(re.findall(r"\bT (hoisdf_\w+)", syms))


def test_the_limit_is_the_oracles_and_the_queries_are_arithmetic(lib):
    from hoisdf_amd import field_fit_oracle
    assert _lib.CONSTANTS["FIELD_FIT_MAX_ITERS"] == field_fit_oracle.MAX_ITERS == 64
    for iters in (0, 1, 32, 64):
        assert lib.hoisdf_field_fit_launch_count(iters) == iters + 2
    for bad in (-1, 65):
        assert lib.hoisdf_field_fit_launch_count(bad) == INVALID and f"iters={bad}".encode() in lib.hoisdf_last_error()
    q = lib.hoisdf_field_fit_workspace_bytes
    # per sample, in fp64: c 3, extent, R 9, t 3, lambda, 28 sums, the trial pose 12, the start cost; and six 32-bit words
    least = (3 + 1 + 9 + 3 + 1 + 28 + 12 + 1) * 8 + 6 * 4
    assert q(0) == 0 and q(1) % 256 == 0 and least <= q(1) <= least + 256
    assert 22 * least <= q(22) <= 22 * least + 256 and q(44) > q(22)
    for bad in (-1, 65536):
        assert q(bad) == INVALID and f"B={bad}".encode() in lib.hoisdf_last_error()


def test_field_fit_checks_its_arguments_before_any_launch(lib):
    need = lib.hoisdf_field_fit_workspace_bytes(2)

    def fit(values=FAKE, ld=512, grid=FAKE, n=8, points=FAKE, V=100, n_points=None, pivot=None, B=2, iters=32, huber=0.1, lambda0=1e-3,
            step_tol=1e-7, pct=50, rot=FAKE, trans=FAKE, points_out=FAKE, cost=FAKE, info=FAKE, normal=None, pose64=None, ws=FAKE,
            nws=need):
        return lib.hoisdf_field_fit(values, ld, grid, n, points, V, n_points, pivot, B, iters, huber, lambda0, step_tol, pct, rot, trans,
                                    points_out, cost, info, normal, pose64, ws, nws, None)

    for k in ("values", "grid", "points", "rot", "trans", "points_out", "cost", "info"):
        assert fit(**{k: None}) == INVALID and b"null" in lib.hoisdf_last_error() and k.encode() in lib.hoisdf_last_error(), (k, lib.hoisdf_last_error())
    assert fit(ws=None) == INVALID and b"null" in lib.hoisdf_last_error() and b"workspace" in lib.hoisdf_last_error()
    for kw, what in ((dict(n=1), b"n=1"), (dict(n=129, ld=129 ** 3), b"n=129"), (dict(iters=-1), b"iters=-1"), (dict(iters=65), b"iters=65"),
                     (dict(ld=511), b"ld=511"), (dict(ld=0), b"ld=0"), (dict(huber=0.0), b"huber=0"), (dict(huber=-0.1), b"huber=-0.1"),
                     (dict(huber=float("nan")), b"huber"), (dict(lambda0=-1.0), b"lambda0=-1"), (dict(step_tol=-1.0), b"step_tol=-1"),
                     (dict(pct=101), b"min_used_percent=101"), (dict(V=-1), b"V=-1"), (dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"),
                     (dict(nws=need - 1), b"workspace"), (dict(nws=0), b"workspace"), (dict(ws=C.c_void_p(0x100004)), b"aligned")):
        assert fit(**kw) == INVALID and what in lib.hoisdf_last_error(), (kw, lib.hoisdf_last_error())
    assert fit(B=0, values=None, grid=None, points=None, rot=None, trans=None, points_out=None, cost=None, info=None, ws=None, nws=0) == 0


def test_python_surface_and_the_documents():
    from hoisdf_amd import field_fit_oracle, ops, ops_mesh, refine
    assert ops.field_fit is ops_mesh.field_fit
    sig = inspect.signature(ops.field_fit).parameters
    assert list(sig) == ["values", "grid", "n", "points", "n_points", "pivot", "iters", "huber", "lambda0", "step_tol", "min_used_percent",
                         "want"]
    assert [sig[k].default for k in list(sig)[4:]] == [None, None, 32, 0.1, 1e-3, 1e-7, 50, ()]
    oracle = inspect.signature(field_fit_oracle.fit).parameters
    for k in ("iters", "huber", "lambda0", "step_tol", "min_used_percent"):
        assert sig[k].default == oracle[k].default, k
    assert callable(refine.fit_pair) and callable(refine.fit_in_camera_frame)
    assert list(inspect.signature(refine.fit_in_camera_frame).parameters)[:6] == ["values", "grid", "n", "points_cam", "centre", "scale"]
    assert "not in the tree" not in field_fit_oracle.__doc__ and "one-launch" not in field_fit_oracle.__doc__
    text = " ".join(re.sub(r"^ \*", " ", open(_lib.HEADER_PATH).read(), flags=re.M).split())      # comment lines joined
    for phrase in ("x = R (p - c) + c + t", "J = [g, r x g]", "lambda <- max(lambda / 10, 1e-9)", "no kernel has a barrier inside a loop",
                   "((wave 0 + wave 1) + wave 2) + wave 3", "each rounded once from fp64", "iters + 2 launches"):
        assert phrase in text, phrase
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    makefile = open(os.path.join(root, "hoisdf_amd", "csrc", "Makefile")).read()
    assert "field_fit.hip" in re.search(r"^SRCS = (.*)$", makefile, re.M)[1]
    src = open(os.path.join(root, "hoisdf_amd", "csrc", "field_fit.hip")).read()
    assert "#pragma clang fp contract(off)" in src, "the Makefile builds with -ffp-contract=on"


def test_refinement_is_opt_in(monkeypatch):
    import torch
    from hoisdf_amd import metrics, refine
    from hoisdf_amd.config import Config
    monkeypatch.delenv("HOISDF_REFINE", raising=False)
    c = Config()
    assert c.eval_refine is False and c.refine_pad_cells == 4 and c.refine_grid is None and c.refine_iters == 32
    assert not refine.enabled(c)
    monkeypatch.setenv("HOISDF_REFINE", "1")
    assert refine.enabled(Config())
    monkeypatch.delenv("HOISDF_REFINE")
    c.eval_refine = True
    assert refine.enabled(c)
    ev = inspect.signature(metrics.Evaluator.__init__).parameters
    assert ev["refine"].default is False and list(ev)[-2:] == ["refine", "field"], "``field`` stays the last one (tests/test_isosurf_capi.py)"
    with pytest.raises(ValueError, match="template_faces"):
        metrics.Evaluator(c, torch.zeros(2, 8, 3), refine=True)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "--refine" in open(os.path.join(root, "test.py")).read()
