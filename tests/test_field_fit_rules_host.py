"""CPU: hoisdf_amd/csrc/field_fit_rules.h - the text the field-fit kernels compile - held to hoisdf_amd/field_fit_oracle.py without a
GPU.  tests/c/field_fit_rules_host.cpp includes the header with its qualifiers defined away (g++ -O2 -ffp-contract=off) and runs the
whole fit in the 256-lane order with plain loops on a case this test writes to a file.  Required: the sums of the start pose
(``normal`` / ``normal_abs``) equal the oracle's bit for bit (products, sums and divisions only); ``info`` and the accept / reject
sequence are identical; ``rot``, ``trans`` and ``points_out`` agree within 1e-12 - the bar tests/test_field_fit_oracle.py holds between
the two summation orders (sqrt and sin may differ in the last place, hence no bit claim after the first step).  Every case is
asserted ``clear_of_rounding`` here, so none of this hinges on a rounding-level branch (a case that is not is replaced, the condition
stays)."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from hoisdf_amd import field_fit_oracle as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GXX = shutil.which("g++")
DEFAULTS = dict(iters=32, huber=0.1, lambda0=1e-3, step_tol=1e-7, min_used_percent=50)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if GXX is None:
        pytest.skip("needs g++")
    out = str(tmp_path_factory.mktemp("ff_host") / "field_fit_rules_host")
    r = subprocess.run([GXX, "-O2", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "hoisdf_amd", "csrc"),
                        os.path.join(ROOT, "tests", "c", "field_fit_rules_host.cpp"), "-o", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _sphere_points():
    d = np.random.default_rng(2).normal(size=(300, 3))
    return (0.3 * d / np.linalg.norm(d, axis=1, keepdims=True) + [0.06, -0.04, 0.05]).astype(np.float32)


def _cases():
    box, ball = F.box_field(), F.sphere_field()
    p = [F.box_case(k)["points"] for k in range(4)]
    holed = box.copy()                                               # the node below the first point of case 2: its cell is skipped
    ix, iy, iz = np.floor((p[2][0].astype(np.float64) - F.BOX_GRID[:3]) / F.BOX_GRID[3:6]).astype(int)
    holed[ix + F.BOX_N * (iy + F.BOX_N * iz)] = np.inf
    tail = np.concatenate([p[0], np.full((20, 3), np.nan, np.float32)])
    cases = [(f"box{k}", box, p[k], {}, None) for k in range(4)]
    cases += [("shifted", box, p[1] + np.float32([0.4, 0, 0]), {}, [267, 300, 8, 8]),
              ("three points", box, p[1][:3], {}, [3, 3, 10, 6]),
              ("one point", box, p[1][:1], {}, None),
              ("sphere", ball, _sphere_points(), {}, [300, 300, 32, 13]),
              ("sphere 64", ball, _sphere_points(), dict(iters=64), [300, 300, 39, 16]),
              ("iters 0", box, p[0], dict(iters=0), [300, 300, 0, 0]),
              ("iters 3", box, p[0], dict(iters=3), None),
              ("pivot", box, p[0], dict(pivot=np.float32([0.1, -0.2, 0.05])), None),
              ("nan tail", box, tail, dict(n_points=300), None),
              ("one node not finite", holed, p[2], {}, None),
              ("outside", box, p[0] + np.float32(5.0), {}, [0, 0, 0, 0])]
    return cases


CASES = _cases()


def _run(exe, tmp_path, values, points, kw):
    par = dict(DEFAULTS)
    par.update({k: v for k, v in kw.items() if k in DEFAULTS})
    pivot, n_points = kw.get("pivot"), kw.get("n_points")
    path = str(tmp_path / "case.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", F.BOX_N, len(points), -1 if n_points is None else n_points, int(pivot is not None), par["iters"],
                            par["min_used_percent"]))
        f.write(np.float32([par["huber"], par["lambda0"], par["step_tol"]]).tobytes())
        f.write(np.asarray(F.BOX_GRID, "<f4").tobytes())
        f.write(np.asarray(np.zeros(3) if pivot is None else pivot, "<f4").tobytes())
        f.write(np.asarray(values, "<f4").tobytes())
        f.write(np.ascontiguousarray(points, "<f4").tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        name, _, rest = line.partition(" ")
        if name in ("info", "status"):
            out[name] = [int(x) for x in rest.split()]
        elif name == "decisions":
            out[name] = [c == "1" for c in rest.strip("[]")]
        else:
            out[name] = np.array([float.fromhex(x) for x in rest.split()])
    return out


@pytest.mark.parametrize("name,values,points,kw,info", CASES, ids=[c[0] for c in CASES])
def test_the_rules_header_runs_the_fit_the_oracle_runs(exe, tmp_path, name, values, points, kw, info):
    ref = F.fit(values, F.BOX_GRID, F.BOX_N, points, **kw)
    assert F.clear_of_rounding(ref), "the case itself must keep clear of rounding-level branches"
    if info is not None:
        assert ref["info"].tolist() == info, ref["info"]
    got = _run(exe, tmp_path, values, points, kw)
    print(name, "info", got["info"], "stopped by", ref["stopped_by"], "decisions", "".join("ar"[not d] for d in got["decisions"]))
    assert np.array_equal(got["normal"][:28], ref["normal"]) and np.array_equal(got["normal"][28:], ref["normal_abs"]), \
        np.abs(got["normal"][:28] - ref["normal"]).max()
    assert got["info"] == ref["info"].tolist()
    assert got["decisions"] == [d[2] for d in ref["decisions"]]
    assert got["status"][0] == {"iters": 1, "step": 2, "lambda": 3, "none": 4}[ref["stopped_by"]]
    diffs = [np.abs(got["rot"].reshape(3, 3) - ref["rot"]).max(), np.abs(got["trans"] - ref["trans"]).max(),
             np.abs(got["cost"] - ref["cost"]).max()]
    pts = got["points"].reshape(-1, 3)
    assert pts.shape == ref["points_out"].shape
    if pts.size:
        diffs.append(np.abs(pts - ref["points_out"]).max())
    print(name, "rot / trans / cost / points against the oracle:", ["%.1e" % d for d in diffs])
    assert max(diffs) < 1e-12, diffs


def test_the_listed_cases_take_the_paths_they_are_there_for():
    """the rejected-step path, a stop by `iters` with rejections, a stop by step after 64 are allowed, points that start outside"""
    box, ball = F.box_field(), F.sphere_field()
    three = F.fit(box, F.BOX_GRID, F.BOX_N, F.box_case(1)["points"][:3])
    assert three["info"].tolist() == [3, 3, 10, 6] and not all(d[2] for d in three["decisions"])
    sphere = F.fit(ball, F.BOX_GRID, F.BOX_N, _sphere_points())
    assert sphere["stopped_by"] == "iters" and sphere["info"][2] - sphere["info"][3] == 19
    more = F.fit(ball, F.BOX_GRID, F.BOX_N, _sphere_points(), iters=64)
    assert more["stopped_by"] == "step" and more["info"].tolist()[2:] == [39, 16]
    assert F.fit(box, F.BOX_GRID, F.BOX_N, F.box_case(0)["points"], iters=3)["stopped_by"] == "iters"
    holed = next(c for c in CASES if c[0] == "one node not finite")
    assert not np.isfinite(holed[1]).all() and 0 < F.fit(holed[1], F.BOX_GRID, F.BOX_N, holed[2])["info"][0] < 300
