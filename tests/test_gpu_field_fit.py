"""GPU: csrc/field_fit.hip (hoisdf_field_fit, ops.field_fit, refine.py) against hoisdf_amd/field_fit_oracle.py, the numpy float64
statement of the rules.  One batch of eight samples that stop after 5 to 32 rounds: the four box cases of the oracle's own test,
case 1 shifted so that points start outside the grid, its first three points (the rejected-step path; 297 NaN rows beyond the count),
a sphere (the rotation is unobservable: 19 rejections, stopped by ``iters``) and a sample wholly outside.  The sums of the start
pose are products, sums and divisions in one order: compared BIT FOR BIT.  After the first step sqrt and sin may differ in the last
place: the fp64 pose and the costs within 1e-12 (the bar tests/test_field_fit_oracle.py holds between two summation orders), every
f32 output within one f32 spacing of the oracle's value rounded to f32, ``info`` identical - the cases keep clear of rounding-level
branches, which the oracle's tests and tests/test_field_fit_rules_host.py assert."""
import os
import subprocess

import numpy as np
import pytest
import torch

from hoisdf_amd import field_fit_oracle as F
from hoisdf_amd import ops, refine

pytestmark = pytest.mark.gpu
N, V = F.BOX_N, 300
COUNTS = [300, 300, 300, 300, 300, 3, 300, 300]
NAMES = ["box0", "box1", "box2", "box3", "shifted", "three", "sphere", "outside"]


def _sphere_points():
    d = np.random.default_rng(2).normal(size=(300, 3))
    return (0.3 * d / np.linalg.norm(d, axis=1, keepdims=True) + [0.06, -0.04, 0.05]).astype(np.float32)


@pytest.fixture(scope="module")
def batch():
    """-> values (8, n^3), grid (8, 8), points (8, 300, 3) float32 numpy, and the oracle's result per sample (computed once)"""
    box, ball = F.box_field(), F.sphere_field()
    p = [F.box_case(k)["points"] for k in range(4)]
    three = np.full((V, 3), np.nan, np.float32)
    three[:3] = p[1][:3]
    points = np.stack(p + [p[1] + np.float32([0.4, 0, 0]), three, _sphere_points(), p[0] + np.float32(5.0)])
    values = np.stack([box] * 6 + [ball, box])
    grid = np.stack([F.BOX_GRID] * 8)
    refs = [F.fit(values[b], grid[b], N, points[b], n_points=COUNTS[b]) for b in range(8)]
    assert all(F.clear_of_rounding(r) for r in refs)
    assert [r["info"].tolist() for r in refs[4:]] == [[267, 300, 8, 8], [3, 3, 10, 6], [300, 300, 32, 13], [0, 0, 0, 0]]
    return values, grid, points, refs


def _fit(values, grid, points, counts, sel=slice(None), **kw):
    dev = "cuda"
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev)
    nv = None if counts is None else torch.tensor(counts, dtype=torch.int32)[sel].to(dev)
    kw.setdefault("want", ("normal", "pose64"))
    return {k: v.cpu().numpy() for k, v in ops.field_fit(t(values), t(grid), N, t(points), n_points=nv, **kw).items()}


@pytest.fixture(scope="module")
def result(batch):
    values, grid, points, _ = batch
    return _fit(values, grid, points, COUNTS)


def _within_one_spacing(got, ref64):
    want = np.asarray(ref64, np.float64).astype(np.float32)
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64))


def test_the_batch_against_the_oracle(batch, result):
    _, _, _, refs = batch
    r = result
    assert r["info"].dtype == np.int32 and r["cost"].dtype == np.float64 and r["rot"].shape == (8, 3, 3) and r["points_out"].shape == (8, V, 3)
    for b, ref in enumerate(refs):
        normal = np.concatenate([ref["normal"], ref["normal_abs"]])
        pose = np.concatenate([ref["rot"].ravel(), ref["trans"]])
        dp, dc = np.abs(r["pose64"][b] - pose).max(), np.abs(r["cost"][b] - ref["cost"]).max()
        print(f"{NAMES[b]}: info {r['info'][b].tolist()} (oracle {ref['info'].tolist()}, stopped by {ref['stopped_by']}), normal equal bits "
              f"{np.array_equal(r['normal'][b], normal)}, pose64 {dp:.1e}, cost {dc:.1e}")
        assert np.array_equal(r["normal"][b], normal), (NAMES[b], np.abs(r["normal"][b] - normal).max())
        assert r["info"][b].tolist() == ref["info"].tolist(), NAMES[b]
        assert dp < 1e-12 and dc < 1e-12, (NAMES[b], dp, dc)
        nv = COUNTS[b]
        assert _within_one_spacing(r["rot"][b], ref["rot"]) and _within_one_spacing(r["trans"][b], ref["trans"]), NAMES[b]
        assert _within_one_spacing(r["points_out"][b, :nv], ref["points_out"]), NAMES[b]
        assert not r["points_out"][b, nv:].any(), "rows beyond the count are not written"
    assert r["info"][:, 2].min() == 0 and sorted(r["info"][:7, 2].tolist())[0] == 5 and r["info"][:, 2].max() == 32
    assert (r["cost"][:, 1] <= r["cost"][:, 0]).all()


def test_each_sample_of_the_batch_equals_the_sample_run_alone_and_two_calls_give_the_same_bits(batch, result):
    """the samples stop after 5 to 32 rounds: a workgroup that returns early must not disturb one that goes on"""
    values, grid, points, _ = batch
    again = _fit(values, grid, points, COUNTS)
    for k in result:
        assert np.array_equal(result[k], again[k], equal_nan=True), k
    for b in range(8):
        alone = _fit(values, grid, points, COUNTS, sel=slice(b, b + 1))
        for k in result:
            assert np.array_equal(result[k][b], alone[k][0], equal_nan=True), (NAMES[b], k)


def test_iters_pivot_and_defaults(batch, result):
    values, grid, points, refs = batch
    one = slice(0, 1)
    zero = _fit(values, grid, points, None, sel=one, iters=0)
    assert zero["info"][0].tolist() == [300, 300, 0, 0] and zero["cost"][0, 0] == zero["cost"][0, 1] > 0
    assert np.array_equal(zero["rot"][0], np.eye(3, dtype=np.float32)) and not zero["trans"].any()
    assert zero["cost"][0, 0] == refs[0]["cost"][0]
    three = _fit(values, grid, points, None, sel=one, iters=3)
    ref3 = F.fit(values[0], grid[0], N, points[0], iters=3)
    assert ref3["stopped_by"] == "iters" and three["info"][0].tolist() == ref3["info"].tolist() == [300, 300, 3, 3]
    assert np.abs(three["pose64"][0] - np.concatenate([ref3["rot"].ravel(), ref3["trans"]])).max() < 1e-12
    # a given pivot moves R, t - not the points (1e-5: the bar of the oracle's own test)
    pv = np.float32([[0.1, -0.2, 0.05]])
    given = _fit(values, grid, points, None, sel=one, pivot=torch.from_numpy(pv).cuda())
    refp = F.fit(values[0], grid[0], N, points[0], pivot=pv[0])
    assert given["info"][0].tolist() == refp["info"].tolist()
    assert np.abs(given["pose64"][0] - np.concatenate([refp["rot"].ravel(), refp["trans"]])).max() < 1e-12
    assert np.abs(given["trans"][0] - result["trans"][0]).max() > 1e-3
    assert np.abs(given["points_out"][0].astype(np.float64) - result["points_out"][0]).max() < 1e-5
    # no counts: all V rows; no optional outputs unless asked
    plain = ops.field_fit(*(torch.from_numpy(a[:1]).cuda() for a in (values, grid)), N, torch.from_numpy(points[:1]).cuda())
    assert set(plain) == {"rot", "trans", "points_out", "cost", "info"} and np.array_equal(plain["rot"].cpu().numpy(), result["rot"][:1])
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.field_fit(torch.from_numpy(values[:1]), torch.from_numpy(grid[:1]), N, torch.from_numpy(points[:1]))
    with pytest.raises(ValueError, match="want"):
        ops.field_fit(*(torch.from_numpy(a[:1]).cuda() for a in (values, grid)), N, torch.from_numpy(points[:1]).cuda(), want=("normals",))


def test_fit_in_camera_frame_is_the_plain_call_mapped_back(batch):
    values, grid, points, _ = batch
    sel = slice(0, 5)
    dev = "cuda"
    v, g = torch.from_numpy(values[sel]).to(dev), torch.from_numpy(grid[sel].copy()).to(dev)
    scale = 6.2
    centre = torch.tensor([[0.03, -0.02, 0.71], [0.0, 0.0, 0.6], [-0.05, 0.04, 0.8], [0.01, 0.01, 0.55], [0.02, -0.06, 0.9]], device=dev)
    cam = torch.from_numpy(points[sel]).to(dev) / scale + centre[:, None]
    got = refine.fit_in_camera_frame(v, g, N, cam, centre, scale, want=("pose64",))
    field_pts = (cam - centre[:, None]) * scale                                   # what the helper hands to the fit, bit for bit
    plain = ops.field_fit(v, g, N, field_pts, want=("pose64",))
    assert torch.equal(got["rot"], plain["rot"]) and torch.equal(got["info"], plain["info"]) and torch.equal(got["cost"], plain["cost"])
    assert torch.equal(got["trans_field"], plain["trans"])
    back = plain["points_out"].double().cpu().numpy() / scale + centre.double().cpu().numpy()[:, None]
    assert _within_one_spacing(got["points_out"].cpu().numpy(), back)
    assert _within_one_spacing(got["trans"].cpu().numpy(), plain["trans"].double().cpu().numpy() / scale)
    # the fit brings the camera-frame points back to where the field's frame says they belong
    moved = float((got["points_out"] - cam).norm(dim=2).mean())
    assert 0.05 / scale / 2 < moved < 1.0 / scale, moved


def test_c_host_field_fit(tmp_path):
    """A plain C host (tests/c/test_field_fit_host.c: tanh of a sphere's distance sampled on the host, points of the sphere moved by a
    known translation) gets the translation back to a quarter of a cell and a sane info"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_field_fit_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_field_fit_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    res = subprocess.run([exe, "33"], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0 and "c host field fit ok" in res.stdout, res.stdout + res.stderr


# ---- the opt-in outputs of the eval forward and the Evaluator's Refined block ---------------------------------------------------------
def test_eval_forward_refines_only_when_asked(monkeypatch, tmp_path):
    """the synthetic evaluation of tests/test_gpu_isosurf.py (ResNet-18, 96 + 32 points, B = 2, untrained) with the switch off and on:
    off, every output tensor and results.txt are what they are without the feature; on, the ten new outputs are there and finite,
    no sample tried more than ``iters`` steps and no cost rose.  Untrained weights: plumbing only, no claim about the metrics."""
    from hoisdf_amd import testing as T
    from hoisdf_amd.config import Config
    from hoisdf_amd.engine import Tester
    from hoisdf_amd.nets import mano as MANO
    from hoisdf_amd.sdf_data import procedural_templates
    monkeypatch.delenv("HOISDF_REFINE", raising=False)
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = 96, 32
    c.field_grid, c.refine_iters = 12, 8
    assert c.eval_refine is False and c.refine_pad_cells == 4
    torch.manual_seed(0)
    tester = Tester(c, torch.device("cuda", 0))
    ml = MANO.ManoLayer(MANO.synthetic_assets(0)).cuda()
    inputs, targets, meta = T.synthetic_batch(2, 96, 32, seed=5)
    tmpl = procedural_templates()
    cls = torch.tensor([1, 2])
    meta["obj_cls"] = cls
    verts = tmpl["verts"].cuda()
    tensors = lambda out: {k: v.detach().clone() for k, v in out.items() if torch.is_tensor(v)}
    # What is compared is everything BEHIND the image encoder: its convolutions are outside the HIP scope and not run-to-run
    # reproducible on every MIOpen build (tests/test_gpu_deterministic.py), so its first output is kept and handed out again, and
    # the hot path runs in its order-fixed mode.  Then the eval forward repeats its bits and every comparison below is bitwise.
    dec, memo = tester.model.decoder_net, []
    real_forward = dec.forward

    def frozen(*a, **kw):
        if not memo:
            memo.append(real_forward(*a, **kw))
        return memo[0]

    dec.forward = frozen
    ops.set_deterministic(True)
    try:
        _refine_on_and_off(monkeypatch, tmp_path, c, tester, ml, inputs, targets, meta, tmpl, cls, verts, tensors)
    finally:
        ops.set_deterministic(False)
        del dec.forward
        c.native_infer, c.eval_refine = False, False


def _refine_on_and_off(monkeypatch, tmp_path, c, tester, ml, inputs, targets, meta, tmpl, cls, verts, tensors):
    import re
    from hoisdf_amd import metrics as M
    from hoisdf_amd.render import PairSource
    off = tensors(tester.predict(inputs, targets, meta, mano_layer=ml))
    off2 = tensors(tester.predict(inputs, targets, meta, mano_layer=ml))
    off3 = tensors(tester.predict(inputs, targets, meta, mano_layer=ml))
    ev_on = M.Evaluator(c, verts, native=True, refine=True, template_faces=tmpl, hand_faces=ml.th_faces)
    c.eval_refine = True
    with pytest.raises(RuntimeError, match="set_refine_source"):
        tester.predict(inputs, targets, meta, mano_layer=ml)
    tester.model.set_refine_source(PairSource(c, verts, tmpl, ml.th_faces))
    on = tensors(tester.predict(inputs, targets, meta, mano_layer=ml))
    c.eval_refine = False
    after = tensors(tester.predict(inputs, targets, meta, mano_layer=ml))
    added = {f"refined_{k}_verts" for k in ("hand", "obj")} | {f"refine_{k}_{w}" for k in ("hand", "obj") for w in ("rot", "trans", "cost", "info")}
    assert not any(k.startswith("refine") for k in off) and set(on) == set(off) | added and set(after) == set(off)
    # the option adds no arithmetic to any other output: every key that the eval forward itself repeats bit for bit over three
    # runs (with the encoder's output held and the order-fixed mode: all of them are expected to) and every integer key is
    # compared bit for bit; a key the forward does not repeat could only be held to 1e-5 of its scale
    repeated = {k for k in off if torch.equal(off2[k], off[k]) and torch.equal(off3[k], off[k])}
    print(f"the eval forward repeats the bits of {len(repeated)} of {len(off)} outputs; not of", sorted(set(off) - repeated))
    assert {"mano_mesh_out", "hand_joints_out", "obj_rot_out", "obj_trans_out"} <= repeated, "the model's own outputs must be compared bit for bit"
    for other in (on, after):
        for k in off:
            if k in repeated or not off[k].is_floating_point():
                assert torch.equal(other[k], off[k]), k
            else:
                assert float((other[k] - off[k]).abs().max()) <= 1e-5 * max(float(off[k].abs().max()), 1e-30), k
    assert on["refined_hand_verts"].shape == (2, 778, 3) and on["refined_obj_verts"].shape == (2,) + tuple(verts.shape[1:])
    for kind in ("hand", "obj"):
        info, cost = on[f"refine_{kind}_info"], on[f"refine_{kind}_cost"]
        print(kind, "info", info.tolist(), "cost", cost.tolist())
        assert on[f"refine_{kind}_rot"].shape == (2, 3, 3) and on[f"refine_{kind}_trans"].shape == (2, 3) and info.shape == (2, 4)
        assert all(bool(torch.isfinite(on[k]).all()) for k in (f"refined_{kind}_verts", f"refine_{kind}_rot", f"refine_{kind}_trans", f"refine_{kind}_cost"))
        assert int(info[:, 2].max()) <= 8 and bool((info[:, 3] <= info[:, 2]).all()) and bool((cost[:, 1] <= cost[:, 0]).all())
    # results.txt: byte-identical with the option off; with it on, the file of the same outputs without the option, then one block
    files = {}
    for name, ev, out in (("plain", M.Evaluator(c, verts, native=True), off),
                          ("off", M.Evaluator(c, verts, native=True, refine=False, template_faces=tmpl, hand_faces=ml.th_faces), off),
                          ("plain_on", M.Evaluator(c, verts, native=True), on),
                          ("on", ev_on, on)):
        ev.feed(out, targets, meta, cls)
        files[name] = open(ev.write(str(tmp_path / name)), "rb").read()
    assert files["off"] == files["plain"] and b"Refined" not in files["plain"] and b"Refined" not in files["plain_on"]
    assert files["on"].startswith(files["plain_on"]) and len(files["on"]) > len(files["plain_on"])
    block = files["on"][len(files["plain_on"]):].decode()
    print(block)
    line = r"%s_vertex_error=[\d.]+ cm -> [\d.]+ cm, %s_cost=[\d.]+ -> [\d.]+, %s_steps=[\d.]+, %s_left_out=[\d.]+\n"
    assert re.fullmatch("Refined:\n" + line % (("hand",) * 4) + line % (("obj",) * 4), block), block
    with pytest.raises(ValueError, match="template_faces"):
        M.Evaluator(c, verts, native=True, refine=True)
    c.native_infer, c.eval_refine = True, True
    with pytest.raises(ValueError, match="one-call"):
        tester.predict(inputs, targets, meta, mano_layer=ml)
