"""-m gpu: SDF supervision from meshes (csrc/mesh_sdf.hip: hoisdf_mesh_prepare / _sample_points / _sdf / _sdf_rows; ops.mesh_sdf,
ops.mesh_sample_points, ops.mesh_sdf_rows, sdf_data.MeshSdfSource, Trainer(sdf_source=...)) against the fp64 numpy restatement
hoisdf_amd/mesh_sdf_oracle.py on procedural meshes at hand size and camera depth.

The bars.  Distance: | |sdf| - |sdf64| | <= 5e-7 m on every point - one fp32 ulp at 0.7 m is 6e-8 and 5e-7 leaves about 5 x over
an fp32 evaluation in camera coordinates for contraction and summation order (the oracle itself run in fp32 on these points is
2.0e-8 m off its fp64 run).  Sign: equal to fp64 wherever
|sdf64| >= 1e-5 m (closed meshes; at most 1 % of the points may lie below) or |winding64 - 0.5| > 0.05 (open mesh; at most 1 %
excluded).  Nearest face: indices are NOT compared (ties on shared edges); the fp64 distance to the reported face is within 5e-7 m
of the fp64 minimum.  Labels: compared where the oracle's set of defensible labels (faces within 1e-6 m of the minimum, corners
within 1e-3 of the largest weight) is a singleton; at most 1 % ambiguous."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from hoisdf_amd import mesh_sdf_oracle as O
from hoisdf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR = 5e-7
SCALE, CENTRE = 0.08, np.array([0.03, -0.02, 0.7])
TILE = 128                                                    # HOISDF_MESH_TILE (asserted below)


def unit_mesh(name):
    if name == "torus":
        return O.torus(16, 12)
    v, f = O.icosphere(2)
    if name == "open":                                        # the cap around -z removed: 260 faces, a hole
        f = f[v[f].mean(1)[:, 2] >= -0.6]
    return v, f


def sector_labels(v):
    return (np.floor((np.arctan2(v[:, 1], v[:, 0]) + np.pi) / (2 * np.pi) * 6).astype(np.int32)) % 6


def make_points(v, f, seed):
    """3000 area-weighted surface points pushed along the face normal by +-10^U(-4,-2) / N(0, 0.005) / N(0, 0.02) (at least 1e-4 in
    size), 1000 uniform in a +-0.15 m box, 100 points 2e-4 .. 1e-3 m off vertices and edge midpoints; float32 values"""
    r = np.random.default_rng(seed)
    m = O.prepare(v, f, recentre=False)
    tri = m["tri"]
    pick = r.choice(len(f), 3000, p=m["area"] / m["area"].sum())
    s, u2 = np.sqrt(r.random(3000)), r.random(3000)
    w = np.stack([1 - s, s * (1 - u2), s * u2], 1)
    surf = (tri[pick] * w[:, :, None]).sum(1)
    n = np.cross(tri[pick, 1] - tri[pick, 0], tri[pick, 2] - tri[pick, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    off = np.concatenate([r.choice([-1.0, 1.0], 1000) * 10 ** r.uniform(-4, -2, 1000), r.normal(0, 0.005, 1000), r.normal(0, 0.02, 1000)])
    off = np.where(np.abs(off) < 1e-4, np.where(off < 0, -1e-4, 1e-4), off)
    box = r.uniform(-0.15, 0.15, (1000, 3)) + CENTRE
    e = f[r.integers(0, len(f), 50)]
    anchors = np.concatenate([v[r.integers(0, len(v), 50)], 0.5 * (v[e[:, 0]] + v[e[:, 1]])])
    d = r.normal(size=(100, 3))
    d *= (r.uniform(2e-4, 1e-3, 100) / np.linalg.norm(d, axis=1))[:, None]
    return np.concatenate([surf + n * off[:, None], box, anchors + d]).astype(np.float32)


_CASES = {}


def case(name):
    """mesh `name` at hand size and camera depth, its 4100 points and the fp64 oracle's answer on them: computed once, never changed"""
    if name not in _CASES:
        assert ops._lib.CONSTANTS["MESH_TILE"] == TILE
        v, f = unit_mesh(name)
        lab = sector_labels(v)
        v32 = (v * SCALE + CENTRE).astype(np.float32)
        pts = make_points(v32.astype(np.float64), f, seed={"icosphere": 1, "torus": 2, "open": 3}[name])
        ref = O.mesh_sdf(pts, v32, f, lab, label_sets=True)
        for a in ref.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[name] = dict(verts=v32, faces=f, labels=lab, points=pts, ref=ref)
    return _CASES[name]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(c, n=None, **kw):
    pts = c["points"][:n]
    out = ops.mesh_sdf(gpu(pts)[None], gpu(c["verts"])[None], gpu(c["faces"]), vert_label=gpu(c["labels"]), extras=True, **kw)
    torch.cuda.synchronize()
    return {k: v[0].cpu().numpy() for k, v in out.items()}


def check_distance(got_sdf, ref, what):
    err = np.abs(np.abs(got_sdf.astype(np.float64)) - ref["dist"][:len(got_sdf)])
    print(f"{what}: distance: max | |sdf| - |sdf64| | = {err.max():.3e} m over {len(err)} points")
    assert err.max() <= BAR, f"{what}: {err.max():.3e} m > {BAR:.0e}"


@pytest.mark.parametrize("name", ["icosphere", "torus", "open"])
def test_distance_sign_face_and_label(name):
    c = case(name)
    ref, n = c["ref"], len(c["points"])
    assert len(c["faces"]) == {"icosphere": 320, "torus": 384, "open": 260}[name] and n == 4100
    got = run(c)
    check_distance(got["sdf"], ref, name)
    # sign
    if name == "open":
        judged = np.abs(ref["winding"] - 0.5) > 0.05
        rule = "|winding64 - 0.5| > 0.05"
    else:
        judged = ref["dist"] >= 1e-5
        rule = "|sdf64| >= 1e-5 m"
        assert np.abs(ref["winding"] - np.round(ref["winding"])).max() < 1e-9
    wrong = int(((got["sdf"] < 0) != (ref["sdf"] < 0))[judged].sum())
    print(f"{name}: sign: {100 * (1 - judged.mean()):.2f} % of the points outside the rule ({rule}), {wrong} mismatches; "
          f"{int((ref['sdf'] < 0).sum())} inside")
    assert (1 - judged.mean()) <= 0.01 and wrong == 0
    assert (ref["sdf"] < 0).sum() > 300 and (ref["sdf"] > 0).sum() > 300
    werr = np.abs(got["winding"] - ref["winding"]).max()
    print(f"{name}: winding: max abs err {werr:.2e}")
    assert werr < 1e-3                                              # (320 .. 384 fp32 angles of <= 2 pi each; the sign rule needs 0.05)
    # nearest face: the fp64 distance to the face the kernel names is the fp64 minimum
    assert got["face"].min() >= 0 and got["face"].max() < len(c["faces"])
    d_named = O.distance_to_face(c["points"], c["verts"], c["faces"], got["face"])
    gap = (d_named - ref["dist"]).max()
    print(f"{name}: nearest face: fp64 distance to the named face exceeds the fp64 minimum by at most {gap:.3e} m; "
          f"{int((got['face'] != ref['face']).sum())} indices differ from the fp64 argmin")
    assert gap <= BAR
    bsum = np.abs(got["bary"].sum(1) - 1).max()
    assert bsum < 1e-5 and got["bary"].min() > -1e-5
    # labels
    single = np.array([len(s) == 1 for s in ref["label_sets"]])
    want = np.array([next(iter(s)) if len(s) == 1 else -1 for s in ref["label_sets"]])
    bad = int((got["label"] != want)[single].sum())
    print(f"{name}: labels: {100 * (1 - single.mean()):.2f} % ambiguous, {bad} mismatches among the rest")
    assert (1 - single.mean()) <= 0.01 and bad == 0
    assert all(int(l) in s for l, s in zip(got["label"], ref["label_sets"]))


@pytest.mark.parametrize("F", [1, TILE + 1, 320])
def test_point_and_face_counts_that_can_go_wrong(F):
    """N = 1, 257, 1000 (one thread, one block + 1, several blocks) x F = 1, one LDS tile + 1, 320; every point is independent of the
    others, so a shorter call gives the bits of the longer one"""
    c = dict(case("icosphere"))
    c["faces"] = c["faces"][:F]
    ref = O.mesh_sdf(c["points"][:1000], c["verts"], c["faces"], c["labels"])
    outs = {n: run(c, n) for n in (1, 257, 1000)}
    check_distance(outs[1000]["sdf"], ref, f"F={F}")
    judged = np.abs(ref["winding"] - 0.5) > 0.05
    assert not ((outs[1000]["sdf"] < 0) != (ref["sdf"] < 0))[judged].any()
    d_named = O.distance_to_face(c["points"][:1000], c["verts"], c["faces"], outs[1000]["face"])
    assert (d_named - ref["dist"]).max() <= BAR and outs[1000]["face"].max() < F
    for n in (1, 257):
        for k in outs[n]:
            assert outs[n][k].shape[0] == n and np.array_equal(outs[n][k], outs[1000][k][:n]), (n, k)


def test_batch_with_three_face_counts_and_padding_that_must_not_be_read():
    """B = 3, per-sample topology, n_faces = 320 / 384 / 260 under max_faces = 384 (+ 3 rows beyond, for the stride): the padded face rows hold
    indices far outside the mesh; every sample gets the bits of its own single-mesh call"""
    cs = [case(n) for n in ("icosphere", "torus", "open")]
    V, Fm, N = 192, 387, 1000
    verts = np.stack([np.concatenate([c["verts"], np.repeat(c["verts"][:1], V - len(c["verts"]), 0)]) for c in cs])
    faces = np.full((3, Fm, 3), 2 ** 30, np.int32)
    for b, c in enumerate(cs):
        faces[b, :len(c["faces"])] = c["faces"]
    labels = np.stack([np.concatenate([c["labels"], np.zeros(V - len(c["labels"]), np.int32)]) for c in cs])
    pts = np.stack([c["points"][:N] for c in cs])
    nf = [len(c["faces"]) for c in cs]
    assert nf == [320, 384, 260]
    out = ops.mesh_sdf(gpu(pts), gpu(verts), gpu(faces), n_faces=torch.tensor(nf), vert_label=gpu(labels), extras=True)
    torch.cuda.synchronize()
    for b, c in enumerate(cs):
        one = run(c, N)
        for k in one:
            assert np.array_equal(out[k][b].cpu().numpy(), one[k]), (b, k)
        check_distance(out["sdf"][b].cpu().numpy(), c["ref"], f"sample {b}")
    # a count beyond max_faces is clamped, a negative one is an empty mesh: +huge everywhere, no face
    m = ops.PreparedMesh(gpu(verts), gpu(faces[:, :384]), n_faces=torch.tensor([10 ** 6, 384, -5]))
    o = ops.mesh_sdf(gpu(pts), m, extras=True)
    assert bool((o["face"][2] == -1).all()) and bool((o["sdf"][2] > 1e37).all()) and torch.equal(o["sdf"][1], out["sdf"][1])


def test_shared_and_per_sample_topology_agree():
    c = case("torus")
    verts = np.stack([c["verts"], c["verts"] * np.float32(1.25) + np.float32(0.01)])
    pts = gpu(np.stack([c["points"][:700], c["points"][700:1400]]))
    a = ops.mesh_sdf(pts, gpu(verts), gpu(c["faces"]), vert_label=gpu(c["labels"]), extras=True)
    b = ops.mesh_sdf(pts, gpu(verts), gpu(np.stack([c["faces"], c["faces"]])), vert_label=gpu(np.stack([c["labels"]] * 2)), extras=True)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["sdf"][0], a["sdf"][1])
    check_distance(a["sdf"][0].cpu().numpy(), c["ref"], "sample 0 of the shared topology")


def test_an_exactly_degenerate_face_changes_nothing():
    c = case("icosphere")
    base = run(c, 1000)
    d = dict(c)
    extra = np.asarray([[5, 5, 9], [40, 7, 7]], np.int32)
    d["faces"] = np.concatenate([c["faces"][:130], extra, c["faces"][130:]])     # in the second LDS tile
    got = run(d, 1000)
    for k in ("sdf", "bary", "label"):
        assert np.array_equal(got[k], base[k]), k
    # (the angle sum is taken in an order that follows a face's position in the list: the same 320 terms, other roundings)
    assert np.abs(got["winding"] - base["winding"]).max() < 1e-5
    assert np.array_equal(got["face"], np.where(base["face"] >= 130, base["face"] + 2, base["face"]))
    m = ops.PreparedMesh(gpu(d["verts"])[None], gpu(d["faces"]))
    area = m.area[0].cpu().numpy()
    assert area[130] == 0 and area[131] == 0 and (np.delete(area, [130, 131]) > 0).all()
    ref = O.prepare(d["verts"], d["faces"])
    assert np.abs(area - ref["area"]).max() < 1e-6 * ref["area"].max()
    cdf = m.cdf[0].cpu().numpy()
    assert cdf[131] == cdf[129] and np.all(np.diff(cdf) >= 0) and abs(cdf[-1] - ref["cdf"][-1]) < 1e-5 * ref["cdf"][-1]
    box = m.box[0].cpu().numpy()
    assert np.abs(box[:3] - ref["centre"]).max() < 1e-6 and np.abs(box[4:7] - ref["half"]).max() < 1e-6 and box[3] == cdf[-1]


def test_strided_output_into_a_row_block_and_two_calls_bit_identical():
    c = case("torus")
    N = 1000
    pts = gpu(c["points"][:N])[None]
    plain = ops.mesh_sdf(pts, gpu(c["verts"])[None], gpu(c["faces"]))
    again = ops.mesh_sdf(pts, gpu(c["verts"])[None], gpu(c["faces"]))
    rows = torch.full((1, N, 6), -7.0, device=DEV)
    rows[..., :3] = pts
    m = ops.PreparedMesh(gpu(c["verts"])[None], gpu(c["faces"]))
    r3 = ops.mesh_sdf(rows[..., :3], m, out=rows[..., 3])                         # reads columns 0-2 of the block, writes column 3
    assert r3.data_ptr() == rows[..., 3].data_ptr()
    ops.mesh_sdf(rows[..., :3], m, out=rows[..., 4])
    torch.cuda.synchronize()
    assert torch.equal(plain, again)
    assert torch.equal(rows[..., 3], plain) and torch.equal(rows[..., 4], plain)
    assert torch.equal(rows[..., :3], pts) and bool((rows[..., 5] == -7.0).all())
    check_distance(plain[0].cpu().numpy(), c["ref"], "torus, plain call")


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
N_SAMP, SEED = 65536, 20240
_SAMP = {}


def torus_samples():
    if not _SAMP:
        c = case("torus")
        m = ops.PreparedMesh(gpu(c["verts"])[None], gpu(c["faces"]))
        kw = dict(n_points=N_SAMP, uniform_every=16, pad=0.05, with_faces=True)
        _SAMP["on"] = ops.mesh_sample_points(m, sigma=(0.0, 0.0), seed=SEED, **kw)
        _SAMP["on2"] = ops.mesh_sample_points(m, sigma=(0.0, 0.0), seed=SEED, **kw)
        _SAMP["noisy"] = ops.mesh_sample_points(m, sigma=(0.01, 0.01), seed=SEED, **kw)
        _SAMP["other"] = ops.mesh_sample_points(m, sigma=(0.0, 0.0), seed=SEED + 1, **kw)
        _SAMP["mesh"] = m
        torch.cuda.synchronize()
    return _SAMP


def test_sampler_surface_points_and_face_counts():
    c, s = case("torus"), torus_samples()
    pts, face = s["on"][0][0].cpu().numpy(), s["on"][1][0].cpu().numpy()
    kind = O.point_kind(np.arange(N_SAMP), 16)
    assert np.array_equal(face < 0, kind == 2) and int((face < 0).sum()) == N_SAMP // 16     # the uniform kind: exactly the index rule
    near = face >= 0
    d = O.distance_to_face(pts[near], c["verts"], c["faces"], face[near])
    print(f"sampler, sigma 0: {near.sum()} surface points, max fp64 distance to the named face {d.max():.2e} m")
    assert d.max() <= 1e-6
    area = O.prepare(c["verts"], c["faces"])["area"]
    p = area / area.sum()
    n = int(near.sum())
    cnt = np.bincount(face[near], minlength=len(p))
    z = (cnt - n * p) / np.sqrt(n * p * (1 - p))
    print(f"sampler: face counts within {np.abs(z).max():.2f} sigma of N p (384 faces, area ratio {area.max() / area.min():.2f})")
    assert np.abs(z).max() <= 5
    # the box points: inside the padded box, and filling it
    m = O.prepare(c["verts"], c["faces"])
    q = (pts[~near] - m["centre"]) / (m["half"] + 0.05)
    assert np.abs(q).max() <= 1 + 1e-6 and np.abs(q).max(0).min() > 0.99 and np.abs(q.mean(0)).max() < 0.05


def test_sampler_noise_and_seeds():
    s = torus_samples()
    assert torch.equal(s["on"][0], s["on2"][0]) and torch.equal(s["on"][1], s["on2"][1])                 # the same seed: the same bits
    assert torch.equal(s["on"][1], s["noisy"][1])                                                      # sigma moves the points, not the picks
    assert not torch.equal(s["on"][0], s["other"][0]) and not torch.equal(s["on"][1], s["other"][1])
    face = s["on"][1][0].cpu().numpy()
    near = face >= 0
    off = (s["noisy"][0][0] - s["on"][0][0]).cpu().numpy().astype(np.float64)[near]
    sd = off.std(0, ddof=1)
    print(f"sampler, sigma 0.01: per-axis standard deviation of the offsets {sd}, mean {off.mean(0)}")
    assert np.abs(sd / 0.01 - 1).max() <= 0.02
    assert np.abs(off.mean(0)).max() <= 5 * 0.01 / np.sqrt(near.sum())
    assert np.abs(np.corrcoef(off.T) - np.eye(3)).max() < 0.02
    assert np.array_equal(s["noisy"][0][0].cpu().numpy()[~near], s["on"][0][0].cpu().numpy()[~near])     # box points carry no noise


# ---- rows, source, trainer -------------------------------------------------------------------------------------------------------
def test_rows_composite_against_the_oracle():
    h, o, o1 = case("open"), case("torus"), case("icosphere")
    B, nh, no, clamp = 2, 300, 100, 0.004
    shift = np.float32([0.05, 0.01, -0.02])
    hv = np.stack([h["verts"], h["verts"] + shift])
    # per-sample object topology: the torus (192 vertices, 384 faces) and the icosphere (162, 320) under one padded shape
    ov = np.stack([o["verts"] + shift, np.concatenate([o1["verts"], np.repeat(o1["verts"][:1], 30, 0)])])
    of = np.full((B, 390, 3), -1, np.int32)
    of[0, :384], of[1, :320] = o["faces"], o1["faces"]
    args = (gpu(hv), gpu(h["faces"]), gpu(ov), gpu(of), torch.tensor([384, 320]), gpu(h["labels"]), nh, no)
    kw = dict(sigma=(0.01, 0.003), uniform_every=16, pad=0.05, clamp=clamp, seed=5)
    rows = ops.mesh_sdf_rows(*args, **kw)
    rows2 = ops.mesh_sdf_rows(*args, **kw)
    other = ops.mesh_sdf_rows(*args, **dict(kw, seed=6))
    torch.cuda.synchronize()
    assert rows.shape == (B, nh + no, 6) and torch.equal(rows, rows2) and not torch.equal(rows[..., :3], other[..., :3])
    r = rows.cpu().numpy()
    for b in range(B):
        ofb = of[b, :[384, 320][b]]
        want = O.sdf_rows(r[b, :nh, :3], r[b, nh:, :3], hv[b], h["faces"], ov[b], ofb, h["labels"], clamp)
        for col, name in ((3, "sdf_hand"), (4, "sdf_obj")):
            err = np.abs(np.abs(r[b, :, col].astype(np.float64)) - np.abs(want[:, col])).max()
            print(f"rows, sample {b}: {name}: max | |sdf| - |sdf64| | = {err:.3e} m")
            assert err <= BAR
        # hand rows lie around the hand mesh, object rows around the object: the near-surface share is 15/16 of each set
        assert np.mean(np.abs(want[:nh, 3]) < 0.05) > 0.9 and np.mean(np.abs(want[nh:, 4]) < 0.05) > 0.9
        wh = O.mesh_sdf(r[b, :, :3], hv[b], h["faces"])["winding"]
        ok_h, ok_o = np.abs(wh - 0.5) > 0.05, np.abs(want[:, 4]) >= 1e-5          # the hand mesh is open, the objects are closed
        print(f"rows, sample {b}: sign judged on {100 * ok_h.mean():.2f} % (hand) / {100 * ok_o.mean():.2f} % (object) of the rows")
        assert ok_h.mean() >= 0.99 and ok_o.mean() >= 0.99
        assert np.array_equal((r[b, :, 3] < 0)[ok_h], (want[:, 3] < 0)[ok_h]) and np.array_equal((r[b, :, 4] < 0)[ok_o], (want[:, 4] < 0)[ok_o])
        # labels: -1 on object rows and beyond the clamp, the hand part otherwise (where the fp64 answer is not at the clamp's edge)
        lab = r[b, :, 5]
        assert np.all(lab[nh:] == -1)
        far, close = np.abs(want[:nh, 3]) > clamp + 1e-6, np.abs(want[:nh, 3]) < clamp - 1e-6
        assert close.sum() > 50 and far.sum() > 50 and np.all(lab[:nh][far] == -1)
        sets = O.mesh_sdf(r[b, :nh, :3], hv[b], h["faces"], h["labels"], label_sets=True)["label_sets"]
        assert all(int(l) in s for l, s, c in zip(lab[:nh], sets, close) if c)


@pytest.fixture(scope="module")
def source():
    from hoisdf_amd.config import Config
    from hoisdf_amd.nets import mano as MANO
    from hoisdf_amd.sdf_data import MeshSdfSource, procedural_templates
    c = Config()
    c.num_samp_hand, c.num_samp_obj = 96, 32
    layer = MANO.ManoLayer(MANO.synthetic_assets(0)).to(DEV)
    return MeshSdfSource(layer, procedural_templates(), c)


def test_mesh_source_make_inputs(source):
    from hoisdf_amd import testing as T
    from hoisdf_amd.sdf_data import synthetic_store
    c, B, nh, no = source.cfg, 2, 96, 32
    _, targets, meta = T.synthetic_batch(B, nh, no, seed=9)
    targets, meta = T.to_device(targets, DEV), T.to_device(meta, DEV)
    meta["obj_cls"] = torch.tensor([1, 2], device=DEV)
    args = (targets, meta, nh, no, c.points_filter_dist, c.hand_sdf_scale, c.obj_sdf_scale)
    out = source.make_inputs(*args, train=True, seed=3)
    cand = source.last_candidates.clone()
    again = source.make_inputs(*args, train=True, seed=3)
    torch.cuda.synchronize()
    store = synthetic_store(2, rows_hand=800, rows_obj=500)
    want = store.make_inputs([0, 1], meta["mano_root"], meta["obj_center_cam"], nh, no, 0.15, 3.1, 3.1, train=True, seed=1)
    assert set(out) == set(want)
    for k in want:
        assert out[k].shape == want[k].shape and out[k].dtype == want[k].dtype, k
        assert torch.equal(out[k], again[k]), k
    assert cand.shape == (B * 4 * (nh + no), 6)
    ev = source.make_inputs(*args, train=False, seed=3)
    assert set(ev) == set(store.make_inputs([0, 1], meta["mano_root"], meta["obj_center_cam"], nh, no, 0.15, 3.1, 3.1, train=False, seed=1))
    # the drawn rows: distinct, hand draws among the hand candidates and object draws among the object candidates of their sample
    rows = out["rows"].cpu().numpy()
    n = 4 * (nh + no)
    for b in range(B):
        loc = rows[b] - b * n
        for seg, lo, hi in ((loc[:nh], 0, 4 * nh), (loc[nh:nh + no], 4 * nh, n), (loc[nh + no:2 * nh + no], 0, 4 * nh), (loc[2 * nh + no:], 4 * nh, n)):
            assert len(set(seg.tolist())) == len(seg) and seg.min() >= lo and seg.max() < hi
    cn = cand.cpu().numpy()
    hand_v, hand_f, obj_v, obj_f, obj_n = (t.cpu().numpy() for t in source.meshes(targets, meta))
    root, oc = meta["mano_root"].cpu().numpy(), meta["obj_center_cam"].cpu().numpy()
    for b in range(B):
        d = cn[rows[b]]
        # what is handed to the model is the candidate row, centred and scaled
        assert np.abs(out["hand_sdf_points"][b].cpu().numpy() / c.hand_sdf_scale + root[b] - d[:nh, :3]).max() < 1e-6
        assert np.abs(out["obj_sdf_points"][b].cpu().numpy() / c.obj_sdf_scale + oc[b] - d[nh:nh + no, :3]).max() < 1e-6
        assert np.array_equal(out["hand_sdf"][b].cpu().numpy(), d[:nh, 3] * np.float32(c.hand_sdf_scale))
        assert np.array_equal(out["obj_sdf"][b].cpu().numpy(), d[nh:nh + no, 4] * np.float32(c.obj_sdf_scale))
        # ... and its distances are the oracle's at the candidate's own coordinates.  (The synthetic MANO asset's faces are a random
        # triangle soup: the unsigned distance is what can be compared for the hand; the templates are closed: signed.)
        ref_h = O.mesh_sdf(d[:nh, :3], hand_v[b], hand_f)
        ref_o = O.mesh_sdf(d[nh:nh + no, :3], obj_v[b], obj_f[b, :obj_n[b]])
        eh = np.abs(np.abs(out["hand_sdf"][b].cpu().numpy().astype(np.float64)) - c.hand_sdf_scale * ref_h["dist"]).max()
        eo = np.abs(np.abs(out["obj_sdf"][b].cpu().numpy().astype(np.float64)) - c.obj_sdf_scale * ref_o["dist"]).max()
        print(f"source, sample {b}: hand_sdf err {eh:.3e}, obj_sdf err {eo:.3e} (scaled units; bar {BAR * c.hand_sdf_scale:.2e})")
        assert eh <= BAR * c.hand_sdf_scale and eo <= BAR * c.obj_sdf_scale
        sure = ref_o["dist"] >= 1e-5
        assert np.array_equal((out["obj_sdf"][b].cpu().numpy() < 0)[sure], (ref_o["sdf"] < 0)[sure])
        # every "pre" point has |sdf| < dist
        assert (np.abs(d[nh + no:2 * nh + no, 3]) < c.points_filter_dist).all() and (np.abs(d[2 * nh + no:, 4]) < c.points_filter_dist).all()
        assert np.abs(out["hand_pre_points"][b].cpu().numpy() / c.hand_sdf_scale + root[b] - d[nh + no:2 * nh + no, :3]).max() < 1e-6
    # too few candidates for the draw: the store's ValueError
    with pytest.raises(ValueError, match="eligible"):
        source.make_inputs(targets, meta, nh, no, 1e-7, c.hand_sdf_scale, c.obj_sdf_scale, train=True, seed=3)
    source.cfg.mesh_sdf_candidates = 0
    try:
        with pytest.raises(ValueError, match="candidates"):
            source.make_inputs(*args, train=True, seed=3)
    finally:
        source.cfg.mesh_sdf_candidates = 4


def test_default_hand_part_labels_come_from_the_layer(source):
    w = source.layer.th_weights.cpu().numpy()
    assert source.vert_label.shape == (778,) and np.array_equal(source.vert_label.cpu().numpy(), O.vertex_part_labels(w))
    assert set(source.vert_label.cpu().tolist()) <= set(range(6))


def test_trainer_computes_its_points_from_the_meshes():
    """Trainer(sdf_source=...): the dataset yields labels and no point sets; three steps at ResNet-18, B = 2, run with a finite loss"""
    from hoisdf_amd.config import Config
    from hoisdf_amd.engine import Trainer
    from hoisdf_amd.sdf_data import MeshSdfSource, procedural_templates
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = 96, 32
    c.sdf_source = "mesh"
    dev = torch.device("cuda", 0)
    tr = Trainer(c, dev, batch_size=2, tune_encoder=False)
    assert isinstance(tr.sdf_source, MeshSdfSource) and tr.sdf_source.layer is tr.model.mano_head.mano_layer
    explicit = Trainer(c, dev, batch_size=2, tune_encoder=False,
                       sdf_source=MeshSdfSource(tr.model.mano_head.mano_layer, procedural_templates(), c))
    assert type(explicit.batch_generator.dataset).__name__ == "SyntheticMeshSdfDataset"
    it = iter(tr.batch_generator)
    losses = []
    for _ in range(3):
        inputs, targets, meta = next(it)
        assert "hand_sdf_points" not in inputs and "hand_sdf" not in targets and "obj_cls" in meta
        total, loss = tr.train_step(inputs, targets, meta, 0, 0.0)
        losses.append(float(total))
    print("trainer on mesh SDF: losses", losses)
    assert all(np.isfinite(losses)) and "sdfhand_loss" in loss and float(loss["sdfhand_loss"]) > 0 and float(loss["sdfobj_loss"]) > 0
    # the last step's candidates: the hand column is the oracle's unsigned distance to the MANO mesh of that step
    cand = tr.sdf_source.last_candidates.cpu().numpy()[:200]
    tg, mt = {k: v.to(dev) for k, v in targets.items()}, {k: v.to(dev) for k, v in meta.items()}
    hv, hf = (t.cpu().numpy() for t in tr.sdf_source.meshes(tg, mt)[:2])
    err = np.abs(np.abs(cand[:, 3].astype(np.float64)) - O.mesh_sdf(cand[:, :3], hv[0], hf)["dist"]).max()
    print(f"trainer: candidate rows vs oracle, unsigned hand distance: {err:.3e} m")
    assert err <= BAR


# ---- C host ----------------------------------------------------------------------------------------------------------------------
def test_c_host_mesh_sdf(tmp_path):
    """A plain C host (tests/c/test_mesh_sdf_host.c: hoisdf_mesh_prepare + hoisdf_mesh_sdf on a dumped mesh and points) gets the bits
    the Python call gets"""
    cs = [case("icosphere"), case("open")]
    V, F, N = 162, 320, 500
    verts = np.stack([c["verts"] for c in cs])
    faces = np.full((2, F, 3), -1, np.int32)
    for b, c in enumerate(cs):
        faces[b, :len(c["faces"])] = c["faces"]
    nf = np.asarray([320, 260], np.int32)
    pts = np.stack([c["points"][:N] for c in cs])
    lab = cs[0]["labels"]
    out = ops.mesh_sdf(gpu(pts), gpu(verts), gpu(faces), n_faces=torch.from_numpy(nf), vert_label=gpu(lab), extras=True)
    torch.cuda.synchronize()

    def arr(f, a, dt):
        a = np.ascontiguousarray(a).reshape(-1).astype(dt)
        f.write(struct.pack("<q", a.size))
        f.write(a.tobytes())

    src, dst = str(tmp_path / "mesh_in.bin"), str(tmp_path / "mesh_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<5i", 2, V, F, N, 1))
        arr(f, verts, "<f4"), arr(f, faces, "<i4"), arr(f, nf, "<i4"), arr(f, pts, "<f4"), arr(f, lab, "<i4")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_mesh_sdf_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_mesh_sdf_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    res = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0 and "c host mesh sdf ok" in res.stdout, res.stdout + res.stderr
    c_sdf = np.fromfile(dst, dtype="<f4", count=2 * N)
    c_face, c_label = np.split(np.fromfile(dst, dtype="<i4", offset=4 * 2 * N), 2)
    assert np.array_equal(c_sdf.view(np.uint32), out["sdf"].cpu().numpy().reshape(-1).view(np.uint32))
    assert np.array_equal(c_face, out["face"].cpu().numpy().reshape(-1)) and np.array_equal(c_label, out["label"].cpu().numpy().reshape(-1))
