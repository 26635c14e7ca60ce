"""-m gpu: hand-object interaction metrics (csrc/interact.hip: hoisdf_eval_interaction; ops.eval_interaction; metrics.Evaluator(
interaction=True)) against the fp64 numpy restatement hoisdf_amd/interaction_oracle.py on procedural meshes at hand size and camera
depth (scale 0.08 m about (0.03, -0.02, 0.7), as tests/test_gpu_mesh_sdf.py).

The bars are that test's, since the distances come from the same kernel at the same scale.  pen_hand, pen_obj, min_dist: within
5e-7 m of fp64.  contact_verts, in_contact, inside_count and the inside mask: equal to fp64 outside the AMBIGUOUS set - against a
closed mesh a vertex whose | |sdf64| - threshold | < 1e-5 m (threshold 0 for the sign, contact_dist for contact) and a cell centre
whose fp64 distance to the mesh is < 1e-5 m; against the open mesh a vertex or centre with |winding64 - 0.5| <= 0.05.  The mask is
compared cell by cell outside that set, a count may differ by at most the size of the set, volume is inside_count x the cell
volume bit for bit.  Conditions, asserted: the set holds at most 1 % of a sample's vertices and of its cells, and no vertex that
attains pen_* or min_dist is in it.

One call of B = 3, made so that every way the kernels index is taken:
  0  closed icosphere (320 faces) x torus (384 faces = 3 tiles of 128), interpenetrating: 18 x 38 x 13 = 8892 cells (139 blocks of 64 - 4)
  1  open icosphere (260 faces = 2 tiles + a ragged third; the hole at -z, away from the object) x box (192 of 384 face rows, 150 of
     192 vertex rows; the padding rows sit INSIDE the hand), 4.5 mm apart: in contact, nothing penetrates
  2  closed icosphere x torus 0.2 m away: disjoint bounding boxes, no cell
and one sample at 0.5 mm voxels whose grid is cut to 64 cells along x."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest
import torch

from hoisdf_amd import interaction_oracle as I
from hoisdf_amd import mesh_sdf_oracle as O
from hoisdf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR, NEAR, WIND = 5e-7, 1e-5, 0.05
SCALE, CENTRE = 0.08, np.array([0.03, -0.02, 0.7])
CD, VOX = 0.005, 0.004
CELLS = 64 ** 3
FLOATS, INTS = ("pen_hand", "pen_obj", "min_dist", "volume"), ("contact_verts", "in_contact", "inside_count")


def placed(mesh, shift=(0.0, 0.0, 0.0)):
    v, f = mesh
    return (v * SCALE + CENTRE + np.asarray(shift)).astype(np.float32), np.asarray(f, np.int32)


def open_icosphere():
    v, f = O.icosphere(2)
    return v, f[v[f].mean(1)[:, 2] >= -0.6]                   # the cap around -z removed: 260 faces, a hole


def pack(samples):
    """[(hand verts, hand faces, obj verts, obj faces, obj padding vertex or None, hand is closed)] -> the padded arrays of one call;
    face padding rows name vertices far outside the mesh"""
    Vh, Fh = max(len(s[0]) for s in samples), max(len(s[1]) for s in samples)
    Vo, Fo = max(len(s[2]) for s in samples), max(len(s[3]) for s in samples)
    B = len(samples)
    c = dict(hv=np.zeros((B, Vh, 3), np.float32), hf=np.full((B, Fh, 3), 2 ** 30, np.int32), hn=np.zeros(B, np.int32),
             ov=np.zeros((B, Vo, 3), np.float32), of=np.full((B, Fo, 3), 2 ** 30, np.int32), on=np.zeros(B, np.int32),
             onv=np.zeros(B, np.int32), closed=[s[5] for s in samples])
    for b, (hv, hf, ov, of, pad, _) in enumerate(samples):
        assert len(hv) == Vh
        c["hv"][b], c["hf"][b, :len(hf)], c["hn"][b] = hv, hf, len(hf)
        c["ov"][b, :len(ov)], c["of"][b, :len(of)], c["on"][b], c["onv"][b] = ov, of, len(of), len(ov)
        if len(ov) < Vo:
            c["ov"][b, len(ov):] = pad
    return c


def ambiguity(ref, hand_closed):
    """the sets outside which the fp64 answer is binding (the object is closed in every case of this file)"""
    def unsure(r, closed, threshold=0.0):
        return np.abs(r["dist"] - threshold) < NEAR if closed else np.abs(r["winding"] - 0.5) <= WIND
    hv, ov = ref["hand_vert"], ref["obj_vert"]
    return dict(hand_sign=unsure(hv, True), hand_contact=unsure(hv, True, CD), obj_sign=unsure(ov, hand_closed),
                cell=unsure(ref["vox_obj"], True) | unsure(ref["vox_hand"], hand_closed))


def with_reference(c, voxel):
    c["voxel"], c["ref"], c["amb"] = voxel, [], []
    for b in range(len(c["hn"])):
        r = I.eval_interaction(c["hv"][b], c["hf"][b, :c["hn"][b]], c["ov"][b], c["of"][b, :c["on"][b]], int(c["onv"][b]), CD, voxel)
        for a in list(r.values()) + [x for k in ("hand_vert", "obj_vert", "vox_obj", "vox_hand") for x in r[k].values()]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        c["ref"].append(r)
        c["amb"].append(ambiguity(r, c["closed"][b]))
    return c


_CASES = {}


def case(name):
    """the arrays of one call and the fp64 oracle's answer per sample: computed once, never changed"""
    if name not in _CASES:
        assert ops._lib.CONSTANTS["MESH_TILE"] == 128 and ops._lib.CONSTANTS["INTERACT_MAX_GRID"] == 64
        ico, opn, torus, box = O.icosphere(2), open_icosphere(), O.torus(16, 12), O.box()
        if name == "three":
            inside_hand = (CENTRE + [0.03, 0.03, 0.0]).astype(np.float32)
            samples = [(*placed(ico), *placed(torus, (0.09, 0.01, 0.02)), None, True),
                       (*placed(opn), *placed(box, (0.139, 0.115, 0.01)), inside_hand, False),
                       (*placed(ico), *placed(torus, (0.2, 0.0, 0.0)), None, True)]
            _CASES[name] = with_reference(pack(samples), VOX)
        else:                                                   # a rod of 160 x 4.8 x 4 mm through the side of the sphere
            _CASES[name] = with_reference(pack([(*placed(ico), *placed(O.box(1.0, 0.03, 0.025), (0.08, 0.05, 0.0)), None, True)]), 0.0005)
    return _CASES[name]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(c, rows=None, fill=0xAA):
    s = slice(None) if rows is None else rows
    B = len(c["hn"][s])
    mask = torch.full((B, CELLS), fill, device=DEV, dtype=torch.uint8)
    out = ops.eval_interaction(gpu(c["hv"][s]), gpu(c["hf"][s]), gpu(c["ov"][s]), gpu(c["of"][s]), torch.from_numpy(c["on"][s]),
                               torch.from_numpy(c["onv"][s]), CD, c["voxel"], want_mask=mask, hand_n_faces=torch.from_numpy(c["hn"][s]))
    torch.cuda.synchronize()
    assert out["inside"].data_ptr() == mask.data_ptr()
    return {k: v.cpu().numpy() for k, v in out.items()}


_RUNS = {}


def result(name):
    if name not in _RUNS:
        _RUNS[name] = run(case(name))
    return _RUNS[name]


def check_sample(what, got, b, ref, amb, expect_cells):
    """every rule of the module docstring for sample b of a call"""
    g = ref["grid"]
    n = int(np.prod(g["n"]))
    # the conditions the comparison rests on
    nh, no = len(amb["hand_sign"]), max(len(amb["obj_sign"]), 1)
    unsure_hand = amb["hand_sign"] | amb["hand_contact"]
    print(f"{what}: ambiguous: {int(unsure_hand.sum())} of {nh} hand vertices, {int(amb['obj_sign'].sum())} of {no} object vertices, "
          f"{int(amb['cell'].sum())} of {n} cells")
    assert unsure_hand.sum() <= 0.01 * nh and amb["obj_sign"].sum() <= 0.01 * no and amb["cell"].sum() <= 0.01 * n
    hv, ov = ref["hand_vert"], ref["obj_vert"]
    assert not amb["hand_sign"][np.argmax(-hv["sdf"])] and not amb["hand_sign"][np.argmin(hv["dist"])]
    assert not len(ov["sdf"]) or not amb["obj_sign"][np.argmax(-ov["sdf"])]
    # the grid: the very same fp32 numbers
    grid = got["grid"][b]
    assert n == expect_cells and int(grid[6:7].view(np.int32)[0]) == I.pack_n(g["n"]) and grid[7] == 0
    assert np.array_equal(grid[:3].view(np.uint32), g["lo"].view(np.uint32))
    assert np.array_equal(grid[3:6].view(np.uint32), g["cell"].view(np.uint32))
    # distances
    for k in ("pen_hand", "pen_obj", "min_dist"):
        err = abs(float(got[k][b]) - ref[k])
        print(f"{what}: {k} = {got[k][b]:.7f} m, fp64 {ref[k]:.7f} m, off by {err:.2e} m")
        assert err <= BAR, (k, err)
    # counts over the vertices
    sure_contact = hv["sdf"] <= CD
    lo, hi = int((sure_contact & ~amb["hand_contact"]).sum()), int((sure_contact | amb["hand_contact"]).sum())
    assert lo <= got["contact_verts"][b] <= hi and abs(int(got["contact_verts"][b]) - ref["contact_verts"]) <= amb["hand_contact"].sum()
    pen_sure, pen_may = (ov["sdf"] < 0) & ~amb["obj_sign"], (ov["sdf"] < 0) | amb["obj_sign"]
    assert int(lo > 0 or pen_sure.any()) <= got["in_contact"][b] <= int(hi > 0 or pen_may.any())
    assert got["in_contact"][b] == int(got["contact_verts"][b] > 0 or got["pen_obj"][b] > 0)
    # cells
    mask = got["inside"][b]
    judged = ~amb["cell"]
    wrong = int((mask[:n].astype(bool) != ref["inside"])[judged].sum())
    print(f"{what}: {n} cells, {ref['inside_count']} inside both in fp64, {got['inside_count'][b]} on the GPU; {wrong} of the judged cells differ")
    assert wrong == 0 and set(np.unique(mask[:n]).tolist()) <= {0, 1}
    assert int(mask[:n].sum()) == got["inside_count"][b] and abs(int(got["inside_count"][b]) - ref["inside_count"]) <= amb["cell"].sum()
    assert (mask[n:] == 0xAA).all()                            # bytes from n on are not touched
    want = np.float32(got["inside_count"][b]) * grid[3] * grid[4] * grid[5]
    assert got["volume"][b:b + 1].view(np.uint32)[0] == np.asarray([want], np.float32).view(np.uint32)[0]


def test_three_samples_against_the_oracle():
    c, got = case("three"), result("three")
    assert c["hn"].tolist() == [320, 260, 320] and c["on"].tolist() == [384, 192, 384] and c["onv"].tolist() == [192, 150, 192]
    assert c["hv"].shape == (3, 162, 3) and c["ov"].shape == (3, 192, 3)
    for b, cells in enumerate((18 * 38 * 13, 13 * 13 * 20, 0)):
        assert cells % 64 != 0 or cells == 0
        check_sample(f"sample {b}", got, b, c["ref"][b], c["amb"][b], cells)
    r0, r1, r2 = c["ref"]
    # sample 0 overlaps: enough cells on either side for the mask comparison to mean something
    assert r0["inside_count"] > 200 and len(r0["inside"]) - r0["inside_count"] > 200 and got["inside_count"][0] > 200
    assert r0["pen_hand"] > 0.01 and r0["pen_obj"] > 0.01 and got["in_contact"][0] == 1 and got["volume"][0] > 1e-4
    # sample 1 touches and does not penetrate; its padding vertex rows lie 3 cm inside the hand and are left out of pen_obj - while
    # they do widen the object's bounding box, so that the hand pass runs on the open mesh (some cells are inside the box)
    assert got["pen_hand"][1] == 0 and got["pen_obj"][1] == 0 and got["in_contact"][1] == 1 and got["contact_verts"][1] == r1["contact_verts"] > 0
    assert CD - 1e-3 < got["min_dist"][1] < CD and got["inside_count"][1] == 0 and got["volume"][1] == 0
    assert (r1["vox_obj"]["winding"] > 0.5).sum() > 200 and (r1["vox_hand"]["winding"] > 0.5).sum() > 200
    with_padding = O.mesh_sdf(c["ov"][1], c["hv"][1], c["hf"][1, :260])["sdf"]
    assert with_padding[150:].max() < -0.02 and with_padding[:150].min() > 0
    assert np.abs(r1["vox_hand"]["winding"] - 0.5).min() > 0.2   # the hole stays clear of the overlap box
    # sample 2: nothing
    assert got["inside_count"][2] == 0 and got["volume"][2] == 0 and got["in_contact"][2] == 0 and got["contact_verts"][2] == 0
    assert got["pen_hand"][2] == 0 and got["pen_obj"][2] == 0 and abs(got["min_dist"][2] - r2["min_dist"]) <= BAR and r2["min_dist"] > 0.03
    assert (got["inside"][2] == 0xAA).all()


def test_a_grid_cut_to_64_cells_per_axis():
    c, got = case("clamp"), result("clamp")
    r = c["ref"][0]
    assert r["grid"]["n"].tolist() == [64, 10, 8]
    assert abs(float(r["grid"]["cell"][0]) - 0.08 / 64) < 1e-6 and r["grid"]["cell"][0] > 2 * np.float32(0.0005)
    check_sample("64-cell axis", got, 0, r, c["amb"][0], 64 * 10 * 8)
    assert r["inside_count"] > 200 and 64 * 10 * 8 - r["inside_count"] > 200


def test_two_calls_give_the_same_bits():
    first, again = result("three"), run(case("three"))
    for k in first:
        assert np.array_equal(first[k].view(np.uint8), again[k].view(np.uint8)), k


def test_a_batch_is_its_samples():
    """every output of the B = 3 call, bit for bit, from three calls of B = 1 on the same padded rows"""
    c, got = case("three"), result("three")
    for b in range(3):
        one = run(c, slice(b, b + 1))
        for k in got:
            assert one[k].shape[0] == 1 and np.array_equal(one[k].view(np.uint8), got[k][b:b + 1].view(np.uint8)), (b, k)


def test_shape_errors_are_value_errors():
    c = case("three")
    hv, hf, ov, of = gpu(c["hv"]), gpu(c["hf"]), gpu(c["ov"]), gpu(c["of"])
    for args, kw in (((hv, hf, ov[:2], of), {}), ((hv, hf[:2], ov, of), {}), ((hv[0], hf, ov, of), {}), ((hv, hf, ov, of, [384, 192]), {}),
                     ((hv, hf, ov, of), dict(obj_n_verts=[1, 2])), ((hv, hf, ov, of), dict(want_mask=torch.zeros(3, 8, device=DEV, dtype=torch.uint8)))):
        with pytest.raises(ValueError):
            ops.eval_interaction(*args, **kw)
    with pytest.raises(ops._lib.HoisdfError, match="voxel"):
        ops.eval_interaction(hv, hf, ov, of, voxel=0.0)


# ---- the Evaluator ---------------------------------------------------------------------------------------------------------------
def _batches():
    """two batches of three (out, targets, meta, obj_cls) in the ho3d layout: an icosphere of 5 cm as the 'hand', the procedural
    templates as objects, predicted 1 - 5 cm apart; one sample without an evaluated object"""
    from hoisdf_amd.sdf_data import procedural_templates
    tmpl = procedural_templates()
    hand_v, hand_f = O.icosphere(2)
    r = np.random.default_rng(11)
    rec = []
    for it in range(2):
        B, P = 3, 8
        f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
        root = f32(r.uniform(-0.05, 0.05, (B, 3)) + [0, 0, 0.7])
        centre = root + f32(r.uniform(-1, 1, (B, 3)) * [0.03, 0.03, 0.01])
        out = {"mano_mesh_out": f32(np.repeat(0.05 * hand_v[None], B, 0)).to(DEV), "mano_joints_out": torch.zeros(B, 21, 3, device=DEV),
               "obj_rot_out": f32(r.normal(0, 0.5, (B, 1, 3)) + r.normal(0, 0.02, (B, P, 3))).to(DEV),
               "obj_trans_out": f32(r.normal(0, 0.004, (B, P, 3))).to(DEV)}
        targets = {"obj_rot": f32(r.normal(0, 0.5, (B, 3))), "rel_obj_trans": f32(r.normal(0, 0.004, (B, 3)))}
        meta = {"mano_root": root, "obj_center_cam": centre}
        cls = torch.tensor([[0, 1, 2], [2, -1, 1]][it])
        rec.append((out, targets, meta, cls))
    return tmpl, torch.from_numpy(hand_f), rec


def test_evaluator_appends_the_block_and_is_silent_without_the_option(tmp_path):
    from hoisdf_amd import metrics as M
    from hoisdf_amd.config import Config
    tmpl, hand_f, rec = _batches()
    c = Config()
    c.apply_setting("ho3d")
    c.contact_dist, c.interaction_voxel = 0.004, 0.003
    verts = tmpl["verts"].to(DEV)
    files = {}
    for name, kw in (("plain", {}), ("off", dict(interaction=False, template_faces=tmpl, hand_faces=hand_f)),
                     ("on", dict(interaction=True, template_faces=tmpl, hand_faces=hand_f))):
        ev = M.Evaluator(c, verts, native=True, **kw)
        for out, targets, meta, cls in rec:
            ev.feed(out, targets, meta, cls)
        files[name] = open(ev.write(str(tmp_path / name)), "rb").read()
    assert files["off"] == files["plain"] and b"Interaction" not in files["plain"]
    assert files["on"].startswith(files["plain"]) and len(files["on"]) > len(files["plain"])
    block = files["on"][len(files["plain"]):].decode()
    print(block)
    m = re.fullmatch(r"Interaction:\npenetration_depth=([\d.]+) cm, contact_ratio=([\d.]+), intersection_volume=([\d.]+) cm\^3, "
                     r"contact_verts=([\d.]+)\n", block)
    assert m, block
    # the same numbers from the per-sample values of ops.eval_interaction on the pair posed here
    vals = []
    for out, _, meta, cls in rec:
        used = cls >= 0
        k = cls.clamp_min(0).to(DEV)
        hand = out["mano_mesh_out"] + meta["mano_root"].to(DEV)[:, None]
        R = M.batch_rodrigues(out["obj_rot_out"].mean(1))
        obj = verts[k] @ R.transpose(1, 2) + (out["obj_trans_out"].mean(1) + meta["obj_center_cam"].to(DEV))[:, None]
        r = ops.eval_interaction(hand, hand_f, obj, tmpl["faces"].to(DEV)[k], tmpl["n_faces"].to(DEV)[k], None, 0.004, 0.003)
        per = np.stack([np.maximum(r["pen_hand"].cpu().numpy(), r["pen_obj"].cpu().numpy()).astype(np.float64) * 100,
                        r["in_contact"].cpu().numpy().astype(np.float64), r["volume"].cpu().numpy().astype(np.float64) * 1e6,
                        r["contact_verts"].cpu().numpy().astype(np.float64)], 1)
        vals.append(per[used.numpy()])
    vals = np.concatenate(vals)
    assert len(vals) == 5
    mean = vals.mean(0)
    print("per-sample [pen cm, in_contact, volume cm^3, contact_verts]:\n", vals)
    # printed with 3 / 3 / 3 / 1 decimals: half a unit of the last one, plus the fp64 sums' own rounding
    for got, want, digits in zip(m.groups(), mean, (3, 3, 3, 1)):
        assert abs(float(got) - want) <= 0.5 * 10 ** -digits + 1e-9, (got, want)
    assert mean[0] > 0.1 and 0 < mean[1] <= 1 and mean[2] > 0.1          # the pairs do interpenetrate: the block is not a row of zeros
    with pytest.raises(ValueError, match="template_faces"):
        M.Evaluator(c, verts, native=True, interaction=True)


# ---- C host ----------------------------------------------------------------------------------------------------------------------
def test_c_host_interaction(tmp_path):
    """A plain C host (tests/c/test_interaction_host.c: one hoisdf_eval_interaction call on the dumped three-sample case) gets the
    bits the Python call gets"""
    c, got = case("three"), result("three")

    def arr(f, a, dt):
        a = np.ascontiguousarray(a).reshape(-1).astype(dt)
        f.write(struct.pack("<q", a.size))
        f.write(a.tobytes())

    src, dst = str(tmp_path / "interaction_in.bin"), str(tmp_path / "interaction_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<5i2f", 3, c["hv"].shape[1], c["hf"].shape[1], c["ov"].shape[1], c["of"].shape[1], CD, VOX))
        arr(f, c["hv"], "<f4"), arr(f, c["hf"], "<i4"), arr(f, c["hn"], "<i4"), arr(f, c["ov"], "<f4"), arr(f, c["of"], "<i4")
        arr(f, c["on"], "<i4"), arr(f, c["onv"], "<i4")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_interaction_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_interaction_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    res = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0 and "c host interaction ok" in res.stdout, res.stdout + res.stderr
    words = np.fromfile(dst, dtype="<u4")
    assert len(words) == 3 * (4 + 3 + 8 + 1)
    for i, k in enumerate(FLOATS + INTS):
        assert np.array_equal(words[3 * i:3 * i + 3], got[k].view(np.uint32)), k
    assert np.array_equal(words[21:45], got["grid"].reshape(-1).view(np.uint32))
    assert np.array_equal(words[45:48].astype(np.int64), got["inside_count"].astype(np.int64))     # the host's mask started at zero
