"""-m gpu: the silhouette loss (csrc/silhouette_loss.hip: hoisdf_mask_edt, hoisdf_silhouette_loss_fwd / _bwd; ops.mask_edt,
ops.silhouette_loss; cfg.silhouette_loss in Model / Trainer) against the fp64 numpy restatement hoisdf_amd/silhouette_loss_oracle.py
on the scenes of tests/test_silhouette_loss_oracle.py.

The bars.  The distance transform, the per-pixel nearest vertex, the per-vertex cell and the projections u, v: bit for bit - they
are integers, or fp64 operations that numpy rounds the same way.  inside and cover: within 1 ulp of float32 of the oracle's fp64
value (an fp64 sum of <= 2^14 terms errs by <= 2^-39 relative, then one rounding).  Gradients: |gpu - oracle| <= 2^-23 |oracle| +
2^-40 abs_terms, for the same reason.

One call of B = 3 at 40 x 48 (h x w), V = 192 vertex rows = three LDS tiles of 64, 1920 pixels = 30 full record tiles:
  0  icosphere, 162 of 192 rows        1  torus at focal length 250, 192 rows
  2  box at focal length 420, 150 of 192 rows, 59 of them off the map
The padding rows sit at the centre of the hand and carry non-zero weight.  And one call of B = 1 at 33 x 70: 2310 pixels = 36
record tiles and a partial one, a row wider than one wave and no multiple of 32.  The oracle test's kink condition is asserted
again for exactly these inputs."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

import test_silhouette_loss_oracle as T
from hoisdf_amd import ops
from hoisdf_amd import silhouette_loss_oracle as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEAR = T.NEAR
# upstream gradients [sample][inside, cover]: the float32 values the kernel is handed, widened, so that the oracle is given the same numbers
G = np.array([[0.7, 1.3], [1.1, 0.6], [0.8, 1.2]], np.float32).astype(np.float64)


def gpu(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the case's arrays are read-only)


def pack(names, V=192):
    scs = [T.scene(n) for n in names]
    B, h, w = len(scs), scs[0]["h"], scs[0]["wd"]
    c = dict(verts=np.zeros((B, V, 3), np.float32), nv=np.zeros(B, np.int32), K=np.stack([s["K"] for s in scs]),
             cover=np.stack([s["cover"] for s in scs]), allow=np.stack([s["allow"] for s in scs]), d2=np.stack([s["d2"] for s in scs]),
             w=np.random.default_rng(17).uniform(0.5, 1.5, (B, V)).astype(np.float32), h=h, wd=w, G=G[:B])
    for b, s in enumerate(scs):
        n = len(s["verts"])
        c["verts"][b, :n], c["verts"][b, n:], c["nv"][b] = s["verts"], T.BASE.astype(np.float32), n
    return c


def sample(c, b):
    """sample b of a packed case as the oracle test's helpers take a scene"""
    return {"verts": c["verts"][b], "K": c["K"][b], "d2": c["d2"][b], "cover": c["cover"][b], "w": c["w"][b], "h": c["h"], "wd": c["wd"]}


_CASES = {}


def case(which="three"):
    """the arrays of a call and the fp64 oracle's answer per sample with the upstream gradients G: computed once, never changed"""
    if which not in _CASES:
        assert ops._lib.CONSTANTS["SIL_LOSS_TILE"] == 64 and ops._lib.CONSTANTS["EDT_NONE"] == S.EDT_NONE
        c = pack(["icosphere", "torus250", "box"]) if which == "three" else pack(["torus"])
        assert c["nv"].tolist() == ([162, 192, 150] if which == "three" else [192])
        assert (c["h"], c["wd"]) == ((40, 48) if which == "three" else (33, 70))
        c["ref"] = [S.silhouette_loss(c["verts"][b], int(c["nv"][b]), c["K"][b], c["d2"][b], c["cover"][b], c["w"][b], NEAR, *c["G"][b])
                    for b in range(len(c["nv"]))]
        for b, r in enumerate(c["ref"]):
            assert 0.05 < r["inside"] < 4 and 0.05 < r["cover"] < 4 and r["use"][:c["nv"][b]].all()
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[which] = c
    return _CASES[which]


def run(c, rows=slice(None), weight="w", verts=None, d2=None, cover=None, g=None):
    """values and the gradient of sum_b G[b] . (inside, cover)[b] for the samples `rows` -> numpy arrays"""
    v = gpu(c["verts"][rows] if verts is None else verts).requires_grad_()
    wt = None if weight is None else gpu(c["w"][rows] if isinstance(weight, str) else weight)
    vals = ops.silhouette_loss(v, gpu(c["K"][rows]), gpu(c["d2"][rows] if d2 is None else d2), gpu(c["cover"][rows] if cover is None else cover),
                               torch.from_numpy(c["nv"][rows]), wt, NEAR)
    up = gpu((c["G"][rows] if g is None else g).astype(np.float32))
    (torch.stack(vals, 1) * up).sum().backward()
    torch.cuda.synchronize()
    return {"inside": vals[0].detach().cpu().numpy(), "cover": vals[1].detach().cpu().numpy(), "d_verts": v.grad.cpu().numpy()}


_RUNS = {}


def result(which="three"):
    if which not in _RUNS:
        _RUNS[which] = run(case(which))
    return _RUNS[which]


def within_one_ulp(got, want):
    return abs(float(got) - want) <= float(np.spacing(np.float32(abs(want))))


def assert_gradient(got, ref, what):
    err = np.abs(got.astype(np.float64) - ref["d_verts"])
    bar = 2.0 ** -23 * np.abs(ref["d_verts"]) + 2.0 ** -40 * ref["abs_terms"]
    print(f"{what}: largest gradient {np.abs(ref['d_verts']).max():.4f}, largest error {err.max():.3e}, worst error / bar "
          f"{float((err / np.where(bar > 0, bar, 1)).max()):.3f}, {int((np.abs(ref['d_verts']).max(1) > 0).sum())} of {len(err)} rows non-zero")
    assert (err <= bar).all(), what


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which,b", [("three", 0), ("three", 1), ("three", 2), ("one", 0)])
def test_the_inputs_meet_the_kink_condition(which, b):
    c = case(which)
    n = int(c["nv"][b])
    _, _, _, kink = T.differences(sample(c, b), n, extrapolate=False)
    print(f"{which} sample {b}: {int(kink.sum())} of {n} vertices within 1e-6 m of a kink")
    assert kink.sum() <= 0.05 * n and not kink[n:].any()


# ---- the distance transform ------------------------------------------------------------------------------------------------------------
def test_edt_bit_for_bit():
    r = np.random.default_rng(11)
    masks = dict(T.masks())
    masks["67x130"] = T.disk(67, 130, 100, 20, 15) | T.disk(67, 130, 5, 60, 9) | (r.uniform(size=(67, 130)) < 0.004)
    masks["512x512"] = r.uniform(size=(512, 512)) < 0.0002         # the largest map: every thread of the widest block
    for name, m in masks.items():
        d2, nearest = ops.mask_edt(gpu(m.astype(np.float32)[None]), want_nearest=True)
        want = S.edt(m) if m.size < 10000 else S.edt_brute(m)
        assert d2.dtype == torch.int32 and tuple(d2.shape) == (1,) + m.shape
        assert np.array_equal(d2[0].cpu().numpy(), want[0]) and np.array_equal(nearest[0].cpu().numpy(), want[1]), name
    c = case()
    a, b = T.disk(40, 48, 12, 12, 6).astype(np.float32), T.disk(40, 48, 30, 25, 8).astype(np.float32)
    first = np.stack([a, c["allow"][0], np.zeros_like(a)])        # a batch: a union, a mask with NULL's share empty, a sample without a pixel
    second = np.stack([0.75 * b, np.zeros_like(a), 0.5 * b])
    d2, nearest = ops.mask_edt(gpu(first), gpu(second), want_nearest=True)
    for k, (m, mo) in enumerate(zip(first, second)):
        want = S.edt(m, mo)
        assert np.array_equal(d2[k].cpu().numpy(), want[0]) and np.array_equal(nearest[k].cpu().numpy(), want[1]), k
    assert (d2[2] == S.EDT_NONE).all() and (nearest[2] == -1).all()
    assert torch.equal(ops.mask_edt(gpu(c["allow"])), gpu(c["d2"])) and torch.equal(ops.mask_edt(gpu(first), gpu(second)), d2)


# ---- the loss --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["three", "one"])
def test_what_the_forward_keeps_equals_the_oracle(which):
    """u, v, the cell of every vertex and the nearest vertex of every pixel, read from the workspace through the header's layout"""
    c = case(which)
    B, V, h, w = len(c["nv"]), c["verts"].shape[1], c["h"], c["wd"]
    t = [gpu(c[k]) for k in ("verts", "nv", "K", "d2", "cover", "w")]
    ws, nws = ops._workspace("hoisdf_silhouette_loss_workspace_bytes", B, V, w, h, torch.device(DEV))
    out = torch.empty(2, B, device=DEV)
    p = ops._p
    ops.call("hoisdf_silhouette_loss_fwd", p(t[0]), p(t[1]), V, p(t[2]), B, p(t[3]), p(t[4]), w, h, NEAR, p(t[5]), V, p(out[0]), p(out[1]), p(ws), nws, ops._st())
    torch.cuda.synchronize()
    kept = {k: v.cpu().numpy() for k, v in ops.silhouette_workspace_views(ws, B, V, h, w).items()}
    for b, ref in enumerate(c["ref"]):
        ok = ref["valid"]
        assert ok.sum() == c["nv"][b]
        assert np.array_equal(kept["nearest"][b], ref["nearest"]), (which, b)
        assert np.array_equal(kept["cell"][b], np.where(ok, ref["cell"][:, 1] * w + ref["cell"][:, 0], -1)), (which, b)
        assert np.array_equal(kept["u"][b][ok], ref["u"][ok]) and np.array_equal(kept["v"][b][ok], ref["v"][ok]), (which, b)
        assert kept["den"][b, 1] == (c["cover"][b] > 0.5).sum() and abs(kept["den"][b, 0] - c["w"][b, :c["nv"][b]].astype(np.float64).sum()) < 1e-9
        assert float(out[0, b]) == result(which)["inside"][b] and float(out[1, b]) == result(which)["cover"][b]


@pytest.mark.parametrize("which", ["three", "one"])
def test_values_and_gradients_against_the_oracle(which):
    c, got = case(which), result(which)
    for b, ref in enumerate(c["ref"]):
        for k in ("inside", "cover"):
            print(f"{which} sample {b}: {k} = {got[k][b]:.7f} px, fp64 {ref[k]:.7f} px, off by {abs(float(got[k][b]) - ref[k]):.2e}")
            assert within_one_ulp(got[k][b], ref[k]), (which, b, k)
        assert_gradient(got["d_verts"][b], ref, f"{which} sample {b}")
        assert np.abs(ref["d_verts"]).max() > 1.0
        assert not got["d_verts"][b, c["nv"][b]:].any()           # padding rows: exactly zero


def test_two_calls_give_the_same_bits():
    first, again = result(), run(case())
    for k in first:
        assert np.array_equal(first[k].view(np.uint32), again[k].view(np.uint32)), k


def test_a_batch_is_its_samples():
    c, got = case(), result()
    for b in range(3):
        one = run(c, slice(b, b + 1))
        for k in got:
            assert one[k].shape[0] == 1 and np.array_equal(one[k].view(np.uint32), got[k][b:b + 1].view(np.uint32)), (b, k)


def test_shared_weights_and_none():
    c = case()
    shared, none = run(c, weight=c["w"][1]), run(c, weight=None)
    tiled = run(c, weight=np.repeat(c["w"][1:2], 3, 0))
    for k in shared:
        assert np.array_equal(shared[k].view(np.uint32), tiled[k].view(np.uint32)), k
    for b in range(3):
        for got, wt in ((shared, c["w"][1]), (none, None)):
            ref = S.silhouette_loss(c["verts"][b], int(c["nv"][b]), c["K"][b], c["d2"][b], c["cover"][b], wt, NEAR, *c["G"][b])
            assert within_one_ulp(got["inside"][b], ref["inside"]) and within_one_ulp(got["cover"][b], ref["cover"])
            assert_gradient(got["d_verts"][b], ref, f"sample {b}, weights {'shared' if wt is not None else 'None'}")


def test_what_takes_no_part_gets_zero_gradient():
    c = case()
    verts = c["verts"].copy()
    verts[0, 5, 2] = 0.005                                       # behind near
    verts[1, 9, 1] = np.nan
    verts[1, 10, 0] = np.inf
    got = run(c, verts=verts)
    assert np.isfinite(got["d_verts"]).all() and np.isfinite(got["inside"]).all() and np.isfinite(got["cover"]).all()
    assert not got["d_verts"][0, 5].any() and not got["d_verts"][1, 9].any() and not got["d_verts"][1, 10].any()
    for b in range(3):
        ref = S.silhouette_loss(verts[b], int(c["nv"][b]), c["K"][b], c["d2"][b], c["cover"][b], c["w"][b], NEAR, *c["G"][b])
        assert ref["valid"].sum() == c["nv"][b] - (1, 2, 0)[b]
        assert within_one_ulp(got["inside"][b], ref["inside"]) and within_one_ulp(got["cover"][b], ref["cover"])
        assert_gradient(got["d_verts"][b], ref, f"sample {b} with invalid vertices")
        assert not got["d_verts"][b, c["nv"][b]:].any()
    # an empty allow mask: inside = 0 and nothing comes back from it; an empty cover mask likewise
    d2 = c["d2"].copy()
    d2[1] = S.EDT_NONE
    only_inside = np.array([[1.0, 0.0]] * 3)
    got = run(c, d2=d2, g=only_inside)
    assert got["inside"][1] == 0 and not got["d_verts"][1].any() and got["inside"][0] > 0 and got["d_verts"][0].any()
    assert got["cover"][1] == result()["cover"][1]
    cover = c["cover"].copy()
    cover[2] = 0
    got = run(c, cover=cover, g=1 - only_inside)
    assert got["cover"][2] == 0 and not got["d_verts"][2].any() and got["cover"][0] > 0 and got["d_verts"][0].any()
    assert got["inside"][2] == result()["inside"][2]
    # no vertex that counts at all
    none = ops.silhouette_loss(gpu(c["verts"]), gpu(c["K"]), gpu(c["d2"]), gpu(c["cover"]), torch.zeros(3, dtype=torch.int32))
    assert not none[0].any() and not none[1].any()
    with pytest.raises(ValueError, match="weight"):
        ops.silhouette_loss(gpu(c["verts"]), gpu(c["K"]), gpu(c["d2"]), gpu(c["cover"]), weight=torch.ones(5))
    with pytest.raises(ValueError, match="allow_d2"):
        ops.silhouette_loss(gpu(c["verts"]), gpu(c["K"]), gpu(c["d2"][:2]), gpu(c["cover"]))
    with pytest.raises(ops._lib.HoisdfError, match="near"):
        ops.silhouette_loss(gpu(c["verts"]), gpu(c["K"]), gpu(c["d2"]), gpu(c["cover"]), near=0.0)


# ---- the model -------------------------------------------------------------------------------------------------------------------------
def _small_cfg():
    from hoisdf_amd.config import Config
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = 96, 32
    return c


HEADS = ("linear_pose", "linear_obj_rot", "linear_obj_rel_trans")     # the MANO head's pose input and the two vote heads


def _trainer_step(on):
    from hoisdf_amd.engine import Trainer
    c = _small_cfg()
    c.sdf_source = "mesh"
    c.silhouette_loss = on
    tr = Trainer(c, torch.device("cuda", 0), batch_size=2, tune_encoder=False)
    inputs, targets, meta = next(iter(tr.batch_generator))
    total, loss = tr.train_step(inputs, targets, meta, 0, 0.0)
    torch.cuda.synchronize()
    grads = {n: torch.cat([p.grad.detach().flatten().clone() for p in getattr(tr.model, n).parameters()]) for n in HEADS}
    return tr, float(total), {k: float(v) for k, v in loss.items()}, grads


def test_one_trainer_step_with_and_without_the_loss(monkeypatch):
    monkeypatch.delenv("HOISDF_SILHOUETTE_LOSS", raising=False)
    monkeypatch.delenv("HOISDF_INTERACTION_LOSS", raising=False)
    was = ops.deterministic()
    ops.set_deterministic(True)                                # order-fixed gradients: a difference below is the loss's, not the atomics'
    det, bench = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        _, total_off, loss_off, g_off = _trainer_step(False)
        tr, total_on, loss_on, g_on = _trainer_step(True)
    finally:
        ops.set_deterministic(was)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det, bench
    assert "silhouette_in" not in loss_off and "silhouette_cover" not in loss_off and tr.interaction_source is tr.sdf_source
    assert set(loss_on) == set(loss_off) | {"silhouette_in", "silhouette_cover"}
    for k, v in loss_off.items():                              # every other entry: the same bits
        assert struct.pack("<d", v) == struct.pack("<d", loss_on[k]), (k, v, loss_on[k])
    print("silhouette_in", loss_on["silhouette_in"], "silhouette_cover", loss_on["silhouette_cover"], "total", total_on, "without", total_off)
    assert np.isfinite(total_on) and loss_on["silhouette_in"] >= 0 and loss_on["silhouette_cover"] > 0
    assert np.isfinite(loss_on["silhouette_in"]) and np.isfinite(loss_on["silhouette_cover"])
    for n in HEADS:
        assert torch.isfinite(g_on[n]).all() and g_on[n].any() and not torch.equal(g_on[n], g_off[n]), n


def test_the_mask_grid_camera_puts_the_minimum_at_the_label_pose():
    """the masks of the label meshes (MeshSegSource) against those same meshes shifted sideways by -1 .. +1 mask pixels' worth of
    metres: silhouette_in + silhouette_cover is smallest at shift 0, with the raster sampled at pixel corners and at pixel centres"""
    from hoisdf_amd.engine import SyntheticMeshSdfDataset
    from hoisdf_amd.nets.mano import ManoLayer
    from hoisdf_amd.render import MeshSegSource, mask_camera_rows
    from hoisdf_amd.sdf_data import procedural_templates
    for half in (False, True):
        c = _small_cfg()
        c.raster_half_pixel = half
        seg = MeshSegSource(ManoLayer().to(DEV), c, templates=procedural_templates())
        ds = SyntheticMeshSdfDataset(c, seg.n_templates, seed=3)
        _, targets, meta = next(iter(torch.utils.data.DataLoader(ds, batch_size=2)))
        tg, mt = {k: v.to(DEV) for k, v in targets.items()}, {k: v.to(DEV) for k, v in meta.items()}
        masks = seg.render(tg, mt, want=())
        hand, _, obj, _, _ = seg.meshes(tg, mt)
        nv = seg.source.templates["n_verts"][mt["obj_cls"].long()]
        K = mask_camera_rows(mt["cam_intr"], c)
        allow = ops.mask_edt(masks["hand_seg"], masks["obj_seg"])
        assert masks["hand_seg"].sum() > 100 and masks["obj_seg"].sum() > 20
        per_pixel = hand[:, :, 2].mean(1) / K[:, 0]             # metres along x that move the projection by one mask pixel
        totals = []
        for shift in (-1.0, -0.5, 0.0, 0.5, 1.0):
            d = torch.zeros_like(hand[:, :1])
            d[:, 0, 0] = shift * per_pixel
            ih, ch = ops.silhouette_loss(hand + d, K, allow, masks["hand_seg"], near=c.raster_near)
            io, co = ops.silhouette_loss(obj + d, K, allow, masks["obj_seg"], n_verts=nv, near=c.raster_near)
            totals.append((ih + ch + io + co).cpu().numpy())
        totals = np.stack(totals)                                # [shift][sample]
        print(f"half_pixel {half}: in + cover per shift of -1, -0.5, 0, 0.5, 1 mask pixels:\n{np.round(totals, 4)}")
        assert (totals.argmin(0) == 2).all(), totals


def test_the_ik_variant_refuses_the_loss():
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import get_model
    c = Config()
    c.resnet_type = 18
    c.apply_setting("ho3d_render")
    c.silhouette_loss = True
    with pytest.raises(ValueError, match="silhouette_loss"):
        get_model("train", cfg=c, with_encoder=False)


# ---- C host ----------------------------------------------------------------------------------------------------------------------------
def test_c_host_silhouette_loss(tmp_path):
    """A plain C host (tests/c/test_silhouette_loss_host.c: the distance transform, one forward and one backward call on the dumped
    three-sample case) agrees with the oracle and gets the bits the Python calls get"""
    c, got = case(), result()

    def arr(f, a, dt):
        a = np.ascontiguousarray(a).reshape(-1).astype(dt)
        f.write(struct.pack("<q", a.size))
        f.write(a.tobytes())

    src, dst = str(tmp_path / "silhouette_loss_in.bin"), str(tmp_path / "silhouette_loss_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4i1f", 3, 192, c["wd"], c["h"], NEAR))
        arr(f, c["verts"], "<f4"), arr(f, c["nv"], "<i4"), arr(f, c["K"], "<f4"), arr(f, c["allow"], "<f4"), arr(f, c["cover"], "<f4")
        arr(f, c["w"], "<f4"), arr(f, c["G"].T, "<f4")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_silhouette_loss_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_silhouette_loss_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    res = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0 and "c host silhouette loss ok" in res.stdout, res.stdout + res.stderr
    words = np.fromfile(dst, dtype="<u4")
    npix = 3 * c["h"] * c["wd"]
    assert len(words) == npix + 6 + 3 * 192 * 3
    assert np.array_equal(words[:npix].view(np.int32).reshape(c["d2"].shape), c["d2"])
    vals = words[npix:].view(np.float32)
    for b, ref in enumerate(c["ref"]):
        assert within_one_ulp(vals[b], ref["inside"]) and within_one_ulp(vals[3 + b], ref["cover"])
        assert_gradient(vals[6:].reshape(3, 192, 3)[b], ref, f"c host, sample {b}")
    assert np.array_equal(words[npix:npix + 3], got["inside"].view(np.uint32)) and np.array_equal(words[npix + 3:npix + 6], got["cover"].view(np.uint32))
    assert np.array_equal(words[npix + 6:], got["d_verts"].reshape(-1).view(np.uint32))
