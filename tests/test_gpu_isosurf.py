"""GPU: csrc/isosurf.hip against hoisdf_amd/isosurf_oracle.py.  The extraction is compared EXACTLY - counts, faces and the bits of
every vertex - with the oracle's float32 mode on the same uploaded float32 field; the refined grid and the node positions
likewise; hoisdf_eval_surface against a float64 brute force.  Every input is an analytic field."""
import ctypes as C

import numpy as np
import pytest
import torch

from hoisdf_amd import _lib, ops
from hoisdf_amd import isosurf_oracle as iso
from hoisdf_amd.mesh_sdf_oracle import icosphere

pytestmark = pytest.mark.gpu
EPS32 = float(np.finfo(np.float32).eps)
# n = 5: 125 nodes, less than one block of 256; 9: 729, three blocks, the last partly filled; 17: 4913 nodes, 20 blocks, no multiple
# of the block; 41: 68921 nodes = 270 blocks, MORE than the 256 threads of the scan over a sample's block totals, so a thread of
# that scan owns two blocks: the shuffle scan inside a wave, the offsets across the four waves, the serial run of a thread over
# its blocks and the block offsets added in the vertex and face kernels are all crossed.  (128^3 nodes make 8192 blocks = 32 per
# thread: the same code, a longer run.)
SIZES = (5, 9, 17, 41)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def batches():
    """n -> (grid (3, 8), values (3, n^3), [(verts, faces)] of the float32 oracle): three different fields in one batch - a sphere,
    an empty sample, a torus on an anisotropic grid - so the per-sample offsets and a zero count between two full ones are used"""
    out = {}
    for n in SIZES:
        g = np.stack([iso.cube_grid(-0.5, 0.5, n), iso.cube_grid(-0.5, 0.5, n),
                      np.float32([-0.55, -0.5, -0.45, 1.1 / (n - 1), 1.0 / (n - 1), 0.9 / (n - 1), 0, 0])])
        vals = np.stack([iso.sphere_field(iso.grid_points(g[0], n, np.float64)), np.ones(n ** 3, np.float32),
                         iso.torus_field(iso.grid_points(g[2], n, np.float64))])
        out[n] = (g, vals, [iso.extract(vals[b], g[b], n, 0.0, np.float32) for b in range(3)])
    return out


def _raw_extract(values, ld, grid, n, B, iso_level=0.0, verts=None, faces=None, scale=1.0, shift=None):
    dev = grid.device
    nws = _lib.lib().hoisdf_iso_extract_workspace_bytes(B, n)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    nv = torch.full((B,), -7, device=dev, dtype=torch.int32)
    nf = torch.full((B,), -7, device=dev, dtype=torch.int32)
    _lib.call("hoisdf_iso_extract", _ptr(values), ld, _ptr(grid), n, B, iso_level, scale, _ptr(shift), _ptr(verts),
              0 if verts is None else verts.shape[1], _ptr(faces), 0 if faces is None else faces.shape[1], _ptr(nv), _ptr(nf), _ptr(ws),
              nws, _stream())
    return nv.cpu().numpy(), nf.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("n", SIZES)
def test_extract_equals_the_float32_oracle_exactly(batches, n):
    g, vals, ref = batches[n]
    grid, values = torch.from_numpy(g).cuda(), torch.from_numpy(vals).cuda()
    verts, faces, nv, nf = ops.iso_surface(values, grid, n)
    nv, nf = nv.cpu().numpy(), nf.cpu().numpy()
    assert nv.tolist() == [len(r[0]) for r in ref] and nf.tolist() == [len(r[1]) for r in ref]
    assert nv[1] == 0 and nf[1] == 0 and nv[0] > 0 and nv[2] > 0
    assert verts.shape == (3, nv.max(), 3) and faces.shape == (3, nf.max(), 3), "sized from the counts: an exact allocation"
    for b in range(3):
        assert np.array_equal(faces[b, :nf[b]].cpu().numpy(), ref[b][1]), (n, b)
        assert _same_bits(verts[b, :nv[b]].cpu().numpy(), ref[b][0]), (n, b)
    again = ops.iso_surface(values, grid, n)
    assert all(torch.equal(x, y) for x, y in zip(again, (verts, faces, torch.from_numpy(nv).cuda(), torch.from_numpy(nf).cuda())))


def test_extract_reads_a_strided_column_and_applies_scale_and_shift(batches):
    n = 9
    g, vals, _ = batches[n]
    grid = torch.from_numpy(g).cuda()
    rows = torch.full((3, n ** 3, 3), float("nan"), device="cuda")
    rows[..., 1] = torch.from_numpy(vals).cuda()
    shift = np.float32([[0.01, -0.02, 0.6], [0.0, 0.0, 0.5], [-0.03, 0.04, 0.7]])
    scale = float(np.float32(1.0 / 3.1))
    verts, faces, nv, nf = ops.iso_surface(rows[..., 1], grid, n, out_scale=scale, out_shift=torch.from_numpy(shift).cuda())
    for b in range(3):
        rv, rf = iso.extract(vals[b], g[b], n, 0.0, np.float32, out_scale=scale, out_shift=shift[b])
        assert int(nv[b]) == len(rv) and int(nf[b]) == len(rf)
        assert np.array_equal(faces[b, :len(rf)].cpu().numpy(), rf) and _same_bits(verts[b, :len(rv)].cpu().numpy(), rv), b


def test_extract_counts_only_and_keeps_to_its_capacities(batches):
    n = 17
    g, vals, ref = batches[n]
    grid, values = torch.from_numpy(g).cuda(), torch.from_numpy(vals).cuda()
    need_v, need_f = [len(r[0]) for r in ref], [len(r[1]) for r in ref]
    nv, nf = _raw_extract(values, 1, grid, n, 3)                                  # both outputs NULL: the call only counts
    assert nv.tolist() == need_v and nf.tolist() == need_f
    cap_v, cap_f = max(need_v) - 1, max(need_f) - 1                               # one below the largest need: sample 0 or 2 overflows
    # sample b's rows start at b x capacity: what lies beyond a capacity is the next sample's first row, or - for the last sample -
    # the 16 guard rows behind the buffers
    vflat = torch.full((3 * cap_v + 16, 3), -123.0, device="cuda")
    fflat = torch.full((3 * cap_f + 16, 3), -77, device="cuda", dtype=torch.int32)
    vbuf, fbuf = vflat[:3 * cap_v].view(3, cap_v, 3), fflat[:3 * cap_f].view(3, cap_f, 3)
    nv, nf = _raw_extract(values, 1, grid, n, 3, verts=vbuf, faces=fbuf)
    assert nv.tolist() == need_v and nf.tolist() == need_f, "the counts still report the need"
    for b in range(3):
        kv, kf = min(need_v[b], cap_v), min(need_f[b], cap_f)
        assert _same_bits(vbuf[b, :kv].cpu().numpy(), ref[b][0][:kv]) and np.array_equal(fbuf[b, :kf].cpu().numpy(), ref[b][1][:kf])
        assert torch.all(vbuf[b, kv:] == -123.0) and torch.all(fbuf[b, kf:] == -77), "rows from the count on keep their canary"
    assert torch.all(vflat[3 * cap_v:] == -123.0) and torch.all(fflat[3 * cap_f:] == -77), "nothing is written beyond the capacity"
    assert int(fbuf.max()) == max(need_v) - 1, "a written face names the vertex beyond the capacity by its true id"


def test_refine_grid_equals_the_oracle_exactly():
    n, n_out = 9, 17
    g = np.stack([iso.cube_grid(-1.0, 1.0, n), np.float32([-1.0, -0.8, -1.2, 0.25, 0.2, 0.3, 0, 0]), iso.cube_grid(-1.0, 1.0, n)])
    fields = [iso.sphere_field(iso.grid_points(g[0], n, np.float64), (0.1, -0.05, 0.2), 0.3),          # well inside: no clipping
              iso.sphere_field(iso.grid_points(g[1], n, np.float64), (-0.9, 0.7, -1.1), 0.5),          # at a corner: clipped on three sides
              np.ones(n ** 3, np.float32)]                                                            # no inside node: the fallback
    vals = np.stack(fields)
    rows = torch.zeros(3, n ** 3, 2, device="cuda")
    rows[..., 0] = torch.from_numpy(vals).cuda()
    for pad in (0, 1, 3):
        got = ops.iso_refine_grid(rows[..., 0], torch.from_numpy(g).cuda(), n, 0.0, pad, n_out).cpu().numpy()
        for b in range(3):
            assert _same_bits(got[b], iso.refine_grid(vals[b], g[b], n, 0.0, pad, n_out)), (pad, b)
    assert np.array_equal(got[2][:3], g[2][:3]) and got[1][0] == g[1][0] and got[0][0] > g[0][0]


def test_grid_points_equal_the_oracle_exactly():
    n = 7
    g = np.float32([[-1.0, 0.5, 2.0, 0.1, 0.2, 0.3, 0, 0], [0.3, -0.7, 0.01, 1.0 / 3, 1e-3, 7.0, 0, 0]])
    pts, idx = ops.iso_grid_points(torch.from_numpy(g).cuda(), n)
    assert pts.shape == (2 * n ** 3, 3) and idx.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), np.repeat(np.arange(2, dtype=np.int32), n ** 3))
    assert _same_bits(pts.cpu().numpy(), np.concatenate([iso.grid_points(g[b], n) for b in range(2)]))


def test_eval_surface_against_float64_brute_force():
    """Bound, per direction: 1e-6 relative plus the per-point bound carried through the square.  A coordinate enters with at most
    delta = 8 eps32 max|coordinate| of error (the subtraction of the mesh's centre or of the other point at camera depth, and a few
    operations at the size of the mesh), a distance d therefore with at most delta, its square with 2 d delta + delta^2, and the
    mean of that over the points is at most 2 sqrt(mean d^2) delta + delta^2."""
    rng = np.random.default_rng(5)
    gv, gf = icosphere(0)                                                         # 12 vertices, 20 faces
    B, max_verts, n_samples = 5, 300, 700
    centre = np.array([0.02, -0.03, 0.6])
    gt = np.stack([(0.05 * (1 + 0.1 * b) * gv + centre).astype(np.float32) for b in range(B)])
    n_verts = np.int32([300, 50, 0, 123, 77])
    gt_n_faces = np.int32([20, 20, 20, 20, 0])                                    # the last sample has no ground-truth face
    d = rng.normal(size=(B, max_verts, 3))
    pred = (centre + 0.05 * (1 + 0.2 * rng.uniform(-1, 1, (B, max_verts, 1))) * d / np.linalg.norm(d, axis=2, keepdims=True)).astype(np.float32)
    pred[0, 7] = pred[0, 3]                                                       # an exact tie: the lower index must win
    out = ops.eval_surface(torch.from_numpy(pred).cuda(), torch.from_numpy(n_verts).cuda(), torch.from_numpy(gt).cuda(),
                           torch.from_numpy(gf).cuda(), torch.from_numpy(gt_n_faces).cuda(), n_samples=n_samples, seed=11, extras=True)
    again = ops.eval_surface(torch.from_numpy(pred).cuda(), torch.from_numpy(n_verts).cuda(), torch.from_numpy(gt).cuda(),
                             torch.from_numpy(gf).cuda(), torch.from_numpy(gt_n_faces).cuda(), n_samples=n_samples, seed=11, extras=True)
    assert all(torch.equal(out[k], again[k]) for k in out), "two calls give the same bits"
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert got["n_used"].tolist() == [300, 50, 0, 123, 0]
    delta = 8 * EPS32 * float(max(np.abs(pred).max(), np.abs(gt).max()))
    for b in range(B):
        ref = iso.eval_surface(pred[b, :n_verts[b]], gt[b], gf[:gt_n_faces[b]], got["samples"][b])
        if ref["n_used"] == 0:
            assert got["pred_to_gt"][b] == 0 and got["gt_to_pred"][b] == 0 and got["chamfer"][b] == 0
            continue
        # the drawn points lie on the surface: their float64 distance to the mesh is rounding only
        on = iso.point_triangle_d2(got["samples"][b].astype(np.float64)[:, None], *(gt[b].astype(np.float64)[gf[:, k]][None] for k in range(3))).min(1)
        assert np.sqrt(on.max()) <= delta, (b, np.sqrt(on.max()))
        for k in ("pred_to_gt", "gt_to_pred"):
            tol = 1e-6 * ref[k] + 2 * np.sqrt(ref[k]) * delta + delta ** 2
            err = abs(float(got[k][b]) - ref[k])
            print(f"sample {b} {k}: {got[k][b]:.9e} reference {ref[k]:.9e} error {err:.2e} bound {tol:.2e}")
            assert err <= tol, (b, k, err, tol)
        assert abs(float(got["chamfer"][b]) - ref["chamfer"]) <= 2e-6 * ref["chamfer"] + 4 * np.sqrt(ref["chamfer"]) * delta
        s64, p64 = got["samples"][b].astype(np.float64), pred[b, :n_verts[b]].astype(np.float64)
        d2 = ((s64[:, None] - p64[None]) ** 2).sum(-1)
        srt = np.sort(d2, 1)
        clear = srt[:, 1] - srt[:, 0] > 4 * np.sqrt(srt[:, 1]) * delta            # the nearest is decided beyond rounding
        assert np.array_equal(got["nearest"][b][clear], d2.argmin(1)[clear])
    assert not np.any(got["nearest"][0] == 7), "vertex 7 copies vertex 3: wherever it is the nearest, the lower index wins the tie"
    assert np.all(got["nearest"][2] == -1)


# ---- Model.field_surface: plumbing on the small model the GPU model tests build (no trained weights exist) --------------------------
FIELD_N, FIELD_COARSE = 17, 9


@pytest.fixture(scope="module")
def small_model():
    from hoisdf_amd import testing as T
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import get_model
    from hoisdf_amd.nets import mano as MANO
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = 300, 100
    model = get_model("test", cfg=c, mano_layer=MANO.ManoLayer(MANO.synthetic_assets(0)), with_encoder=False)
    sd = model.state_dict()
    for k in sd:
        if not k.startswith("mano_head"):
            sd[k] = T.det_param(k, sd[k].shape)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    B = 2
    pyr_cpu = T.synthetic_pyramid(B, seed=4)
    pyr = ops.PyramidNHWC([v.cuda().permute(0, 2, 3, 1).contiguous() for v in pyr_cpu.values()])
    _, _, meta = T.synthetic_batch(B, 300, 8, seed=5)
    dm = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in meta.items()}
    res = {kind: model.field_surface(pyr, dm, kind, n=FIELD_N, coarse_n=FIELD_COARSE, return_values=True) for kind in ("hand", "obj")}
    return model, c, pyr, pyr_cpu, meta, dm, res


@pytest.mark.parametrize("kind", ["hand", "obj"])
def test_field_surface_is_the_oracle_on_its_own_values(small_model, kind):
    model, c, _, _, meta, _, res = small_model
    verts, faces, nv, nf, ex = res[kind]
    scale = c.hand_sdf_scale if kind == "hand" else c.obj_sdf_scale
    centre = (meta["mano_root"] if kind == "hand" else meta["obj_center_cam"]).numpy().reshape(-1, 3)
    values, grid = ex["values"].cpu().numpy(), ex["grid"].cpu().numpy()
    coarse, coarse_grid = ex["coarse_values"].cpu().numpy(), ex["coarse_grid"].cpu().numpy()
    nv, nf = nv.cpu().numpy(), nf.cpu().numpy()
    print(kind, "vertices", nv.tolist(), "faces", nf.tolist())
    assert nv.min() > 0, "the deterministic weights give a field with a zero level set: the comparison is not empty"
    assert verts.shape == (2, nv.max(), 3) and faces.shape == (2, nf.max(), 3)
    for b in range(2):
        assert _same_bits(coarse_grid[b], iso.cube_grid(-1.0, 1.0, FIELD_COARSE))
        assert _same_bits(grid[b], iso.refine_grid(coarse[b], coarse_grid[b], FIELD_COARSE, 0.0, 1, FIELD_N))
        # camera metres = the scaled-frame vertex / scale + centre: x * (1 / scale) + centre, product, then sum
        rv, rf = iso.extract(values[b], grid[b], FIELD_N, 0.0, np.float32, out_scale=1.0 / scale, out_shift=centre[b])
        assert nv[b] == len(rv) and nf[b] == len(rf)
        assert np.array_equal(faces[b, :nf[b]].cpu().numpy(), rf) and _same_bits(verts[b, :nv[b]].cpu().numpy(), rv), (kind, b)
        sv, _ = iso.extract(values[b], grid[b], FIELD_N, 0.0, np.float32)
        assert _same_bits(rv, sv * np.float32(1.0 / scale) + centre[b].astype(np.float32))


def test_field_values_agree_with_the_cpu_oracle(small_model):
    """the bar of test_gpu_ops.py::test_sdf_query_one_call_matches_the_op_chain: 2e-5 of the tensor's scale, on the clamped sdf (what
    oracle.sdf_forward returns); the extraction reads the unclamped value, which differs only beyond the clamp"""
    from hoisdf_amd import testing as T
    from oracle import hoisdf_oracle as R
    model, c, _, pyr_cpu, meta, _, res = small_model
    ex = res["hand"][4]
    pts = torch.stack([torch.from_numpy(iso.grid_points(g, FIELD_N)) for g in ex["grid"].cpu().numpy()])
    P_ = T.det_params(T.hot_path_param_shapes(992))
    o_sdf, _ = R.sdf_forward(P_, R.OracleCfg(), pyr_cpu, pts, meta["mano_root"], meta["cam_intr"], c.hand_sdf_scale, "hand", False)
    got = ex["values"].cpu().clamp(-c.ClampingDistance, c.ClampingDistance).reshape(-1).double()
    ref = o_sdf.reshape(-1).double()
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"field values against the oracle: max error {err:.3e}, scale {scale:.3e}")
    assert err <= 2e-5 * scale + 1e-12


@pytest.mark.parametrize("kind", ["hand", "obj"])
def test_field_surface_does_not_depend_on_chunks_or_on_the_module_mode(small_model, kind):
    model, _, pyr, _, _, dm, res = small_model
    verts, faces, nv, nf, ex = res[kind]
    # 2 x 17^3 = 9826 rows in chunks of at most 4096: three chunks of 3328, 3328 and 3170 rows - both boundaries inside a sample
    # (4913 rows each), every chunk above the 2047 rows at which the small-row GEMM would take over
    chunked = model.field_surface(pyr, dm, kind, n=FIELD_N, coarse_n=FIELD_COARSE, return_values=True, chunk_rows=4096)
    model.train()                                                                 # decoder dropout would be on
    try:
        trained = model.field_surface(pyr, dm, kind, n=FIELD_N, coarse_n=FIELD_COARSE, return_values=True)
    finally:
        model.eval()
    for other in (chunked, trained):
        assert torch.equal(other[4]["values"], ex["values"]) and torch.equal(other[4]["coarse_values"], ex["coarse_values"])
        assert all(torch.equal(x, y) for x, y in zip(other[:4], (verts, faces, nv, nf)))
    # fixed capacities: no read-back, the same rows; a box instead of the lattice cube
    cap = model.field_surface(pyr, dm, kind, n=FIELD_N, coarse_n=FIELD_COARSE, max_verts=int(nv.max()) + 5, max_faces=int(nf.max()) + 5)
    assert torch.equal(cap[2], nv) and torch.equal(cap[0][:, :verts.shape[1]], verts) and torch.equal(cap[1][:, :faces.shape[1]], faces)
    box = torch.tensor([[[-0.5, -0.5, -0.5], [0.5, 0.25, 0.5]], [[-1.0, -1.0, 0.0], [0.0, 1.0, 1.0]]], device="cuda")
    boxed = model.field_surface(pyr, dm, kind, n=FIELD_N, coarse_n=FIELD_COARSE, box=box, return_values=True)[4]
    assert torch.equal(boxed["coarse_grid"][:, :3], box[:, 0])
    assert _same_bits(boxed["coarse_grid"][:, 3:6].cpu().numpy(), ((box[:, 1] - box[:, 0]) / float(FIELD_COARSE - 1)).cpu().numpy())


# ---- the opt-in outputs of the eval forward and the Evaluator's Field block ------------------------------------------------------------
def test_eval_forward_adds_the_surfaces_only_when_asked(monkeypatch):
    """the existing synthetic evaluation (tests/test_gpu_eval_native.py: ResNet-18, 96 + 32 points, B = 2) with the switch off and on, on
    both eval paths: the same tensors plus the eight field outputs in their fixed-capacity shapes, by the configuration and by the
    environment"""
    from hoisdf_amd import testing as T
    from hoisdf_amd.config import Config
    from hoisdf_amd.engine import Tester
    from hoisdf_amd.nets import mano as MANO
    monkeypatch.delenv("HOISDF_FIELD", raising=False)
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = 96, 32
    c.field_grid, c.field_max_verts = 12, 3000
    assert c.eval_field is False
    torch.manual_seed(0)
    tester = Tester(c, torch.device("cuda", 0))
    ml = MANO.ManoLayer(MANO.synthetic_assets(0)).cuda()
    inputs, targets, meta = T.synthetic_batch(2, 96, 32, seed=5)
    for native in (False, True):
        c.native_infer = native
        c.eval_field = False
        off = {k: v.detach().clone() for k, v in tester.predict(inputs, targets, meta, mano_layer=ml).items() if torch.is_tensor(v)}
        off2 = {k: v.detach().clone() for k, v in tester.predict(inputs, targets, meta, mano_layer=ml).items() if torch.is_tensor(v)}
        c.eval_field = True
        on = {k: v.detach().clone() for k, v in tester.predict(inputs, targets, meta, mano_layer=ml).items() if torch.is_tensor(v)}
        c.eval_field = False
        monkeypatch.setenv("HOISDF_FIELD", "1")
        env = tester.predict(inputs, targets, meta, mano_layer=ml)
        monkeypatch.delenv("HOISDF_FIELD")
        added = {f"field_{kind}_{what}" for kind in ("hand", "obj") for what in ("verts", "faces", "n_verts", "n_faces")}
        assert not any(k.startswith("field_") for k in off) and set(on) == set(off) | added and added <= set(env), native
        # the option changes no other output: bit for bit where the eval forward itself repeats its bits, else to 1e-5 of the scale
        repeats = all(torch.equal(off2[k], off[k]) for k in off)
        print("native" if native else "python", "eval forward repeats its bits:", repeats)
        for k in off:
            if repeats or not off[k].is_floating_point():
                assert torch.equal(on[k], off[k]), (native, k)
            else:
                assert float((on[k] - off[k]).abs().max()) <= 1e-5 * max(float(off[k].abs().max()), 1e-30), (native, k)
        assert on["field_hand_verts"].shape == (2, 3000, 3) and on["field_obj_faces"].shape == (2, 6000, 3)
        assert on["field_hand_n_verts"].dtype == torch.int32 and on["field_hand_n_faces"].shape == (2,)
        assert all(env[k].shape == on[k].shape and env[k].dtype == on[k].dtype for k in added)
        if repeats:
            assert all(torch.equal(env[k], on[k]) for k in added), native
    c.native_infer = False


def _field_batches():
    """two batches of three (out, targets, meta, obj_cls) in the dexycb layout.  Ground truth: an icosphere of 5 cm as the 'hand', the
    procedural templates as objects.  Field surfaces: spheres extracted by ops.iso_surface around the hand's and the object's
    place, a few millimetres off; one empty hand surface, one object surface that overflows its capacity, one unknown object.
    -> (templates, hand faces, the batches, the vertex capacity)"""
    from hoisdf_amd.sdf_data import procedural_templates
    tmpl = procedural_templates()
    hand_v, hand_f = icosphere(2)
    r = np.random.default_rng(3)
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    n, cap = 13, 1400
    rec = []
    for it in range(2):
        B, P = 3, 8
        root = f32(r.uniform(-0.05, 0.05, (B, 3)) + [0, 0, 0.7])
        centre = root + f32(r.uniform(-1, 1, (B, 3)) * [0.03, 0.03, 0.01])
        out = {"mano_mesh_out": f32(np.repeat(0.05 * hand_v[None], B, 0) + r.normal(0, 0.002, (B, len(hand_v), 3))).cuda(),
               "mano_mesh_gt_out": f32(np.repeat(0.05 * hand_v[None], B, 0)).cuda(),
               "mano_joints_out": f32(r.normal(0, 0.03, (B, 21, 3))).cuda(), "mano_joints_gt_out": f32(r.normal(0, 0.03, (B, 21, 3))).cuda(),
               "obj_rot_out": f32(r.normal(0, 0.5, (B, P, 3))).cuda(), "obj_trans_out": f32(r.normal(0, 0.004, (B, P, 3))).cuda()}
        targets = {"obj_rot": f32(r.normal(0, 0.5, (B, 3))), "rel_obj_trans": f32(r.normal(0, 0.004, (B, 3)))}
        meta = {"mano_root": root, "obj_center_cam": centre}
        # radii of 3 to 4.7 cells give 490 to 1200 vertices; 5.25 cells (the first batch's last object) about 1540: over the capacity
        for kind, c0, radii in (("hand", root, (0.052, 0.057, 0.062)), ("obj", centre + targets["rel_obj_trans"], (0.04, 0.044, 0.07 if it == 0 else 0.048))):
            g = np.stack([iso.cube_grid(-0.08, 0.08, n)] * B)
            vals = np.stack([iso.sphere_field(iso.grid_points(g[b], n, np.float64), r.normal(0, 0.003, 3), radii[b]) for b in range(B)])
            if kind == "hand" and it == 1:
                vals[2] = 1.0                                                     # an empty surface
            v, f, nv, nf = ops.iso_surface(torch.from_numpy(vals).cuda(), torch.from_numpy(g).cuda(), n, 0.0, cap, 2 * cap,
                                           out_scale=1.0, out_shift=c0.cuda())
            out.update({f"field_{kind}_verts": v, f"field_{kind}_faces": f, f"field_{kind}_n_verts": nv, f"field_{kind}_n_faces": nf})
        cls = torch.tensor([[0, 1, 2], [2, -1, 1]][it])
        rec.append((out, targets, meta, cls))
    return tmpl, torch.from_numpy(hand_f), rec, cap


def test_evaluator_appends_the_field_block_and_is_silent_without_the_option(tmp_path):
    import re
    from hoisdf_amd import metrics as M
    from hoisdf_amd.config import Config
    tmpl, hand_f, rec, cap = _field_batches()
    c = Config()
    c.apply_setting("dexycb")
    c.eval_mesh = True
    c.field_samples = 600
    verts = tmpl["verts"].cuda()
    files = {}
    for name, kw in (("plain", {}), ("off", dict(field=False, template_faces=tmpl, hand_faces=hand_f)),
                     ("on", dict(field=True, template_faces=tmpl, hand_faces=hand_f))):
        ev = M.Evaluator(c, verts, native=True, **kw)
        for out, targets, meta, cls in rec:
            ev.feed(out, targets, meta, cls)
        files[name] = open(ev.write(str(tmp_path / name)), "rb").read()
    assert files["off"] == files["plain"] and b"Field" not in files["plain"]
    assert files["on"].startswith(files["plain"]) and len(files["on"]) > len(files["plain"])
    block = files["on"][len(files["plain"]):].decode()
    print(block)
    m = re.fullmatch(r"Field:\nhand_chamfer=([\d.]+) cm\^2, obj_chamfer=([\d.]+) cm\^2, hand_left_out=([\d.]+), obj_left_out=([\d.]+)\n", block)
    assert m, block
    # the same numbers from ops.eval_surface applied by hand; the seed of a feed is the number of samples fed before it
    sums = {"hand": [], "obj": []}
    left = {"hand": 0, "obj": 0}
    seen = 0
    for out, targets, meta, cls in rec:
        k = cls.clamp_min(0).cuda()
        gt_hand = out["mano_mesh_gt_out"] + meta["mano_root"].cuda()[:, None]
        R = M.batch_rodrigues(targets["obj_rot"].cuda())
        gt_obj = verts[k] @ R.transpose(1, 2) + (targets["rel_obj_trans"] + meta["obj_center_cam"]).cuda()[:, None]
        seen += len(cls)
        for kind, gv, gf, gn in (("hand", gt_hand, hand_f, None), ("obj", gt_obj, tmpl["faces"].cuda()[k], tmpl["n_faces"].cuda()[k])):
            res = ops.eval_surface(out[f"field_{kind}_verts"], out[f"field_{kind}_n_verts"], gv, gf, gn, n_samples=600, seed=seen)
            nv, nf = out[f"field_{kind}_n_verts"].cpu().numpy(), out[f"field_{kind}_n_faces"].cpu().numpy()
            for b in range(len(cls)):
                ok = nv[b] > 0 and nv[b] <= cap and nf[b] <= 2 * cap and (kind == "hand" or cls[b] >= 0)
                if ok:
                    sums[kind].append(float(res["chamfer"][b]) * 1e4)
                else:
                    left[kind] += 1
    print("per-sample Chamfer distances [cm^2]:", sums, "left out:", left)
    assert left["hand"] >= 1 and left["obj"] >= 1 and len(sums["hand"]) >= 3 and len(sums["obj"]) >= 3
    want = (np.mean(sums["hand"]), np.mean(sums["obj"]), left["hand"] / 6, left["obj"] / 6)
    for got, w, digits in zip(m.groups(), want, (4, 4, 3, 3)):
        assert abs(float(got) - w) <= 0.5 * 10 ** -digits + 1e-9, (got, w)
    # surfaces some millimetres to 2 cm off a 5 cm ball, the objects are not balls: square centimetres, and not a row of zeros
    assert 0.01 < want[0] < 10.0 and 0.01 < want[1] < 100.0
    with pytest.raises(ValueError, match="template_faces"):
        M.Evaluator(c, verts, native=True, field=True)


# ---- C host --------------------------------------------------------------------------------------------------------------------------
def test_c_host_iso_surface(tmp_path):
    """A plain C host (tests/c/test_iso_surface_host.c: a sphere sampled on the host, counted, extracted, checked closed, outward and of
    the right volume by the host itself) gets the mesh the oracle gets from the same field, bit for bit"""
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe, dst = str(tmp_path / "hoisdf_test_iso_surface_host"), str(tmp_path / "iso_out.bin")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_iso_surface_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    n = 33
    res = subprocess.run([exe, str(n), dst], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0 and "c host iso surface ok" in res.stdout, res.stdout + res.stderr
    raw = open(dst, "rb").read()
    hd = np.frombuffer(raw, "<i4", 3)
    assert hd[0] == n
    field = np.frombuffer(raw, "<f4", n ** 3, 12)
    verts = np.frombuffer(raw, "<f4", 3 * hd[1], 12 + 4 * n ** 3).reshape(-1, 3)
    faces = np.frombuffer(raw, "<i4", 3 * hd[2], 12 + 4 * n ** 3 + 12 * hd[1]).reshape(-1, 3)
    rv, rf = iso.extract(field, iso.cube_grid(-0.5, 0.5, n), n, 0.0, np.float32)
    assert len(rv) == hd[1] and len(rf) == hd[2] and np.array_equal(faces, rf) and _same_bits(verts, rv)
    rep = iso.mesh_report(verts, faces)
    assert rep["closed"] and rep["oriented"] and rep["euler"] == 2 and rep["volume"] > 0
