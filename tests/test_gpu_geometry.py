"""-m gpu: projection, bilinear gather and lattice held to inputs WITHOUT the symmetries every other test has.

Everywhere else cam_intr is one symmetric diagonal matrix repeated over the batch (fx == fy, cx == cy, zero off-diagonals), the boxes
are copies, the image is 256 x 256 and every pyramid level is square - reading K transposed, taking sample 0's K or box for every
sample, or exchanging H and W anywhere between Python and the kernels changes no number there.  Here (hoisdf_amd.testing.
asymmetric_geometry / nonsquare_pyramid): per-sample intrinsics rotated about the image centre with fx != fy, cx != cy, per-sample
boxes and centres, a 192 x 320 (and 320 x 192) image, levels of 96 x 160 ... 6 x 10 and of odd sizes.

The ratio rule.  With non-zero off-diagonals the three-term sum K . cam is not exact in any order, and one ulp of uv times a
pixel-to-pixel feature step puts the fp32 ORACLE ~6e-5 of the tensor's scale from its own fp64 run, so the old rel = 2e-5 bar against
the fp32 oracle does not carry over.  A kernel result is instead held to
    err(kernel, fp64) <= 3 x err(fp32 oracle, fp64) + 1e-12           (max-abs over the same tensor)
both being fp32 roundings of the same coordinate chain: another summation order may land on the other side of the truth (factor 2),
the third unit is slack.  A wrong geometry is off by O(1), five orders above that.

Every figure the checks compare is printed on a line starting with "GEOM" (pytest -s)."""
import random

import numpy as np
import pytest
import torch

from conftest import load_golden
from hoisdf_amd import testing as T
from test_gpu_model import build, nhwc_pyramid, oracle_cfg
from test_gpu_ops import _mlp_params, assert_close, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda"
HW = (192, 320)
SPECS = {"encoder": T.PYRAMID_ENCODER_LIKE, "encoder_big": T.PYRAMID_ENCODER_LIKE_BIG, "odd": T.PYRAMID_ODD}


def ops():
    from hoisdf_amd import ops as O
    return O


def oracle():
    from oracle import hoisdf_oracle as R
    return R


def ratio_rule(got, ref32, ref64, what, fails=None):
    """err(kernel, fp64) <= 3 x err(fp32 oracle, fp64) + 1e-12; with ``fails`` a violation is collected instead of raised"""
    got, ref32, ref64 = (t.detach().cpu().double() for t in (got, ref32, ref64))
    assert got.shape == ref64.shape == ref32.shape, (what, got.shape, ref32.shape, ref64.shape)
    e_k, e_o = float((got - ref64).abs().max()), float((ref32 - ref64).abs().max())
    scale = float(ref64.abs().max())
    print(f"GEOM ratio {what}: err(kernel, fp64) {e_k:.3e}  err(fp32 oracle, fp64) {e_o:.3e}  ratio {e_k / max(e_o, 1e-300):.2f}"
          f"  (scale {scale:.3e})")
    if not e_k <= 3.0 * e_o + 1e-12:
        msg = f"{what}: err(kernel, fp64) {e_k:.3e} > 3 x err(fp32 oracle, fp64) {e_o:.3e} (scale {scale:.3e})"
        if fails is None:
            raise AssertionError(msg)
        fails.append(msg)


def query_points(B, P, seed=5):
    """the first 150 rows of every sample uniform in +-0.45 (inside the image), the rest in +-2.5 (most of them outside)"""
    g = np.random.default_rng(seed)
    n_in = min(150, P)
    return torch.from_numpy(np.concatenate([g.uniform(-0.45, 0.45, (B, n_in, 3)), g.uniform(-2.5, 2.5, (B, P - n_in, 3))], 1).astype(np.float32))


# ---------------------------------------------------------------------------------------------
# op level: project + gather, forward and the three backward paths
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("img_hw", [(192, 320), (320, 192)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("spec", ["encoder", "encoder_big", "odd"])
def test_project_gather_forward_and_every_backward_path_against_fp64(spec, img_hw):
    """hoisdf_project_gather_fwd / _bwd against R.project_points + R.sample_pyramid (F.grid_sample) run in fp64, by the ratio rule;
    ``cam`` at rel = 1e-6.  B = 3, P = 301 (ragged against the four-rows-per-block grid).  In turn: the forward (C / 4 <= 256:
    gather_fwd4_kernel; "encoder_big": gather_fwd_kernel); the default backward (atomic + the two LDS-privatised coarse launches:
    240 and 60 pixels; "odd": a level of 8 channels and one of 64 at 561 pixels stay atomic); the deterministic backward (16 x 16
    tile owners, ragged tiles at 24 x 40 / 12 x 20 and at every odd level) directly against fp64; and the per-row sample_idx form
    with the samples' rows interleaved (plain atomic kernel), forward and backward.  (320, 192) runs the transposed levels: a swap
    that cancels in one orientation does not in the other."""
    O, R = ops(), oracle()
    B, P = 3, 301
    levels_spec = SPECS[spec] if img_hw == HW else T.transposed(SPECS[spec])
    pyr = T.nonsquare_pyramid(B, levels_spec, seed=4, nonneg=False)
    names = list(pyr)
    meta = T.asymmetric_geometry(B, img_hw)
    root, K = meta["mano_root"], meta["cam_intr"]
    pts = query_points(B, P)
    C = sum(c for c, _, _ in levels_spec)
    gy = rnd(B, P, C, seed=6)
    ref = {}
    for dt in (torch.float32, torch.float64):
        req = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in pyr.items()}
        cam, grid = R.project_points(pts.to(dt), root.to(dt), K.to(dt), 3.1, img_hw)
        feat = R.sample_pyramid(req, grid, names)
        feat.backward(gy.to(dt))
        ref[dt] = (feat.detach(), cam, [req[k].grad.permute(0, 2, 3, 1) for k in names], grid)
    f32, f64 = ref[torch.float32], ref[torch.float64]
    gx, gyy = f64[3][..., 0], f64[3][..., 1]
    out_x, out_y = (gx < -1) | (gx > 1), (gyy < -1) | (gyy > 1)
    share = float((out_x | out_y).double().mean())
    print(f"GEOM outside share {spec} {img_hw[0]}x{img_hw[1]}: {share:.3f} (x {float(out_x.double().mean()):.3f}, y {float(out_y.double().mean()):.3f})")
    assert 0.3 <= share <= 0.8, share                     # interior taps and both border clamps are all populated
    assert bool(out_x.any()) and bool(out_y.any()) and bool((~out_x & ~out_y).any())

    tag = f"{spec} {img_hw[0]}x{img_hw[1]}"
    fails = []
    rootd, Kd, ptsd, gyd = root.to(DEV), K.to(DEV), pts.to(DEV), gy.to(DEV)

    def levels():
        return [v.to(DEV).permute(0, 2, 3, 1).contiguous().requires_grad_(True) for v in pyr.values()]

    def check_grads(lv, what):
        for i, (l, (c, h, w)) in enumerate(zip(lv, levels_spec)):
            ratio_rule(l.grad, f32[2][i], f64[2][i], f"{tag} {what} d level {i} ({c}x{h}x{w})", fails)

    # forward + default backward
    lv = levels()
    feat, cam = O.project_gather(O.PyramidNHWC(lv), ptsd, rootd, Kd, 3.1, img_hw)
    ratio_rule(feat.view(B, P, -1), f32[0], f64[0], f"{tag} gather fwd", fails)
    assert_close(cam.view(B, P, 3), f32[1], rel=1e-6, what="cam")
    feat.backward(gyd.view(B * P, -1))
    check_grads(lv, "bwd default")
    # deterministic backward: tile owners
    keep_det = O.deterministic()
    O.set_deterministic(True)
    try:
        lv = levels()
        feat, _ = O.project_gather(O.PyramidNHWC(lv), ptsd, rootd, Kd, 3.1, img_hw)
        feat.backward(gyd.view(B * P, -1))
        first = [l.grad.clone() for l in lv]
        check_grads(lv, "bwd deterministic")
        lv = levels()
        feat, _ = O.project_gather(O.PyramidNHWC(lv), ptsd, rootd, Kd, 3.1, img_hw)
        feat.backward(gyd.view(B * P, -1))
        for i, (a, l) in enumerate(zip(first, lv)):
            if not torch.equal(a, l.grad):
                fails.append(f"{tag} deterministic backward of level {i} differs between two runs")
    finally:
        O.set_deterministic(keep_det)
    # per-row sample index, the samples' rows interleaved: the same sums in another row order
    perm = torch.from_numpy(np.random.default_rng(7).permutation(B * P))
    sidx = (perm // P).to(torch.int32)
    lv = levels()
    feat, cam = O.project_gather(O.PyramidNHWC(lv), ptsd.view(-1, 3)[perm.to(DEV)].contiguous(), rootd, Kd, 3.1, img_hw,
                                 sample_idx=sidx.to(DEV))
    ratio_rule(feat, f32[0].view(B * P, -1)[perm], f64[0].view(B * P, -1)[perm], f"{tag} ragged fwd", fails)
    assert_close(cam, f32[1].view(B * P, 3)[perm], rel=1e-6, what="ragged cam")
    feat.backward(gyd.view(B * P, -1)[perm.to(DEV)].contiguous())
    check_grads(lv, "bwd ragged")
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------
# op level: lattice
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [16, 20, 64])
@pytest.mark.parametrize("kind", ["hand", "obj"])
def test_lattice_candidates_with_per_sample_intrinsics_boxes_and_centres(kind, bins):
    """hoisdf_lattice_count / _fill with per-sample K, centre and box against R.lattice_bbox_mask per sample, at the conditions of
    test_lattice_candidates_match_oracle.  On these inputs the fp32 and the fp64 oracle agree on every lattice point at bins 16, 20
    AND 64 (0 flips, checked on the CPU and asserted here), so the reference alone stays inside the allowance.  The per-sample counts
    are pairwise different (hand: 327 / 239 / 378 at 16, 647 / 480 / 743 at 20, 22808 / 16776 / 26118 at 64 on the CPU): taking
    another sample's K, centre or box cannot hide."""
    O, R = ops(), oracle()
    B = 3
    meta = T.asymmetric_geometry(B, HW)
    center, box = meta["mano_root" if kind == "hand" else "obj_center_cam"], meta["bbox_" + kind]
    pts, sidx, lidx, counts, offsets, _ = O.lattice_candidates(center.to(DEV), meta["cam_intr"].to(DEV), box.to(DEV), 3.1, bins)
    lat = R.dense_lattice(bins)
    start, flips = 0, []
    for b in range(B):
        keep, _ = R.lattice_bbox_mask(lat, center[b], meta["cam_intr"][b], box[b], 3.1)
        keep64, _ = R.lattice_bbox_mask(lat.double(), center[b].double(), meta["cam_intr"][b].double(), box[b].double(), 3.1)
        flips.append(int((keep != keep64).sum()))
        ref_idx = torch.nonzero(keep).squeeze(1)
        got_idx = lidx[start:start + counts[b]].cpu().long()
        sym = set(ref_idx.tolist()) ^ set(got_idx.tolist())
        assert len(sym) <= max(2, len(ref_idx) // 2000), (b, len(sym), len(ref_idx))
        assert torch.equal(pts[start:start + counts[b]].cpu(), lat[got_idx])          # coordinates bit-exact
        assert bool((got_idx[1:] > got_idx[:-1]).all())                              # ascending lattice order
        assert bool((sidx[start:start + counts[b]] == b).all())
        start += counts[b]
    print(f"GEOM lattice {kind} bins {bins}: counts per sample {counts}  fp32-vs-fp64 oracle flips {flips}")
    assert flips == [0] * B, flips
    assert len(set(counts)) == B, counts


# ---------------------------------------------------------------------------------------------
# the coarse entries and the model: B = 2, 48 + 16 points, bins 16, 192 x 320, the encoder-like pyramid
# ---------------------------------------------------------------------------------------------
NH, NO, BINS, NB = 48, 16, 16, 2


def asym_model(train=False, img_hw=HW):
    model, c = build("dexycb", NH, NO, BINS, train=train)
    c.input_img_shape = tuple(img_hw)
    assert model.cfg is c
    return model, c


def asym_inputs(seed=151, pyr_seed=15):
    pyr = T.nonsquare_pyramid(NB, T.PYRAMID_ENCODER_LIKE, seed=pyr_seed)
    inputs, targets, _ = T.synthetic_batch(NB, NH, NO, seed=seed)
    return pyr, inputs, targets, T.asymmetric_geometry(NB, HW)


def no_dropout(model, c):
    c.dropout = 0.0
    for m in model.modules():
        if hasattr(m, "p"):
            m.p = 0.0
        if hasattr(m, "dropout_prob"):
            m.dropout_prob = 0.0


def test_sdf_query_one_call_at_the_asymmetric_geometry():
    """hoisdf_sdf_query_fwd against the op chain at the bars of test_sdf_query_one_call_matches_the_op_chain (raw / sdf 1e-5, pe 1e-6,
    shared gather, per-row sample index bit-identical); its comparison with the fp32 oracle is a quantity downstream of the gather:
    ratio rule against the oracle in fp64."""
    O, R = ops(), oracle()
    model, c = asym_model()
    pyr_cpu, inputs, _, meta = asym_inputs()
    pyr, _ = nhwc_pyramid(pyr_cpu)
    pts_cpu = inputs["hand_sdf_points"] * 1.2
    pts, root, K = pts_cpu.to(DEV), meta["mano_root"].to(DEV), meta["cam_intr"].to(DEV)
    with torch.no_grad():
        ref_sdf, ref_raw, ref_pe, _ = model._sdf_rows(pyr, pts, root, K, 3.1, "hand")
        sdf, raw, pe, feat = model._sdf_query(pyr, pts, root, K, 3.1, "hand", want_feat=True)
        assert_close(raw, ref_raw, rel=1e-5, what="raw"); assert_close(sdf, ref_sdf, rel=1e-5, what="sdf")
        assert_close(pe, ref_pe, rel=1e-6, what="pe")
        _, raw2, _, _ = model._sdf_query(pyr, pts, root, K, 3.1, "obj", feat=feat)
        assert_close(raw2, model._sdf_rows(pyr, pts, root, K, 3.1, "obj")[1], rel=1e-5, what="raw obj via shared gather")
        sidx = torch.arange(NB, device=DEV, dtype=torch.int32).repeat_interleave(NH)
        _, raw3, _, _ = model._sdf_query(pyr, pts.reshape(-1, 3), root, K, 3.1, "hand", sample_idx=sidx)
        assert torch.equal(raw3, raw)
    P_ = T.det_params(T.hot_path_param_shapes(992))
    ocfg = R.OracleCfg(input_img_shape=HW)
    with torch.no_grad():
        o32, _ = R.sdf_forward(P_, ocfg, pyr_cpu, pts_cpu, meta["mano_root"], meta["cam_intr"], 3.1, "hand", False)
        d = lambda t: t.double()
        o64, _ = R.sdf_forward({k: d(v) for k, v in P_.items()}, ocfg, {k: d(v) for k, v in pyr_cpu.items()}, d(pts_cpu),
                               d(meta["mano_root"]), d(meta["cam_intr"]), 3.1, "hand", False)
    ratio_rule(sdf, o32.reshape(-1), o64.reshape(-1), "sdf_query one call: sdf")


def test_sdf_query_train_entries_at_the_asymmetric_geometry():
    """hoisdf_sdf_query_train_fwd / hoisdf_sdf_query_bwd against the op chain, bars of
    test_coarse_sdf_query_train_entries_equal_the_op_chain (the pyramid gradient's tile owners see ragged tiles here)."""
    O = ops()
    model, c = asym_model()
    pyr_cpu, inputs, _, meta = asym_inputs()
    pts = (inputs["hand_sdf_points"] * 1.2).to(DEV)
    root, K = meta["mano_root"].to(DEV), meta["cam_intr"].to(DEV)
    gs = rnd(NB * NH, seed=3).to(DEV)
    res = {}
    keep, keep_det = O._SDF_QUERY_TRAIN_C, O.deterministic()
    O.set_deterministic(True)
    try:
        for coarse in (True, False):
            O._SDF_QUERY_TRAIN_C = coarse
            model.zero_grad(set_to_none=True)
            pyr, levels = nhwc_pyramid(pyr_cpu, requires_grad=True)
            sdf, raw, pe, cam = model._sdf_rows(pyr, pts, root, K, 3.1, "hand")
            assert (raw is None) == coarse
            (sdf * gs).sum().backward()
            named = [(n, p.grad.clone()) for n, p in model.named_parameters() if p.grad is not None]
            res[coarse] = (sdf.detach(), pe, cam, [lv.grad.clone() for lv in levels], named)
    finally:
        O._SDF_QUERY_TRAIN_C = keep
        O.set_deterministic(keep_det)
    a, b = res[True], res[False]
    assert_close(a[0], b[0], rel=5e-6, what="sdf")
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for i, (x, y) in enumerate(zip(a[3], b[3])):
        assert float(y.abs().max()) > 0
        assert_close(x, y, rel=2e-5, what=f"d pyramid level {i}")
    assert [n for n, _ in a[4]] == [n for n, _ in b[4]] and len(a[4]) == 18
    for (n, x), (_, y) in zip(a[4], b[4]):
        assert_close(x, y, rel=2e-5, what="d " + n)


def test_tokens_entry_at_the_asymmetric_geometry():
    """hoisdf_tokens_fwd / _bwd against ops.linear x 4 + ops.token_build on rows gathered at the asymmetric geometry (camera points,
    positional encoding and sdf of the same query): bit-identical in deterministic mode, as in
    test_coarse_tokens_entry_equals_the_op_chain; the gradient goes on through the gather into the non-square pyramid."""
    O = ops()
    model, c = asym_model()
    pyr_cpu, inputs, _, meta = asym_inputs()
    pts = inputs["hand_pre_points"].to(DEV)
    root, K = meta["mano_root"].to(DEV), meta["cam_intr"].to(DEV)
    P, S, D = NH, NH + NO, 256
    ws, bs = _mlp_params([992, 1024, 512, 256, D - 33], seed=60)
    gtok = rnd(NB, S, D, seed=12).to(DEV)
    keep_det = O.deterministic()
    O.set_deterministic(True)
    res = {}
    try:
        for coarse in (True, False):
            for t in ws + bs:
                t.grad = None
            pyr, levels = nhwc_pyramid(pyr_cpu, requires_grad=True)
            f, cam = O.project_gather(pyr, pts, root, K, 3.1, HW)
            with torch.no_grad():
                sdf, _, pe, _ = model._sdf_query(pyr, pts, root, K, 3.1, "hand", feat=f.detach())
            beta = torch.full((1,), 0.07, device=DEV, requires_grad=True)
            tok = torch.zeros(NB, S, D, device=DEV)
            if coarse:
                tok, fea = O.tokens(tok, f, cam, root, pe, sdf, beta, 0, ws, bs)
            else:
                h = f
                for w_, b_ in zip(ws, bs):
                    h = O.linear(h, w_, b_, act=True)
                fea = h.detach()
                tok = O.token_build(tok, cam, root, pe, h, sdf, beta, 0)
            (tok * gtok).sum().backward()
            res[coarse] = [tok.detach(), fea, beta.grad] + [lv.grad.clone() for lv in levels] + [t.grad.clone() for t in ws + bs]
    finally:
        O.set_deterministic(keep_det)
    assert float(res[True][3].abs().max()) > 0
    for i, (a, b) in enumerate(zip(res[True], res[False])):
        assert torch.equal(a, b), f"output / gradient {i} differs: {float((a - b).abs().max()):.3e}"


def _point_sets(pts):
    return [{tuple(r) for r in p.cpu().numpy().round(6).tolist()} for p in pts]


@pytest.mark.parametrize("kind", ["hand", "obj"])
def test_sdf_infer_selects_the_oracle_set_at_the_asymmetric_geometry(kind):
    """ops.sdf_infer (lattice, gather, SDF MLPs, selection in one call) against R.sdf_infer the way
    test_sdf_infer_selects_the_oracle_set compares them: per-sample K, centre and box, 192 x 320, bins 16."""
    R = oracle()
    model, c = asym_model()
    pyr_cpu, _, _, meta = asym_inputs()
    pyr, _ = nhwc_pyramid(pyr_cpu)
    n = NH if kind == "hand" else NO
    cen, box = "mano_root" if kind == "hand" else "obj_center_cam", "bbox_" + kind
    P = T.det_params(T.hot_path_param_shapes(992))
    pts_r, sdf_r, _ = R.sdf_infer(P, oracle_cfg(c, input_img_shape=HW), pyr_cpu, meta[cen], meta["cam_intr"], meta[box], 3.1, n, kind)
    m = T.to_device(meta, DEV)
    pts, sdf, pe, _ = model.sdf_infer(pyr, m[cen], m["cam_intr"], m[box], 3.1, n, kind)
    for i, (sa, sb) in enumerate(zip(_point_sets(pts), _point_sets(pts_r))):
        assert len(sa ^ sb) <= 4, len(sa ^ sb)
        assert abs(float(sdf[i].abs().sum().cpu() - sdf_r[i].abs().sum())) < 1e-3
        assert bool((sdf[i, 1:, 0].abs() >= sdf[i, :-1, 0].abs() - 1e-7).all())      # ascending |sdf|
    assert _point_sets(pts)[0] != _point_sets(pts)[1]                                # the samples select different points


def check_eval_outputs(res, ref, what):
    """the bars of test_gpu_model.test_eval_forward_matches_reference_goldens: joints / meshes 1e-4 m, losses 2e-4 relative,
    per-point object outputs as means over the points -> the number of outputs compared"""
    n = 0
    for k, r in ref.items():
        if not torch.is_tensor(r) or k.startswith("_"):
            continue
        assert k in res, f"missing output {k}"
        got, r = res[k].detach().float().cpu(), r.detach().float()
        if k in ("obj_rot_out", "obj_trans_out"):
            got, r = got.mean(1), r.mean(1)
        if "loss" in k or k in ("obj_rot", "obj_trans"):
            if got.shape != r.shape:                         # (per-sample sums against the oracle's scalar)
                got, r = got.mean(), r.mean()
            tol = 2e-4 * max(1.0, float(r.abs().nan_to_num(0.0).max()))
        else:
            tol = 1e-4
        assert got.shape == r.shape, (k, got.shape, r.shape)
        assert torch.isnan(got).equal(torch.isnan(r)), k
        err = (got - r).abs().nan_to_num(0.0).max().item()
        print(f"GEOM {what} {k}: max abs err {err:.3e} (bar {tol:.1e})")
        assert err <= tol, f"{what} {k}: max abs err {err:.3e} > {tol:.1e}"
        n += 1
    return n


def _eval_outputs():
    model, c = asym_model()
    pyr_cpu, inputs, targets, meta = asym_inputs()
    pyr, _ = nhwc_pyramid(pyr_cpu)
    di, dt, dm = (T.to_device(x, DEV) for x in (inputs, targets, meta))
    with torch.no_grad():
        loss, out = model.hot_path(pyr, di, dt, dm, "eval")
    return model, c, pyr, dm, {**loss, **out}


def test_eval_hot_path_matches_the_oracle_at_the_asymmetric_geometry():
    """Model.hot_path(..., "eval") with cfg.input_img_shape = (192, 320) against R.hot_path_forward under the same image shape;
    every sample keeps >= 184 lattice survivors, nothing raises."""
    from hoisdf_amd.nets import mano as MANO
    R = oracle()
    model, c, _, _, res = _eval_outputs()
    pyr_cpu, inputs, targets, meta = asym_inputs()
    layer = MANO.ManoLayer(MANO.synthetic_assets(0))
    with torch.no_grad():
        ref = R.hot_path_forward(T.det_params(T.hot_path_param_shapes(992)), oracle_cfg(c, input_img_shape=HW), pyr_cpu, inputs, targets,
                                 meta, "eval", mano_layer=layer, hands_mean=layer.th_hands_mean)
    assert check_eval_outputs(res, ref, "eval vs oracle") >= 10


def test_eval_hot_path_matches_the_reference_fixture_at_the_asymmetric_geometry():
    """the same run against tests/golden/g15_asym_geometry.npz - the REFERENCE's own eval forward on these inputs (make_golden.py
    asym_geometry_golden) - at the bars of test_eval_forward_matches_reference_goldens."""
    g = {k[4:]: v for k, v in load_golden("g15_asym_geometry").items() if k.startswith("e2e.")}
    _, _, _, _, res = _eval_outputs()
    assert check_eval_outputs(res, g, "eval vs g15") >= 6


def test_infer_native_next_to_the_python_path_at_the_asymmetric_geometry():
    """Model.infer_native (hoisdf_pose_infer; img_h / img_w from the descriptor) next to the Python path on the same inputs, as
    test_infer_native_next_to_the_python_path: the differences are printed, both are held to the reference's outputs (g15)."""
    from test_gpu_pose_infer import check_against_fixture
    g = {k[4:]: v for k, v in load_golden("g15_asym_geometry").items() if k.startswith("e2e.")}
    model, c, pyr, dm, py = _eval_outputs()
    nat = model.infer_native(pyr, dm, debug=True)
    torch.cuda.synchronize()
    for k in sorted(nat):
        if k in py:
            assert nat[k].shape == py[k].shape, (k, nat[k].shape, py[k].shape)
            print(f"GEOM native vs python {k}: max |native - python| = {(nat[k] - py[k]).abs().max().item():.3e}")
    assert check_against_fixture(nat, g, "GEOM native ") >= 4
    assert check_against_fixture(py, g, "GEOM python ") >= 4


def test_training_step_matches_the_oracle_at_the_asymmetric_geometry():
    """one hot-path training step (dropout off, the jitter hook) as test_training_step_with_the_option_switches_matches_the_oracle
    without switches: losses at 2e-4, the same four parameter gradients at 2e-3 of their norm, and the gradient of the 24 x 40 pyramid
    level (ragged tiles) at the same 2e-3."""
    from hoisdf_amd.nets import mano as MANO
    R = oracle()
    model, c = asym_model(train=True)
    no_dropout(model, c)
    pyr, inputs, targets, meta = asym_inputs()
    P_, levels = nhwc_pyramid(pyr, requires_grad=True)
    di, dt, dm = (T.to_device(x, DEV) for x in (inputs, targets, meta))
    torch.manual_seed(1234)
    jit = [torch.empty_like(inputs["hand_pre_points"]).uniform_(-0.05, 0.05), torch.empty_like(inputs["obj_pre_points"]).uniform_(-0.05, 0.05)]
    model._jitter = lambda like, d: jit.pop(0).to(DEV)
    model._py_random = random.Random(0)
    loss, out = model.hot_path(P_, di, dt, dm, "train", 0, 0.5)
    total = sum(v.mean() for v in loss.values())
    total.backward()
    Pm = {k: v.clone().requires_grad_(True) for k, v in T.det_params(T.hot_path_param_shapes(992)).items()}
    pyr_req = {k: v.clone().requires_grad_(True) for k, v in pyr.items()}
    ocfg = oracle_cfg(c, dropout=0.0, sdf_dropout=0.0, input_img_shape=HW)
    layer_cpu = MANO.ManoLayer(MANO.synthetic_assets(0))
    torch.manual_seed(1234)
    ref = R.hot_path_forward(Pm, ocfg, pyr_req, inputs, targets, meta, "train", mano_layer=layer_cpu, hands_mean=layer_cpu.th_hands_mean,
                             epoch_cnt=0, batch_ratio=0.5, rng=random.Random(0))
    rl = {k: v for k, v in ref.items() if not k.endswith("_out")}
    for k, v in loss.items():
        a, r_ = float(v.mean()), float(rl[k].mean())
        print(f"GEOM train step loss {k}: {a:.7g} vs oracle {r_:.7g}")
        assert abs(a - r_) <= 2e-4 * max(1.0, abs(r_)), (k, a, r_)
    sum(v.mean() for v in rl.values()).backward()
    sd = dict(model.named_parameters())
    pairs = [(k, sd[k].grad.cpu(), Pm[k].grad) for k in ("linear_transformerin.layers.0.weight", "hand_transformer.encoder.layers.0.linear1.weight",
                                                         "obj_transformer.encoder.layers.2.norm2.weight", "hand_sdf_decoder.linh4.weight")]
    assert levels[2].shape[1:3] == (24, 40)
    pairs.append(("pyramid level 24x40", levels[2].grad.permute(0, 3, 1, 2).cpu(), pyr_req["stride8"].grad))
    for k, ga, gr in pairs:
        d, nrm = float((ga - gr).norm()), float(gr.norm())
        print(f"GEOM train step d {k}: |got - oracle| {d:.3e} of norm {nrm:.3e} ({d / nrm:.2e})")
        assert d <= 2e-3 * nrm + 1e-9, (k, d, nrm)
