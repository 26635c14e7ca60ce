"""-m gpu: the small hot-path kernels of csrc/pointwise.hip, csrc/vote.hip and csrc/select.hip against the fp64 references of
hoisdf_amd.testing, at the smallest shapes that reach each of their paths (ragged widths, leading dimensions with a pad, the
grid-stride loops, the thresholds between two kernels) and at the edges of their value ranges.

Bars (those tests/test_gpu_ops.py holds the same outputs to): 2e-5 of the reference's largest magnitude for values and per-element
gradients, 1e-4 for gradients reduced over rows, 2e-6 absolute for posenc, exact where a value is a copy, a zero or an index.  Tensors
whose slices span decades (dcls / doff / joints per (l, b, j); dv, dx, dr, dfeat per row) are measured slice by slice as well, each slice
against its own largest reference magnitude; that bar is the larger of the tensor-wide bar and four times the slice-wise error of the
same formula evaluated in float32 on the CPU (hoisdf_amd.testing.slice_bar).  Every figure is printed before it is asserted (-s)."""
import ctypes as C

import pytest
import torch

from hoisdf_amd import testing as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = -777.25                   # what a buffer holds where no kernel may write
VAL, RED = 2e-5, 1e-4            # values and per-element gradients / gradients reduced over rows


def ops():
    from hoisdf_amd import ops as O
    return O


def call(name, *args):
    from hoisdf_amd._lib import call as c
    c(name, *args)


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(*ts):
    out = tuple(None if t is None else t.to(DEV).contiguous() for t in ts)
    return out if len(out) > 1 else out[0]


def sent(*shape):
    return torch.full(shape, SENT, device=DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def gen(*key):
    return T._gen("small-kernels", *key)


def check(op, name, got, ref, bar):
    err = T.rel_err(got, ref)
    print(f"FIG|{op}|{name}|tensor|{err:.3e}|{bar:.0e}|")
    assert err <= bar, f"{op} {name}: {err:.3e} of the reference's max (bar {bar:.0e})"


def check_slices(op, name, got, ref64, ref32, slice_dims, tensor_bar, tensor_wide=True):
    """the tensor-wide bar and the slice-wise one (module docstring); tensors come with the slice dimensions first"""
    if tensor_wide:
        check(op, name, got, ref64, tensor_bar)
    bar, e32 = T.slice_bar(ref32, ref64, slice_dims, tensor_bar)
    err = T.slice_err(got, ref64, slice_dims)
    print(f"FIG|{op}|{name}|slices|{err:.3e}|{bar:.3e}|{e32:.3e}")
    assert err <= bar, f"{op} {name}: worst slice {err:.3e} of its own max (bar {bar:.3e}; the same formula in fp32: {e32:.3e})"


class deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.was = ops().deterministic()
        ops().set_deterministic(self.on)

    def __exit__(self, *exc):
        ops().set_deterministic(self.was)


# ---- posenc ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 30000])                # (30 000 x 36 slots > 4096 blocks x 256 threads: the loop strides)
def test_posenc_pe_and_x0_forms(n):
    O = ops()
    pts = torch.rand(n, 3, generator=gen("posenc", n)) * 8.0 - 4.0
    if n >= 3:
        pts[1] = torch.tensor([0.0, -0.0, -4.0])
        pts[2] = 1e-30
        pts[n - 1, 0] = 4.0
    else:
        pts[0] = torch.tensor([0.0, -0.0, 1e-30])
    d_pts = dev(pts)
    pe = O.posenc(d_pts)
    err = float((pe.cpu().double() - T.reference_posenc_rows(pts)).abs().max())
    print(f"FIG|posenc|pe|abs|{err:.3e}|2e-06|")
    assert err <= 2e-6
    for ld, col0 in ((33, 0), (34, 0), (36, 0), (40, 4), (296, 256)):
        x0a, x0b, pe_b = sent(n, ld), sent(n, ld), sent(n, 30)
        call("hoisdf_posenc_fwd", P(d_pts), n, P(x0a), ld, col0, None, st())
        call("hoisdf_posenc_fwd", P(d_pts), n, P(x0b), ld, col0, P(pe_b), st())
        assert same_bits(x0a, x0b) and same_bits(pe_b, pe), (ld, col0)
        assert same_bits(x0a[:, col0:col0 + 30], pe), (ld, col0)
        assert same_bits(x0a[:, col0 + 30:col0 + 33], d_pts), (ld, col0)               # (-0 stays -0)
        pad_end = min(col0 + 36, ld)
        assert bool((bits(x0a[:, col0 + 33:pad_end]) == 0).all()), (ld, col0)
        other = torch.ones(ld, dtype=torch.bool)
        other[col0:pad_end] = False
        assert bool((x0a.cpu()[:, other] == SENT).all()), (ld, col0)
        ref = T.reference_posenc_rows(pts, ld, col0, SENT)
        assert float((x0a.cpu().double() - ref).abs().max()) <= 2e-6


# ---- weight norm ----------------------------------------------------------------------------------------------------------------------
def _weightnorm(out, inn, ldw, v, g, op):
    dW = torch.randn(out, ldw, generator=gen("wn-dW", out, inn, ldw))
    r64 = T.reference_weight_norm(v, g, dW, ldw)
    r32 = T.reference_weight_norm(v, g, dW, ldw, dtype=torch.float32)
    d_v, d_g, d_dW = dev(v, g, dW)
    W, norms = sent(out, ldw), sent(out)
    call("hoisdf_weightnorm_fwd", P(d_v), P(d_g), P(W), ldw, P(norms), out, inn, st())
    assert bool((bits(W[:, inn:]) == 0).all()), "the pad columns of W are exactly 0"
    check_slices(op, "W", W[:, :inn], r64["W"][:, :inn], r32["W"][:, :inn], 1, VAL)
    check(op, "norms", norms, r64["norms"], VAL)
    dv, dg = sent(out, inn), sent(out)
    call("hoisdf_weightnorm_bwd", P(d_v), P(d_g), P(d_dW), ldw, P(dv), P(dg), out, inn, st())
    return dv, dg, r64, r32, (d_v, d_g, d_dW, W)


@pytest.mark.parametrize("out,inn,ldw", [(1, 4, 4), (5, 3, 8), (223, 512, 512), (6, 289, 292), (64, 1000, 1000)])
def test_weightnorm_widths_and_pads(out, inn, ldw):
    O = ops()
    g0 = gen("wn", out, inn, ldw)
    v, g = torch.randn(out, inn, generator=g0), torch.randn(out, generator=g0).abs() + 0.5
    dv, dg, r64, r32, (d_v, d_g, d_dW, W) = _weightnorm(out, inn, ldw, v, g, "weightnorm")
    check_slices("weightnorm", "dv", dv, r64["dv"], r32["dv"], 1, VAL)
    check("weightnorm", "dg", dg, r64["dg"], VAL)
    if ldw == inn:                                          # the Python wrapper's form of the same call
        vg, gg = d_v.clone().requires_grad_(True), d_g.view(out, 1).clone().requires_grad_(True)
        W2 = O.weight_norm(vg, gg)
        W2.backward(d_dW)
        assert same_bits(W2, W) and same_bits(vg.grad, dv) and same_bits(gg.grad.view(-1), dg)


def test_weightnorm_row_norms_spanning_nine_decades():
    """||v_row|| from 1e-6 to 1e3: dv ~ 1 / ||v_row||, so one tensor-wide maximum would see the quietest row only - dv is judged row by row"""
    out, inn, ldw = 37, 289, 292
    g0 = gen("wn-span")
    v = torch.randn(out, inn, generator=g0)
    v = v / v.norm(dim=1, keepdim=True) * torch.logspace(-6, 3, out)[:, None]
    g = torch.randn(out, generator=g0).abs() + 0.5
    dv, dg, r64, r32, _ = _weightnorm(out, inn, ldw, v, g, "weightnorm-span")
    span = r64["norms"].max() / r64["norms"].min()
    assert span > 1e8
    check_slices("weightnorm-span", "dv", dv, r64["dv"], r32["dv"], 1, VAL, tensor_wide=False)
    check("weightnorm-span", "dg", dg, r64["dg"], VAL)


# ---- SDF head -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", T.HEAD_MS)            # (9001 rows: a wave of the backward takes two trips, the last row unpaired)
@pytest.mark.parametrize("K", T.HEAD_KS)
def test_sdf_head_widths_rows_and_modes(M, K):
    O = ops()
    from hoisdf_amd._lib import HoisdfError
    clamp = T.HEAD_CLAMP
    h, w, b, dsdf, _ = T.head_case_inputs(M, K)
    assert T.head_rows_margin(h, w, b, clamp) >= 1e-5             # a condition on the inputs: no row sits on the clamp
    r64 = T.reference_sdf_head(h, w, b, clamp, dsdf)
    outside = r64["raw"].abs() > clamp
    op = "sdf_head"
    d_h, d_w, d_b, d_dsdf = dev(h, w, b, dsdf)
    # forward: the wrapper (ldh = K) and raw pointers (ldh = K + 4, the pad never read)
    hp = sent(M, K + 4)
    hp[:, :K] = d_h
    raw_p, sdf_p = sent(M), sent(M)
    call("hoisdf_sdf_head_fwd", P(hp), K + 4, P(d_w), P(d_b), P(raw_p), P(sdf_p), M, K, clamp, st())
    check(op, "raw", raw_p, r64["raw"], VAL)
    check(op, "sdf", sdf_p, r64["sdf"], VAL)
    sat = T.head_saturated_rows(M)
    assert bool((raw_p.cpu()[sat].abs() == 1.0).all())
    if K > 512:                                                   # the backward serves K <= 512: refused before any launch
        dh, dw, db = sent(M, K), torch.zeros(K, device=DEV), torch.zeros(1, device=DEV)
        with pytest.raises(HoisdfError):
            call("hoisdf_sdf_head_bwd", P(d_dsdf), P(raw_p), P(d_h), K, P(d_w), P(dh), K, P(dw), P(db), M, K, clamp, st())
        torch.cuda.synchronize()
        assert bool((dh == SENT).all()) and float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
        hg = d_h.clone().requires_grad_(True)
        sdf, raw = O.sdf_head(hg, d_w.view(1, K), d_b, clamp)
        assert same_bits(raw, raw_p) and same_bits(sdf, sdf_p)
        return
    runs = {}
    for det in (False, True, True):
        with deterministic(det):
            hg, wg, bg = (t.clone().requires_grad_(True) for t in (d_h, d_w.view(1, K), d_b))
            sdf, raw = O.sdf_head(hg, wg, bg, clamp)
            sdf.backward(d_dsdf)
            assert same_bits(raw, raw_p) and same_bits(sdf, sdf_p)
            tag = f"det={int(det)}"
            check(op, "dh " + tag, hg.grad, r64["dh"], VAL)
            check(op, "dw " + tag, wg.grad.view(-1), r64["dw"], RED)
            check(op, "db " + tag, bg.grad, r64["db"], RED)          # (K < 512: db is parked beside dw[K - 1] in LDS)
            assert float(hg.grad[outside.to(DEV)].abs().max() if bool(outside.any()) else 0.0) == 0.0
            if det and "det" in runs:
                for a, c in zip(runs["det"], (hg.grad, wg.grad, bg.grad)):
                    assert same_bits(a, c), "two deterministic runs differ"
            runs["det" if det else "atomic"] = (hg.grad.clone(), wg.grad.clone(), bg.grad.clone())
            # raw pointers: ldh = lddh = K + 4, the pad of dh untouched
            dhp, dw, db = sent(M, K + 4), torch.zeros(K, device=DEV), torch.zeros(1, device=DEV)
            call("hoisdf_sdf_head_bwd", P(d_dsdf), P(raw_p), P(hp), K + 4, P(d_w), P(dhp), K + 4, P(dw), P(db), M, K, clamp, st())
            assert same_bits(dhp[:, :K], hg.grad) and bool((dhp[:, K:] == SENT).all())
            check(op, "dw ld " + tag, dw, r64["dw"], RED)
            check(op, "db ld " + tag, db, r64["db"], RED)


# ---- token build ----------------------------------------------------------------------------------------------------------------------
TOKEN_SHAPES = [(1, 1, 1, 0, 37), (2, 50, 70, 10, 256), (3, 33, 33, 0, 256), (2, 40, 64, 24, 100),
                (3, 1400, 1400, 0, 64),        # 4200 rows > 1024 blocks x 4 waves: the backward strides
                (5, 1700, 1700, 0, 40)]        # 8500 rows > 2048 blocks x 4 waves: the forward strides


@pytest.mark.parametrize("beta", [0.08, 2e-3, 1e-4])            # (1e-4 is below the 2e-3 clamp: values and dbeta are those of 2e-3)
@pytest.mark.parametrize("B,Pn,S,row0,D", TOKEN_SHAPES)
def test_token_build_shapes_betas_and_saturation(B, Pn, S, row0, D, beta):
    O = ops()
    F_ = D - 33
    n = B * Pn
    g0 = gen("token", B, Pn, S, row0, D)
    cam, center = torch.randn(B, Pn, 3, generator=g0), torch.randn(B, 3, generator=g0)
    pe, feat = torch.randn(B, Pn, 30, generator=g0), torch.randn(B, Pn, F_, generator=g0)
    sdf = (torch.rand(B, Pn, generator=g0) * 2.0 - 1.0) * 0.15
    if n >= 4:                                                    # z = sdf / beta reaches +-500: sig is 0 or 1 / beta
        flat = sdf.view(-1)
        flat[0], flat[n // 2], flat[n - 1] = 1.0, -1.0, 1.0
    dtok = torch.randn(B, S, D, generator=g0)
    bt = torch.tensor([beta])
    r64 = T.reference_token_build(cam, center, pe, feat, sdf, bt, dtok[:, row0:row0 + Pn])
    r32 = T.reference_token_build(cam, center, pe, feat, sdf, bt, dtok[:, row0:row0 + Pn], dtype=torch.float32)
    assert bool(torch.isfinite(r64["dfeat"]).all()) and bool(torch.isfinite(r64["dbeta"]).all())
    op = "token_build"
    d_cam, d_center, d_pe, d_feat, d_sdf, d_beta, d_dtok = dev(cam.view(n, 3), center, pe, feat.view(n, F_), sdf, bt, dtok)
    fg, bg = d_feat.clone().requires_grad_(True), d_beta.clone().requires_grad_(True)
    tok = O.token_build(sent(B, S, D), d_cam, d_center, d_pe, fg, d_sdf, bg, row0)
    (tok * d_dtok).sum().backward()
    body = tok.detach()[:, row0:row0 + Pn]
    check(op, "tok", body, r64["tok"], VAL)
    assert same_bits(body[..., :3], (d_cam.view(B, Pn, 3) - d_center[:, None])) and same_bits(body[..., 3:33], d_pe)
    rows = torch.ones(S, dtype=torch.bool)
    rows[row0:row0 + Pn] = False
    assert bool((tok.detach().cpu()[:, rows] == SENT).all()), "rows outside [row0, row0 + P) keep what they held"
    check_slices(op, "dfeat", fg.grad.view(n, F_), r64["dfeat"].view(n, F_), r32["dfeat"].view(n, F_), 1, VAL)
    check(op, "dbeta", bg.grad, r64["dbeta"], RED)
    assert bool(torch.isfinite(fg.grad).all()) and bool(torch.isfinite(bg.grad).all())
    # raw pointers: ldfeat = lddfeat = D - 33 + 4; hoisdf_token_build_bwd itself, in both modes
    featp = sent(n, F_ + 4)
    featp[:, :F_] = d_feat
    tok2 = sent(B, S, D)
    call("hoisdf_token_build_fwd", P(d_cam), P(d_center), P(d_pe), P(featp), F_ + 4, P(d_sdf), P(d_beta), P(tok2), B, Pn, S, row0, D, st())
    assert same_bits(tok2, tok)
    for det in (False, True):
        with deterministic(det):
            dfeatp, dbeta = sent(n, F_ + 4), torch.zeros(1, device=DEV)
            call("hoisdf_token_build_bwd", P(d_dtok), P(featp), F_ + 4, P(d_sdf), P(d_beta), P(dfeatp), F_ + 4, P(dbeta), B, Pn, S, row0, D, st())
            assert same_bits(dfeatp[:, :F_], fg.grad.view(n, F_)) and bool((dfeatp[:, F_:] == SENT).all())
            check(op, f"dbeta bwd det={int(det)}", dbeta, r64["dbeta"], RED)


# ---- vote / vote loss -----------------------------------------------------------------------------------------------------------------
def _lbj(t, L, B, Pn, J):
    """(L, B, P, J[, 3]) -> the (l, b, j) slices first"""
    return t.reshape(L, B, Pn, J, -1).permute(0, 1, 3, 2, 4)


def _vote_loss_bwd(d_in, joints, stats, dj, dl3d, dbce, L, B, Pn, J):
    d_off, d_cls, d_pts, d_gt = d_in
    doff, dcls = sent(L, B, Pn, J * 3), sent(L, B, Pn, J)
    call("hoisdf_vote_loss_bwd", P(d_off), P(d_cls), P(d_pts), P(d_gt), T.VOTE_RADIUS, P(joints), P(stats), P(dj), P(dl3d), P(dbce),
         P(doff), P(dcls), L, B, Pn, J, st())
    return doff, dcls


@pytest.mark.parametrize("family", T.VOTE_FAMILIES)
@pytest.mark.parametrize("L,B,Pn,J", T.VOTE_CASES)
def test_vote_and_vote_loss(L, B, Pn, J, family):
    O = ops()
    off, cls, pts, gt, _ = T.vote_case_inputs(L, B, Pn, J, family)
    assert T.vote_points_margin(pts, gt, T.VOTE_RADIUS) >= 1e-6         # a condition on the inputs: no point sits on the radius
    g0 = gen("vote-grads", L, B, Pn, J, family)
    dj, dl3d, dbce = torch.randn(L, B, J, 3, generator=g0), torch.randn(L, B, generator=g0), torch.randn(L, B, generator=g0)
    d_in = dev(off, cls, pts, gt)
    d_off, d_cls, d_pts, d_gt = d_in
    d_dj, d_dl3d, d_dbce = dev(dj, dl3d, dbce)
    sl = lambda t: _lbj(t, L, B, Pn, J)
    # the plain vote
    op = "vote"
    r64, r32 = T.reference_vote(off, cls, pts, dj), T.reference_vote(off, cls, pts, dj, dtype=torch.float32)
    og, cg = d_off.clone().requires_grad_(True), d_cls.clone().requires_grad_(True)
    joints_v = O.vote_aggregate(og, cg, d_pts)
    joints_v.backward(d_dj)
    check_slices(op, "joints", joints_v, r64["joints"], r32["joints"], 3, VAL)
    check_slices(op, "doff", sl(og.grad), sl(r64["doff"]), sl(r32["doff"]), 3, VAL)
    check_slices(op, "dcls", sl(cg.grad), sl(r64["dcls"]), sl(r32["dcls"]), 3, RED)
    # the vote with the loss sums
    op = "vote_loss"
    q64 = T.reference_vote_loss(off, cls, pts, gt, T.VOTE_RADIUS, dj, dl3d, dbce)
    q32 = T.reference_vote_loss(off, cls, pts, gt, T.VOTE_RADIUS, dj, dl3d, dbce, dtype=torch.float32)
    og2, cg2 = d_off.clone().requires_grad_(True), d_cls.clone().requires_grad_(True)
    joints, l3d, bce, near = O.vote_loss(og2, cg2, d_pts, d_gt, T.VOTE_RADIUS)
    torch.autograd.backward([joints, l3d, bce], [d_dj, d_dl3d, d_dbce])
    check_slices(op, "joints", joints, q64["joints"], q32["joints"], 3, VAL)
    check(op, "l3d_sum", l3d, q64["l3d_sum"], VAL)
    check(op, "bce_sum", bce, q64["bce_sum"], VAL)
    assert torch.equal(near.cpu().double(), q64["near_sum"])
    check_slices(op, "doff", sl(og2.grad), sl(q64["doff"]), sl(q32["doff"]), 3, RED)
    check_slices(op, "dcls", sl(cg2.grad), sl(q64["dcls"]), sl(q32["dcls"]), 3, RED)
    # each upstream gradient absent in turn (a null pointer, which the wrapper cannot express)
    stats = sent(L, B, J, 2)
    jo2, l2, b2, n2 = sent(L, B, J, 3), sent(L, B), sent(L, B), sent(B)
    call("hoisdf_vote_loss_fwd", P(d_off), P(d_cls), P(d_pts), P(d_gt), T.VOTE_RADIUS, P(jo2), P(stats), P(l2), P(b2), P(n2), L, B, Pn, J, st())
    assert same_bits(jo2, joints) and same_bits(l2, l3d) and same_bits(b2, bce) and same_bits(n2, near)
    for a, b_, c in ((None, dl3d, dbce), (dj, None, dbce), (dj, dl3d, None)):
        tag = "dj,dl3d,dbce".split(",")[[a is None, b_ is None, c is None].index(True)] + "=None"
        p64 = T.reference_vote_loss(off, cls, pts, gt, T.VOTE_RADIUS, a, b_, c)
        p32 = T.reference_vote_loss(off, cls, pts, gt, T.VOTE_RADIUS, a, b_, c, dtype=torch.float32)
        doff, dcls = _vote_loss_bwd(d_in, jo2, stats, None if a is None else d_dj, None if b_ is None else d_dl3d,
                                    None if c is None else d_dbce, L, B, Pn, J)
        check_slices(op, "doff " + tag, sl(doff), sl(p64["doff"]), sl(p32["doff"]), 3, RED)
        check_slices(op, "dcls " + tag, sl(dcls), sl(p64["dcls"]), sl(p32["dcls"]), 3, RED)
    # the two entries agree: the same joints, and the same gradients when only dj arrives (zeros or null pointers)
    zero = torch.zeros(L, B, device=DEV)
    doff_n, dcls_n = _vote_loss_bwd(d_in, jo2, stats, d_dj, None, None, L, B, Pn, J)
    doff_z, dcls_z = _vote_loss_bwd(d_in, jo2, stats, d_dj, zero, zero, L, B, Pn, J)
    check("vote=vote_loss", "joints", joints, joints_v.detach().double(), VAL)
    for nm, a, ref, bar in (("doff", doff_n, og.grad, VAL), ("doff zeros", doff_z, og.grad, VAL), ("dcls", dcls_n, cg.grad, RED),
                            ("dcls zeros", dcls_z, cg.grad, RED)):
        check_slices("vote=vote_loss", nm, sl(a), sl(r64[nm.split()[0]]), sl(r32[nm.split()[0]]), 3, bar)
        check("vote=vote_loss", nm + " mutual", a, ref.double(), bar)
    if Pn != 1025:      # every shape but the P = 1025 ones runs the loss forward in one segment (hoisdf_vote_loss_fwd cuts the points only
                        # when P > 512 and L * B <= 256): the same sums in the same order as hoisdf_vote_fwd, so equal
        assert torch.equal(joints, joints_v) and torch.equal(doff_n, og.grad) and torch.equal(dcls_n, cg.grad)     # (up to the sign of 0)


def test_vote_loss_sample_without_a_point_inside_the_radius():
    O = ops()
    from hoisdf_amd.nets.heads import JointvoteLoss
    L, B, Pn, J = 3, 2, 257, 20
    off, cls, pts, gt, _ = T.vote_case_inputs(L, B, Pn, J, "randn", far_sample=1)
    assert T.vote_points_margin(pts, gt, T.VOTE_RADIUS) >= 1e-6
    g0 = gen("vote-far")
    dl3d = torch.randn(L, B, generator=g0)
    q64 = T.reference_vote_loss(off, cls, pts, gt, T.VOTE_RADIUS, None, dl3d, None)
    assert float(q64["near_sum"][1]) == 0.0 and float(q64["near_sum"][0]) > 0.0
    d_in = dev(off, cls, pts, gt)
    d_off, d_cls, d_pts, d_gt = d_in
    joints, l3d, bce, near = O.vote_loss(d_off, d_cls, d_pts, d_gt, T.VOTE_RADIUS)
    assert torch.equal(near.cpu().double(), q64["near_sum"]) and float(near[1]) == 0.0
    assert float(l3d[:, 1].abs().max()) == 0.0
    check("vote_loss-far", "l3d_sum", l3d, q64["l3d_sum"], VAL)
    check("vote_loss-far", "bce_sum", bce, q64["bce_sum"], VAL)
    stats = sent(L, B, J, 2)
    jo2, l2, b2, n2 = sent(L, B, J, 3), sent(L, B), sent(L, B), sent(B)
    call("hoisdf_vote_loss_fwd", P(d_off), P(d_cls), P(d_pts), P(d_gt), T.VOTE_RADIUS, P(jo2), P(stats), P(l2), P(b2), P(n2), L, B, Pn, J, st())
    doff, dcls = _vote_loss_bwd(d_in, jo2, stats, None, dev(dl3d), None, L, B, Pn, J)
    assert float(doff[:, 1].abs().max()) == 0.0 and float(dcls.abs().max()) == 0.0
    check("vote_loss-far", "doff", doff, q64["doff"], RED)
    og, cg = d_off.clone().requires_grad_(True), d_cls.clone().requires_grad_(True)
    losses = JointvoteLoss(T.VOTE_RADIUS)(d_pts, og, cg, d_gt, batch_first=True)
    total = losses[0] + losses[1] + losses[2]
    total.backward()
    assert bool(torch.isfinite(total)) and bool(torch.isfinite(og.grad).all()) and bool(torch.isfinite(cg.grad).all())


# ---- select / gather ------------------------------------------------------------------------------------------------------------------
def _select_ref(vals, offsets, counts, k):
    rows = []
    for b in range(len(counts)):
        if int(counts[b]) < k:
            rows.append(torch.full((k,), -1, dtype=torch.long))
            continue
        seg = vals[int(offsets[b]): int(offsets[b]) + int(counts[b])].abs()
        rows.append(torch.sort(seg, stable=True)[1][:k] + int(offsets[b]))
    return torch.stack(rows)


def _select(vals, counts, k):
    O = ops()
    counts = torch.tensor(counts, dtype=torch.int32)
    offsets = torch.zeros(len(counts), dtype=torch.int32)
    offsets[1:] = torch.cumsum(counts, 0)[:-1]
    sel = O.select_smallest_abs(dev(vals), dev(offsets), dev(counts), k)
    return sel, _select_ref(vals, offsets, counts, k)


@pytest.mark.parametrize("n,k", [(1, 1), (1024, 1), (1025, 1024), (9000, 8192), (5000, 600)])
def test_select_smallest_abs_sizes(n, k):
    g0 = gen("select", n, k)
    vals = torch.tanh(torch.randn(2 * n, generator=g0) * 0.3)
    if n > 100:
        vals[::97] = vals[1::97][: len(vals[::97])]
        vals[5::31] = -vals[6::31][: len(vals[5::31])]                # ties of opposite sign
    sel, ref = _select(vals, [n, n], k)
    assert torch.equal(sel.cpu().long(), ref)


def test_select_run_of_ties_across_three_chunks():
    """2500 consecutive rows from row 700 hold the k-th smallest |x| (some negated): rows 700 .. 3199 lie in the 1024-row chunks 0 - 3 of
    the compaction; 1300 of them are taken, the lowest rows"""
    n, t = 5000, 0.25
    g0 = gen("select-ties")
    vals = torch.rand(n, generator=g0) * 0.2 + 0.3                   # above t
    below = torch.randperm(n, generator=g0)[:1800]
    vals[below] = torch.rand(1800, generator=g0) * 0.2               # below t
    vals[700:3200] = t
    vals[700:3200:3] = -t
    vals[torch.rand(n, generator=g0) < 0.5] *= -1.0
    vals[700:3200] = vals[700:3200].sign() * t
    m = int((vals.abs() < t).sum())
    k = m + 1300
    sel, ref = _select(torch.cat([vals, torch.rand(64, generator=g0)]), [n, 64], k)      # (a second segment of 64 rows < k)
    assert int(ref[1, 0]) == -1
    assert torch.equal(sel.cpu().long(), ref)
    taken = sel[0].cpu().long()[m:]
    assert torch.equal(taken, torch.arange(700, 2000)), "the ties taken are the 1300 lowest rows, in row order"
    assert bool((sel[1] == -1).all())


def test_select_zeros_denormals_inf_and_nan():
    n = 1500
    g0 = gen("select-special")
    vals = torch.randn(n, generator=g0)
    vals[10], vals[11], vals[400], vals[1300] = 0.0, -0.0, -0.0, 0.0
    vals[20], vals[21], vals[22] = 1e-40, -1e-40, 1e-45              # denormals
    vals[30], vals[900], vals[31] = float("inf"), float("-inf"), float("inf")
    vals[40], vals[1100] = float("nan"), float("nan")
    for k in (n, 7, n - 3):
        sel, ref = _select(vals, [n], k)
        assert torch.equal(sel.cpu().long(), ref), k
    sel, _ = _select(vals, [n], n)
    order = sel[0].cpu().tolist()
    assert order[:4] == [10, 11, 400, 1300]                           # +0 and -0 tie: row order
    assert order[4:7] == [22, 20, 21]
    assert order[-5:] == [30, 31, 900, 40, 1100]                      # Inf after every finite value, NaN after Inf


def test_select_short_sample_gives_minus_one_and_gather_zero_rows():
    O = ops()
    k = 300
    counts = [k + 5, k - 1, k]
    g0 = gen("select-short")
    vals = torch.randn(sum(counts), generator=g0)
    sel, ref = _select(vals, counts, k)
    assert torch.equal(sel.cpu().long(), ref)
    assert bool((sel[1] == -1).all()) and bool((sel[0] >= 0).all()) and bool((sel[2] >= 0).all())
    src = torch.randn(sum(counts), 6, generator=g0)
    out = O.gather_rows(dev(src), sel).cpu().view(3, k, 6)
    assert bool((bits(out[1]) == 0).all())
    assert same_bits(out[0], src[ref[0]]) and same_bits(out[2], src[ref[2]])


@pytest.mark.parametrize("width,n_sel", [(1, 1), (1, 5000), (6, 700), (223, 4800)])     # (223 x 4800 > 4096 blocks x 256: the loop strides)
def test_gather_rows_widths_and_strided_source(width, n_sel):
    O = ops()
    g0 = gen("gather", width, n_sel)
    n_src = 1000
    src = torch.randn(n_src, width + 3, generator=g0)
    sel = torch.randint(0, n_src, (n_sel,), generator=g0).int()
    if n_sel > 10:
        sel[3], sel[n_sel - 1] = -1, -1
    d_src = dev(src)
    out = O.gather_rows(d_src[:, :width], dev(sel)).cpu()              # a view: row stride width + 3
    want = src[sel.long().clamp(min=0), :width].clone()
    want[sel < 0] = 0.0
    assert same_bits(out, want)
    outp = sent(n_sel, width + 2)                                      # ldo > width through raw pointers
    call("hoisdf_gather_rows", P(d_src), width + 3, P(dev(sel)), n_sel, width, P(outp), width + 2, st())
    assert same_bits(outp[:, :width], want) and bool((outp[:, width:] == SENT).all())


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
def _dropout_mask(M, D, p, seed):
    if p == 0.0:
        return torch.ones(M, D, dtype=torch.bool)
    ones, kept = torch.ones(M, D, device=DEV), torch.empty(M, D, device=DEV)
    call("hoisdf_residual_dropout", None, P(ones), P(kept), M, D, float(p), seed, st())       # the same (seed, row, column) function
    mask = kept.cpu() > 0
    assert 0.5 * p < 1.0 - float(mask.double().mean()) < 1.5 * p
    return mask


@pytest.mark.parametrize("M,D,p", [(3, 4, 0.0), (37, 260, 0.3), (130, 1024, 0.1),
                                   (16400, 64, 0.0),        # > 1024 blocks x 16 rows: the backward of the D <= 256 form strides
                                   (32800, 8, 0.0)])        # > 2048 blocks x 16 rows: its forward strides
def test_add_layernorm_widths_dropout_and_dx_add(M, D, p):
    import hoisdf_amd.ops as OO
    seed = (11 << 32) + 3
    mask = _dropout_mask(M, D, p, seed)
    g0 = gen("ln", M, D)
    x, r = torch.randn(M, D, generator=g0), torch.randn(M, D, generator=g0)
    gam, bet = 1 + 0.1 * torch.randn(D, generator=g0), torch.randn(D, generator=g0)
    gy, add = torch.randn(M, D, generator=g0), torch.randn(M, D, generator=g0)
    r64 = T.reference_add_layernorm(x, r, mask, p, gam, bet, 1e-5, gy)
    r32 = T.reference_add_layernorm(x, r, mask, p, gam, bet, 1e-5, gy, dtype=torch.float32)
    op = "add_layernorm"
    xs = [t.requires_grad_(True) for t in dev(x, r, gam, bet)]
    y = OO._AddLayerNorm.apply(*xs, 1e-5, p, seed)
    y.backward(dev(gy))
    check_slices(op, "y", y, r64["y"], r32["y"], 1, VAL)
    check_slices(op, "dx", xs[0].grad, r64["dx"], r32["dx"], 1, VAL)
    check_slices(op, "dr", xs[1].grad, r64["dr"], r32["dr"], 1, VAL)
    check(op, "dgamma", xs[2].grad, r64["dgamma"], RED)
    check(op, "dbeta", xs[3].grad, r64["dbeta"], RED)
    if p > 0:
        assert float(xs[1].grad.cpu()[~mask].abs().max()) == 0.0
    # dx_add through raw pointers: dx = (the dx without it) + dx_add.  The compiler may fuse the last product of dx into the sum, so the
    # unrounded dx (within half an ulp of dx0) is added: the two sums differ by at most ulp(dx0) / 2 + ulp(sum), bounded from above below
    d_x, d_r, d_gam, d_bet = (t.detach() for t in xs)
    d_gy, d_add = dev(gy, add)
    yy, mean, rstd = sent(M, D), sent(M), sent(M)
    call("hoisdf_add_layernorm_fwd", P(d_x), P(d_r), P(d_gam), P(d_bet), P(yy), P(mean), P(rstd), M, D, 1e-5, float(p), seed, st())
    assert same_bits(yy, y)
    dx, dr, dgb = sent(M, D), sent(M, D), torch.zeros(2, D, device=DEV)
    call("hoisdf_add_layernorm_bwd", P(d_gy), P(d_x), P(d_r), P(d_gam), P(mean), P(rstd), P(d_add), P(dx), P(dr), P(dgb[0]), P(dgb[1]),
         M, D, float(p), seed, st())
    assert same_bits(dr, xs[1].grad)
    dx0 = xs[0].grad
    slack = dx0.abs() * 2.0 ** -24 + (dx0 + d_add).abs() * 2.0 ** -23
    assert bool(((dx - (dx0 + d_add)).abs() <= slack).all()), "dx with dx_add is not dx + dx_add within ulp(dx0) / 2 + ulp(sum)"
    check(op, "dgamma dx_add", dgb[0], r64["dgamma"], RED)
    check(op, "dbeta dx_add", dgb[1], r64["dbeta"], RED)


@pytest.mark.parametrize("G,R,Tk,D", [(5, 7, 3, 260), (3, 4, 4, 1024)])
def test_layernorm_rows_wide(G, R, Tk, D):
    g0 = gen("ln-rows", G, R, Tk, D)
    x = torch.randn(G * R, D, generator=g0)
    gam, bet = 1 + 0.3 * torch.randn(D, generator=g0), torch.randn(D, generator=g0)
    gy, add = torch.randn(G * Tk, D, generator=g0), torch.randn(G * R, D, generator=g0)
    taken = x.view(G, R, D)[:, :Tk].reshape(G * Tk, D)
    r64 = T.reference_add_layernorm(taken, None, None, 0.0, gam, bet, 1e-5, gy)
    r32 = T.reference_add_layernorm(taken, None, None, 0.0, gam, bet, 1e-5, gy, dtype=torch.float32)
    op = "layernorm_rows"
    d_x, d_gam, d_bet, d_gy, d_add = dev(x, gam, bet, gy, add)
    y, mean, rstd = sent(G * Tk, D), sent(G * Tk), sent(G * Tk)
    call("hoisdf_layernorm_rows_fwd", P(d_x), P(d_gam), P(d_bet), P(y), P(mean), P(rstd), G, R, Tk, D, 1e-5, st())
    check_slices(op, "y", y, r64["y"], r32["y"], 1, VAL)
    live = torch.zeros(G, R, dtype=torch.bool)
    live[:, :Tk] = True
    live = live.view(-1)
    for use_add in (True, False):
        dx, dg, db = sent(G * R, D), torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        call("hoisdf_layernorm_rows_bwd", P(d_gy), P(d_x), P(d_gam), P(mean), P(rstd), P(d_add) if use_add else None, P(dx), P(dg), P(db),
             G, R, Tk, D, st())
        dxc = dx.cpu()
        if bool((~live).any()):
            want = add[~live] if use_add else torch.zeros_like(add[~live])
            assert same_bits(dxc[~live], want), "rows with t >= take receive exactly dx_add, or 0"
        want64 = r64["dx"] + (add[live].double() if use_add else 0.0)
        want32 = r32["dx"] + (add[live] if use_add else 0.0)
        check_slices(op, f"dx add={int(use_add)}", dxc[live], want64, want32, 1, VAL)
        check(op, "dgamma", dg, r64["dgamma"], RED)
        check(op, "dbeta", db, r64["dbeta"], RED)


@pytest.mark.parametrize("M,D", [(37, 64), (37, 260)])
def test_layernorm_rows_of_large_mean(M, D):
    """rows of mean 1e4 and unit spread: x - mean cancels four digits, so the only fair bar is what float32 itself can do - the larger
    of 2e-5 and four times the row-wise error of the same formula in float32 on the CPU"""
    O = ops()
    g0 = gen("ln-mean", M, D)
    x = torch.randn(M, D, generator=g0) + 1e4
    gam, bet = 1 + 0.1 * torch.randn(D, generator=g0), torch.randn(D, generator=g0)
    r64 = T.reference_add_layernorm(x, None, None, 0.0, gam, bet)
    r32 = T.reference_add_layernorm(x, None, None, 0.0, gam, bet, dtype=torch.float32)
    y = O.add_layernorm(dev(x), None, dev(gam), dev(bet))
    check_slices("add_layernorm-mean", "y", y, r64["y"], r32["y"], 1, VAL, tensor_wide=False)
