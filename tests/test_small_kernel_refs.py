"""The fp64 references of hoisdf_amd.testing that tests/test_gpu_small_kernels.py holds the small hot-path kernels to, checked without a
GPU against what the project already trusts (the CPU oracle, torch's own operators, the fp32 expressions of tests/test_gpu_ops.py) at
1e-5 of scale, and the two input conditioners at every shape the GPU file uses."""
import math

import pytest
import torch
import torch.nn.functional as F

from hoisdf_amd import testing as T
from oracle import hoisdf_oracle as R


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(got, ref, rel=1e-5, what=""):
    err = T.rel_err(got, ref)
    assert err <= rel, f"{what}: {err:.3e} of the reference's max (bar {rel:.0e})"


@pytest.mark.parametrize("P", [1, 5, 130])
def test_reference_vote_loss_agrees_with_the_oracle(P):
    L, B, J = 3, 2, 20
    off, cls, pts, gt, _ = T.vote_case_inputs(L, B, P, J, "randn")
    gj = rnd(L, B, J, 3, seed=1)
    o32, c32 = off.clone().requires_grad_(True), cls.clone().requires_grad_(True)
    l1, l2, _l3, joints = R.joint_vote(pts, o32.permute(0, 2, 1, 3), c32.permute(0, 2, 1, 3), gt, T.VOTE_RADIUS)
    (0.3 * l1 + 0.7 * l2 + (joints * gj).sum()).backward()
    near_total = float(T.vote_near(pts, gt, T.VOTE_RADIUS)[1].sum())
    assert near_total > 0
    ref = T.reference_vote_loss(off, cls, pts, gt, T.VOTE_RADIUS, dj=gj, dl3d=torch.full((L, B), 0.3 / (near_total * 3.0 * L)),
                                dbce=torch.full((L, B), 0.7 / (L * B * P * J)))
    close(ref["joints"], joints, what="joints")
    assert float(ref["near_sum"].sum()) == near_total
    close((ref["l3d_sum"].sum(1) / near_total / 3.0).mean(), l1, what="loss_joint_3d")
    close(ref["bce_sum"].sum() / (L * B * P * J), l2, what="loss_joint_cls")
    close(ref["doff"], o32.grad, what="doff")
    close(ref["dcls"], c32.grad, what="dcls")
    plain = T.reference_vote(off, cls, pts, dj=gj)
    assert torch.equal(plain["joints"], ref["joints"])
    only_j = T.reference_vote_loss(off, cls, pts, gt, T.VOTE_RADIUS, dj=gj)
    assert torch.equal(plain["doff"], only_j["doff"]) and torch.equal(plain["dcls"], only_j["dcls"])


def test_reference_posenc_rows_agrees_with_the_oracle():
    pts = rnd(777, 3, seed=9) * 1.2
    close(T.reference_posenc_rows(pts), R.posenc(pts), what="pe")
    buf = T.reference_posenc_rows(pts, ld=40, col0=4, fill=-7.0)
    assert torch.equal(buf[:, 4:34], T.reference_posenc_rows(pts))
    assert torch.equal(buf[:, 34:37], pts.double()) and float(buf[:, 37:40].abs().max()) == 0.0
    assert bool((buf[:, :4] == -7.0).all())
    assert bool((T.reference_posenc_rows(pts, ld=34, col0=0, fill=-7.0)[:, 33] == 0.0).all())     # one pad column fits, it is zero


@pytest.mark.parametrize("beta", [0.08, 2e-3, 1e-4])
def test_reference_token_build_agrees_with_the_fp32_expression(beta):
    """the expression of test_token_build_and_vote, at the clamped beta: below 2e-3 the values and dbeta are those of 2e-3"""
    B, P, D = 2, 50, 256
    cam, center = rnd(B, P, 3, seed=50), rnd(B, 3, seed=51)
    pe, feat = rnd(B, P, 30, seed=52), rnd(B, P, D - 33, seed=53).requires_grad_(True)
    sdf = rnd(B, P, 1, seed=54) * 0.1
    be = torch.tensor([max(beta, T.TOKEN_BETA_MIN)], requires_grad=True)
    expr = torch.cat([cam - center[:, None], pe, feat * (torch.sigmoid(sdf / be) / be)], 2)
    gt = rnd(B, P, D, seed=55)
    (expr * gt).sum().backward()
    ref = T.reference_token_build(cam, center, pe, feat, sdf.view(B, P), torch.tensor([beta]), dtok=gt)
    close(ref["tok"], expr, what="tok")
    close(ref["dfeat"], feat.grad, what="dfeat")
    close(ref["dbeta"], be.grad, what="dbeta")
    assert float(ref["beta_eff"]) == max(float(torch.tensor(beta)), T.TOKEN_BETA_MIN)


def test_references_agree_with_torch_operators():
    v, g = rnd(7, 13, seed=1), rnd(7, 1, seed=2).abs() + 0.5
    dW = rnd(7, 16, seed=3)
    ref = T.reference_weight_norm(v, g, dW=dW, ldw=16)
    v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
    W = v64 * (g64 / v64.norm(dim=1, keepdim=True))
    W.backward(dW[:, :13].double())
    close(ref["W"][:, :13], W, 1e-12, "W"); close(ref["dv"], v64.grad, 1e-12, "dv"); close(ref["dg"], g64.grad.view(-1), 1e-12, "dg")
    assert float(ref["W"][:, 13:].abs().max()) == 0.0
    close(ref["norms"], v.double().norm(dim=1), 1e-12, "norms")

    h, w, b, gs = rnd(40, 8, seed=4), rnd(8, seed=5) * 0.1, torch.tensor([-0.05]), rnd(40, seed=6)
    ref = T.reference_sdf_head(h, w, b, 0.15, dsdf=gs)
    h64, w64, b64 = h.double().requires_grad_(True), w.double().view(1, 8).requires_grad_(True), b.double().requires_grad_(True)
    raw = torch.tanh(F.linear(h64, w64, b64)).view(-1)
    raw.clamp(-0.15, 0.15).backward(gs.double())
    close(ref["raw"], raw, 1e-12, "raw"); close(ref["dh"], h64.grad, 1e-12, "dh")
    close(ref["dw"], w64.grad.view(-1), 1e-12, "dw"); close(ref["db"], b64.grad, 1e-12, "db")
    assert 0 < int((ref["raw"].abs() > 0.15).sum()) < 40

    x, r = rnd(9, 12, seed=7), rnd(9, 12, seed=8)
    gam, bet, gy = 1 + 0.1 * rnd(12, seed=9), rnd(12, seed=10), rnd(9, 12, seed=11)
    keep = rnd(9, 12, seed=12) > -0.5
    ref = T.reference_add_layernorm(x, r, keep, 0.3, gam, bet, dy=gy)
    xs = [t.double().requires_grad_(True) for t in (x, r, gam, bet)]
    y = F.layer_norm(xs[0] + xs[1] * keep.double() / 0.7, (12,), xs[2], xs[3], 1e-5)
    y.backward(gy.double())
    close(ref["y"], y, 1e-12, "y")
    for n, t in zip(("dx", "dr", "dgamma", "dbeta"), xs):
        close(ref[n], t.grad, 1e-11, n)
    assert T.reference_add_layernorm(x, None, None, 0.0, gam, bet, dy=gy)["dr"] is None


def test_slice_measure_sees_what_the_tensor_measure_hides():
    ref = torch.ones(3, 4, 50, dtype=torch.float64)
    ref[1, 2] *= 1e-8                                   # a slice many decades below the loudest
    got = ref.clone()
    got[1, 2, 7] *= 1.5
    assert T.rel_err(got, ref) < 1e-8
    assert abs(T.slice_err(got, ref, 2) - 0.5) < 1e-12
    bar, e32 = T.slice_bar(ref.float(), ref, 2, 2e-5)
    assert bar == 2e-5 and e32 < 1e-7


@pytest.mark.parametrize("M", T.HEAD_MS)
@pytest.mark.parametrize("K", T.HEAD_KS)
def test_head_conditioner_holds_at_every_shape(M, K):
    h, w, b, _, _ = T.head_case_inputs(M, K)
    assert T.head_rows_margin(h, w, b, T.HEAD_CLAMP) >= 1e-5
    raw = T.reference_sdf_head(h, w, b, T.HEAD_CLAMP)["raw"]
    sat = T.head_saturated_rows(M)
    assert bool((raw[sat].abs() == 1.0).all())          # tanh(+-20) is exactly +-1 in float64 (and in float32)
    assert bool((torch.tanh(T.reference_sdf_head(h, w, b, T.HEAD_CLAMP, dtype=torch.float32)["pre"][sat]).abs() == 1.0).all())
    if M >= 4097:
        outside = float((raw.abs() > T.HEAD_CLAMP).double().mean())
        assert 0.25 < outside < 0.42, outside


def test_head_conditioner_redraws_what_sits_on_the_clamp():
    K = 8
    w, b = rnd(K, seed=1) * 0.05, torch.tensor([-0.02])
    h = rnd(300, K, seed=2)
    for r, t in ((5, 0.15), (17, -0.15), (200, 0.150004)):            # rows put on / beside the threshold
        h[r] = w * ((math.atanh(t) + 0.02) / float(w.double().pow(2).sum()))
    assert T.head_rows_margin(h, w, b, 0.15) < 1e-5
    h2, n = T.condition_head_rows(h, w, b, 0.15, lambda g, m: torch.randn(m, K, generator=g), 3)
    assert n >= 3 and T.head_rows_margin(h2, w, b, 0.15) >= 1e-5
    keep = torch.ones(300, dtype=torch.bool); keep[[5, 17, 200]] = False
    assert torch.equal(h2[keep], h[keep])


@pytest.mark.parametrize("L,B,P,J", T.VOTE_CASES)
def test_vote_conditioner_holds_at_every_shape(L, B, P, J):
    for far in (None, 1) if (B, P, J) == (2, 257, 20) else (None,):
        _, _, pts, gt, _ = T.vote_case_inputs(L, B, P, J, "equal", far_sample=far)
        assert T.vote_points_margin(pts, gt, T.VOTE_RADIUS) >= 1e-6
        near = T.vote_near(pts, gt, T.VOTE_RADIUS)[1]
        assert int(near[0].sum()) > 0
        if far is not None:
            assert int(near[far].sum()) == 0


def test_vote_conditioner_is_needed_and_ends_at_1025_points_64_joints():
    """65 600 (point, joint) pairs against a 2e-6 m shell: about four draws in ten have a point inside it.  The first stream of 64 that
    has one (whichever the generator makes it) shows the loop is needed; the loop replaces the point and ends"""
    margins = ((s, T.vote_points_margin(*T.vote_case_points(1, 1025, 64, salt=s)[:2], T.VOTE_RADIUS)) for s in range(64))
    salt = next(s for s, m in margins if m < 1e-6)
    pts, gt, _ = T.vote_case_points(1, 1025, 64, salt=salt)
    _, _, cond, _, redrawn = T.vote_case_inputs(1, 1, 1025, 64, "equal", salt=salt)
    assert redrawn >= 1
    assert T.vote_points_margin(cond, gt, T.VOTE_RADIUS) >= 1e-6
    assert 1 <= int((cond != pts).any(-1).sum()) <= redrawn                 # (a point may be drawn twice)
