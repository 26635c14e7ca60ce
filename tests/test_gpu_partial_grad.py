"""-m gpu: the autograd nodes of hoisdf_amd/ops.py with a PROPER SUBSET of their inputs requiring a gradient (frozen BatchNorm affine
parameters, query points and targets, a checkpoint fine-tuned with most of it frozen), each against the same operation in plain torch
fp64 run with the same subset: every tensor that requires a gradient gets one within the bar of the op's all-trainable test at that
shape, every other tensor keeps ``.grad is None``.  Also the paths of csrc/bnact.hip no other test reaches (the capped streaming
grid's second trip, 256 slices in one finishing block, a ragged last slice, 255 channel chunks, the backward without gamma).

ReLU gates: a pre-activation within fp32 rounding of zero may legitimately flip and would put a whole dy element into a column sum,
so every case chooses inputs whose fp64 REFERENCE is clear of zero and asserts that on the reference before anything is compared;
no element is excluded from any comparison."""
import math

import pytest
import torch
import torch.nn.functional as F

from hoisdf_amd import testing as T

pytestmark = pytest.mark.gpu

DEV = "cuda"


def ops():
    from hoisdf_amd import ops as O
    return O


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def close(got, want, bar, what):
    """max abs error <= bar * max |reference| (the measure of test_gpu_bnact.rel and test_gpu_ops.assert_close)"""
    got = got.detach().double()
    want = want.detach().double().to(got.device)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-30)
    err = float((got - want).abs().max())
    print(f"{what}: max abs err {err:.3e}, scale {scale:.3e}, rel {err / scale:.2e} (bar {bar:.0e})")
    assert err <= bar * scale + 1e-12, f"{what}: max abs err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e}, bar {bar:.0e})"


def grads_match(pairs, bar):
    """pairs: (name, tensor of the run under test, its fp64 twin or None).  A twin that requires a gradient: both have one, within the
    bar; otherwise the tensor under test must not have been given one."""
    for name, t, ref in pairs:
        if t is None:
            continue
        if ref is not None and ref.requires_grad:
            assert ref.grad is not None, name
            assert t.grad is not None, f"d{name} is missing"
            close(t.grad, ref.grad, bar[name] if isinstance(bar, dict) else bar, "d" + name)
        else:
            assert t.grad is None, f"{name} requires no gradient and got one"


# ---------------------------------------------------------------------------------------------
# A. ops.bn_act: the requires-grad matrix
# ---------------------------------------------------------------------------------------------
BN_BAR = 2e-5                       # tests/test_gpu_bnact.py: max abs error <= 2e-5 of max |reference|, y and every gradient
BN_SHAPES = {(2, 32, 5, 6): 101, (3, 96, 7, 5): 108}        # shape -> seed (the no-residual gates of both are clear of zero: asserted)
ALL = ("x", "weight", "bias", "residual")


def bn_inputs(shape, seed, dev="cpu"):
    n, c, h, w = shape
    g = torch.Generator(device=dev).manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    return dict(x=r(n, c, h, w) * 1.7 + 0.6, residual=r(n, c, h, w), weight=torch.rand(c, generator=g, device=dev) + 0.5, bias=r(c) * 0.3,
                rm=r(c) * 0.1, rv=torch.rand(c, generator=g, device=dev) + 0.5, gy=r(n, c, h, w))


def nudge_residual(pre64, res):
    """every residual element that leaves the fp64 pre-activation within 1e-3 of zero is pushed out by 2e-3 (the residual does not enter
    the statistics, so ``pre64 = bn(x)`` stands)"""
    t = pre64 + res.double()
    out = (res.double() + torch.where(t >= 0, 2e-3, -2e-3)).float()
    return torch.where(t.abs() < 1e-3, out, res)


def bn_reference(d, subset, relu, has_res, affine, momentum=0.1, eps=1e-5):
    """torch's batch_norm (+ add) (+ relu) in fp64 with the given requires-grad subset -> (leaves, y, running mean, running var);
    d["residual"] is nudged in place of the gates first, and the gates are asserted clear"""
    dev = d["x"].device
    w0, b0 = (d["weight"].double(), d["bias"].double()) if affine else (None, None)
    with torch.no_grad():
        pre = F.batch_norm(d["x"].double(), None, None, w0, b0, True, momentum, eps)
        if has_res:
            d["residual"] = nudge_residual(pre, d["residual"])
            t = pre + d["residual"].double()
            assert float(t.abs().min()) >= 1e-3
        elif relu:
            assert float(pre.abs().min()) >= 1e-5, float(pre.abs().min())
    leaf = {k: d[k].double().clone().requires_grad_(k in subset) for k in ALL if (k != "residual" or has_res) and (affine or k in ("x", "residual"))}
    rm, rv = d["rm"].double().clone(), d["rv"].double().clone()
    y = F.batch_norm(leaf["x"], rm, rv, leaf.get("weight"), leaf.get("bias"), True, momentum, eps)
    if has_res:
        y = y + leaf["residual"]
    y = F.relu(y) if relu else y
    y.backward(d["gy"].double().to(dev))
    return leaf, y.detach(), rm, rv


def laid_out(t, layout):
    """a CPU (N, C, H, W) map -> a leaf on the device: channels_last-dense | NCHW-contiguous | a channel slice of a wider channels_last map"""
    t = t.to(DEV)
    n, c, h, w = t.shape
    if layout == "cl":
        return t.contiguous(memory_format=torch.channels_last)
    if layout == "nchw":
        return t.contiguous()
    wide = torch.zeros(n, h, w, c + 24, device=DEV).permute(0, 3, 1, 2)
    wide[:, 8:8 + c] = t
    return wide[:, 8:8 + c].detach()


def _bn_cases():
    out = []
    for shape in BN_SHAPES:
        for layout in ("cl", "nchw", "slice"):
            for relu in (True, False):
                for has_res in (False, True):
                    subsets = [("x",), ("weight",), ("bias",), ("weight", "bias"), ("x", "weight", "bias") + (("residual",) if has_res else ())]
                    if has_res:
                        subsets += [("x", "residual"), ("residual",)]          # (x, residual): the freeze_stages configuration
                    for s in subsets:
                        out.append((shape, layout, relu, has_res, True, s))
                    out.append((shape, layout, relu, has_res, False, ("x",)))   # weight = bias = None: the backward with a null gamma
    return [pytest.param(*c, id="-".join(["x".join(map(str, c[0])), c[1], "relu" if c[2] else "lin", "res" if c[3] else "nores",
                                          "affine" if c[4] else "plain", "+".join(c[5])])) for c in out]


@pytest.mark.parametrize("shape,layout,relu,has_res,affine,subset", _bn_cases())
def test_bn_act_with_a_subset_requiring_gradients(shape, layout, relu, has_res, affine, subset):
    O = ops()
    d = bn_inputs(shape, BN_SHAPES[shape])
    ref, y64, rm64, rv64 = bn_reference(d, subset, relu, has_res, affine)
    x = laid_out(d["x"], layout).requires_grad_("x" in subset)
    res = laid_out(d["residual"], layout).requires_grad_("residual" in subset) if has_res else None
    wt = d["weight"].to(DEV).requires_grad_("weight" in subset) if affine else None
    bs = d["bias"].to(DEV).requires_grad_("bias" in subset) if affine else None
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    y = O.bn_act(x, wt, bs, rm, rv, True, 0.1, 1e-5, relu, res)
    assert y.is_contiguous(memory_format=torch.channels_last)
    y.backward(d["gy"].to(DEV).contiguous(memory_format=torch.channels_last))
    close(y, y64, BN_BAR, "y")
    close(rm, rm64, 1e-6, "running mean"); close(rv, rv64, 1e-5, "running var")
    grads_match([("x", x, ref["x"]), ("weight", wt, ref.get("weight")), ("bias", bs, ref.get("bias")), ("residual", res, ref.get("residual"))], BN_BAR)


def test_bn_act_refuses_a_cumulative_average_of_running_statistics():
    """momentum=None is torch's 1 / num_batches_tracked average: the kernels take a number (0.0 would leave the statistics where they are)"""
    O = ops()
    d = bn_inputs((2, 32, 5, 6), 1)
    x = laid_out(d["x"], "cl")
    rm, rv = d["rm"].to(DEV), d["rv"].to(DEV)
    with pytest.raises((ValueError, RuntimeError), match="momentum"):
        O.bn_act(x, d["weight"].to(DEV), d["bias"].to(DEV), rm, rv, True, None, 1e-5, True, None)
    assert torch.equal(rm.cpu(), d["rm"]) and torch.equal(rv.cpu(), d["rv"])
    y = O.bn_act(x, None, None, None, None, True, None, 1e-5, False, None)           # nothing to update: momentum is not read
    close(y, F.batch_norm(x.double(), None, None, None, None, True, 0.0, 1e-5), BN_BAR, "y")


def test_encoder_bn_act_with_momentum_none_tracks_the_cumulative_average():
    """nets/encoder.bn_act routes BatchNorm2d(momentum=None) to torch: running statistics after two steps vs the fp64 module"""
    from hoisdf_amd.nets import encoder as E
    c = 32
    bn = torch.nn.BatchNorm2d(c, momentum=None).to(DEV).train()
    bn64 = torch.nn.BatchNorm2d(c, momentum=None).to(DEV).double().train()
    with torch.no_grad():
        bn.weight.copy_(rnd(c, seed=1) * 0.2 + 1.0); bn.bias.copy_(rnd(c, seed=2) * 0.3)
        bn64.weight.copy_(bn.weight.double()); bn64.bias.copy_(bn.bias.double())
    for step in range(2):
        x = laid_out(rnd(3, c, 7, 5, seed=10 + step) * (1.0 + step) + 0.5 * step, "cl")
        res = laid_out(rnd(3, c, 7, 5, seed=20 + step), "cl")
        y = E.bn_act(bn, x, True, residual=res)
        E.flush_bn_counters()
        y64 = F.relu(bn64(x.double()) + res.double())
        close(y, y64, BN_BAR, f"y (step {step})")
    assert int(bn.num_batches_tracked) == 2
    # (the library's f32 statistics, not this project's kernels: 1e-5 of scale; statistics that never moved would be off by their whole size)
    close(bn.running_mean, bn64.running_mean, 1e-5, "running mean"); close(bn.running_var, bn64.running_var, 1e-5, "running var")


@pytest.mark.parametrize("which", ["x", "weight", "bias", "residual"])
def test_bn_act_evaluation_mode_refuses_a_gradient_path(which):
    """training=False keeps nothing for a backward: refused at the call, by name, not by a tuple-unpack error in backward"""
    O = ops()
    d = bn_inputs((2, 32, 5, 6), 3)
    t = dict(x=laid_out(d["x"], "cl"), residual=laid_out(d["residual"], "cl"), weight=d["weight"].to(DEV), bias=d["bias"].to(DEV))
    t[which].requires_grad_(True)
    with pytest.raises(RuntimeError, match="bn_act"):
        O.bn_act(t["x"], t["weight"], t["bias"], d["rm"].to(DEV), d["rv"].to(DEV), False, 0.1, 1e-5, True, t["residual"])
    with torch.no_grad():                                      # (no gradient path: evaluation as before)
        y = O.bn_act(t["x"], t["weight"], t["bias"], d["rm"].to(DEV), d["rv"].to(DEV), False, 0.1, 1e-5, True, t["residual"])
    want = F.relu(F.batch_norm(d["x"].double(), d["rm"].double(), d["rv"].double(), d["weight"].double(), d["bias"].double(), False, 0.1, 1e-5)
                  + d["residual"].double())
    close(y, want, BN_BAR, "y")


# ---------------------------------------------------------------------------------------------
# B. csrc/bnact.hip: the paths no other test runs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [
    pytest.param((1, 2048, 129, 128), id="C2048-M16512"),      # 16512 block iterations > 4 x 4096 blocks: the second trip of the capped streaming loop (forward, dx)
    pytest.param((1, 8, 512, 512), id="C8-M262144"),           # 256 slices of 1024 rows: the most one finishing block folds
    pytest.param((1, 8, 513, 512), id="C8-M262656"),           # rows_per_block doubles: 129 slices, the last one of 512 rows
    pytest.param((2, 2040, 7, 5), id="C2040-M70"),             # chunk = 8: 255 chunks of one slice (smax clamped to 16)
])
def test_bn_act_paths_of_the_kernels_no_other_test_reaches(shape):
    """forward, running statistics and every gradient against fp64, ReLU + residual, everything trainable"""
    O = ops()
    d = bn_inputs(shape, 77, dev=DEV)
    ref, y64, rm64, rv64 = bn_reference(d, ALL, True, True, True)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    x, res = cl(d["x"]).requires_grad_(True), cl(d["residual"]).requires_grad_(True)
    wt, bs = d["weight"].clone().requires_grad_(True), d["bias"].clone().requires_grad_(True)
    rm, rv = d["rm"].clone(), d["rv"].clone()
    y = O.bn_act(x, wt, bs, rm, rv, True, 0.1, 1e-5, True, res)
    y.backward(cl(d["gy"]))
    close(y, y64, BN_BAR, "y")
    close(rm, rm64, 1e-6, "running mean"); close(rv, rv64, 1e-5, "running var")
    grads_match([("x", x, ref["x"]), ("weight", wt, ref["weight"]), ("bias", bs, ref["bias"]), ("residual", res, ref["residual"])], BN_BAR)


# ---------------------------------------------------------------------------------------------
# C. ops.linear
# ---------------------------------------------------------------------------------------------
LIN_ROUTES = [(17, 60, 256), (300, 223, 289), (544, 1024, 256)]      # M, N, K: small-row route | ragged f32 route | emulated route
LIN_SUBSETS = [("x",), ("W",), ("b",), ("W", "b"), ("x", "b"), ("x", "nob"), ("W", "nob")]      # "nob": b = None
LIN_NOB_SEED = {17: 100, 300: 101, 544: 111}        # x seeds whose bias-FREE sums are clear of zero as well (seed 1 leaves one at 4e-7)


@pytest.mark.parametrize("subset", LIN_SUBSETS, ids=lambda s: "+".join(s))
@pytest.mark.parametrize("act", [False, True], ids=["lin", "relu"])
@pytest.mark.parametrize("M,N,K", LIN_ROUTES)
def test_linear_with_a_subset_requiring_gradients(M, N, K, act, subset):
    """the inputs (and so the gates) of test_gpu_ops.test_linear_fwd_bwd; without the bias, another x"""
    O = ops()
    has_b = "nob" not in subset
    x0, W0, b0, gy = rnd(M, K, seed=1 if has_b or not act else LIN_NOB_SEED[M]), rnd(N, K, seed=2) / math.sqrt(K), rnd(N, seed=3), rnd(M, N, seed=4)
    x, W = x0.double().requires_grad_("x" in subset), W0.double().requires_grad_("W" in subset)
    b = b0.double().requires_grad_("b" in subset) if has_b else None
    ref = F.linear(x, W, b)
    if act:
        assert float(ref.detach().abs().min()) >= 1e-6            # (f32 rounding of these sums of O(1) is ~1e-7: no gate flips)
        ref = F.relu(ref)
    ref.backward(gy.double())
    xg, Wg = x0.to(DEV).requires_grad_("x" in subset), W0.to(DEV).requires_grad_("W" in subset)
    bg = b0.to(DEV).requires_grad_("b" in subset) if has_b else None
    y = O.linear(xg, Wg, bg, act=act)
    y.backward(gy.to(DEV))
    close(y, ref, 2e-5, "y")
    grads_match([("x", xg, x), ("W", Wg, W), ("b", bg, b)], 2e-5)


def test_linear_dropout_with_only_the_bias_trainable():
    """db = the column sums of gy * kept / (1 - p), kept read from the kernel's own output (as test_linear_dropout_statistics_and_backward_mask)"""
    O = ops()
    O.manual_seed(123)
    M, N, K, p = 2048, 512, 256, 0.2
    x = rnd(M, K, seed=7).to(DEV)
    W = (rnd(N, K, seed=8) / 16).to(DEV)
    b = torch.full((N,), 0.5, device=DEV).requires_grad_(True)
    gy = rnd(M, N, seed=9).to(DEV)
    y = O.linear(x, W, b, act=True, drop_p=p)
    base = F.relu(F.linear(x.double(), W.double(), b.detach().double()))
    kept = y.detach() > 0
    assert not bool((kept & ~(base > 0)).any())
    frac = kept.sum().item() / (base > 0).sum().item()
    assert abs(frac - (1 - p)) < 0.01, frac
    close(y.detach()[kept], base[kept] / (1 - p), 2e-5, "kept scaling")
    y.backward(gy)
    close(b.grad, (gy.double() * kept.double() / (1 - p)).sum(0), 2e-5, "db")
    assert x.grad is None and W.grad is None


# ---------------------------------------------------------------------------------------------
# D. attention nodes
# ---------------------------------------------------------------------------------------------
def ref_attention(q, k, v, H, kv_len=None, mask=None):
    B, Lq, E = q.shape
    Lk = k.shape[1]
    dh = E // H
    qh = q.reshape(B, Lq, H, dh).transpose(1, 2) / math.sqrt(dh)
    kh = k.reshape(B, Lk, H, dh).transpose(1, 2)
    vh = v.reshape(B, Lk, H, dh).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2)
    if kv_len is not None:
        s = s.masked_fill((torch.arange(Lk, device=s.device) >= kv_len)[None, None, None], float("-inf"))
    if mask is not None:
        s = s.masked_fill(mask[None, None], float("-inf"))
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Lq, E)


@pytest.mark.parametrize("subset", [("q",), ("kv",)], ids=lambda s: s[0])
def test_attention_cross_with_one_side_trainable(subset):
    """the 17 queries x 300 keys of test_gpu_ops.test_attention_cross_17_queries and its bars"""
    O = ops()
    B, Lq, Lk, E, H, kv = 2, 17, 300, 256, 4, 230
    q0, kv0, go = rnd(B, Lq, E, seed=22), rnd(B, Lk, 2 * E, seed=23), rnd(B, Lq, E, seed=24)
    q, kvt = q0.double().requires_grad_("q" in subset), kv0.double().requires_grad_("kv" in subset)
    ref = ref_attention(q, kvt[..., :E], kvt[..., E:], H, kv)
    ref.backward(go.double())
    qg, kg = q0.to(DEV).requires_grad_("q" in subset), kv0.to(DEV).requires_grad_("kv" in subset)
    o = O.attention_cross(qg, kg, H, kv)
    o.backward(go.to(DEV))
    close(o, ref, 2e-5, "cross out")
    grads_match([("q", qg, q), ("kv", kg, kvt)], 5e-5)


def test_attention_self_gradient_free_forward_then_a_trainable_one():
    """the output read under no_grad first, and from a detached copy (needs_input_grad follows the tensors, not the grad mode: only the
    detached call is the forward that keeps nothing), then a fresh forward that a backward follows: same values"""
    O = ops()
    B, L, kv, E, H = 2, 300, 230, 256, 4
    qkv0, go = rnd(B, L, 3 * E, seed=20), rnd(B, L, E, seed=21)
    qkv = qkv0.double().requires_grad_(True)
    ref = ref_attention(qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], H, kv)
    ref.backward(go.double())
    x = qkv0.to(DEV).requires_grad_(True)
    with torch.no_grad():
        o0 = O.attention_self(x, H, kv)
        o00 = O.attention_self(x.detach(), H, kv)
    assert not o0.requires_grad and not o00.requires_grad
    o = O.attention_self(x, H, kv)
    assert torch.equal(o0, o.detach()) and torch.equal(o00, o.detach())
    o.backward(go.to(DEV))
    close(o, ref, 2e-5, "attn out")
    close(x.grad, qkv.grad, 5e-5, "attn dqkv")
    assert float(x.grad[:, kv:, E:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# E. the coarse layers
# ---------------------------------------------------------------------------------------------
ENC_NAMES = ["w_in", "b_in", "w_out", "b_out", "g1", "be1", "w1", "b1", "w2", "b2", "g2", "be2", "g3", "be3"]
DEC_NAMES = ["sa_w_in", "sa_b_in", "sa_w_out", "sa_b_out", "ca_w_in", "ca_b_in", "ca_w_out", "ca_b_out", "w1", "b1", "w2", "b2",
             "g1", "be1", "g2", "be2", "g3", "be3", "gn", "ben"]
LAYER_SUBSETS = ["inputs", "vectors", "w1", "all"]        # only the input(s) | only biases and LayerNorm gains / biases | only w1 | all
E_, F_, H_ = 256, 1024, 4


def layer_params(names, seed):
    shape = lambda n: ((3 * E_, E_) if n.endswith("w_in") else (E_, E_) if n.endswith("w_out") else (F_, E_) if n == "w1" else (E_, F_) if n == "w2"
                       else (3 * E_,) if n.endswith("b_in") else (F_,) if n == "b1" else (E_,))
    return [rnd(*shape(n), seed=seed + i) * (1.0 / math.sqrt(shape(n)[-1]) if len(shape(n)) == 2 else 0.1) + (1.0 if n[0] == "g" else 0.0)
            for i, n in enumerate(names)]


def trainable(name, subset, inputs):
    matrix = name in ("w1", "w2") or name.endswith("w_in") or name.endswith("w_out")
    return (subset == "all" or (subset == "inputs" and name in inputs) or (subset == "w1" and name == "w1")
            or (subset == "b_in only" and name == "b_in") or (subset == "vectors" and name not in inputs and not matrix))


def ln(x, g, b, eps=1e-5):
    return F.layer_norm(x, (x.shape[-1],), g, b, eps)


def ffn(x, w1, b1, w2, b2):
    pre = F.linear(x, w1, b1)
    assert float(pre.detach().abs().min()) >= 1e-5, float(pre.detach().abs().min())       # the hidden layer's gates, on the reference
    return F.linear(F.relu(pre), w2, b2)


def encoder_layer_ref(x, nq, ni, P):
    """common/nets/transformer.py forward_post + the stack's inter_norm: rows < n_query produced, rows < n_inter normed"""
    w_in, b_in, w_out, b_out, g1, be1, w1, b1, w2, b2, g2, be2, g3, be3 = P
    qkv = F.linear(x, w_in, b_in)
    o = ref_attention(qkv[:, :nq, :E_], qkv[..., E_:2 * E_], qkv[..., 2 * E_:], H_)
    x1 = ln(x[:, :nq] + F.linear(o, w_out, b_out), g1, be1)
    x2 = ln(x1 + ffn(x1, w1, b1, w2, b2), g2, be2)
    return x2, ln(x2[:, :ni], g3, be3)


def decoder_layer_ref(tgt, mem, qpos, mask, kv_len, P):
    """common/nets/transformer.py decoder layer, post-norm, + the stack's norm of its output"""
    sw, sb, sow, sob, cw, cb, cow, cob, w1, b1, w2, b2, g1, be1, g2, be2, g3, be3, gn, ben = P
    qk = F.linear(tgt + qpos, sw[:2 * E_], sb[:2 * E_])
    v = F.linear(tgt, sw[2 * E_:], sb[2 * E_:])
    o = ref_attention(qk[..., :E_], qk[..., E_:], v, H_, mask=mask)
    tgt = ln(tgt + F.linear(o, sow, sob), g1, be1)
    q = F.linear(tgt + qpos, cw[:E_], cb[:E_])
    kv = F.linear(mem, cw[E_:], cb[E_:])
    o = ref_attention(q, kv[..., :E_], kv[..., E_:], H_, kv_len)
    tgt = ln(tgt + F.linear(o, cow, cob), g2, be2)
    out = ln(tgt + ffn(tgt, w1, b1, w2, b2), g3, be3)
    return out, ln(out, gn, ben)


ENC_SHAPES = [(2, 64, None, None, 13), (3, 100, 40, 17, 11)]        # B, S, n_query, n_inter of test_coarse_encoder_layer_entry_equals_the_op_chain (p = 0), x seed
ENC_BAR = 2e-5                                                      # that test's bar for gradients that are not bit-identical
DEC_BAR = 1e-5                                                      # test_coarse_decoder_layer_entry_equals_the_op_chain


def run_encoder_layer(B, S, nq, ni, xseed, subset, coarse, f16=False):
    O = ops()
    nqe = S if nq is None else nq
    nie = nqe if ni is None else ni
    x0, P0 = rnd(B, S, E_, seed=xseed), layer_params(ENC_NAMES, 20)
    gx2, gy = rnd(B, nqe, E_, seed=5), rnd(B, nie, E_, seed=6)
    x = x0.double().requires_grad_(trainable("x", subset, ("x",)))
    P = [t.double().requires_grad_(trainable(n, subset, ("x",))) for n, t in zip(ENC_NAMES, P0)]
    x2r, yr = encoder_layer_ref(x, nqe, nie, P)
    ((x2r * gx2.double()).sum() + (yr * gy.double()).sum()).backward()
    xg = x0.to(DEV).requires_grad_(x.requires_grad)
    Pg = [t.to(DEV).requires_grad_(r.requires_grad) for t, r in zip(P0, P)]
    keep = O._ENCODER_LAYER_C
    O._ENCODER_LAYER_C = coarse
    O.set_attention_f16_eval(f16)
    try:
        x2, y = O.encoder_layer(xg, nq, 0.0, H_, *Pg, eps=1e-5, n_inter=ni)
        ((x2 * gx2.to(DEV)).sum() + (y * gy.to(DEV)).sum()).backward()
    finally:
        O._ENCODER_LAYER_C = keep
        O.set_attention_f16_eval(False)
    close(x2, x2r, ENC_BAR, "x2"); close(y, yr, ENC_BAR, "y")
    grads_match([("x", xg, x)] + [(n, t, r) for n, t, r in zip(ENC_NAMES, Pg, P)], ENC_BAR)
    return x2.detach(), y.detach()


@pytest.mark.parametrize("subset", LAYER_SUBSETS)
@pytest.mark.parametrize("coarse", [True, False], ids=["entry", "node"])
@pytest.mark.parametrize("B,S,nq,ni,xseed", ENC_SHAPES)
def test_encoder_layer_with_a_subset_requiring_gradients(B, S, nq, ni, xseed, coarse, subset):
    run_encoder_layer(B, S, nq, ni, xseed, subset, coarse)


@pytest.mark.parametrize("coarse", [True, False], ids=["entry", "node"])
def test_encoder_layer_f16_eval_switch_with_only_a_bias_trainable(coarse):
    """set_attention_f16_eval(True) is for gradient-free calls: with b_in trainable a backward follows, so the layer must take the f32
    path (the f16 forward keeps no log-sum-exp) - the result is the f32-path result, to the bit in deterministic mode (order-fixed sums)"""
    O = ops()
    B, S, nq, ni, xseed = ENC_SHAPES[0]
    keep = O.deterministic()
    O.set_deterministic(True)
    try:
        out32 = run_encoder_layer(B, S, nq, ni, xseed, "b_in only", coarse, f16=False)
        out16 = run_encoder_layer(B, S, nq, ni, xseed, "b_in only", coarse, f16=True)
    finally:
        O.set_deterministic(keep)
    assert torch.equal(out32[0], out16[0]) and torch.equal(out32[1], out16[1])
    assert not O._ATTENTION_F16_EVAL


@pytest.mark.parametrize("subset", LAYER_SUBSETS)
def test_decoder_layer_with_a_subset_requiring_gradients(subset):
    O = ops()
    B, S, kv, Q = 2, 64, 48, 17                       # test_coarse_decoder_layer_entry_equals_the_op_chain's p = 0 shape
    g = torch.Generator().manual_seed(3)
    mask = torch.rand(Q, Q, generator=g) < 0.2
    mask[torch.arange(Q), torch.arange(Q)] = False
    ins = ("tgt", "memory", "query_pos")
    t0, m0, q0, P0 = rnd(B, Q, E_, seed=7), rnd(B, S, E_, seed=8), rnd(Q, E_, seed=9) * 0.5, layer_params(DEC_NAMES, 40)
    g_out, g_y = rnd(B, Q, E_, seed=10), rnd(B, Q, E_, seed=13)
    tgt, mem, qpos = (t.double().requires_grad_(trainable(n, subset, ins)) for n, t in zip(ins, (t0, m0, q0)))
    P = [t.double().requires_grad_(trainable(n, subset, ins)) for n, t in zip(DEC_NAMES, P0)]
    outr, yr = decoder_layer_ref(tgt, mem, qpos, mask, kv, P)
    ((outr * g_out.double()).sum() + (yr * g_y.double()).sum()).backward()
    tg, mg, qg = (t.to(DEV).requires_grad_(r.requires_grad) for t, r in zip((t0, m0, q0), (tgt, mem, qpos)))
    Pg = [t.to(DEV).requires_grad_(r.requires_grad) for t, r in zip(P0, P)]
    out, y = O.decoder_layer(tg, mg, qg, mask.to(torch.uint8).to(DEV), kv, 0.0, H_, 1e-5, *Pg)
    ((out * g_out.to(DEV)).sum() + (y * g_y.to(DEV)).sum()).backward()
    close(out, outr, DEC_BAR, "out"); close(y, yr, DEC_BAR, "y")
    grads_match([("tgt", tg, tgt), ("memory", mg, mem), ("query_pos", qg, qpos)] + [(n, t, r) for n, t, r in zip(DEC_NAMES, Pg, P)], DEC_BAR)


# ---------------------------------------------------------------------------------------------
# F. project_gather / PyramidNHWC.shared_grad
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("subset", ["levels", "points"])
def test_project_gather_with_only_levels_or_only_points_trainable(subset, det):
    """the small shape of test_gpu_ops.test_project_gather_vs_grid_sample against grid_sample in fp64.  The sampling grid carries no
    gradient (main/model.py:157 detaches it), so a trainable point set gets none - and must not make shared_grad build its accumulator."""
    from oracle import hoisdf_oracle as R
    O = ops()
    B, P = 2, 300
    pyr = T.synthetic_pyramid(B, big=False, seed=4, nonneg=False)
    inputs, _, meta = T.synthetic_batch(B, P, 8, seed=5)
    pts0 = inputs["hand_sdf_points"] * 2.5
    pyr64 = {k: v.double().requires_grad_(subset == "levels") for k, v in pyr.items()}
    pts64 = pts0.double().requires_grad_(subset == "points")
    cam_ref, grid = R.project_points(pts64, meta["mano_root"].double(), meta["cam_intr"].double(), 3.1)
    feat_ref = R.sample_pyramid(pyr64, grid, list(pyr))
    gy = rnd(B, P, feat_ref.shape[-1], seed=6)
    assert feat_ref.requires_grad == (subset == "levels")
    if feat_ref.requires_grad:
        feat_ref.backward(gy.double())
    assert pts64.grad is None

    levels = [v.to(DEV).permute(0, 2, 3, 1).contiguous().requires_grad_(subset == "levels") for v in pyr.values()]
    pts = pts0.to(DEV).requires_grad_(subset == "points")
    keep = O.deterministic()
    O.set_deterministic(det)
    try:
        base = O.PyramidNHWC(levels)
        shared = base.shared_grad()
        assert (shared is base) == (subset == "points" or det)
        feat, cam = O.project_gather(shared, pts, meta["mano_root"].to(DEV), meta["cam_intr"].to(DEV), 3.1)
        close(feat.view(B, P, -1), feat_ref, 2e-5, "gather fwd")
        close(cam.view(B, P, 3), cam_ref, 1e-6, "cam")
        assert feat.requires_grad                       # (a Function's output does whenever an input does: the backward runs)
        feat.backward(gy.to(DEV).view(B * P, -1))
    finally:
        O.set_deterministic(keep)
    assert pts.grad is None
    for lv, (name, ref) in zip(levels, pyr64.items()):
        if subset == "levels":
            close(lv.grad.permute(0, 3, 1, 2), ref.grad, 5e-5, f"dpyr {name}")
        else:
            assert lv.grad is None, name
