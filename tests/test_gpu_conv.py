"""-m gpu: the NHWC implicit-GEMM convolution forward (include/hoisdf.h hoisdf_conv2d_fwd / hoisdf_conv_transpose2d_fwd /
hoisdf_maxpool2d_fwd / hoisdf_conv_pack_weight, csrc/conv.hip) against torch.nn.functional in float64 on the CPU.

Bar: max |y - truth| <= max(2e-6 max |truth|, 2 x the distance of torch's own float32 CPU call from the same truth).  2e-6 of the
tensor's maximum is the project's bar for the exact-f32 contraction (tests/test_gpu_emu.py); the second term covers contractions of
several thousand terms, where plain f32 accumulation itself sits above 2e-6 - it is measured here against torch, never against the
code under test.  Shapes are the smallest at which each index path can go wrong; inputs randn, weights scaled by 1 / sqrt(K)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def held(y_nhwc, truth, f32, label):
    """y (NHWC, GPU) against truth (NCHW, f64, CPU); f32 = torch's float32 CPU result of the same call"""
    got = y_nhwc.detach().cpu().permute(0, 3, 1, 2).double()
    assert got.shape == truth.shape, (got.shape, truth.shape)
    err = float((got - truth).abs().max())
    own = float((f32.double() - truth).abs().max())
    bar = max(2e-6 * float(truth.abs().max()), 2 * own)
    print(f"{label}: max |y - truth| {err:.3e}  torch f32 {own:.3e}  max |truth| {float(truth.abs().max()):.3e}  bar {bar:.3e}")
    assert torch.isfinite(got).all()
    assert err <= bar, (label, err, bar)


def problem(seed, B, Ci, H, W, Co, k, transposed=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=g)
    K = (4 if transposed else k * k) * Ci
    w = torch.randn(*((Ci, Co, k, k) if transposed else (Co, Ci, k, k)), generator=g) / K ** 0.5
    b = torch.randn(Co, generator=g)
    return x, w, b


CONV = [  # label, B, C_in, H, W, C_out, k, stride, pad
    ("stem 7x7 s2 p3, K = 147", 2, 3, 18, 14, 64, 7, 2, 3),
    ("3x3 s1 p1 on odd sides", 2, 64, 9, 7, 64, 3, 1, 1),
    ("3x3 s2 p1, M = 40", 2, 128, 9, 7, 128, 3, 2, 1),
    ("1x1 s2 downsample", 2, 256, 6, 4, 512, 1, 2, 0),
    ("1x1 2048 -> 512, M = 6", 1, 2048, 2, 3, 512, 1, 1, 0),
    ("3x3 512 -> 512, K = 4608, M = 4", 1, 512, 2, 2, 512, 3, 1, 1),
    ("1x1 32 -> 32 aux hidden", 2, 32, 8, 8, 32, 1, 1, 0),
    ("3x3 s1 p1, two 128-row tiles x two column tiles", 2, 16, 96, 96, 192, 3, 1, 1),
]


@pytest.mark.parametrize("case", CONV, ids=[c[0] for c in CONV])
def test_conv2d_matches_float64(case):
    from hoisdf_amd import ops
    label, B, Ci, H, W, Co, k, s, p = case
    x, w, b = problem(1, B, Ci, H, W, Co, k)
    truth = F.conv2d(x.double(), w.double(), b.double(), s, p)
    f32 = F.conv2d(x, w, b, s, p)
    y = ops.conv2d_nhwc(nhwc(x), ops.ConvWeight(w.to(DEV), b.to(DEV)), s, p)
    held(y, truth, f32, label)


def test_the_big_tile_is_what_the_large_case_takes():
    from hoisdf_amd import ops
    assert ops.conv_plan(2 * 96 * 96, 192, 9 * 16) == (128, 1)
    assert ops.conv_plan(40, 128, 9 * 128)[0] == 64


def test_few_rows_cut_the_contraction_and_stay_bit_reproducible():
    """1x1 2048 -> 512 on 1 x 2 x 3: six output rows, so K is cut over workgroups (partial tiles + an ordered reduce)"""
    from hoisdf_amd import ops
    tile, splitk = ops.conv_plan(6, 512, 2048)
    assert splitk > 1, (tile, splitk)
    assert ops.conv_plan(4, 512, 4608)[1] > 1 and ops.conv_plan(4, 256, 8192, 4)[1] > 1
    x, w, b = problem(2, 1, 2048, 2, 3, 512, 1)
    cw, xg = ops.ConvWeight(w.to(DEV), b.to(DEV)), nhwc(x)
    a = ops.conv2d_nhwc(xg, cw)
    c = ops.conv2d_nhwc(xg, cw)
    torch.cuda.synchronize()
    assert torch.equal(a, c)
    held(a, F.conv2d(x.double(), w.double(), b.double()), F.conv2d(x, w, b), "split-K 1x1")


@pytest.mark.parametrize("case", [("4/2/1 256 -> 128", 2, 256, 3, 2, 128), ("4/2/1 2048 -> 256, K = 8192", 1, 2048, 2, 2, 256),
                                  ("4/2/1 16 -> 64, unsplit", 2, 16, 40, 24, 64)], ids=lambda c: c[0])
def test_conv_transpose2d_matches_float64(case):
    from hoisdf_amd import ops
    label, B, Ci, H, W, Co = case
    x, w, _ = problem(3, B, Ci, H, W, Co, 4, transposed=True)
    truth = F.conv_transpose2d(x.double(), w.double(), None, 2, 1)
    f32 = F.conv_transpose2d(x, w, None, 2, 1)
    cw = ops.ConvWeight(w.to(DEV), transposed=True)
    y = ops.conv2d_nhwc(nhwc(x), cw)
    assert tuple(y.shape) == (B, 2 * H, 2 * W, Co)
    held(y, truth, f32, label)
    assert torch.equal(y, ops.conv2d_nhwc(nhwc(x), cw))


@pytest.mark.parametrize("Co,act", [(1, "sigmoid"), (1, None), (32, "sigmoid")])
def test_aux_head_widths(Co, act):
    from hoisdf_amd import ops
    x, w, b = problem(4, 2, 32, 8, 8, Co, 1)
    fn = (lambda t: t.sigmoid()) if act else (lambda t: t)
    truth, f32 = fn(F.conv2d(x.double(), w.double(), b.double())), fn(F.conv2d(x, w, b))
    # written as channel 1 of a three-channel map, as the heads write the auxiliary output
    wide = torch.full((2, 8, 8, Co + 2), 7.0, device=DEV)
    ops.conv2d_nhwc(nhwc(x), ops.ConvWeight(w.to(DEV), b.to(DEV)), act=act, out=wide[..., 1:1 + Co])
    held(wide[..., 1:1 + Co], truth, f32, f"C_out = {Co} {act}")
    assert bool((wide[..., 0] == 7.0).all()) and bool((wide[..., 1 + Co:] == 7.0).all())


@pytest.mark.parametrize("c0", [8, 3], ids=["aligned slice", "unaligned slice"])
def test_epilogue_and_channel_slices(c0):
    """bias + residual + ReLU against the composition; the input read as a channel slice (ldx > C_in), the output written as a slice
    (ldy > C_out, c_off > 0) of a sentinel-filled map whose other channels and the guard row behind it stay untouched"""
    from hoisdf_amd import ops
    B, Ci, H, W, Co = 2, 64, 9, 7, 64
    x, w, b = problem(5, B, Ci, H, W, Co, 3)
    res = torch.randn(B, Co, H, W, generator=torch.Generator().manual_seed(6))
    truth = F.relu(F.conv2d(x.double(), w.double(), b.double(), 1, 1) + res.double())
    f32 = F.relu(F.conv2d(x, w, b, 1, 1) + res)
    x_wide = torch.randn(B, H, W, Ci + 16, device=DEV)
    x_wide[..., c0:c0 + Ci] = nhwc(x)
    res_wide = torch.randn(B, H, W, Co + 5, device=DEV)
    res_wide[..., 5:] = nhwc(res)
    ldy, off, sentinel = Co + 32, 16 + (c0 & 3), -12345.0
    flat = torch.full((B * H * W * ldy + ldy,), sentinel, device=DEV)
    ymap = flat[:B * H * W * ldy].view(B, H, W, ldy)
    # (the destination once as the whole map + c_off, once as a slice view: the same addresses either way)
    dst = dict(out=ymap, c_off=off) if c0 == 8 else dict(out=ymap[..., off:off + Co])
    ops.conv2d_nhwc(x_wide[..., c0:c0 + Ci], ops.ConvWeight(w.to(DEV), b.to(DEV)), 1, 1, "relu", residual=res_wide[..., 5:], **dst)
    torch.cuda.synchronize()
    held(ymap[..., off:off + Co], truth, f32, f"bias + residual + ReLU, slices at {c0}")
    assert bool((ymap[..., :off] == sentinel).all()) and bool((ymap[..., off + Co:] == sentinel).all()), "a neighbouring channel was written"
    assert bool((flat[B * H * W * ldy:] == sentinel).all()), "the guard row behind the map was written"


def test_maxpool_keeps_a_negative_maximum():
    from hoisdf_amd import ops
    g = torch.Generator().manual_seed(7)
    x = -torch.rand(2, 64, 9, 7, generator=g) - 0.5                      # negative only: a zero from the padding must not win
    want = F.max_pool2d(x.double(), 3, 2, 1)
    y = ops.maxpool2d_nhwc(nhwc(x))
    assert tuple(y.shape) == (2, 5, 4, 64)
    assert torch.equal(y.cpu().permute(0, 3, 1, 2).double(), want)
    assert float(y.max()) < 0


@pytest.mark.parametrize("transposed", [False, True], ids=["conv", "deconv"])
def test_batchnorm_fold(transposed):
    """conv (with a bias) + evaluation-mode BatchNorm2d with a non-default eps, folded by hoisdf_conv_pack_weight, against the unfused
    float64 composition"""
    from hoisdf_amd import ops
    B, Ci, H, W, Co, eps = 2, 48, 7, 5, 40, 3e-3
    x, w, b = problem(8, B, Ci, H, W, Co, 4 if transposed else 3, transposed)
    g = torch.Generator().manual_seed(9)
    gamma, beta = torch.rand(Co, generator=g) + 0.5, 0.1 * torch.randn(Co, generator=g)
    mean, var = 0.5 * torch.randn(Co, generator=g), 1.5 * torch.rand(Co, generator=g) + 0.5
    if transposed:
        b = None
        conv = lambda t, ww, bb: F.conv_transpose2d(t, ww, bb, 2, 1)
    else:
        conv = lambda t, ww, bb: F.conv2d(t, ww, bb, 1, 1)
    d = lambda t: None if t is None else t.double()
    truth = F.relu(F.batch_norm(conv(x.double(), w.double(), d(b)), mean.double(), var.double(), gamma.double(), beta.double(), False, 0.0, eps))
    f32 = F.relu(F.batch_norm(conv(x, w, b), mean, var, gamma, beta, False, 0.0, eps))
    to = lambda t: None if t is None else t.to(DEV)
    cw = ops.ConvWeight(to(w), to(b), bn=(to(gamma), to(beta), to(mean), to(var), eps), transposed=transposed)
    y = ops.conv2d_nhwc(nhwc(x), cw, 1, 0 if transposed else 1, "relu")
    held(y, truth, f32, f"fold {'deconv' if transposed else 'conv'}")
