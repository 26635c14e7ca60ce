"""-m gpu: the fp32-emulating linear kernels (csrc/gemm_emu.hip and its kernel units gemm_emu_b3.hip / gemm_emu_h2.hip / gemm_emu_dw.hip; default form "h2": two scaled f16 pieces per operand, three f16
MFMA products, f32 accumulation; form "b3", HOISDF_EMU_FORM=b3: exact three-way bf16 split, six products - this file runs its
linear-layer tests under both, the second in a child process) are held to the bars of the exact-f32 MFMA kernel:
  * against fp64 at the exact kernel's tolerance (2e-6 of the tensor's max on rows spanning 8 decades, ragged shapes, ReLU +
    dropout through the sign bitmap, accumulate-into);
  * element-wise error against fp64, normalised by sum |a||b|, no larger than the exact-f32 kernel's on the same inputs;
  * exactness of the split itself (x0 + x1 + x2 == x bit for bit) on values across the whole f32 exponent range."""
import ctypes as C
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from hoisdf_amd import ops as O
    return O


def pieces():
    """2: the f16x2 form, 3: bf16x3 (process-wide, HOISDF_EMU_FORM)"""
    from hoisdf_amd._lib import lib
    return lib().hoisdf_linear_emu_pieces()


def assert_close(a, b, rel, what=""):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    scale = max(float(b.abs().max()), 1e-30)
    err = float((a - b).abs().max())
    assert err <= rel * scale + 1e-12, f"{what}: max abs err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e})"


@pytest.fixture(autouse=True)
def _emu_on():
    O = ops()
    keep = O.gemm_emu()
    O.set_gemm_emu(True)
    yield
    O.set_gemm_emu(keep)


@pytest.mark.parametrize("M,N,K,act,p", [(4096, 512, 992, True, 0.0), (2500, 223, 292, True, 0.2), (2176, 128, 224, False, 0.0),
                                         (3000, 96, 516, True, 0.0), (2048, 768, 256, False, 0.0), (2049, 60, 256, False, 0.0),
                                         (5000, 1024, 256, True, 0.1), (2304, 3, 256, True, 0.0), (2100, 256, 20, False, 0.0),
                                         # masked grad-input over N >= 768 with a k tail on 208 tiles: emu_h2_kernel<true, true, 4>, the wide tile
                                         (53248, 776, 256, True, 0.1)])
def test_emulated_linear_matches_fp64_at_the_exact_kernels_bar(M, N, K, act, p):
    """forward, grad-input (plain and accumulating) through hoisdf_linear_fwd_emu / _bwd_input_emu, grad-weight through the f32
    kernel, against fp64 at 2e-6 of each tensor's max.  Rows of x and dy span 8 decades, all-zero rows, ragged M (row clamp),
    N not a multiple of 128 (zero rows in the image, guarded stores), K not a multiple of 16 (k tail)."""
    O = ops()
    O.manual_seed(77)
    g = torch.Generator().manual_seed(M + N + K)
    decades = lambda n: torch.pow(10.0, -8.0 * torch.rand(n, 1, generator=g))
    x = (torch.randn(M, K, generator=g) * decades(M)).to(DEV).requires_grad_(True)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV).requires_grad_(True)
    b = (torch.randn(N, generator=g) * 1e-3).to(DEV).requires_grad_(True)
    gy = (torch.randn(M, N, generator=g) * 1e-5 * decades(M)).to(DEV)
    gy[::7] = 0.0
    with torch.no_grad():
        x[5::11] = 0.0
    assert O._emu_ok(M, x, K, K)                                      # these shapes really take the emulated kernels
    y = O.linear(x, W, b, act=act, drop_p=p)
    y.backward(gy)
    dx_acc = torch.full((M, K), 0.25, device=DEV)
    if N % 4 == 0:
        O._lin_bwd_input(gy, None, 0.0, W.detach(), dx_acc, True)
    pre = x.detach().double() @ W.detach().double().t() + b.detach().double()
    if act:
        kept = y.detach() > 0
        pos = pre > 0
        assert (kept & ~pos).sum().item() <= 2                 # a kept element is positive in fp64 too (up to rounding at 0)
        if p > 0:
            frac = (kept & pos).sum().item() / max(pos.sum().item(), 1)
            assert abs(frac - (1 - p)) < 0.01, frac
        else:
            assert (pos & ~kept).sum().item() <= 2
        scale = kept.double() / (1 - p)
    else:
        scale = torch.ones_like(pre)
    assert_close(y, pre * scale, rel=2e-6, what="y")
    dye = gy.double() * scale
    assert_close(x.grad, dye @ W.detach().double(), rel=2e-6, what="dx")
    assert_close(W.grad, dye.t() @ x.detach().double(), rel=2e-6, what="dW")
    assert_close(b.grad, dye.sum(0), rel=2e-6, what="db")
    if N % 4 == 0:
        assert_close(dx_acc, gy.double() @ W.detach().double() + 0.25, rel=2e-6, what="dx accumulate")


@pytest.mark.parametrize("M,N,K,act,p", [(8192, 256, 256, False, 0.0), (16384, 1024, 256, True, 0.1), (9000, 224, 516, True, 0.0),
                                         (8192, 768, 256, False, 0.0), (70000, 256, 1024, True, 0.0), (8200, 64, 992, False, 0.0),
                                         # one or two 256-tiles of output: the 128-wide k-tile form (two workgroups per CU), ragged too
                                         (9000, 224, 256, True, 0.1), (8200, 512, 252, True, 0.0), (65536, 256, 256, False, 0.0),
                                         # K <= 128: the 128-wide k-tile form (two workgroups per CU) is still the one that runs
                                         (8300, 256, 128, True, 0.1), (9000, 320, 96, False, 0.0)])
def test_emulated_grad_weight_matches_fp64(M, N, K, act, p):
    """hoisdf_linear_bwd_weight_emu (in-kernel transposing split of both activation operands, partial tiles + ordered reduce)
    through ops.linear's backward: dW, db against fp64 at the exact kernel's 2e-6; ragged M (row tail inside a slab and a short
    last slice), N / K that are not multiples of 256 (guarded tile edges), ReLU + dropout through the sign bitmap; two runs
    are bit-identical (no atomics)."""
    O = ops()
    O.manual_seed(5)
    g = torch.Generator().manual_seed(M + N + K)
    decades = lambda n: torch.pow(10.0, -6.0 * torch.rand(n, 1, generator=g))
    x = (torch.randn(M, K, generator=g) * decades(M)).to(DEV).requires_grad_(True)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV).requires_grad_(True)
    b = (torch.randn(N, generator=g) * 1e-3).to(DEV).requires_grad_(True)
    gy = (torch.randn(M, N, generator=g) * decades(M)).to(DEV)
    gy[::7] = 0.0
    y = O.linear(x, W, b, act=act, drop_p=p)
    y.backward(gy)
    scale = (y.detach() > 0).double() / (1 - p) if act else torch.ones(M, N, device=DEV, dtype=torch.float64)
    dye = gy.double() * scale
    assert_close(W.grad, dye.t() @ x.detach().double(), rel=2e-6, what="dW")
    assert_close(b.grad, dye.sum(0), rel=2e-6, what="db")
    # determinism + the switch really selects the emulated kernel
    dW1, db1 = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    dW2, db2 = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    O._gemm_bwd_weight(gy, N, None, 0.0, x.detach(), K, dW1, db1, M, N, K)
    O._gemm_bwd_weight(gy, N, None, 0.0, x.detach(), K, dW2, db2, M, N, K)
    assert torch.equal(dW1, dW2) and torch.equal(db1, db2)
    O.set_gemm_emu(False)
    dW3, db3 = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    O._gemm_bwd_weight(gy, N, None, 0.0, x.detach(), K, dW3, db3, M, N, K)
    assert not torch.equal(dW1, dW3)
    assert_close(dW1, dW3, rel=2e-6, what="emulated vs exact-f32 dW")


@pytest.mark.parametrize("M,N,K,masked", [(8192, 256, 256, False), (16384, 1024, 256, True), (9000, 224, 516, True), (70000, 256, 1024, False),
                                          (8200, 64, 992, False), (8200, 512, 252, True), (8300, 256, 128, True)])
def test_f16x2_grad_weight_matches_fp64(M, N, K, masked):
    """hoisdf_linear_bwd_weight_emu_mag (emu_dw2h_kernel: both operands scaled and split into two f16 pieces in the staging registers,
    three products): dW, db against fp64 at the exact kernel's 2e-6 with rows spanning 6 decades, ragged edges, the sign bitmap;
    magnitudes measured by the library or handed over as magnitude words (same results bit for bit); K <= 128 keeps the bf16x3
    tile.  Two runs are bit-identical."""
    if pieces() != 2:
        pytest.skip("f16x2 form only")
    O = ops()
    from hoisdf_amd._lib import lib
    g = torch.Generator().manual_seed(M + N + K)
    decades = lambda n: torch.pow(10.0, -6.0 * torch.rand(n, 1, generator=g))
    x = (torch.randn(M, K, generator=g) * decades(M)).to(DEV)
    gy = (torch.randn(M, N, generator=g) * 1e-4 * decades(M)).to(DEV)
    gy[::7] = 0.0
    bits, p, scale = None, 0.0, torch.ones(M, N, device=DEV, dtype=torch.float64)
    if masked:
        keep = torch.rand(M, N, generator=g) < 0.6
        nw = (N + 31) // 32
        pad = torch.zeros(M, nw * 32, dtype=torch.bool); pad[:, :N] = keep
        words = (pad.view(M, nw, 32).long() << torch.arange(32)).sum(-1)
        bits = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).to(DEV)
        p = 0.2
        scale = keep.to(DEV).double() / (1 - p)
    dye = gy.double() * scale
    outs = []
    assert lib().hoisdf_mag_words(M) == M
    ymag = gy.abs().amax(1).contiguous().view(torch.int32)       # row magnitudes (include/hoisdf.h): one word per row
    xmag = x.abs().amax(1).contiguous().view(torch.int32)
    for kw in (dict(form="h2"), dict(form="h2"), dict(dy_mag=ymag, x_mag=xmag), dict(dy_mag=ymag)):
        dW, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
        O._gemm_bwd_weight(gy, N, bits, p, x, K, dW, db, M, N, K, **kw)
        outs.append((dW, db))
    assert_close(outs[0][0], dye.t() @ x.double(), rel=2e-6, what="dW")
    assert_close(outs[0][1], dye.sum(0), rel=2e-6, what="db")
    for dW, db in outs[1:]:
        assert torch.equal(dW, outs[0][0]) and torch.equal(db, outs[0][1])


@pytest.mark.parametrize("M,N,K,act,p", [(544, 256, 256, False, 0.0), (544, 1024, 256, True, 0.1), (544, 256, 1024, False, 0.0),
                                         (17, 256, 256, True, 0.0), (1, 64, 32, False, 0.0), (100, 60, 20, True, 0.2),
                                         (2047, 224, 292, True, 0.0), (33, 36, 516, False, 0.0), (700, 4, 256, True, 0.0)])
def test_small_row_emulated_linear_matches_fp64_and_the_exact_kernels_masks(M, N, K, act, p):
    """hoisdf_linear_fwd_emu_small / _bwd_input_emu_small / _bwd_weight_emu_small (one wave per 32 x 32 tile; the decoder stack's and
    the heads' row counts) through ops.linear: y, dx (plain and accumulating), dW, db against fp64 at the exact kernel's 2e-6; ragged
    M / N / K (partial tiles, k tails), ReLU + dropout through the sign bitmap; the dropout mask and the sign map are the exact-f32
    kernel's (same hash, same convention) wherever the pre-activation is not at rounding level; two runs are bit-identical."""
    O = ops()
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K)
    decades = lambda n: torch.pow(10.0, -6.0 * torch.rand(n, 1, generator=g))
    x0 = (torch.randn(M, K, generator=g) * decades(M)).to(DEV)
    W0 = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    b0 = (torch.randn(N, generator=g) * 1e-3).to(DEV)
    gy = (torch.randn(M, N, generator=g) * decades(M)).to(DEV)
    gy[::7] = 0.0
    assert O._emu_small_ok(M, x0, K, W0, N, K)
    res = {}
    for mode in ("small", "small", "f32"):
        O.set_gemm_emu(mode == "small")
        O.manual_seed(77)
        x, W, b = x0.clone().requires_grad_(True), W0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
        y = O.linear(x, W, b, act=act, drop_p=p)
        y.backward(gy)
        res.setdefault(mode, []).append((y.detach(), x.grad, W.grad, b.grad))
    O.set_gemm_emu(True)
    (y, dx, dW, db), again, (yf, _, _, _) = res["small"][0], res["small"][1], res["f32"][0]
    for a_, b_ in zip((y, dx, dW, db), again):
        assert torch.equal(a_, b_)
    pre = x0.double() @ W0.double().t() + b0.double()
    if act:
        kept = y > 0
        # the exact-f32 kernel keeps / drops the same elements, up to pre-activations within rounding of zero
        assert ((kept != (yf > 0)) & (pre.abs() > 1e-6 * pre.abs().max())).sum().item() == 0
        scale = kept.double() / (1 - p)
    else:
        scale = torch.ones_like(pre)
    assert_close(y, pre * scale, rel=2e-6, what="y")
    dye = gy.double() * scale
    assert_close(dx, dye @ W0.double(), rel=2e-6, what="dx")
    assert_close(dW, dye.t() @ x0.double(), rel=2e-6, what="dW")
    assert_close(db, dye.sum(0), rel=2e-6, what="db")
    dx_acc = torch.full((M, K), 0.25, device=DEV)
    O._lin_bwd_input(gy, None, 0.0, W0, dx_acc, True)
    assert_close(dx_acc, gy.double() @ W0.double() + 0.25, rel=2e-6, what="dx accumulate")


def test_small_row_and_batch_entries_edge_cases():
    """empty problems are accepted and touch nothing; operands the one-wave-per-tile form cannot take (K or a leading dimension that is
    not a multiple of 4, a misaligned pointer, too many rows) are refused by the entry with HOISDF_ERR_INVALID and routed to the
    exact-f32 kernel by ops.linear; an empty image batch is a no-op."""
    O = ops()
    from hoisdf_amd._lib import lib
    L = lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    x = torch.randn(64, 32, device=DEV); W = torch.randn(16, 32, device=DEV); y = torch.full((64, 16), 7.0, device=DEV)
    assert L.hoisdf_linear_fwd_emu_small(p(x), 32, p(W), 32, None, p(y), 16, 0, 16, 32, 0, 0.0, 0, None, st) == 0
    assert L.hoisdf_linear_bwd_input_emu_small(p(y), 16, None, 0.0, p(W), 32, p(x), 32, 0, 16, 32, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert L.hoisdf_linear_emu_prepare_batch(None, 0, 0, st) == 0
    mx = L.hoisdf_linear_emu_small_max_rows()
    assert L.hoisdf_linear_emu_small_supported(p(x), 32, p(W), 32, 64, 16, 32) == 1
    assert L.hoisdf_linear_emu_small_supported(p(x), 32, p(W), 32, mx + 1, 16, 32) == 0
    assert L.hoisdf_linear_emu_small_supported(p(x), 30, p(W), 32, 64, 16, 32) == 0            # leading dimension
    assert L.hoisdf_linear_emu_small_supported(C.c_void_p(x.data_ptr() + 4), 32, p(W), 32, 63, 16, 32) == 0   # alignment
    assert L.hoisdf_linear_fwd_emu_small(p(x), 32, p(W), 32, None, p(y), 16, mx + 1, 16, 32, 0, 0.0, 0, None, st) < 0
    assert b"linear_fwd_emu_small" in L.hoisdf_last_error()
    # ragged K (not a multiple of 4): ops.linear takes the exact-f32 kernel and stays correct
    x2 = torch.randn(100, 17, device=DEV, requires_grad=True); W2 = torch.randn(12, 17, device=DEV, requires_grad=True)
    assert not O._emu_small_ok(100, x2, 17, W2, 12, 17)
    y2 = O.linear(x2, W2)
    y2.sum().backward()
    assert_close(y2, x2.detach().double() @ W2.detach().double().t(), rel=2e-6, what="ragged K forward")
    assert_close(W2.grad, torch.ones(100, 12, device=DEV).double().t() @ x2.detach().double(), rel=2e-6, what="ragged K dW")


@pytest.mark.parametrize("M,N,K", [(8192, 1024, 256), (4096, 256, 1024), (4096, 512, 992)])
def test_emulated_linear_is_no_less_accurate_than_the_exact_f32_kernel(M, N, K):
    """element-wise |err vs fp64| / sum_k |a_k||b_k| of the emulated kernels next to the exact-f32 MFMA kernels AND the vendor's
    fp32 GEMM (torch.mm -> hipBLASLt, TF32 off) on identical inputs, forward and grad-input: neither the maximum nor the RMS may
    exceed the larger of the two fp32 implementations' by more than 10 % (tools/emu_accuracy.py prints the table: the emulated
    kernels sit at or below the library everywhere; the exact kernel is ahead only where its small-grid split-k sums pairwise)."""
    O = ops()
    g = torch.Generator().manual_seed(9 + K)
    x = torch.randn(M, K, generator=g).to(DEV)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    dy = torch.randn(M, N, generator=g).to(DEV)

    def run(emu):
        O.set_gemm_emu(emu)
        y = torch.empty(M, N, device=DEV)
        dx = torch.empty(M, K, device=DEV)
        O._gemm_fwd(x, K, W, None, y, N, M, N, K, 0, 0.0, 0, None)
        O._gemm_bwd_input(dy, N, None, 0.0, W, dx, K, M, N, K, 0)
        return y, dx
    ye, dxe = run(True)
    yf, dxf = run(False)
    assert not torch.equal(ye, yf)                                    # the switch selected other kernels
    keep_tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yl, dxl = x @ W.t(), dy @ W
    torch.backends.cuda.matmul.allow_tf32 = keep_tf32
    xd, Wd, dyd = x.double(), W.double(), dy.double()
    for name, got_e, got_f, got_l, ref, den in (("fwd", ye, yf, yl, xd @ Wd.t(), xd.abs() @ Wd.abs().t()),
                                                ("dx", dxe, dxf, dxl, dyd @ Wd, dyd.abs() @ Wd.abs())):
        ee = ((got_e.double() - ref).abs() / den)
        ef = ((got_f.double() - ref).abs() / den)
        el = ((got_l.double() - ref).abs() / den)
        rms = lambda e: float((e ** 2).mean().sqrt())
        assert float(ee.max()) <= 1.1 * max(float(ef.max()), float(el.max())) + 1e-9, (name, float(ee.max()), float(ef.max()), float(el.max()))
        assert rms(ee) <= 1.1 * max(rms(ef), rms(el)) + 1e-10, (name, rms(ee), rms(ef), rms(el))
        assert float(ee.max()) < 6e-7, (name, float(ee.max()))       # ~ 5 ulp of the absolute sum at these K


def test_three_way_bf16_split_is_exact_over_the_f32_range():
    """x0 + x1 + x2 == x bit for bit (every normal f32 whose lowest piece stays a normal bf16, i.e. |x| >= 2^-110): checked
    through the kernel itself - an identity weight makes y[m][n] = x[m][n] as x0 + x1 + x2 with nothing else to add."""
    if pieces() != 3:
        pytest.skip("the exact split is the bf16x3 form's (test_the_bf16x3_form_meets_the_same_bars runs this under HOISDF_EMU_FORM=b3)")
    O = ops()
    g = torch.Generator().manual_seed(3)
    M, K = 2048, 256
    mant = torch.rand(M, K, generator=g) + 1.0
    expo = torch.randint(-100, 100, (M, K), generator=g).float()
    sign = torch.where(torch.rand(M, K, generator=g) < 0.5, -1.0, 1.0)
    x = (sign * mant * torch.pow(2.0, expo)).to(DEV)
    eye = torch.eye(K, device=DEV)
    y = torch.empty(M, K, device=DEV)
    O._gemm_fwd(x, K, eye, None, y, K, M, K, K, 0, 0.0, 0, None)
    assert torch.equal(y, x)


def test_f16x2_split_keeps_its_stated_accuracy():
    """the f16x2 form through the kernel itself (identity weight: y = (hi + lo) / s): every element within max(2^-22 |x|,
    2^-38 max |x|) of itself (include/hoisdf.h: two 11-bit pieces; below 2^-16 max |x| the low piece is an f16 subnormal and the
    error turns absolute); the scale follows the largest magnitude wherever it sits in the f32 range."""
    if pieces() != 2:
        pytest.skip("f16x2 form only")
    O = ops()
    g = torch.Generator().manual_seed(5)
    M, K = 2048, 256
    for top in (-60, 0, 17, 90):
        mant = torch.rand(M, K, generator=g) + 1.0
        expo = torch.randint(top - 45, top + 1, (M, K), generator=g).float()
        sign = torch.where(torch.rand(M, K, generator=g) < 0.5, -1.0, 1.0)
        x = (sign * mant * torch.pow(2.0, expo)).to(DEV)
        x[::9] = 0.0
        y = torch.empty(M, K, device=DEV)
        O._gemm_fwd(x, K, torch.eye(K, device=DEV), None, y, K, M, K, K, 0, 0.0, 0, None)
        amax = float(x.abs().max())
        err = (y.double() - x.double()).abs()
        bound = torch.maximum(x.double().abs() * 2.0 ** -22, torch.full_like(err, amax * 2.0 ** -38))
        assert bool((err <= bound).all()), (top, float((err / bound).max()))


def test_f16x2_form_at_the_ends_of_the_f32_range():
    """the operand scale is a power of two clamped so that neither it nor its inverse leaves the normal f32 range (common.h
    mag_scale / mag_inv_scale): an all-zero operand gives exactly bias, an operand whose maximum sits just under FLT_MAX or in
    the last normal binades comes back through an identity weight finite and within the form's bound; forward, grad-input and
    grad-weight alike."""
    if pieces() != 2:
        pytest.skip("f16x2 form only")
    O = ops()
    g = torch.Generator().manual_seed(11)
    M, K = 2048, 256
    eye = torch.eye(K, device=DEV)
    bias = torch.randn(K, generator=g).to(DEV)
    y = torch.empty(M, K, device=DEV)
    O._gemm_fwd(torch.zeros(M, K, device=DEV), K, eye, bias, y, K, M, K, K, 0, 0.0, 0, None)
    assert torch.equal(y, bias.expand(M, K))
    dw = torch.zeros(K, K, device=DEV); db = torch.zeros(K, device=DEV)
    O._gemm_bwd_weight(torch.zeros(M, K, device=DEV), K, None, 0.0, torch.randn(M, K, generator=g).to(DEV), K, dw, db, M, K, K, form="h2")
    assert float(dw.abs().max()) == 0.0 and float(db.abs().max()) == 0.0
    for top in (127, -110, -126):
        x = ((torch.rand(M, K, generator=g) * 2 - 1) * 2.0 ** top).to(DEV)
        x[3, 5] = 1.999 * 2.0 ** top
        O._gemm_fwd(x, K, eye, None, y, K, M, K, K, 0, 0.0, 0, None)
        assert bool(torch.isfinite(y).all())
        amax = float(x.double().abs().max())
        err = (y.double() - x.double()).abs()
        bound = torch.maximum(x.double().abs() * 2.0 ** -22, torch.full_like(err, max(amax * 2.0 ** -38, 2.0 ** -149)))
        if top > -120:                       # (below: the clamped scale leaves fewer than 22 bits, stated in include/hoisdf.h)
            assert bool((err <= bound).all()), (top, float((err / bound).max()))
        else:
            assert float(err.max()) <= amax * 2.0 ** -9, (top, float(err.max()) / amax)
        dx = torch.empty(M, K, device=DEV)
        O._gemm_bwd_input(x, K, None, 0.0, eye, dx, K, M, K, K, False)
        assert bool(torch.isfinite(dx).all()) and float((dx.double() - x.double()).abs().max()) <= amax * 2.0 ** -9


def test_magnitude_words_travel_from_producer_to_consumer():
    """hoisdf_linear_fwd_emu_mag / _bwd_input_emu_mag: the row magnitudes a contraction leaves for its output hold max |y[row][:]| of
    every row, exactly; a consumer given them computes bit-identically to one that measures the operand itself."""
    if pieces() != 2:
        pytest.skip("f16x2 form only")
    O = ops()
    from hoisdf_amd._lib import call, lib
    g = torch.Generator().manual_seed(6)
    M, N, K = 4100, 512, 256
    x = torch.randn(M, K, generator=g).to(DEV)
    W1 = (torch.randn(N, K, generator=g) / 16).to(DEV)
    W2 = (torch.randn(K, N, generator=g) / 16).to(DEV)
    ymag = torch.zeros(M, dtype=torch.int32, device=DEV)          # row magnitudes: one word per row, zero before the producer runs
    zmag = torch.zeros(M, dtype=torch.int32, device=DEV)
    y = torch.empty(M, N, device=DEV); z = torch.empty(M, K, device=DEV); z0 = torch.empty(M, K, device=DEV)
    st = O._st()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    call("hoisdf_linear_fwd_emu_mag", p(x), K, p(O._emu_image(W1, False)), None, p(y), N, M, N, K, 1, 0.0, 0, None, None, p(ymag), st)
    assert torch.equal(ymag.view(torch.float32), y.abs().amax(1))        # every row's own maximum, exactly
    call("hoisdf_linear_fwd_emu_mag", p(y), N, p(O._emu_image(W2, False)), None, p(z), K, M, K, N, 0, 0.0, 0, None, p(ymag), p(zmag), st)
    call("hoisdf_linear_fwd_emu", p(y), N, p(O._emu_image(W2, False)), None, p(z0), K, M, K, N, 0, 0.0, 0, None, st)
    assert torch.equal(z, z0)
    assert torch.equal(zmag.view(torch.float32), z.abs().amax(1))
    assert_close(z, torch.relu(x.double() @ W1.double().t()) @ W2.double().t(), rel=2e-6, what="two chained contractions")
    # grad-input with the words of dy; accumulate = 1 leaves dx_mag alone
    dx = torch.empty(M, K, device=DEV); dx0 = torch.empty(M, K, device=DEV)
    dmag = torch.zeros(M, dtype=torch.int32, device=DEV)
    call("hoisdf_linear_bwd_input_emu_mag", p(y), N, None, 0.0, p(O._emu_image(W1, True)), p(dx), K, M, N, K, 0, p(ymag), p(dmag), st)
    call("hoisdf_linear_bwd_input_emu", p(y), N, None, 0.0, p(O._emu_image(W1, True)), p(dx0), K, M, N, K, 0, st)
    assert torch.equal(dx, dx0) and torch.equal(dmag.view(torch.float32), dx.abs().amax(1))
    dmag.zero_()
    call("hoisdf_linear_bwd_input_emu_mag", p(y), N, None, 0.0, p(O._emu_image(W1, True)), p(dx), K, M, N, K, 1, p(ymag), p(dmag), st)
    assert int(dmag.abs().max()) == 0
    assert_close(dx, 2 * dx0.double(), rel=1e-6, what="accumulate")


@pytest.mark.parametrize("M,N,K", [(4096, 512, 256), (2500, 224, 292), (65536, 256, 1024)])
def test_f16x2_rows_are_scaled_one_by_one(M, N, K):
    """Round 6: the row operand of a forward / grad-input contraction has one power-of-two scale PER ROW (include/hoisdf.h).
    (a) rows whose magnitudes span 60 decades each come back at the form's accuracy relative to THEIR OWN largest output (one scale per
    matrix left every row more than 2^16 below the largest with an absolute error instead); (b) a row's result does not depend on the
    other rows of the matrix: the first 2048 rows are bit-identical next to quiet and next to x 1e6 louder companions - forward,
    masked grad-input and the magnitudes the epilogue leaves."""
    if pieces() != 2:
        pytest.skip("f16x2 form only")
    O = ops()
    g = torch.Generator().manual_seed(M + N)
    mags = torch.pow(10.0, 60.0 * torch.rand(M, 1, generator=g) - 30.0)
    x = (torch.randn(M, K, generator=g) * mags).to(DEV)
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    y = torch.empty(M, N, device=DEV)
    O._gemm_fwd(x, K, W, None, y, N, M, N, K, 0, 0.0, 0, None)
    ref = x.double() @ W.double().t()
    rowmax = ref.abs().amax(1, keepdim=True).clamp_min(1e-300)
    assert float(((y.double() - ref).abs() / rowmax).max()) <= 2e-6
    dx = torch.empty(M, K, device=DEV)
    gy = (torch.randn(M, N, generator=g) * mags).to(DEV)
    O._gemm_bwd_input(gy, N, None, 0.0, W, dx, K, M, N, K, False)
    refd = gy.double() @ W.double()
    assert float(((dx.double() - refd).abs() / refd.abs().amax(1, keepdim=True).clamp_min(1e-300)).max()) <= 2e-6
    # (b) companions
    R = 2048
    x2 = x.clone(); x2[R:] = torch.randn(M - R, K, generator=g).to(DEV) * 1e6
    y2 = torch.empty(M, N, device=DEV)
    O._gemm_fwd(x2, K, W, None, y2, N, M, N, K, 0, 0.0, 0, None)
    assert torch.equal(y2[:R], y[:R]) and not torch.equal(y2[R:], y[R:])
    gy2 = gy.clone(); gy2[R:] = torch.randn(M - R, N, generator=g).to(DEV) * 1e-9
    dx2 = torch.empty(M, K, device=DEV)
    O._gemm_bwd_input(gy2, N, None, 0.0, W, dx2, K, M, N, K, False)
    assert torch.equal(dx2[:R], dx[:R])


def test_attention_f16x2_samples_do_not_see_each_other():
    """one scale per (sample, head) for Q, K, V and dO (round 6; round 5: one per projected matrix): sample 0's attention output, LSE
    and gradients are bit-identical whatever the other samples of the batch hold - here samples 300 x louder."""
    if pieces() != 2:
        pytest.skip("f16x2 form only")
    O = ops()
    B, L, E, H = 4, 1024, 256, 4
    g = torch.Generator().manual_seed(3)
    res = []
    base = torch.randn(B, L, 3 * E, generator=g)
    go0 = torch.randn(B, L, E, generator=g)
    for loud in (1.0, 300.0):
        qkv = base.clone(); qkv[1:] *= loud
        go = go0.clone(); go[1:] *= loud
        qkv, go = qkv.to(DEV), go.to(DEV)
        q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
        hm = O._head_measure(qkv, 3 * E, B * L, 3 * H, L)
        heads = (hm, hm[H * B:], hm[2 * H * B:])
        o, lse = O._attn_fwd_emu(q, k, v, H, L, 0.1, 5, heads=heads)
        dqkv = torch.empty_like(qkv)
        O._attn_bwd_emu(q, k, v, o, lse, go, dqkv[..., :E], dqkv[..., E:2 * E], dqkv[..., 2 * E:], H, L, 0.1, 5, heads=heads)
        res.append((o, lse, dqkv))
    for a_, b_ in zip(*res):
        assert torch.equal(a_[0], b_[0]) and not torch.equal(a_[1], b_[1])


def test_a_stale_row_magnitude_clips_instead_of_overflowing():
    """what a wrong (too small) magnitude does.  The splitting kernels run with f16 saturation on (MODE.FP16_OVFL):
    a word up to 4 x below the row's true maximum is inside the head room of the [2^13, 2^14) target - results unchanged to rounding;
    a word 2^12 below it clips the row's largest elements at 65504 / scale - wrong for that row, but finite (no Inf / NaN reaches the
    next layer) and the OTHER rows are untouched; a correct word next to it keeps its row exact."""
    if pieces() != 2:
        pytest.skip("f16x2 form only")
    O = ops()
    from hoisdf_amd._lib import call
    g = torch.Generator().manual_seed(8)
    M, N, K = 8448, 256, 256
    x = torch.randn(M, K, generator=g).to(DEV)
    W = (torch.randn(N, K, generator=g) / 16).to(DEV)
    img = O._emu_image(W, False)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    good = x.abs().amax(1).contiguous().view(torch.int32)
    def fwd(words):
        y = torch.empty(M, N, device=DEV)
        call("hoisdf_linear_fwd_emu_mag", p(x), K, p(img), None, p(y), N, M, N, K, 0, 0.0, 0, None, p(words), None, O._st())
        return y
    y0 = fwd(good)
    ref = x.double() @ W.double().t()
    assert_close(y0, ref, rel=2e-6, what="correct words")
    stale4 = (x.abs().amax(1) / 4).contiguous().view(torch.int32)
    assert_close(fwd(stale4), ref, rel=2e-6, what="4 x stale: inside the head room")
    bad = good.clone()
    bad[7] = (x[7].abs().max() / 4096).view(torch.int32)               # row 7: 2^12 too small; a zero word for row 9 (an all-zero row's word on data)
    bad[9] = 0
    yb = fwd(bad)
    assert bool(torch.isfinite(yb).all())
    keep = torch.ones(M, dtype=torch.bool, device=DEV); keep[7] = keep[9] = False
    assert torch.equal(yb[keep], y0[keep])
    assert float((yb[7] - y0[7]).abs().max()) > 0                     # (clipped: wrong, finite)
    # the same through the grad-weight (its row slices take the largest word of their rows): finite
    dW, db = torch.zeros(N, K, device=DEV), torch.zeros(N, device=DEV)
    gy = torch.randn(M, N, generator=g).to(DEV)
    O._gemm_bwd_weight(gy, N, None, 0.0, x, K, dW, db, M, N, K, dy_mag=gy.abs().amax(1).contiguous().view(torch.int32), x_mag=bad)
    assert bool(torch.isfinite(dW).all())


def test_the_bf16x3_form_meets_the_same_bars():
    """the linear-layer tests of this file once more with HOISDF_EMU_FORM=b3 (the form is fixed per process: a child runs them)"""
    if os.environ.get("HOISDF_EMU_FORM_CHILD"):
        pytest.skip("already the child")
    env = dict(os.environ, HOISDF_EMU_FORM="b3" if pieces() == 2 else "h2", HOISDF_EMU_FORM_CHILD="1")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-k",
                          "linear or split or image or batch", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-1000:]
    assert " passed" in out.stdout


def test_emulated_image_cache_follows_weight_updates_and_owners():
    """the weight image is rebuilt when the weight changes in place (version counter) and when ANOTHER tensor takes over the
    address; the sign bitmap of the emulated forward equals the exact kernel's wherever |y| is not at rounding level."""
    O = ops()
    g = torch.Generator().manual_seed(4)
    M, N, K = 2048, 256, 256
    x = torch.randn(M, K, generator=g).to(DEV)
    W = (torch.randn(N, K, generator=g) / 16).to(DEV)
    y1 = O.linear(x, W)
    with torch.no_grad():
        W.mul_(2.0)
    y2 = O.linear(x, W)
    assert_close(y2, 2 * y1.double(), rel=1e-6, what="in-place update")
    ptr = W.data_ptr()
    del W
    W2 = (torch.randn(N, K, generator=g) / 16).to(DEV)            # usually lands on the freed block
    y3 = O.linear(x, W2)
    assert_close(y3, x.double() @ W2.double().t(), rel=2e-6, what=f"new owner (same address: {W2.data_ptr() == ptr})")
    bits_e = torch.empty(M, N // 32, device=DEV, dtype=torch.int32)
    bits_f = torch.empty_like(bits_e)
    ye = torch.empty(M, N, device=DEV)
    yf = torch.empty(M, N, device=DEV)
    O._gemm_fwd(x, K, W2, None, ye, N, M, N, K, 1, 0.0, 0, bits_e)
    O.set_gemm_emu(False)
    O._gemm_fwd(x, K, W2, None, yf, N, M, N, K, 1, 0.0, 0, bits_f)
    diff = (bits_e ^ bits_f)
    n_diff = sum(bin(int(v) & 0xffffffff).count("1") for v in diff[diff != 0].cpu().tolist())
    assert n_diff <= 4, n_diff                                        # only elements within rounding of zero may differ


def test_batched_image_refresh_equals_the_single_builds():
    """ops.bump_weight_generation() (what FusedAdamW calls after its HIP update) rebuilds every cached image in one
    hoisdf_linear_emu_prepare_batch launch: images bit-identical to hoisdf_linear_emu_prepare's, both orientations, ragged
    shapes and a row slice of a weight (the attention in-projection's q / kv parts); a weight that died is skipped."""
    O = ops()
    from hoisdf_amd._lib import call, lib
    g = torch.Generator().manual_seed(7)
    shapes = [(256, 256), (1024, 256), (256, 1024), (768, 256), (60, 256), (200, 60), (512, 292), (3, 1000)]
    Ws = [(torch.randn(n, k, generator=g) / 8).to(DEV) for n, k in shapes]
    x = torch.randn(2048, 256, generator=g).to(DEV)
    imgs = []
    for W in Ws:
        for tr in (False, True):
            imgs.append((W, tr, O._emu_image(W, tr)))
    sl = Ws[3][256:]                                             # a view: rows 256 .. 767
    imgs.append((sl, False, O._emu_image(sl, False)))
    dead = (torch.randn(128, 64, generator=g)).to(DEV)
    O._emu_image(dead, False)
    del dead
    with torch.no_grad():
        for W in Ws:
            W.mul_(1.5).add_(0.01)                                # (also bumps torch's version counters)
    O.bump_weight_generation()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for W, tr, img in imgs:
        N, K = W.shape
        ref = torch.empty_like(img)
        call("hoisdf_linear_emu_prepare", p(W), W.stride(0), N, K, int(tr), p(ref), st)
        assert torch.equal(img, ref), (tuple(W.shape), tr)
        assert O._emu_image(W, tr) is img                        # and the entry is current: no rebuild at the next use
    n_before = len(O._EMU_CACHE)
    y = O.linear(x, Ws[0])
    assert_close(y, x.double() @ Ws[0].double().t(), rel=2e-6, what="linear after the batched refresh")
    assert len(O._EMU_CACHE) == n_before


def test_purge_keeps_live_images_and_drops_dead_ones():
    """WeightImageCache.purge(): the entries of weights that died leave the cache, their images parked in the graveyard for one more
    cycle (a kernel on another stream may still read them); the entries of live weights stay as they are - same image tensor, no
    rebuild - and still serve the emulated linear layer."""
    O = ops()
    cache = O._EMU_CACHE
    g = torch.Generator().manual_seed(11)
    cache.purge()                                                 # (what earlier tests left behind is not counted below)
    live = [(torch.randn(n, k, generator=g) / 8).to(DEV) for n, k in ((64, 64), (60, 256), (256, 64))]
    imgs = [(W, tr, O._emu_image(W, tr)) for W in live for tr in (False, True)]
    temps = [torch.randn(4 * i + 8, 64, generator=g).to(DEV) for i in range(8)]       # eight shapes: eight keys
    dead = [O._emu_image(t, False) for t in temps]
    n_before = len(cache)
    del temps
    cache.purge()
    assert len(cache) == n_before - len(dead)
    for W, tr, img in imgs:
        assert O._emu_image(W, tr) is img, (tuple(W.shape), tr)
    assert len(cache.graveyard) == len(dead) and all(a is b for a, b in zip(cache.graveyard, dead))
    cache.purge()
    assert cache.graveyard == [] and len(cache) == n_before - len(dead)
    for W in live:
        x = torch.randn(2048, W.shape[1], generator=g).to(DEV)
        assert O._emu_ok(2048, x, W.shape[1], W.shape[1])
        assert_close(O.linear(x, W), x.double() @ W.double().t(), rel=2e-6, what=f"linear after the purge {tuple(W.shape)}")


def test_image_built_on_one_stream_is_safe_to_read_on_another():
    """an image built late on a side stream is read on the current stream without any synchronisation by the caller (the cache's
    build event), and rebuilt on the side stream after the current one read it and then changed the weight (the reader waits)."""
    O = ops()
    g = torch.Generator().manual_seed(12)
    M, N, K = 2048, 64, 64
    x = torch.randn(M, K, generator=g).to(DEV)
    W = (torch.randn(N, K, generator=g) / 8).to(DEV)
    ref = x.double() @ W.double().t()
    a = torch.randn(4096, 4096, generator=g).to(DEV)
    assert O._emu_ok(M, x, K, K)
    cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(cur)                                         # the inputs were made on the current stream
    with torch.cuda.stream(side):
        b = a
        for _ in range(6):
            b = torch.matmul(b, a)                                # a few milliseconds ahead of the build: it finishes late
        y_side = O.linear(x, W)
    y = O.linear(x, W)                                            # no wait for the side stream here: the cache has to
    assert_close(y, ref, rel=2e-6, what="read on the current stream")
    W.mul_(2)
    side.wait_stream(cur)                                         # as real callers do: the new weight values
    with torch.cuda.stream(side):
        y2 = O.linear(x, W)
    cur.wait_stream(side)
    assert_close(y_side, ref, rel=2e-6, what="built on the side stream")
    assert_close(y2, 2 * ref, rel=2e-6, what="rebuilt on the side stream")
    assert_close(y2, 2 * y.double(), rel=2e-6, what="twice the first")


def _ref_attn64(q, k, v, H, kv=None):
    B, Lq, E = q.shape
    qh, kh, vh = (t.view(t.shape[0], t.shape[1], H, 64).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-1, -2)) / 8.0
    if kv is not None:
        s[..., kv:] = -float("inf")
    return (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, Lq, E)


@pytest.mark.parametrize("B,Lq,Lk,kv", [(2, 2048, 2048, 2048), (2, 300, 300, 230), (1, 1536, 2048, 1536), (3, 33, 700, 700),
                                        (1, 512, 2048, 2048)])
def test_emulated_attention_is_as_accurate_as_the_exact_f32_kernels(B, Lq, Lk, kv):
    """csrc/attention_emu.hip (bf16x3 forward + fused one-pass backward) against float64 softmax attention, next to the exact-f32
    MFMA kernels on the same inputs: output, dq, dk, dv within the f32 kernels' own bars (2e-5 / 5e-5 of the tensor's max) and
    no further from fp64 than 1.5 x the exact kernels' distance; masked keys get exactly zero gradients; two backward runs are
    bit-identical (no atomics)."""
    O = ops()
    E, H = 256, 4
    g = torch.Generator().manual_seed(Lq + Lk)
    q = torch.randn(B, Lq, E, generator=g)
    kvt = torch.randn(B, Lk, 2 * E, generator=g)
    go = torch.randn(B, Lq, E, generator=g)
    q64, kv64 = q.double().requires_grad_(True), kvt.double().requires_grad_(True)
    ref = _ref_attn64(q64, kv64[..., :E], kv64[..., E:], H, kv)
    ref.backward(go.double())

    import hoisdf_amd.ops as OO
    keep_bwd = OO._ATTN_BWD_EMU
    OO._ATTN_BWD_EMU = True                                         # the fused emulated backward (default: forward only)

    def run(emu):
        O.set_attention_emu(emu)
        qg, kg = q.to(DEV).requires_grad_(True), kvt.to(DEV).requires_grad_(True)
        o = O.attention_cross(qg, kg, H, kv)
        o.backward(go.to(DEV))
        return o.detach(), qg.grad, kg.grad
    keep = O.attention_emu()
    try:
        oe, dqe, dkve = run(True)
        oe2, dqe2, dkve2 = run(True)
        of, dqf, dkvf = run(False)
    finally:
        O.set_attention_emu(keep)
        OO._ATTN_BWD_EMU = keep_bwd
    assert not torch.equal(oe, of)                                  # the switch selected other kernels
    assert torch.equal(oe, oe2) and torch.equal(dqe, dqe2) and torch.equal(dkve, dkve2)      # deterministic
    for name, ge, gf, r, rel in (("out", oe, of, ref, 2e-5), ("dq", dqe, dqf, q64.grad, 5e-5), ("dkv", dkve, dkvf, kv64.grad, 5e-5)):
        assert_close(ge, r, rel=rel, what="emulated " + name)
        mx = float(r.abs().max())
        ee = float((ge.double().cpu() - r).abs().max()) / mx
        ef = float((gf.double().cpu() - r).abs().max()) / mx
        assert ee <= 1.5 * ef + 2e-7, (name, ee, ef)
    if kv < Lk:
        assert float(dkve[:, kv:].abs().max()) == 0.0


@pytest.mark.parametrize("B,Lq,Lk,kv,amp", [(2, 2048, 2048, 2048, 1.0), (2, 300, 300, 230, 1.0), (1, 1536, 2048, 1536, 4.0), (3, 33, 700, 700, 1e-3),
                                            (1, 512, 2048, 2048, 1.0), (1, 128, 256, 256, 1e-24)])
def test_f16x2_attention_forward_is_as_accurate_as_the_bf16x3_one(B, Lq, Lk, kv, amp):
    """hoisdf_attention_fwd_emu_mag (emu_attn_fwd2_kernel<DROP, 2, true>: Q, K, V as scaled hi + lo f16 planes, three f16 MFMA products,
    P carried as 2^6 P) against float64 softmax attention: output within the bf16x3 kernel's bar (2e-5 of max) and no further from fp64
    than 1.5 x the bf16x3 kernel's distance; the LSE (log2 domain) agrees with the bf16x3 kernel's; operands of very different overall
    magnitude (amp: peaked - scores up to ~250 in the log2 domain - and flat softmaxes) ride on the scale from the magnitude words; with
    dropout the mask is the same function.  (The 22-bit operand pieces put ~2^-22 |score| of absolute error on a score: at amp = 30,
    scores of ~2000, the output is 5e-5 of its maximum off - include/hoisdf.h says so; trained attention stays below ~100.)"""
    O = ops()
    from hoisdf_amd._lib import call, lib
    E, H = 256, 4
    g = torch.Generator().manual_seed(Lq + Lk)
    q = (torch.randn(B, Lq, E, generator=g) * amp).to(DEV)
    kvm = (torch.randn(B, Lk, 2 * E, generator=g) * amp).to(DEV)
    kvm[..., :E] *= 0.5
    k, v = kvm[..., :E], kvm[..., E:]
    ref = _ref_attn64(q.double().cpu().contiguous(), k.double().cpu().contiguous(), v.double().cpu().contiguous(), H, kv)
    # head magnitudes (include/hoisdf.h): one scale per (sample, head) and operand - measured for q and for the [k | v] matrix
    hq = O._head_measure(q, E, B * Lq, H, Lq)
    hkv = O._head_measure(kvm, 2 * E, B * Lk, 2 * H, Lk)
    assert torch.equal(hq.view(torch.float32).view(H, B), q.abs().view(B, Lq, H, 64).amax((1, 3)).t())
    heads = (hq, hkv, hkv[H * B:])
    ob, lb = O._attn_fwd_emu(q, k, v, H, kv, 0.0, 0)
    oh, lh = O._attn_fwd_emu(q, k, v, H, kv, 0.0, 0, heads=heads)
    oh2, _ = O._attn_fwd_emu(q, k, v, H, kv, 0.0, 0, heads=heads)
    assert torch.equal(oh, oh2) and not torch.equal(oh, ob)
    assert_close(oh, ref, rel=2e-5, what="f16x2 out")
    mx = float(ref.abs().max())
    eh = float((oh.double().cpu() - ref).abs().max()) / mx
    eb = float((ob.double().cpu() - ref).abs().max()) / mx
    assert eh <= 1.5 * eb + 2e-7, (eh, eb)
    assert float((lh - lb).abs().max()) <= 2e-5 * max(1.0, float(lb.abs().max()))
    # dropout: the same keep decisions as the bf16x3 kernel (same seed): outputs agree to rounding
    od, _ = O._attn_fwd_emu(q, k, v, H, kv, 0.1, 4321)
    oe, _ = O._attn_fwd_emu(q, k, v, H, kv, 0.1, 4321, heads=heads)
    assert_close(oe, od.double(), rel=2e-5, what="f16x2 out with dropout")


@pytest.mark.parametrize("B,Lq,Lk,kv,p,gamp", [(2, 2048, 2048, 2048, 0.0, 1e-3), (2, 300, 300, 230, 0.0, 1e-3), (1, 1536, 2048, 1536, 0.1, 1e-3),
                                               (3, 33, 700, 700, 0.0, 1e-3), (1, 512, 2048, 2048, 0.1, 1e-3),
                                               (2, 300, 300, 230, 0.0, 1e-30), (2, 300, 300, 230, 0.0, 1e20)])
def test_f16x2_attention_backward_is_as_accurate_as_the_bf16x3_one(B, Lq, Lk, kv, p, gamp):
    """hoisdf_attention_bwd_emu_mag (emu_attn_bwd4h_kernel: two f16 pieces for Q, K, V, dO, P, three for dS; 76 MFMAs per query tile)
    against float64 autograd of softmax attention: dq, dk, dv within the bf16x3 kernel's bar (5e-5 of max) and no further from fp64 than
    3 x the bf16x3 kernel's distance; masked keys get exactly zero; two runs bit-identical; with dropout the same mask as the bf16x3
    kernel (gradients agree to rounding)."""
    if pieces() != 2:
        pytest.skip("the Python helpers measure magnitudes only in f16x2 processes")
    O = ops()
    from hoisdf_amd._lib import call, lib
    E, H = 256, 4
    g = torch.Generator().manual_seed(Lq + Lk + 1)
    q = torch.randn(B, Lq, E, generator=g).to(DEV)
    kvm = torch.randn(B, Lk, 2 * E, generator=g).to(DEV)
    go = (torch.randn(B, Lq, E, generator=g) * gamp).to(DEV)          # (gamp: output gradients at both ends of the f32 range too)
    k, v = kvm[..., :E], kvm[..., E:]
    hq = O._head_measure(q, E, B * Lq, H, Lq)
    hkv = O._head_measure(kvm, 2 * E, B * Lk, 2 * H, Lk)
    heads = (hq, hkv, hkv[H * B:])

    def run(h2, seed=99):
        if h2:
            o, lse = O._attn_fwd_emu(q, k, v, H, kv, p, seed, heads=heads)
        else:
            o, lse = O._attn_fwd_emu(q, k, v, H, kv, p, seed)
        dq = torch.empty_like(q); dkv = torch.empty_like(kvm)
        O._attn_bwd_emu(q, k, v, o, lse, go, dq, dkv[..., :E], dkv[..., E:], H, kv, p, seed, **(dict(heads=heads) if h2 else {}))
        return dq, dkv
    dqh, dkvh = run(True)
    dqh2, dkvh2 = run(True)
    dqb, dkvb = run(False)
    assert torch.equal(dqh, dqh2) and torch.equal(dkvh, dkvh2) and not torch.equal(dqh, dqb)
    if kv < Lk:
        assert float(dkvh[:, kv:].abs().max()) == 0.0
    if p == 0.0:
        q64, kv64 = q.double().cpu().requires_grad_(True), kvm.double().cpu().requires_grad_(True)
        ref = _ref_attn64(q64, kv64[..., :E].contiguous(), kv64[..., E:].contiguous(), H, kv)
        ref.backward(go.double().cpu())
        for name, gh, gb, r in (("dq", dqh, dqb, q64.grad), ("dkv", dkvh, dkvb, kv64.grad)):
            assert_close(gh, r, rel=5e-5, what="f16x2 " + name)
            mx = float(r.abs().max())
            eh = float((gh.double().cpu() - r).abs().max()) / mx
            eb = float((gb.double().cpu() - r).abs().max()) / mx
            # (22-bit operand pieces against exact ones: 2.1e-6 vs 0.74e-6 of max on dq at 2048 x 2048; the factor was 2.5 while the bf16x3
            # backward summed its scores in another order than its forward and sat at 0.76e-6)
            assert eh <= 3.0 * eb + 2e-7, (name, eh, eb)
    else:
        assert_close(dqh, dqb.double(), rel=5e-5, what="dq with dropout")
        assert_close(dkvh, dkvb.double(), rel=5e-5, what="dkv with dropout")


@pytest.mark.parametrize("B,Lq,Lk,kv,p", [(2, 300, 300, 230, 0.0), (1, 33, 160, 96, 0.1)])
def test_bf16x3_backward_over_kept_planes_equals_converting_for_itself(B, Lq, Lk, kv, p):
    """the two ways hoisdf_attention_bwd_emu finds its Q, K, V planes: in the workspace a forward with keep = 1 left (layout
    Q rows | K rows | V rows | V^T, carved once in attention_emu.hip) or converted by itself (Q rows | K rows | V rows behind its dO
    planes and dQ partials).  The same conversion kernel writes the same row planes both times, so dq and dkv are bit-equal; the kept
    entry is consumed.  Shapes: ragged query and key tiles with masked keys; one full + one one-row query tile, a key block past
    kv_len, dropout."""
    O = ops()
    import hoisdf_amd.ops as OO
    E, H, seed = 256, 4, 1234
    g = torch.Generator().manual_seed(Lq + Lk + 2)
    q = torch.randn(B, Lq, E, generator=g).to(DEV)
    kvm = torch.randn(B, Lk, 2 * E, generator=g).to(DEV)
    go = torch.randn(B, Lq, E, generator=g).to(DEV)
    k, v = kvm[..., :E], kvm[..., E:]
    key = OO._planes_key(q, k, v, H, kv)

    def run(keep):
        o, lse = O._attn_fwd_emu(q, k, v, H, kv, p, seed, keep=keep)
        assert (key in OO._EMU_PLANES) == keep
        dq = torch.empty_like(q); dkv = torch.empty_like(kvm)
        O._attn_bwd_emu(q, k, v, o, lse, go, dq, dkv[..., :E], dkv[..., E:], H, kv, p, seed)
        assert key not in OO._EMU_PLANES                            # consumed
        return o, dq, dkv
    OO._EMU_PLANES.pop(key, None)
    ok, dqk, dkvk = run(True)
    oc, dqc, dkvc = run(False)
    assert torch.equal(ok, oc)
    assert torch.equal(dqk, dqc) and torch.equal(dkvk, dkvc)
    assert float(dqk.abs().max()) > 0.0 and float(dkvk[:, :kv].abs().max()) > 0.0 and float(dkvk[:, kv:].abs().max()) == 0.0


def test_emulated_attention_dropout_mask_is_the_f32_kernels_mask():
    """same (seed, query, key) hash as attention.hip: with dropout on, the emulated forward / backward agree with the exact-f32
    kernels to rounding (the SAME elements are dropped), and the backward is the adjoint of the forward in V (same mask)."""
    O = ops()
    import hoisdf_amd.ops as OO
    B, L, E, H, p = 2, 256, 256, 4, 0.2
    g = torch.Generator().manual_seed(8)
    qkv = torch.randn(B, L, 3 * E, generator=g).to(DEV)
    go = torch.randn(B, L, E, generator=g).to(DEV)
    seed = 424242
    keep = O.attention_emu()
    keep_bwd = OO._ATTN_BWD_EMU
    OO._ATTN_BWD_EMU = True
    res = []
    try:
        for emu in (True, False):
            O.set_attention_emu(emu)
            x = qkv.clone().requires_grad_(True)
            o = OO._AttentionSelf.apply(x, H, L, p, seed)
            o.backward(go)
            res.append((o.detach(), x.grad))
    finally:
        O.set_attention_emu(keep)
        OO._ATTN_BWD_EMU = keep_bwd
    assert_close(res[0][0], res[1][0], rel=2e-5, what="dropout out")
    assert_close(res[0][1], res[1][1], rel=5e-5, what="dropout dqkv")
