"""-m gpu: the per-(sample, head) scales of the f16x2 attention operands at sample lengths that are NOT multiples of the GEMM's 128-row
wave sub-tile (the reference's default 600 + 200 points: S = 800, n_query = 600).  include/hoisdf.h promises one scale per
(sample, head) - "sample 0 of a batch is bit-identical whatever the other samples are" - which needs head magnitudes that hold each
sample's own maximum and nothing of its neighbour's.
  (a) hoisdf_head_mag_measure against torch on the matrix, word for word;
  (b) hoisdf_linear_fwd_emu_heads / hoisdf_linear_bwd_input_emu_heads: the words they leave are those of the STORED output, exactly
      (samples that share a sub-tile; a last sub-tile with rows past M, which hold the bias);
  (c) the encoder layer (C entry and op chain): sample 0's outputs and input gradient do not change with its batch companions;
  (d) the encoder layer next to x 300 louder companions against a float64 restatement, at the bar of tests/test_gpu_conv.py.
A word is the IEEE bit pattern of a maximum of stored floats: torch computes it exactly, so (a) - (c) compare with torch.equal."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GARBAGE, SENTINEL = 0x7F7FFFFF, 0x5A5A5A5A          # (the largest finite float: an atomic max over a word left uncleared keeps it)


def ops():
    from hoisdf_amd import ops as O
    return O


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(autouse=True)
def _emu_on():
    O = ops()
    keep = O.gemm_emu()
    O.set_gemm_emu(True)
    yield
    O.set_gemm_emu(keep)


def torch_words(y, L, groups):
    """the truth: word[group * nb + sample] = bits of max |y[sample's rows][group's 64 columns]|, nb = ceil(M / L) (a short last sample
    is padded with zero rows: they change no maximum of magnitudes)"""
    M = y.shape[0]
    nb = (M + L - 1) // L
    yp = torch.zeros(nb * L, groups * 64, dtype=torch.float32, device=y.device)
    yp[:M] = y[:, :groups * 64]
    return yp.view(nb, L, groups, 64).abs().amax((1, 3)).t().contiguous().view(torch.int32).reshape(-1)


def measured_words(y, ld, M, groups, L):
    """hoisdf_head_mag_measure into an array pre-filled with garbage, a sentinel behind it"""
    from hoisdf_amd._lib import call, lib
    O = ops()
    n = lib().hoisdf_head_mag_words(M, groups, L)
    assert n == groups * ((M + L - 1) // L)
    words = torch.full((n + 1,), GARBAGE, dtype=torch.int32, device=DEV)
    words[n] = SENTINEL
    call("hoisdf_head_mag_measure", ptr(y), ld, M, groups, L, ptr(words), O._st())
    assert int(words[n]) == SENTINEL, "head_mag_measure wrote behind its words"
    return words[:n]


# ---- (a) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,L,groups,ldx", [(2400, 800, 12, 768),      # the reference's default S
                                            (2193, 129, 12, 768),      # every 128-row block straddles two samples
                                            (2080, 52, 4, 320),        # three samples in one block; ldx > 64 groups
                                            (333, 7, 5, 320),          # several samples inside one wave's 16 rows; groups % 4 != 0; M % 16 != 0
                                            (2400, 700, 3, 192)])      # last sample short (M % L != 0)
def test_head_mag_measure_equals_torch(M, L, groups, ldx):
    g = torch.Generator().manual_seed(M + L)
    nb = (M + L - 1) // L
    loud = torch.pow(10.0, 6.0 * torch.rand(nb, generator=g) - 3.0).repeat_interleave(L)[:M, None]
    x = torch.randn(M, ldx, generator=g) * loud
    x[:, groups * 64:] = 1e30                                            # columns past the groups are not the entry's to read
    x = x.to(DEV)
    got = measured_words(x, ldx, M, groups, L)
    assert torch.equal(got, torch_words(x, L, groups))


# ---- (b) ---------------------------------------------------------------------------------------------------------------------------
SHAPES_B = [(2400, 800, True), (2193, 129, True), (2080, 52, True), (2400, 700, True), (2304, 1152, False)]     # rows, rows per sample, straddles?


def loud_odd_rows(M, K, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    odd = (torch.arange(M) // L) % 2 == 1
    x[odd] *= 300.0
    return x


def assert_case_tells_bound_from_truth(y64, M, L, groups, straddles):
    """from M and L alone: is there a 128-row sub-tile with rows of two samples?  And in one of them: is the louder sample's maximum
    inside the sub-tile more than twice the quieter sample's OWN maximum, in every 64-column group (y64 = the float64 product)?
    Otherwise an upper bound over the sub-tile and the exact word could land on the same value and the case would show nothing."""
    tiles = [(r0, min(r0 + 128, M)) for r0 in range(0, M, 128)]
    mixed = [(r0, r1) for r0, r1 in tiles if r0 // L != (r1 - 1) // L]
    assert bool(mixed) == straddles
    if not straddles:
        return
    a = y64.abs().view(M, groups, 64).amax(2)                            # [row][group]
    for r0, r1 in mixed:
        b0 = r0 // L
        quiet, louder = (b0, b0 + 1) if b0 % 2 == 0 else (b0 + 1, b0)
        own = a[quiet * L:min((quiet + 1) * L, M)].amax(0)
        inside = a[max(louder * L, r0):min((louder + 1) * L, r1)].amax(0)
        if bool((inside > 2 * own).all()):
            return
    raise AssertionError("no sub-tile in which the louder neighbour dominates every group")


@pytest.mark.parametrize("M,L,straddles", SHAPES_B)
def test_linear_fwd_emu_heads_leaves_the_words_of_the_stored_output(M, L, straddles):
    """in-projection geometry (K = E = 256, N = 3 E = 768: 12 groups), odd samples 300 x louder"""
    from hoisdf_amd._lib import call
    O = ops()
    K, N = 256, 768
    g = torch.Generator().manual_seed(M * 3 + L)
    x = loud_odd_rows(M, K, L, seed=M + L)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g) * 0.1
    assert_case_tells_bound_from_truth(x.double() @ W.double().t() + b.double(), M, L, N // 64, straddles)
    x, W, b = x.to(DEV), W.to(DEV), b.to(DEV)
    img, st = O._emu_image(W, False), O._st()
    nb = (M + L - 1) // L
    y, y0 = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
    ymag, ymag0 = torch.zeros(M, dtype=torch.int32, device=DEV), torch.zeros(M, dtype=torch.int32, device=DEV)
    heads = torch.zeros(N // 64 * nb + 1, dtype=torch.int32, device=DEV)          # zero-filled, as the header asks
    heads[-1] = SENTINEL
    call("hoisdf_linear_fwd_emu_heads", ptr(x), K, ptr(img), ptr(b), ptr(y), N, M, N, K, None, ptr(ymag), ptr(heads), L, st)
    call("hoisdf_linear_fwd_emu_mag", ptr(x), K, ptr(img), ptr(b), ptr(y0), N, M, N, K, 0, 0.0, 0, None, None, ptr(ymag0), st)
    assert int(heads[-1]) == SENTINEL
    assert torch.equal(y, y0)                                                     # the same matrix with and without the head words
    assert torch.equal(ymag.view(torch.float32), y.abs().amax(1)) and torch.equal(ymag, ymag0)
    truth = torch_words(y, L, N // 64)
    bad = (heads[:-1] != truth).nonzero().flatten().tolist()
    assert not bad, (f"{len(bad)} of {truth.numel()} head words differ from the stored y's; first: word {bad[0]} (group {bad[0] // nb}, "
                     f"sample {bad[0] % nb}) = {float(heads[bad[0]].view(torch.float32)):.6e}, "
                     f"max |y| there = {float(truth[bad[0]].view(torch.float32)):.6e}")
    assert torch.equal(heads[:-1], measured_words(y, N, M, N // 64, L))


def test_linear_fwd_emu_heads_does_not_count_the_tile_rows_past_M():
    """L = 128 but a short last sample (M = 2100: 52 rows of the last 128-row sub-tile are real).  A GEMM tile computes its rows past M
    from zero operands, so they hold the bias; they are never stored and must not reach a head word either.  The last sample's rows are
    all one vector r and the bias is -0.75 W r: its stored rows are 0.25 W r, a row past M would be three times that in every column."""
    from hoisdf_amd._lib import call
    O = ops()
    M, L, K, N = 2100, 128, 256, 768
    g = torch.Generator().manual_seed(9)
    x = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) / math.sqrt(K)
    x[2048:] = x[2048].clone()
    b = (-0.75 * (W.double() @ x[2048].double())).float()
    y64 = x.double() @ W.double().t() + b.double()
    own = y64[2048:].abs().view(-1, N // 64, 64).amax((0, 2))
    assert bool((b.double().abs().view(N // 64, 64).amax(1) > 2 * own).all())          # a word that took the bias in cannot pass for the truth
    x, W, b = x.to(DEV), W.to(DEV), b.to(DEV)
    nb = (M + L - 1) // L
    y = torch.empty(M, N, device=DEV)
    heads = torch.zeros(N // 64 * nb + 1, dtype=torch.int32, device=DEV)
    heads[-1] = SENTINEL
    call("hoisdf_linear_fwd_emu_heads", ptr(x), K, ptr(O._emu_image(W, False)), ptr(b), ptr(y), N, M, N, K, None, None, ptr(heads), L, O._st())
    assert int(heads[-1]) == SENTINEL
    assert torch.equal(heads[:-1], torch_words(y, L, N // 64))


@pytest.mark.parametrize("M,L,straddles", SHAPES_B)
def test_linear_bwd_input_emu_heads_leaves_the_words_of_the_stored_output(M, L, straddles):
    """out-projection geometry (N = K = E = 256: the 4 heads are the columns of dx), odd samples 300 x louder"""
    from hoisdf_amd._lib import call
    O = ops()
    N = K = 256
    g = torch.Generator().manual_seed(M * 5 + L)
    dy = loud_odd_rows(M, N, L, seed=M + L + 1)
    W = torch.randn(N, K, generator=g) / math.sqrt(N)
    assert_case_tells_bound_from_truth(dy.double() @ W.double(), M, L, K // 64, straddles)
    dy, W = dy.to(DEV), W.to(DEV)
    img, st = O._emu_image(W, True), O._st()
    nb = (M + L - 1) // L
    dx, dx0 = torch.empty(M, K, device=DEV), torch.empty(M, K, device=DEV)
    dmag, dmag0 = torch.zeros(M, dtype=torch.int32, device=DEV), torch.zeros(M, dtype=torch.int32, device=DEV)
    heads = torch.zeros(K // 64 * nb + 1, dtype=torch.int32, device=DEV)
    heads[-1] = SENTINEL
    call("hoisdf_linear_bwd_input_emu_heads", ptr(dy), N, ptr(img), ptr(dx), K, M, N, K, None, ptr(dmag), ptr(heads), L, st)
    call("hoisdf_linear_bwd_input_emu_mag", ptr(dy), N, None, 0.0, ptr(img), ptr(dx0), K, M, N, K, 0, None, ptr(dmag0), st)
    assert int(heads[-1]) == SENTINEL
    assert torch.equal(dx, dx0)
    assert torch.equal(dmag.view(torch.float32), dx.abs().amax(1)) and torch.equal(dmag, dmag0)
    truth = torch_words(dx, L, K // 64)
    bad = (heads[:-1] != truth).nonzero().flatten().tolist()
    assert not bad, (f"{len(bad)} of {truth.numel()} head words differ from the stored dx's; first: word {bad[0]} (group {bad[0] // nb}, "
                     f"sample {bad[0] % nb}) = {float(heads[bad[0]].view(torch.float32)):.6e}, "
                     f"max |dx| there = {float(truth[bad[0]].view(torch.float32)):.6e}")
    assert torch.equal(heads[:-1], measured_words(dx, K, M, K // 64, L))


# ---- (c), (d): the encoder layer ---------------------------------------------------------------------------------------------------
E_, F_, H_ = 256, 1024, 4
NAMES = ["w_in", "b_in", "w_out", "b_out", "g1", "be1", "w1", "b1", "w2", "b2", "g2", "be2", "g3", "be3"]
PSHAPES = [(3 * E_, E_), (3 * E_,), (E_, E_), (E_,), (E_,), (E_,), (F_, E_), (F_,), (E_, F_), (E_,), (E_,), (E_,), (E_,), (E_,)]


def layer_params():
    g = torch.Generator().manual_seed(20)
    return [torch.randn(*s, generator=g) * (1.0 / math.sqrt(s[-1]) if len(s) == 2 else 0.1) + (1.0 if n in ("g1", "g2", "g3") else 0.0)
            for n, s in zip(NAMES, PSHAPES)]


def run_layer(coarse, x0, P0, gx2, gy, nq, ni, p):
    """-> x_out, y, dx of one deterministic-mode training step through ops.encoder_layer"""
    O = ops()
    keep, keep_det = O._ENCODER_LAYER_C, O.deterministic()
    O.set_deterministic(True)
    try:
        O._ENCODER_LAYER_C = coarse
        O.manual_seed(1234)
        x = x0.to(DEV).requires_grad_(True)
        P = [t.to(DEV).requires_grad_(True) for t in P0]
        picked = O._EncoderLayerC if O._coarse_layer_ok(p, x, P[0], P[2], P[6], P[8]) else O._EncoderLayer
        assert (picked is O._EncoderLayerC) == coarse
        x2, y = O.encoder_layer(x, nq, p, H_, *P, eps=1e-5, n_inter=ni)
        ((x2 * gx2.to(DEV)).sum() + (y * gy.to(DEV)).sum()).backward()
        return x2.detach(), y.detach(), x.grad.detach()
    finally:
        O._ENCODER_LAYER_C = keep
        O.set_deterministic(keep_det)


@pytest.mark.parametrize("coarse", [True, False])
@pytest.mark.parametrize("B,S,nq,ni,p", [(3, 800, None, None, 0.1), (4, 800, 600, 600, 0.1), (17, 129, None, None, 0.0)])
def test_encoder_layer_sample_0_does_not_see_its_companions(B, S, nq, ni, p, coarse):
    """the batch as drawn, then samples 1 .. replaced by other data at x 1 and at x 300 (input and upstream gradients): x_out[0], y[0]
    and dx[0] are bit-identical in all three runs, sample 1's really change.  (Parameter gradients sum over the samples.)"""
    O = ops()
    if not O._h2():
        pytest.skip("f16x2 form only")
    g = torch.Generator().manual_seed(B * S)
    nqe = S if nq is None else nq
    nie = nqe if ni is None else ni
    assert B * nqe >= 2048 and S % 128 and nqe % 128                     # the emulated route, samples that share sub-tiles
    P0 = layer_params()
    x0, gx0, gy0 = torch.randn(B, S, E_, generator=g), torch.randn(B, nqe, E_, generator=g), torch.randn(B, nie, E_, generator=g)
    x1, gx1, gy1 = torch.randn(B, S, E_, generator=g), torch.randn(B, nqe, E_, generator=g), torch.randn(B, nie, E_, generator=g)
    ref = run_layer(coarse, x0, P0, gx0, gy0, nq, ni, p)
    for loud in (1.0, 300.0):
        mix = lambda a, b: torch.cat([a[:1], b[1:] * loud])
        got = run_layer(coarse, mix(x0, x1), P0, mix(gx0, gx1), mix(gy0, gy1), nq, ni, p)
        for what, a, b in zip(("x_out", "y", "dx"), got, ref):
            assert not torch.equal(a[1], b[1]), what                                        # the companions really changed
            assert torch.equal(a[0], b[0]), (f"{what}[0] next to x {loud:g} companions: max |difference| "
                                             f"{float((a[0] - b[0]).abs().max()):.3e} of max {float(b[0].abs().max()):.3e}")


def layer_in_torch(x, P, gx2, gy):
    """the post-norm encoder layer (multi-head attention, add + LayerNorm, FFN with ReLU, add + LayerNorm, inter-norm of the output)
    in plain torch at x's precision, no dropout -> x_out, dx under the loss sum(x_out gx2) + sum(y gy)"""
    w_in, b_in, w_out, b_out, g1, be1, w1, b1, w2, b2, g2, be2, g3, be3 = [t.to(x.dtype) for t in P]
    x = x.clone().requires_grad_(True)
    B, S, E = x.shape
    qkv = F.linear(x, w_in, b_in).view(B, S, 3, H_, E // H_).permute(2, 0, 3, 1, 4)
    att = torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / math.sqrt(E // H_), -1) @ qkv[2]
    a = F.linear(att.permute(0, 2, 1, 3).reshape(B, S, E), w_out, b_out)
    x1 = F.layer_norm(x + a, (E,), g1, be1, 1e-5)
    f = F.linear(torch.relu(F.linear(x1, w1, b1)), w2, b2)
    x2 = F.layer_norm(x1 + f, (E,), g2, be2, 1e-5)
    y = F.layer_norm(x2, (E,), g3, be3, 1e-5)
    ((x2 * gx2.to(x.dtype)).sum() + (y * gy.to(x.dtype)).sum()).backward()
    return x2.detach(), x.grad.detach()


@pytest.fixture(scope="module")
def loud_case():
    """(d)'s inputs, the float64 truth and the float32 yardstick: computed once"""
    B, S = 3, 800
    g = torch.Generator().manual_seed(41)
    x = torch.randn(B, S, E_, generator=g)
    x[1:] *= 300.0
    gx2, gy = torch.randn(B, S, E_, generator=g), torch.randn(B, S, E_, generator=g)
    P0 = layer_params()
    truth = layer_in_torch(x.double(), P0, gx2, gy)
    f32 = layer_in_torch(x, P0, gx2, gy)
    return x, gx2, gy, P0, truth, f32


@pytest.mark.parametrize("coarse", [True, False])
def test_encoder_layer_sample_0_keeps_its_accuracy_next_to_loud_companions(loud_case, coarse):
    """B = 3, S = 800, samples 1 and 2 300 x louder, no dropout: sample 0's x_out and dx against the float64 layer.  Bar:
    max(2e-6 max |truth|, 2 x the distance of the same layer in float32 on the CPU from the truth) - tests/test_gpu_conv.py's, neither
    term from the code under test.  Sharing a scale with a 300 x louder neighbour costs sample 0 about 8 of its operand bits.
    Measured (MI355X; torch f32 yardstick 1.200e-06 / 1.786e-06, bars 9.757e-06 / 1.509e-05 for x_out / dx):
      head words folded over shared sub-tiles, C entry:  x_out 2.568e-06, dx 1.793e-04 (12 x the bar);  op chain: 2.330e-06, 3.439e-06
      head words of each sample's own rows, both hosts:  x_out 2.330e-06, dx 3.439e-06"""
    O = ops()
    if not O._h2():
        pytest.skip("f16x2 form only")
    x, gx2, gy, P0, truth, f32 = loud_case
    got = run_layer(coarse, x, P0, gx2, gy, None, None, 0.0)
    fails = []
    for what, a, t, y in zip(("x_out", "dx"), (got[0], got[2]), truth, f32):
        t0 = t[0]
        err = float((a[0].cpu().double() - t0).abs().max())
        own = float((y[0].double() - t0).abs().max())
        bar = max(2e-6 * float(t0.abs().max()), 2 * own)
        print(f"coarse={coarse} {what}[0]: max |got - truth| {err:.3e}  torch f32 {own:.3e}  max |truth| {float(t0.abs().max()):.3e}  bar {bar:.3e}")
        if not err <= bar:
            fails.append((what, err, bar))
    assert not fails, fails
