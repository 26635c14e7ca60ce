"""-m gpu: attention with dropout on, every kernel family against float64 autograd.

The dropout mask is a pure function of (seed, (b H + h) Lq + i, j) and does not depend on the operand values, so the kernels are
made to print it (hoisdf_amd/testing.py): one-hot V reads the dropped probability matrix out of a forward, one-hot dO reads it out of
the dV of a backward.  With the probed mask M the truth is plain float64 autograd of ((softmax(s) * M / (1 - p)) @ V) on the CPU,
which shares no code with the hash or the kernels - so dq and dk, with delta = rowsum(dO * O) from the dropped O and
dS = P (dP * M / (1 - p) - delta), are checked in the configuration training runs.  tests/test_attention_dropout_checks.py shows on the
CPU that each check rejects the mistake it is there for.  Nothing here mirrors the hash: the tests survive a change of it."""
import functools

import pytest
import torch

from hoisdf_amd import testing as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, H = 256, 4

# name: (B, Lq, Lk, kv_len, (p, ...), seed).  The smallest shapes at which each index path can go wrong:
CASES = {
    # ragged query tile (3 x 32 + 4); one 128-key block + a ragged one; a whole 32-key tile past kv_len; odd kv_len: the last valid key
    # shares its hash with a masked partner; three samples x four heads of row keys
    "A": (3, 100, 200, 149, (0.1, 0.3), 424242),
    "B": (2, 160, 160, 160, (0.1,), 99),                        # self-attention through the packed [q | k | v] layout; exact tile multiples
    "C": (1, 33, 31, 31, (0.1,), (7 << 32) + 5),                # one partial key tile (only the prologue's hash decisions); 32 + 1 queries
    "D": (2, 64, 64, 33, (0.1,), 1234),                         # two key tiles, the second with one valid key
    "E": (2, 17, 200, 149, (0.1,), 424242),                     # few-query kernel, one split
    "F": (1, 1, 40, 33, (0.1,), (7 << 32) + 5),                 # few-query kernel, one query
    # few-query kernel: 34 key tiles -> two key splits + the merge kernel (csrc/attention.hip hoisdf_attention_fwd; it falls back to one
    # split only when the library cannot allocate its 70 KB of stream scratch, which no test can see from outside)
    "G": (1, 17, 1100, 1061, (0.1,), 99),
    "H": (3, 17, 17, None, (0.3,), (7 << 32) + 5),              # small kernels under get_mano_tgt_mask()
    "I": (2, 5, 64, None, (0.1,), 424242),                      # small kernels under a random mask whose diagonal is clear
}
LARGE = ("f32", "f32_det", "b3_kept", "b3_conv", "h2")         # exact fused / two-kernel backward, bf16x3 over kept planes / converting, f16x2
FAMILIES = {"A": LARGE, "B": LARGE, "C": LARGE, "D": LARGE, "E": ("f32", "f32_det"), "F": ("f32", "f32_det"), "G": ("f32", "f32_det"),
            "H": ("small", "small_det"), "I": ("small", "small_det")}
RUNS = [(c, p, f) for c, fams in FAMILIES.items() for p in CASES[c][4] for f in fams]


def ops():
    from hoisdf_amd import ops as O
    return O


def _h2_or_skip():
    from hoisdf_amd._lib import lib
    if lib().hoisdf_linear_emu_pieces() != 2:
        pytest.skip("the Python helpers measure magnitudes only in f16x2 processes")


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """CPU float32 q, k, v, dO from a seeded generator, the valid pairs, and the float64 probabilities (shared, never modified)"""
    B, Lq, Lk, kv, _, _ = CASES[case]
    g = torch.Generator().manual_seed(1000 + ord(case))
    q, do = torch.randn(B, Lq, E, generator=g), torch.randn(B, Lq, E, generator=g)
    k, v = torch.randn(B, Lk, E, generator=g), torch.randn(B, Lk, E, generator=g)
    umask = None
    if case == "H":
        from hoisdf_amd.model import get_mano_tgt_mask
        umask = get_mano_tgt_mask()
        assert tuple(umask.shape) == (Lq, Lk)
    elif case == "I":
        umask = torch.rand(Lq, Lk, generator=g) < 0.5
        umask[torch.arange(Lq), torch.arange(Lq)] = False
    valid = (torch.arange(Lk) < kv).view(1, 1, 1, Lk) if umask is None else ~umask.view(1, 1, Lq, Lk)
    return dict(q=q, k=k, v=v, do=do, umask=umask, valid=valid, p64=T.reference_probs(q, k, H, valid))


def _kernel(family, case, p):
    """(fwd, bwd) of one family on CPU tensors (testing.py), through the private entries of hoisdf_amd/ops.py"""
    O = ops()
    B, Lq, Lk, kv, _, seed = CASES[case]
    det = family.endswith("_det")

    def place(q, k, v):
        """operands on the device in the layout the model uses: packed [q | k | v] (case B), else q + packed [k | v]; returns the
        views, gradient views of the same layout, and the head magnitudes for the f16x2 form"""
        if case == "B":
            m = torch.cat([q, k, v], -1).to(DEV)
            d = torch.empty_like(m)
            views, grads = (m[..., :E], m[..., E:2 * E], m[..., 2 * E:]), (d[..., :E], d[..., E:2 * E], d[..., 2 * E:])
            heads = None
            if family == "h2":
                hm = O._head_measure(m, 3 * E, B * Lq, 3 * H, Lq)
                heads = (hm, hm[H * B:], hm[2 * H * B:])
            return views, grads, heads
        qd, m = q.to(DEV), torch.cat([k, v], -1).to(DEV)
        d = torch.empty_like(m)
        heads = None
        if family == "h2":
            hq, hkv = O._head_measure(qd, E, B * Lq, H, Lq), O._head_measure(m, 2 * E, B * Lk, 2 * H, Lk)
            heads = (hq, hkv, hkv[H * B:])
        return (qd, m[..., :E], m[..., E:]), (torch.empty_like(qd), d[..., :E], d[..., E:]), heads

    def in_mode(fn):
        keep = O.deterministic()
        O.set_deterministic(det)
        try:
            out = fn()
            torch.cuda.synchronize()
            return out
        finally:
            O.set_deterministic(keep)

    if family.startswith("small"):
        um = _inputs(case)["umask"].to(torch.uint8).to(DEV)

        def small(q, k, v, do=None):
            qd, kd, vd = (t.to(DEV).requires_grad_(do is not None) for t in (q, k, v))
            o = O._AttentionSmall.apply(qd, kd, vd, um, H, p, seed)
            if do is None:
                return o.cpu()
            o.backward(do.to(DEV))
            return qd.grad.cpu(), kd.grad.cpu(), vd.grad.cpu()
        return (lambda q, k, v: in_mode(lambda: small(q, k, v))), (lambda q, k, v, do: in_mode(lambda: small(q, k, v, do)))

    def forward(views, heads, keep=False):
        if family.startswith("f32"):
            return O._attn_fwd(*views, H, kv, p, seed)
        if family == "h2":
            return O._attn_fwd_emu(*views, H, kv, p, seed, heads=heads)
        return O._attn_fwd_emu(*views, H, kv, p, seed, keep=keep)

    def fwd(q, k, v):
        def run():
            views, _, heads = place(q, k, v)
            o = forward(views, heads)[0].cpu()
            O._EMU_PLANES.clear()
            return o
        return in_mode(run)

    def bwd(q, k, v, do):
        def run():
            views, grads, heads = place(q, k, v)
            O._EMU_PLANES.clear()
            o, lse = forward(views, heads, keep=family == "b3_kept")
            assert len(O._EMU_PLANES) == (1 if family == "b3_kept" else 0)
            if family.startswith("f32"):
                O._attn_bwd(*views, o, lse, do.to(DEV), *grads, H, kv, p, seed)
            else:
                O._attn_bwd_emu(*views, o, lse, do.to(DEV), *grads, H, kv, p, seed, **(dict(heads=heads) if family == "h2" else {}))
            assert not O._EMU_PLANES                               # kept planes are consumed
            return tuple(g.cpu() for g in grads)
        return in_mode(run)
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def _probed(family, case, p):
    """the dropped probability matrices a family's forward and backward give at a case, (Pd forward, Pd backward) on the CPU -
    probed once, shared by the tests below"""
    if family == "h2":
        _h2_or_skip()
    c = _inputs(case)
    fwd, bwd = _kernel(family, case, p)
    return T.probe_dropped_probs_forward(fwd, c["q"], c["k"], H), T.probe_dropped_probs_backward(bwd, c["q"], c["k"], c["v"], H)


@pytest.mark.parametrize("case,p,family", RUNS, ids=[f"{c}-p{p}-{f}" for c, p, f in RUNS])
def test_attention_dropout_matches_fp64_under_the_kernels_own_mask(case, p, family):
    """per family and case: (1) the reference's probabilities are large enough for `Pd > 0` to be the mask; (2) the forward's mask
    is the backward's on every valid (b, h, i, j), excluded pairs give exactly 0; (4) the probed forward matrix is P64 * M / (1 - p)
    to the attention-output bar, 2e-5 of max; (5) o, dq, dk, dv with real V and dO against float64 autograd under M at the bars these
    kernels carry at p = 0 (2e-5 / 5e-5 of max, the emulated forms included), gradients of excluded keys exactly zero."""
    c = _inputs(case)
    smallest = T.check_probe_validity(c["p64"], c["valid"])
    pdf, pdb = _probed(family, case, p)
    m = T.check_same_mask(pdf, pdb, c["valid"])
    kept = T.check_kept_values(pdf, c["p64"], m, p)
    fwd, bwd = _kernel(family, case, p)
    try:
        errs = T.check_forward_and_gradients(fwd, bwd, c["q"], c["k"], c["v"], c["do"], H, c["valid"], m, p)
    except AssertionError as e:
        print(f"attention-dropout case {case} p={p} {family}: {e}")
        raise
    print(f"attention-dropout case {case} p={p} {family:9s} rel. error of max: Pd {kept:.2e} o {errs['o']:.2e} dq {errs['dq']:.2e} "
          f"dk {errs['dk']:.2e} dv {errs['dv']:.2e} (smallest P64 {smallest:.1e}, kept {float(m.sum()) / float(c['valid'].expand(m.shape).sum()):.4f})")


@pytest.mark.parametrize("case,p", [(c, p) for c in CASES for p in CASES[c][4]])
def test_one_mask_for_all_families(case, p):
    """(3) the evidence that the families share one function of (seed, row, column): at each case the probed masks - forward and
    backward - of every family that runs there are torch.equal: exact, bf16x3 and f16x2; fused and two-kernel exact backward; kept-plane
    and self-converting emulated backward; both small backward kernels."""
    from hoisdf_amd._lib import lib
    c = _inputs(case)
    vm = None
    first = None
    for family in FAMILIES[case]:
        if family == "h2" and lib().hoisdf_linear_emu_pieces() != 2:
            print(f"attention-dropout case {case} p={p}: f16x2 left out of the mask comparison (bf16x3 process)")
            continue
        for which, pd in zip(("forward", "backward"), _probed(family, case, p)):
            vm = c["valid"].expand(pd.shape) if vm is None else vm
            m = (pd > 0) & vm
            if first is None:
                first = (family, which, m)
            diff = m != first[2]
            assert torch.equal(m, first[2]), f"{family} {which} and {first[0]} {first[1]} differ on {int(diff.sum())} pairs, first at " \
                                             f"(b, h, i, j) = {tuple(diff.nonzero()[0].tolist())}"


SEEDS = (424242, 99, (7 << 32) + 5)


@functools.lru_cache(maxsize=None)
def _mask_of_case_a(p, seed, emulated=False):
    """the mask of a forward at case A's shape under any seed: the exact kernel's, or the bf16x3 kernel's"""
    B, Lq, Lk, kv, _, _ = CASES["A"]
    c = _inputs("A")
    O = ops()

    def fwd(q, k, v):
        m = torch.cat([k, v], -1).to(DEV)
        return (O._attn_fwd_emu if emulated else O._attn_fwd)(q.to(DEV), m[..., :E], m[..., E:], H, kv, p, seed)[0].cpu()
    return (T.probe_dropped_probs_forward(fwd, c["q"], c["k"], H) > 0) & c["valid"]


@pytest.mark.parametrize("p", [0.1, 0.3])
@pytest.mark.parametrize("seed", SEEDS)
def test_mask_statistics(p, seed):
    """(6) on the probed masks of case A (178,800 valid pairs): the keep fraction within 5 sigma of the binomial around
    1 - floor(p 2^16) / 2^16, and the joint keep frequency of neighbours - the two columns sharing a hash, the next column pair, adjacent
    rows, heads, samples - within 5 sigma of its square; each sigma from the element count (testing.check_mask_statistics).  The mask
    is the exact forward's; the emulated forward gives the same one under every seed here (test_one_mask_for_all_families has one
    seed per case)."""
    kv = CASES["A"][3]
    m = _mask_of_case_a(p, seed)
    assert torch.equal(m, _mask_of_case_a(p, seed, emulated=True))
    try:
        stats = T.check_mask_statistics(m, kv, p)
    except AssertionError as e:
        print(f"attention-dropout statistics p={p} seed={seed}: {e}")
        raise
    for name, (f, prob, n, z) in stats.items():
        print(f"attention-dropout statistics p={p} seed={seed} {name:22s} {f:.5f} over {n:6d}, expected {prob:.5f}: {z:+.2f} sigma")


def test_masks_of_different_seeds_differ():
    """two seeds give two masks - also two seeds that differ only in their high 32 bits - and one seed gives one"""
    p, kv = 0.1, CASES["A"][3]
    a, b, hi = _mask_of_case_a(p, 99), _mask_of_case_a(p, 424242), _mask_of_case_a(p, (7 << 32) + 99)
    assert not torch.equal(a, b) and not torch.equal(a, hi) and not torch.equal(b, hi)
    assert torch.equal(a, _mask_of_case_a.__wrapped__(p, 99))
    for name, x, y in (("99 / 424242", a, b), ("99 / (7 << 32) + 99", a, hi)):
        print(f"attention-dropout seeds {name}: {float((x == y)[..., :kv].double().mean()):.5f} of the decisions agree")
