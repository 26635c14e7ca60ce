"""-m gpu: the fused AdamW step (``hoisdf_adamw_step``, csrc/optim.hip, driven by hoisdf_amd/optim.py) in the form it runs
in under the gradient reducer: gradients that are views into a flat bucket at any 4-byte alignment (the kernel's scalar
branch), permuted channels_last views, parameters whose step counts differ, hyper-parameters that change between steps.

Truth is ``torch.optim.AdamW`` (foreach=False) on float64 CPU copies.  The yardstick is the same optimizer on float32 CPU
copies fed the same float32 gradients: its distance to the truth is what f32 arithmetic costs this update rule, and the HIP
result may be at most twice as far from the truth (fma contraction; ``(lr / bias1) * (m / denom)`` where torch has an
``addcdiv`` with a step size) plus one f32 ulp of the tensor's largest magnitude (for a baseline that happens to be exact).
Where two runs apply the same arithmetic to the same values (other alignment, other chunking, cached or rebuilt chunk
table, resumed from a checkpoint) the requirement is bit equality.

Every bound check prints an ``ADAMW`` line (baseline error, HIP error, ratio) before it asserts;
profiles/adamw_f32_vs_fp64.txt is those lines of one run."""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CHUNK = 16384                       # hoisdf_amd.optim.CHUNK: elements per row of the chunk table
SENTINEL = 12345.0                  # fills every buffer a placed tensor is carved from
PAD = 4                             # sentinel elements in front of offset 0 (16 bytes: offset 0 stays float4-aligned)
TAIL = 8                            # ... and at least this many behind the slice


def fused_adamw():
    from hoisdf_amd.optim import FusedAdamW
    return FusedAdamW


# ---------------------------------------------------------------------------------------------
# placing a tensor at a chosen alignment
# ---------------------------------------------------------------------------------------------
def flat_physical(x):
    """the values of ``x`` in memory order (dense contiguous, or dense channels_last 4-D)"""
    if x.dim() == 4 and not x.is_contiguous():
        assert x.is_contiguous(memory_format=torch.channels_last)
        return x.permute(0, 2, 3, 1).reshape(-1)
    return x.reshape(-1)


def view_like(flat, x):
    """``flat`` (1-D, x.numel() elements) seen with the shape and the strides of ``x``"""
    if x.dim() == 4 and not x.is_contiguous():
        o, i, kh, kw = x.shape
        return flat.view(o, kh, kw, i).permute(0, 3, 1, 2)
    return flat.view(x.shape)


class Placed:
    """A device copy of the host float32 tensor ``x`` that starts ``off`` (0..3) elements behind a 16-byte boundary, carved
    out of a buffer of its own that is pre-filled with SENTINEL.  ``t`` has the shape and the strides of ``x``."""

    def __init__(self, x, off):
        assert x.dtype == torch.float32 and 0 <= off <= 3
        self.n, self.lo = x.numel(), PAD + off
        self.buf = torch.full((self.lo + self.n + TAIL,), SENTINEL, dtype=torch.float32, device=DEV)
        flat = self.buf[self.lo:self.lo + self.n]
        flat.copy_(flat_physical(x))
        self.t = view_like(flat, x)
        assert self.buf.data_ptr() % 16 == 0 and self.t.data_ptr() % 16 == 4 * off
        assert self.t.shape == x.shape and (self.n <= 1 or self.t.stride() == x.stride())

    def bits(self):
        return self.buf.view(torch.int32).cpu()

    def surroundings_untouched(self):
        b, s = self.bits(), int(torch.tensor([SENTINEL]).view(torch.int32))
        return bool((b[:self.lo] == s).all()) and bool((b[self.lo + self.n:] == s).all())


def seed_state(opt, p, m_off, v_off):
    """FusedAdamW makes its moments with zeros_like (allocator-aligned): misaligned ones are put in place before the first step"""
    z = torch.zeros(p.shape, dtype=torch.float32).contiguous(memory_format=torch.channels_last) \
        if (p.dim() == 4 and not p.is_contiguous()) else torch.zeros(p.shape, dtype=torch.float32)
    m, v = Placed(z, m_off), Placed(z, v_off)
    opt.state[p] = {"step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": m.t, "exp_avg_sq": v.t}
    return m, v


class Feeder:
    """Hands one step's gradients (host float32 tensors, or None) to device parameters: as new tensors at element offset
    ``g_offs[i]`` every step (the pointers change, the optimizer rebuilds its chunk table) or, ``inplace``, written into
    tensors that persist (the table stays cached).  Keeps every Placed gradient and the bits that were uploaded."""

    def __init__(self, params, g_offs=None, inplace=False, keep=False):
        self.params, self.inplace, self.keep = params, inplace, keep
        self.g_offs = g_offs or [0] * len(params)
        self.persistent = [None] * len(params)
        self.last, self.uploaded = [], []

    def feed(self, grads):
        now = []
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                p.grad = None
                continue
            if self.inplace:
                if self.persistent[i] is None:
                    self.persistent[i] = Placed(g, self.g_offs[i])
                else:
                    self.persistent[i].t.copy_(g)
                p.grad = self.persistent[i].t
            else:
                pl = Placed(g, self.g_offs[i])
                now.append(pl)
                if self.keep:
                    self.uploaded.append((pl, pl.bits()))
                p.grad = pl.t
        self.last = now                         # last step's gradients stay alive until here: this step's got other addresses


# ---------------------------------------------------------------------------------------------
# 1 + 2: alignment and chunking change nothing, bit for bit; nothing outside [0, n) is written
# ---------------------------------------------------------------------------------------------
SIZES = [1, 2, 3, 4, 5, 7, 255, 256, 257, 1023, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3]
# element offsets of (param, grad, exp_avg, exp_avg_sq); the first is the all-aligned run the others are compared with
PLACEMENTS = [(0, 0, 0, 0), (0, 1, 0, 0), (0, 2, 0, 0), (0, 3, 0, 0), (1, 0, 0, 0), (1, 2, 3, 0)]
HYPER12 = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, grad_scale=0.5)
_RUNS = {}


def placement_values(n, steps=3):
    gen = torch.Generator().manual_seed(1000 + n)
    return torch.randn(n, generator=gen), [torch.randn(n, generator=gen) * 2.0 for _ in range(steps)]


def placement_runs(n):
    """3 steps on the same values per placement, computed once per size and shared by tests 1 and 2"""
    if n not in _RUNS:
        p0, grads = placement_values(n)
        runs = []
        for p_off, g_off, m_off, v_off in PLACEMENTS:
            p = Placed(p0, p_off)
            opt = fused_adamw()([p.t], **HYPER12)
            m, v = seed_state(opt, p.t, m_off, v_off)
            feed = Feeder([p.t], [g_off], keep=True)
            for g in grads:
                feed.feed([g])
                opt.step()
            torch.cuda.synchronize()
            assert opt.state[p.t]["exp_avg"].data_ptr() == m.t.data_ptr()          # the seeded moments were the ones used
            runs.append(dict(p=p, m=m, v=v, grads=feed.uploaded))
        _RUNS[n] = runs
    return _RUNS[n]


@pytest.mark.parametrize("n", SIZES)
def test_result_independent_of_alignment(n):
    """Both branches of the kernel (float4 + tail / scalar) apply the same ``adamw1`` expression by expression: the same
    values give the same bits wherever the four arrays start.  (0, g, 0, 0) with g = 1..3 is the reducer's case."""
    runs = placement_runs(n)
    ref = runs[0]
    assert float(ref["m"].t.abs().max()) > 0.0 and not torch.equal(ref["p"].t.cpu(), placement_values(n)[0])   # it stepped
    for offs, r in zip(PLACEMENTS[1:], runs[1:]):
        for k in ("p", "m", "v"):
            assert torch.equal(r[k].t, ref[k].t), f"n={n} offsets (p, g, m, v)={offs}: {k} differs from the aligned run"


@pytest.mark.parametrize("n", SIZES)
def test_writes_stay_inside_the_arrays(n):
    """Every sentinel in front of and behind the parameter and the two moments is unchanged (bitwise), and the gradient
    buffers - slice and surroundings - are what was uploaded."""
    for offs, r in zip(PLACEMENTS, placement_runs(n)):
        for k in ("p", "m", "v"):
            assert r[k].surroundings_untouched(), f"n={n} offsets (p, g, m, v)={offs}: write outside {k}[0:{n}]"
        assert len(r["grads"]) == 3
        for pl, bits in r["grads"]:
            assert torch.equal(pl.bits(), bits), f"n={n} offsets (p, g, m, v)={offs}: the gradient buffer was written"
            assert pl.surroundings_untouched()


def test_result_independent_of_chunking():
    """2*16384 + 3 values as one tensor (three rows of the chunk table, the last one 3 elements) and as three tensors
    (16384, 16384, 3) in one optimizer: the same bits."""
    n = 2 * CHUNK + 3
    p0, grads = placement_values(n)
    one = p0.clone().to(DEV)
    parts = [c.clone().to(DEV) for c in p0.split(CHUNK)]
    assert [c.numel() for c in parts] == [CHUNK, CHUNK, 3]
    opt1, opt3 = fused_adamw()([one], **HYPER12), fused_adamw()(parts, **HYPER12)
    for g in grads:
        one.grad = g.clone().to(DEV)
        for c, gc in zip(parts, g.split(CHUNK)):
            c.grad = gc.clone().to(DEV)
        opt1.step()
        opt3.step()
    assert not torch.equal(one.cpu(), p0)
    assert torch.equal(torch.cat(parts), one)
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(torch.cat([opt3.state[c][k] for c in parts]), opt1.state[one][k]), k
    assert torch.equal(placement_runs(n)[0]["p"].t, one)            # and the same bits as the placed runs of test 1


# ---------------------------------------------------------------------------------------------
# the bound against fp64, measured against torch's own f32
# ---------------------------------------------------------------------------------------------
def f32_ulp(x: float) -> float:
    """spacing of float32 at magnitude ``x``"""
    return 2.0 ** (max(math.frexp(x)[1] - 1, -126) - 23)


def check_bound(case, what, hip, base, truth):
    """max abs error of the HIP result against the fp64 truth <= 2 x that of torch's f32 run + 1 f32 ulp of the largest value"""
    hip, base, truth = hip.detach().cpu().double(), base.detach().double(), truth.detach()
    assert truth.dtype == torch.float64 and hip.shape == truth.shape
    assert bool(torch.isfinite(hip).all()) and bool(torch.isfinite(truth).all()), f"{case} {what}: not finite"
    e_hip, e_base = float((hip - truth).abs().max()), float((base - truth).abs().max())
    ulp = f32_ulp(float(truth.abs().max()))
    ratio = e_hip / e_base if e_base > 0.0 else float("inf") if e_hip > 0.0 else 0.0
    print(f"ADAMW {case:<26s} {what:<14s} n={truth.numel():<6d} f32_torch={e_base:.3e} hip={e_hip:.3e} ratio={ratio:6.3f} "
          f"ulp={ulp:.3e}")
    assert e_hip <= 2.0 * e_base + ulp, \
        f"{case} {what}: HIP {e_hip:.3e} from fp64, torch f32 {e_base:.3e} (ratio {ratio:.2f}), ulp {ulp:.3e}"


def check_all(case, gpu_p, opt, base_p, base, truth_p, truth):
    for i, (q, b, r) in enumerate(zip(gpu_p, base_p, truth_p)):
        check_bound(case, f"p{i}", q, b, r)
        if "exp_avg" in truth.state.get(r, {}):
            for k in ("exp_avg", "exp_avg_sq"):
                check_bound(case, f"p{i}.{k}", opt.state[q][k], base.state[b][k], truth.state[r][k])
        else:
            assert "exp_avg" not in opt.state.get(q, {})


class Trio:
    """The same parameters under FusedAdamW on the device, torch's AdamW in float32 on the CPU (the baseline) and torch's
    AdamW in float64 on the CPU (the truth).  ``groups``: one dict of hyper-parameters per param group with the indices of
    its members under "idx".  ``offs[i]``: element offsets of (param, grad, exp_avg, exp_avg_sq) of tensor i.  The device
    gradient is the true one divided by ``grad_scale`` (powers of two: exact)."""

    def __init__(self, init, groups, grad_scale=1.0, offs=None, inplace=False):
        offs = offs or [(0, 0, 0, 0)] * len(init)
        self.grad_scale = grad_scale
        self.placed = [Placed(x, o[0]) for x, o in zip(init, offs)]
        self.gpu_p = [pl.t for pl in self.placed]
        self.base_p = [x.clone() for x in init]
        self.truth_p = [x.double() for x in init]

        def grouped(ps):
            return [dict({k: v for k, v in g.items() if k != "idx"}, params=[ps[i] for i in g["idx"]]) for g in groups]
        self.opt = fused_adamw()(grouped(self.gpu_p), grad_scale=grad_scale)
        self.base = torch.optim.AdamW(grouped(self.base_p), foreach=False)
        self.truth = torch.optim.AdamW(grouped(self.truth_p), foreach=False)
        self.moments = [seed_state(self.opt, p, o[2], o[3]) if (o[2], o[3]) != (0, 0) else None
                        for p, o in zip(self.gpu_p, offs)]
        self.feeder = Feeder(self.gpu_p, [o[1] for o in offs], inplace=inplace)

    def step(self, grads):
        self.feeder.feed([None if g is None else g / self.grad_scale for g in grads])
        for b, r, g in zip(self.base_p, self.truth_p, grads):
            b.grad = None if g is None else g.clone()
            r.grad = None if g is None else g.double()
        self.opt.step()
        self.base.step()
        self.truth.step()

    def scale_lr(self, factor):
        for o in (self.opt, self.base, self.truth):
            for g in o.param_groups:
                g["lr"] = g["lr"] * factor

    def check(self, case):
        check_all(case, self.gpu_p, self.opt, self.base_p, self.base, self.truth_p, self.truth)


# ---------------------------------------------------------------------------------------------
# 3: a grid of hyper-parameters
# ---------------------------------------------------------------------------------------------
def grid_init(seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(4099, generator=gen), torch.randn(CHUNK + 5, generator=gen),
            torch.randn(8, 5, 3, 3, generator=gen).contiguous(memory_format=torch.channels_last)], gen


# 4099: aligned, float4 loop + 3-element tail.  16384 + 5: the gradient 3 elements off, as in a bucket (scalar branch, two
# rows).  8x5x3x3 channels_last: all four arrays at different offsets.
GRID_OFFS = [(0, 0, 0, 0), (0, 3, 0, 0), (1, 2, 3, 0)]
REF_SETTING = dict(lr=1e-4, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)          # the reference's setting
GRID = {
    "reference_setting": dict(groups=[dict(REF_SETTING, idx=[0, 1, 2])]),
    "weight_decay_0": dict(groups=[dict(REF_SETTING, weight_decay=0.0, idx=[0, 1, 2])]),
    "betas_0.8_0.9": dict(groups=[dict(REF_SETTING, betas=(0.8, 0.9), idx=[0, 1, 2])]),
    "eps_1e-6": dict(groups=[dict(REF_SETTING, eps=1e-6, idx=[0, 1, 2])]),
    "lr_1e-2_grad_scale_0.25": dict(groups=[dict(REF_SETTING, lr=1e-2, idx=[0, 1, 2])], grad_scale=0.25),
    "lr_x0.1_after_step_5": dict(groups=[dict(REF_SETTING, idx=[0, 1, 2])], decay_after=5),
    "two_param_groups": dict(groups=[dict(REF_SETTING, idx=[0, 2]), dict(REF_SETTING, lr=3e-3, weight_decay=0.1, idx=[1])]),
}


@pytest.mark.parametrize("case", list(GRID))
def test_matches_fp64_over_hyperparameters(case):
    """10 steps per case.  ``lr_x0.1_after_step_5`` changes ``param_groups[0]["lr"]`` as a scheduler does: the cached
    chunk table must not freeze the hyper-parameters."""
    spec = GRID[case]
    init, gen = grid_init(31)
    trio = Trio(init, spec["groups"], grad_scale=spec.get("grad_scale", 1.0), offs=GRID_OFFS, inplace=True)
    for it in range(1, 11):
        trio.step([torch.randn(x.shape, generator=gen).contiguous(memory_format=torch.channels_last) if x.dim() == 4
                   else torch.randn(x.shape, generator=gen) for x in init])
        if it == spec.get("decay_after"):
            trio.scale_lr(0.1)
    trio.check(case)


EXTREMES = torch.tensor([0.0, 1e-30, -1e-30, 1e-12, -1e-12, 1.0, -1.0, 1e12, -1e12])


def test_matches_fp64_on_extreme_gradients():
    """Gradients that are, element by element, one of {0, +-1e-30, +-1e-12, +-1, +-1e12}: squares stay inside the f32 range
    and 1e-60 underflows alike in both f32 runs.  The first nine elements of each tensor keep ONE of the values for all
    steps (element 0: always zero), the others draw a new one every step.  After the first step an element whose gradient
    was exactly zero (zero moments: 0 / eps) holds p * (1 - lr * wd); nothing is ever NaN or infinite."""
    init, gen = grid_init(32)
    trio = Trio(init, [dict(REF_SETTING, idx=[0, 1, 2])], offs=GRID_OFFS, inplace=True)
    decay = 1.0 - REF_SETTING["lr"] * REF_SETTING["weight_decay"]
    for it in range(1, 11):
        grads = []
        for x in init:
            pick = torch.randint(0, len(EXTREMES), (x.numel(),), generator=gen)
            pick[:len(EXTREMES)] = torch.arange(len(EXTREMES))
            grads.append(view_like(EXTREMES[pick], x))
        trio.step(grads)
        for q, m, v in [(q, trio.opt.state[q]["exp_avg"], trio.opt.state[q]["exp_avg_sq"]) for q in trio.gpu_p]:
            assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all()), it
        if it == 1:
            for x, q, g in zip(init, trio.gpu_p, grads):
                zero = g == 0.0
                assert int(zero.sum()) > 0
                assert torch.equal(q.cpu()[zero], (x * decay)[zero])
    trio.check("extreme_gradients")


@pytest.mark.parametrize("flag", ["amsgrad", "maximize"])
def test_unsupported_flags_raise(flag):
    p = torch.ones(8, device=DEV)
    opt = fused_adamw()([p], lr=1e-3)
    opt.param_groups[0][flag] = True
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError):
        opt.step()
    assert torch.equal(p.cpu(), torch.ones(8))


# ---------------------------------------------------------------------------------------------
# 4: long run
# ---------------------------------------------------------------------------------------------
def test_long_run_2000_steps():
    """2000 steps at lr 1e-3, gradient = a fixed signal + per-step seeded noise (the moments settle); the step counter
    counts on the host."""
    gen = torch.Generator().manual_seed(41)
    n, steps = 4096, 2000
    init = [torch.randn(n, generator=gen)]
    signal = torch.randn(n, generator=gen)
    noise = torch.randn(steps, n, generator=gen) * 0.5
    trio = Trio(init, [dict(REF_SETTING, lr=1e-3, idx=[0])], inplace=True)
    for it in range(steps):
        trio.step([signal + noise[it]])
    trio.check("long_run_2000")
    st = trio.opt.state[trio.gpu_p[0]]["step"]
    assert torch.is_tensor(st) and st.device.type == "cpu" and float(st) == 2000.0


# ---------------------------------------------------------------------------------------------
# 5 + 7: parameters with different step counts; resume in the middle
# ---------------------------------------------------------------------------------------------
def uneven_init():
    gen = torch.Generator().manual_seed(51)
    init = [torch.randn(1001, generator=gen), torch.randn(CHUNK + 7, generator=gen),
            torch.randn(8, 5, 3, 3, generator=gen).contiguous(memory_format=torch.channels_last),
            torch.randn(33, generator=gen), torch.randn(257, generator=gen)]
    return init, gen


def uneven_grads(init, gen, it):
    """step ``it`` (1-based) of: A every step, B from step 4 on, C every step but 6 and 7, D never, E only on step 12"""
    gs = [torch.randn(x.shape, generator=gen).contiguous(memory_format=torch.channels_last) if x.dim() == 4
          else torch.randn(x.shape, generator=gen) for x in init]
    use = [True, it >= 4, it not in (6, 7), False, it == 12]
    return [g if u else None for g, u in zip(gs, use)]


UNEVEN_GROUPS = [dict(REF_SETTING, lr=1e-3, idx=[0, 1, 2, 3, 4])]
UNEVEN_STEPS = [12.0, 9.0, 10.0, None, 1.0]
_UNEVEN = {}


def uneven_run(inplace):
    if inplace not in _UNEVEN:
        init, gen = uneven_init()
        trio = Trio(init, UNEVEN_GROUPS, inplace=inplace)
        for it in range(1, 13):
            trio.step(uneven_grads(init, gen, it))
        torch.cuda.synchronize()
        _UNEVEN[inplace] = (init, trio)
    return _UNEVEN[inplace]


@pytest.mark.parametrize("inplace", [False, True], ids=["fresh_grads", "inplace_grads"])
def test_parameters_with_different_step_counts(inplace):
    """torch keeps a step count per parameter and skips a parameter whose grad is None entirely (no weight decay, no
    moment decay); FusedAdamW launches once per distinct step count."""
    init, trio = uneven_run(inplace)
    trio.check("uneven_steps_" + ("inplace" if inplace else "fresh"))
    assert torch.equal(trio.gpu_p[3].cpu(), init[3])                      # D: bit-identical to its initial value
    for q, r, want in zip(trio.gpu_p, trio.truth_p, UNEVEN_STEPS):
        st = trio.opt.state.get(q, {})
        if want is None:
            assert "step" not in st and "step" not in trio.truth.state.get(r, {})
        else:
            assert float(st["step"]) == want == float(trio.truth.state[r]["step"])
            assert st["step"].device.type == "cpu"


def test_cached_and_rebuilt_chunk_tables_agree():
    """fresh gradient tensors every step (table rebuilt) against gradients written in place (table cached): the same bits"""
    (_, a), (_, b) = uneven_run(False), uneven_run(True)
    for qa, qb in zip(a.gpu_p, b.gpu_p):
        assert torch.equal(qa, qb)
        for k in ("exp_avg", "exp_avg_sq"):
            if k in a.opt.state.get(qa, {}) or k in b.opt.state.get(qb, {}):
                assert torch.equal(a.opt.state[qa][k], b.opt.state[qb][k]), k


def test_resume_in_the_middle():
    """state_dict() after step 6 of the uneven-steps run (C has just been skipped: three different step counts) into new
    parameter tensors and a new FusedAdamW; both continue to step 12 on the same gradients."""
    init, gen = uneven_init()
    groups = [dict({k: v for k, v in UNEVEN_GROUPS[0].items() if k != "idx"})]
    pa = [Placed(x, 0).t for x in init]
    oa = fused_adamw()([dict(groups[0], params=pa)])
    fa = Feeder(pa)
    grads = [uneven_grads(init, gen, it) for it in range(1, 13)]
    for g in grads[:6]:
        fa.feed(g)
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    pb = [q.detach().clone() for q in pa]
    assert all(b.stride() == a.stride() or b.numel() <= 1 for a, b in zip(pa, pb))
    ob = fused_adamw()([dict(groups[0], params=pb)])
    ob.load_state_dict(copy.deepcopy(sd))               # the loader adopts the tensors it is given: sd itself stays at step 6
    want = [6.0, 3.0, 5.0, None, None]
    for a, q, w in zip(pa, pb, want):
        st = ob.state.get(q, {})
        if w is None:
            assert "step" not in st
        else:
            assert torch.is_tensor(st["step"]) and st["step"].device.type == "cpu" and st["step"].dtype == torch.float32
            assert float(st["step"]) == w
            assert st["exp_avg"].data_ptr() != oa.state[a]["exp_avg"].data_ptr()
    fb = Feeder(pb)
    for g in grads[6:]:
        fa.feed(g)
        fb.feed(g)
        oa.step()
        ob.step()
    for a, b, w in zip(pa, pb, UNEVEN_STEPS):
        assert torch.equal(a, b)
        if w is not None:
            assert float(oa.state[a]["step"]) == float(ob.state[b]["step"]) == w
            for k in ("exp_avg", "exp_avg_sq"):
                assert torch.equal(oa.state[a][k], ob.state[b][k]), k
    assert not torch.equal(pa[0].cpu(), init[0])
    stock = torch.optim.AdamW([dict(groups[0], params=[q.detach().clone() for q in pa])])
    stock.load_state_dict(copy.deepcopy(sd))                              # the torch layout: loads into a stock AdamW
    assert float(stock.state[stock.param_groups[0]["params"][0]]["step"]) == 6.0


# ---------------------------------------------------------------------------------------------
# 6: the reducer's buckets feeding the optimizer (world 1, no process group)
# ---------------------------------------------------------------------------------------------
def test_reducer_buckets_feed_the_optimizer():
    """GradReducer re-points every p.grad at a view of a flat bucket: behind the first odd-sized member the views are only
    4-byte aligned (the kernel's scalar branch), the 4-D channels_last members are permuted views.  The loss is
    sum((p * 2c_p).sum()), so the gradient is 2c_p exactly and grad_scale = 0.5 makes it c_p.  The (4, 4) parameter is
    used on odd steps only: on even steps finish() hands grad = None back for it, and it ends with step 3."""
    from hoisdf_amd.ddp import GradReducer
    shapes = [(3,), (1,), (223, 289), (60,), (8, 5, 3, 3), (16, 8, 1, 1), (257,), (4, 4)]
    cl = (4, 5)
    gen = torch.Generator().manual_seed(61)
    init = [torch.randn(s, generator=gen) for s in shapes]
    coef = [torch.randn(s, generator=gen) for s in shapes]
    for i in cl:
        init[i] = init[i].contiguous(memory_format=torch.channels_last)
    gpu_p = [x.clone().to(DEV).requires_grad_(True) for x in init]
    coef2 = [(2.0 * c).to(DEV) for c in coef]
    base_p, truth_p = [x.clone() for x in init], [x.double() for x in init]
    hyper = dict(REF_SETTING, lr=1e-3)
    red = GradReducer([(f"p{i}", p) for i, p in enumerate(gpu_p)], bucket_mb=0.05, average=False)
    assert len(red.buckets) >= 2
    opt = fused_adamw()(gpu_p, grad_scale=0.5, **hyper)
    base = torch.optim.AdamW(base_p, foreach=False, **hyper)
    truth = torch.optim.AdamW(truth_p, foreach=False, **hyper)
    for it in range(1, 7):
        used = [i for i in range(len(shapes)) if i != 7 or it % 2 == 1]
        red.zero_grad()
        loss = sum((gpu_p[i] * coef2[i]).sum() for i in used)
        loss.backward()
        red.finish()
        assert any(gpu_p[i].grad.data_ptr() % 16 != 0 for i in used)      # the scalar branch is the one under test
        for i in used:
            assert gpu_p[i].grad.data_ptr() != gpu_p[i].data_ptr() and gpu_p[i].grad._base is not None    # a bucket view
        for i in cl:
            assert gpu_p[i].grad.stride() == gpu_p[i].stride()
        assert not gpu_p[4].grad.is_contiguous()
        assert (gpu_p[7].grad is None) == (it % 2 == 0)
        for i in range(len(shapes)):
            base_p[i].grad = coef[i].clone() if i in used else None
            truth_p[i].grad = coef[i].double() if i in used else None
        opt.step()
        base.step()
        truth.step()
    check_all("reducer_buckets", gpu_p, opt, base_p, base, truth_p, truth)
    assert float(opt.state[gpu_p[7]]["step"]) == 3.0 and float(opt.state[gpu_p[0]]["step"]) == 6.0

