"""-m gpu: the hand-object interaction loss (csrc/interact_loss.hip: hoisdf_interaction_loss_fwd / _bwd; ops.interaction_loss;
cfg.interaction_loss in Model / Trainer) against the fp64 numpy restatement hoisdf_amd/interaction_loss_oracle.py on procedural
meshes at hand size and camera depth (about (0.03, -0.02, 0.7) m, as tests/test_gpu_mesh_sdf.py).

The bars.  Values: within 5e-7 m of fp64 - the project's bar for mesh-SDF distances, and every term is 1-Lipschitz in sdf, a
weighted mean of such terms too.  Gradients: per destination vertex u, sum_i |coef_i| beta_ik 2 delta / d_i + 1e-9 with delta = 5e-7 m
over the query points i that contribute to u (its own term, beta = 1, included): a closest point displaced by delta turns
n = (p - c) / d by at most 2 delta / d (interaction_loss_oracle.grad_tolerance).  Condition: a query point whose fp64 |sdf| < 1e-4 m
or whose winding number is within 0.05 of 0.5 has no binding answer; it gets weight 0 in all its terms through the per-sample
weight arrays, in the oracle and in the kernel alike, and at most 5 % of a sample's query points may be such (asserted; the seed
below has one, a hand vertex of sample 2 that lies 0.09 mm inside the box).

One call of B = 3, every mesh jittered by 0.2 mm and the pair overlapping by about 10 mm:
  0  icosphere (162 vertices = three LDS tiles of 64, the last partial; 320 faces) of 40 mm x icosphere of 30 mm
  1  icosphere x torus (192 vertices = three full tiles, 384 faces)
  2  icosphere x box (150 of 192 vertex rows, 192 of 384 face rows: the padding vertex rows sit INSIDE the hand)"""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch

from hoisdf_amd import interaction_loss_oracle as L
from hoisdf_amd import mesh_sdf_oracle as O
from hoisdf_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAR, ALPHA = 5e-7, 0.01
CENTRE = np.array([0.03, -0.02, 0.7])
G = np.array([[0.7, 1.3, 0.9], [1.1, 0.6, 1.4], [0.8, 1.2, 0.5]])      # upstream gradients [sample][rep_hand, att, rep_obj]
SEED = 5


def samples(seed=SEED):
    r = np.random.default_rng(seed)
    jit = lambda v: (v + r.normal(0, 0.0002, v.shape)).astype(np.float32)
    ico, torus, box = O.icosphere(2), O.torus(), O.box()
    hand = lambda: jit(ico[0] * 0.04 + CENTRE)
    return [(hand(), ico[1], jit(ico[0] * 0.03 + CENTRE + [0.06, 0.004, -0.003]), ico[1]),
            (hand(), ico[1], jit(torus[0] * 0.04 + CENTRE + [0.07, 0.004, -0.003]), torus[1]),
            (hand(), ico[1], jit(box[0] * 0.04 + CENTRE + [0.07, 0.004, -0.003]), box[1])]


def pack(smp):
    B, Vo, Fo = len(smp), max(len(s[2]) for s in smp), max(len(s[3]) for s in smp)
    c = dict(hv=np.stack([s[0] for s in smp]), hf=np.asarray(smp[0][1], np.int32), ov=np.zeros((B, Vo, 3), np.float32),
             of=np.full((B, Fo, 3), 2 ** 30, np.int32), on=np.zeros(B, np.int32), onv=np.zeros(B, np.int32))
    for b, (hv, _, ov, of) in enumerate(smp):
        c["ov"][b, :len(ov)], c["of"][b, :len(of)], c["on"][b], c["onv"][b] = ov, of, len(of), len(ov)
        c["ov"][b, len(ov):] = hv.mean(0)                      # padding rows: in the middle of the hand
    return c


_CASE = {}


def case():
    """the arrays of the call, the weights (random in 0.5 .. 1.5, 0 on near-surface points) and the fp64 oracle's answer per sample
    with the upstream gradients G: computed once, never changed"""
    if not _CASE:
        assert ops._lib.CONSTANTS["INTERACT_LOSS_TILE"] == 64
        c = pack(samples())
        B, Vh, Vo = 3, c["hv"].shape[1], c["ov"].shape[1]
        assert (Vh, Vo, c["hf"].shape[0], c["of"].shape[1]) == (162, 192, 320, 384) and c["onv"].tolist() == [162, 192, 150]
        r = np.random.default_rng(17)
        c["wr"], c["wa"], c["wo"] = (r.uniform(0.5, 1.5, (B, n)).astype(np.float32) for n in (Vh, Vh, Vo))
        c["ref"] = []
        for b in range(B):
            faces = c["of"][b, :c["on"][b]]
            plain = L.interaction_loss(c["hv"][b], c["hf"], c["ov"][b], faces, int(c["onv"][b]), alpha=ALPHA)
            near_h, near_o = L.near_surface(plain["hand_q"]), L.near_surface(plain["obj_q"])
            print(f"sample {b}: near-surface query points: {int(near_h.sum())} of {Vh} hand, {int(near_o.sum())} of {int(c['onv'][b])} object")
            assert near_h.sum() <= 0.05 * Vh and near_o.sum() <= 0.05 * c["onv"][b]
            c["wr"][b, near_h] = c["wa"][b, near_h] = 0
            c["wo"][b, :len(near_o)][near_o] = 0
            ref = L.interaction_loss(c["hv"][b], c["hf"], c["ov"][b], faces, int(c["onv"][b]), c["wr"][b], c["wa"][b], c["wo"][b], ALPHA, *G[b])
            assert (ref["hand_q"]["sdf"] < 0).sum() >= 4 and (ref["obj_q"]["sdf"] < 0).sum() >= 4 and ref["rep_hand"] > 1e-4 and ref["rep_obj"] > 1e-4
            c["ref"].append(ref)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASE.update(c)
    return _CASE


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(c, rows=slice(None), weights=True):
    """values and both gradients of sum_b G[b] . (rep_hand, att, rep_obj)[b] for the samples `rows` -> numpy arrays"""
    hv, ov = gpu(c["hv"][rows]).requires_grad_(), gpu(c["ov"][rows]).requires_grad_()
    w = [gpu(c[k][rows]) for k in ("wr", "wa", "wo")] if weights else [None] * 3
    vals = ops.interaction_loss(hv, gpu(c["hf"]), ov, gpu(c["of"][rows]), torch.from_numpy(c["on"][rows]), torch.from_numpy(c["onv"][rows]),
                                w[0], w[1], w[2], ALPHA)
    g = gpu(G[rows].astype(np.float32))
    (torch.stack(vals, 1) * g).sum().backward()
    torch.cuda.synchronize()
    return {"rep_hand": vals[0].detach().cpu().numpy(), "att": vals[1].detach().cpu().numpy(), "rep_obj": vals[2].detach().cpu().numpy(),
            "d_hand": hv.grad.cpu().numpy(), "d_obj": ov.grad.cpu().numpy()}


_RUN = {}


def result():
    if not _RUN:
        _RUN.update(run(case()))
    return _RUN


def test_values_against_the_oracle():
    c, got = case(), result()
    for b in range(3):
        for k in ("rep_hand", "att", "rep_obj"):
            err = abs(float(got[k][b]) - c["ref"][b][k])
            print(f"sample {b}: {k} = {got[k][b]:.7f} m, fp64 {c['ref'][b][k]:.7f} m, off by {err:.2e} m")
            assert err <= BAR, (b, k, err)


def test_gradients_against_the_oracle():
    c, got = case(), result()
    worst = 0.0
    for b in range(3):
        ref = c["ref"][b]
        tol_h, tol_o = L.grad_tolerance(ref, BAR, 1e-9)
        for name, d, want, tol in (("hand", got["d_hand"][b], ref["d_hand"], tol_h), ("object", got["d_obj"][b], ref["d_obj"], tol_o)):
            err = np.abs(d.astype(np.float64) - want).max(1)
            ratio = float((err / tol).max())
            worst = max(worst, ratio)
            print(f"sample {b}, {name}: largest gradient {np.abs(want).max():.3e}, largest error {err.max():.2e}, worst error / bar {ratio:.3f}, "
                  f"{int((np.abs(want).max(1) > 0).sum())} of {len(want)} rows non-zero")
            assert (err <= tol).all(), (b, name, ratio)
            assert np.abs(want).max() > 1e-3 and np.median(tol) < 1e-2 * np.abs(want).max()        # the bar means something
        assert not got["d_obj"][b, c["onv"][b]:].any()            # padding rows: exactly zero
    print(f"worst error / bar over the three samples: {worst:.3f}")


def test_two_calls_give_the_same_bits():
    first, again = result(), run(case())
    for k in first:
        assert np.array_equal(first[k].view(np.uint32), again[k].view(np.uint32)), k


def test_a_batch_is_its_samples():
    c, got = case(), result()
    for b in range(3):
        one = run(c, slice(b, b + 1))
        for k in got:
            assert one[k].shape[0] == 1 and np.array_equal(one[k].view(np.uint32), got[k][b:b + 1].view(np.uint32)), (b, k)


def test_shared_weights_and_none_are_the_same_as_their_expansion():
    c = case()
    ones = dict(c, wr=np.ones_like(c["wr"]), wa=np.ones_like(c["wa"]), wo=np.ones_like(c["wo"]))
    a, b = run(ones), run(c, weights=False)
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    hv, ov = gpu(c["hv"]), gpu(c["ov"])
    args = (gpu(c["hf"]), ov, gpu(c["of"]), torch.from_numpy(c["on"]), torch.from_numpy(c["onv"]))
    shared = ops.interaction_loss(hv, *args, gpu(c["wr"][0]), gpu(c["wa"][0]), gpu(c["wo"][0]), ALPHA)
    tiled = ops.interaction_loss(hv, *args, *(gpu(np.repeat(c[k][:1], 3, 0)) for k in ("wr", "wa", "wo")), ALPHA)
    for s, t in zip(shared, tiled):
        assert torch.equal(s, t)


def test_edge_cases():
    c = case()
    hv, ov = c["hv"].copy(), c["ov"].copy()
    hv[1, 7] = ov[1, 11]                                       # a hand vertex exactly on an object vertex: d = 0
    on = c["on"].copy()
    on[2] = 0                                                  # an object without faces
    h, o = gpu(hv).requires_grad_(), gpu(ov).requires_grad_()
    vals = ops.interaction_loss(h, gpu(c["hf"]), o, gpu(c["of"]), torch.from_numpy(on), torch.from_numpy(c["onv"]), alpha=ALPHA)
    torch.stack(vals).sum().backward()
    torch.cuda.synchronize()
    for t in (*vals, h.grad, o.grad):
        assert torch.isfinite(t).all()
    assert all(float(v[2]) == 0 for v in vals) and not h.grad[2].any() and not o.grad[2].any()
    ref = L.interaction_loss(hv[1], c["hf"], ov[1], c["of"][1, :on[1]], int(c["onv"][1]), alpha=ALPHA)
    assert ref["hand_q"]["dist"][7] == 0 and ref["hand_q"]["coef"][7] == 0
    assert abs(float(vals[0][1]) - ref["rep_hand"]) <= BAR and abs(float(vals[1][1]) - ref["att"]) <= BAR
    # the vertex on the surface has no direction of its own; as a corner of the object it still receives what others pass on
    far = L.near_surface(ref["hand_q"]) | (np.arange(162) == 7)
    if not L.near_surface(ref["obj_q"]).any() and far.sum() == 1:
        tol_h, tol_o = L.grad_tolerance(ref, BAR, 1e-9)
        assert (np.abs(h.grad[1].cpu().numpy() - ref["d_hand"]).max(1) <= tol_h).all()
        assert (np.abs(o.grad[1].cpu().numpy() - ref["d_obj"]).max(1) <= tol_o).all()
    assert not o.grad[2, 150:].any() and not o.grad[0, 162:].any()
    # no upstream gradient for a term: its share is left out, not read
    h2, o2 = gpu(c["hv"]).requires_grad_(), gpu(c["ov"]).requires_grad_()
    v2 = ops.interaction_loss(h2, gpu(c["hf"]), o2, gpu(c["of"]), torch.from_numpy(c["on"]), torch.from_numpy(c["onv"]), alpha=ALPHA)
    v2[2].sum().backward()
    r0 = L.interaction_loss(c["hv"][0], c["hf"], c["ov"][0], c["of"][0, :c["on"][0]], int(c["onv"][0]), alpha=ALPHA, g_rep_hand=0.0, g_att=0.0)
    tol_h, tol_o = L.grad_tolerance(r0, BAR, 1e-9)
    assert (np.abs(h2.grad[0].cpu().numpy() - r0["d_hand"]).max(1) <= tol_h).all() and (np.abs(o2.grad[0].cpu().numpy() - r0["d_obj"]).max(1) <= tol_o).all()
    with pytest.raises(ValueError):
        ops.interaction_loss(gpu(c["hv"]), gpu(c["hf"]), gpu(c["ov"][:2]), gpu(c["of"]))
    with pytest.raises(ValueError, match="rep_w_hand"):
        ops.interaction_loss(gpu(c["hv"]), gpu(c["hf"]), gpu(c["ov"]), gpu(c["of"]), rep_w_hand=torch.ones(5))
    with pytest.raises(ops._lib.HoisdfError, match="alpha"):
        ops.interaction_loss(gpu(c["hv"]), gpu(c["hf"]), gpu(c["ov"]), gpu(c["of"]), alpha=0.0)


STEPS, STEP = 8, 0.02                                          # of the descent: fixed with the oracle below, before any GPU run


def _descent(grad_and_pen, t0):
    t, pens = t0.copy(), []
    for _ in range(STEPS):
        g, pen = grad_and_pen(t)
        pens.append(pen)
        t = t - STEP * g
    pens.append(grad_and_pen(t)[1])
    return pens


def test_descent_on_the_repulsion_pulls_the_object_out():
    """the object's translation moved along -d(rep_hand + rep_obj)/dt: pen_hand of ops.eval_interaction ends below its start.  The
    steps were fixed with the oracle: on the CPU it brings pen_hand of sample 0 from about 10 mm to under half of that"""
    c = case()
    hv, hf, ov, of = c["hv"][0], c["hf"], c["ov"][0, :162], c["of"][0, :320]

    def cpu(t):
        r = L.interaction_loss(hv, hf, ov + t, of, alpha=ALPHA, g_att=0.0)
        return r["d_obj"].sum(0), float(np.maximum(0, -r["hand_q"]["sdf"]).max())

    def device(t):
        o = gpu((ov + t).astype(np.float32)[None]).requires_grad_()
        v = ops.interaction_loss(gpu(hv[None]), gpu(hf), o, gpu(of))
        (v[0] + v[2]).sum().backward()
        pen = ops.eval_interaction(gpu(hv[None]), gpu(hf), o.detach(), gpu(of))["pen_hand"]
        return o.grad[0].sum(0).double().cpu().numpy(), float(pen)

    want = _descent(cpu, np.zeros(3))
    assert want[0] > 0.008 and want[-1] < 0.5 * want[0], want
    got = _descent(device, np.zeros(3))
    print("pen_hand along the descent, oracle:", np.round(want, 5), "\npen_hand along the descent, GPU:   ", np.round(got, 5))
    assert got[-1] < got[0] and got[-1] < 0.5 * got[0] + 1e-4


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _trainer_step(on):
    from hoisdf_amd.config import Config
    from hoisdf_amd.engine import Trainer
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = 96, 32
    c.sdf_source = "mesh"
    c.interaction_loss = on
    tr = Trainer(c, torch.device("cuda", 0), batch_size=2, tune_encoder=False)
    inputs, targets, meta = next(iter(tr.batch_generator))
    total, loss = tr.train_step(inputs, targets, meta, 0, 0.0)
    torch.cuda.synchronize()
    grads = {n: torch.cat([p.grad.detach().flatten().clone() for p in getattr(tr.model, n).parameters()]) for n in ("linear_pose", "linear_obj_rot")}
    return tr, float(total), {k: float(v) for k, v in loss.items()}, grads


def test_one_trainer_step_with_and_without_the_loss(monkeypatch):
    monkeypatch.delenv("HOISDF_INTERACTION_LOSS", raising=False)
    was = ops.deterministic()
    ops.set_deterministic(True)                                # order-fixed gradients: a difference below is the loss's, not the atomics'
    det, bench = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False      # and the encoder's convolutions likewise
    try:
        _, total_off, loss_off, g_off = _trainer_step(False)
        _, total_off2, loss_off2, g_off2 = _trainer_step(False)
        tr, total_on, loss_on, g_on = _trainer_step(True)
    finally:
        ops.set_deterministic(was)
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = det, bench
    assert "interaction_rep" not in loss_off and "interaction_att" not in loss_off and tr.interaction_source is tr.sdf_source
    assert set(loss_on) == set(loss_off) | {"interaction_rep", "interaction_att"}
    assert loss_off == loss_off2, {k: (v, loss_off2[k]) for k, v in loss_off.items() if v != loss_off2[k]}
    assert struct.pack("<d", total_off) == struct.pack("<d", total_off2)
    print("interaction_rep", loss_on["interaction_rep"], "interaction_att", loss_on["interaction_att"], "total", total_on, "without", total_off)
    assert np.isfinite(loss_on["interaction_rep"]) and np.isfinite(loss_on["interaction_att"]) and np.isfinite(total_on)
    assert loss_on["interaction_rep"] >= 0 and loss_on["interaction_att"] > 0
    for n in g_off:
        assert torch.equal(g_off[n], g_off2[n]), n
        assert torch.isfinite(g_on[n]).all() and not torch.equal(g_on[n], g_off[n]), n
    # and a second step in the default mode: the loss then runs on the model's second stream, next to the vote heads
    inputs, targets, meta = next(iter(tr.batch_generator))
    total, loss = tr.train_step(inputs, targets, meta, 0, 0.0)
    torch.cuda.synchronize()
    print("default mode, two streams:", tr.model._side_stream is not None, "interaction_rep", float(loss["interaction_rep"]),
          "interaction_att", float(loss["interaction_att"]))
    assert bool(torch.isfinite(total)) and bool(torch.isfinite(loss["interaction_rep"])) and bool(torch.isfinite(loss["interaction_att"]))
    assert all(torch.isfinite(p.grad).all() for p in tr.model.linear_pose.parameters())


def test_the_ik_variant_refuses_the_loss():
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import get_model
    c = Config()
    c.resnet_type = 18
    c.apply_setting("ho3d_render")
    c.interaction_loss = True
    with pytest.raises(ValueError, match="interaction_loss"):
        get_model("train", cfg=c, with_encoder=False)


# ---- C host ----------------------------------------------------------------------------------------------------------------------
def test_c_host_interaction_loss(tmp_path):
    """A plain C host (tests/c/test_interaction_loss_host.c: one forward and one backward call on the dumped three-sample case) gets
    the bits the Python call gets"""
    c, got = case(), result()

    def arr(f, a, dt):
        a = np.ascontiguousarray(a).reshape(-1).astype(dt)
        f.write(struct.pack("<q", a.size))
        f.write(a.tobytes())

    src, dst = str(tmp_path / "interaction_loss_in.bin"), str(tmp_path / "interaction_loss_out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<5i1f", 3, 162, 320, 192, 384, ALPHA))
        arr(f, c["hv"], "<f4"), arr(f, c["hf"], "<i4"), arr(f, c["ov"], "<f4"), arr(f, c["of"], "<i4"), arr(f, c["on"], "<i4")
        arr(f, c["onv"], "<i4"), arr(f, c["wr"], "<f4"), arr(f, c["wa"], "<f4"), arr(f, c["wo"], "<f4"), arr(f, G.T, "<f4")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "hoisdf_test_interaction_loss_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "hip", os.path.join(repo, "tests", "c", "test_interaction_loss_host.c"), "-I",
                    os.path.join(repo, "include"), "-L", os.path.join(repo, "hoisdf_amd"), "-lhoisdf_hip",
                    "-Wl,-rpath," + os.path.join(repo, "hoisdf_amd"), "-o", exe], check=True, capture_output=True, timeout=300)
    res = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0 and "c host interaction loss ok" in res.stdout, res.stdout + res.stderr
    words = np.fromfile(dst, dtype="<u4")
    assert len(words) == 9 + 3 * 162 * 3 + 3 * 192 * 3
    for i, k in enumerate(("rep_hand", "att", "rep_obj")):
        assert np.array_equal(words[3 * i:3 * i + 3], got[k].view(np.uint32)), k
    assert np.array_equal(words[9:9 + 1458], got["d_hand"].reshape(-1).view(np.uint32))
    assert np.array_equal(words[9 + 1458:], got["d_obj"].reshape(-1).view(np.uint32))
