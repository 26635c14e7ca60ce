"""The hand-object interaction loss at the training shape: the GPU time of one ops.interaction_loss forward (hoisdf_interaction_loss_fwd:
2 mesh preparations + 2 vertex passes + the reduction) and of forward + backward (hoisdf_interaction_loss_bwd: 2 launches) at B = 32
and at B = 1, a hand of 778 vertices / 1538 faces and an object of 1000 vertices / 2000 faces per sample, alpha = 10 mm, default
weights (ones).  GPU time by events around `--reps` calls in a row, per call (host = the time for those calls to return, per call:
where it equals the GPU time, the window measures how fast Python issues the call, not the kernels); the median of `--rounds` such
windows after `--warmup` of them.  There is no threshold on these numbers: they are recorded, next to the 72 ms of a training step
at B = 32 and the 1.07 ms of hoisdf_eval_interaction at B = 22 (profiles/interaction_microbench.txt).
Also recorded: the worst ratio of gradient error to its bar on the three samples of tests/test_gpu_interaction_loss.py (the bar:
sum_i |coef_i| beta_ik 2 delta / d_i + 1e-9, delta = 5e-7 m; see that file).
The meshes are those of tools/mb_interaction.py: icospheres with 3 subdivisions (642 vertices, 1280 faces) brought to the stated
counts with copies of vertex 0 and with faces added in cancelling pairs; the hand an ellipsoid of 18 x 10 x 8 cm, the object a ball of
8 cm whose lowest point is 2 cm above the hand's centre, 3 cm off along x, a little different in every sample.
  python tools/mb_interaction_loss.py [--rounds 5] [--out profiles/interaction_loss_microbench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

from hoisdf_amd import interaction_loss_oracle as L
from hoisdf_amd import mesh_sdf_oracle as O
from hoisdf_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--out", type=str, default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
dev = torch.device("cuda", 0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def padded(v, f, V, F):
    """(V, 3) vertices and (F, 3) faces from a closed mesh: copies of vertex 0, faces in cancelling pairs"""
    assert (F - len(f)) % 2 == 0 and F >= len(f) and V >= len(v)
    extra = f[:(F - len(f)) // 2]
    return np.concatenate([v, np.repeat(v[:1], V - len(v), 0)]), np.concatenate([f, extra, extra[:, ::-1]]).astype(np.int32)


v, f = O.icosphere(3)
hv, hf = padded(v * [0.09, 0.05, 0.04], f, 778, 1538)
ov, of = padded(v * 0.04, f, 1000, 2000)
r = np.random.default_rng(0)
B = a.batch
centre = np.array([0.03, -0.02, 0.7])
shift = np.array([0.03, 0.0, 0.06]) + r.uniform(-0.01, 0.01, (B, 3))
hand = torch.from_numpy((hv[None] + centre).astype(np.float32).repeat(B, 0)).to(dev)
obj = torch.from_numpy((ov[None] + centre + shift[:, None]).astype(np.float32)).to(dev)
hand_f, obj_f = torch.from_numpy(hf).to(dev), torch.from_numpy(of).to(dev)
n_verts = torch.full((B,), 642, dtype=torch.int32, device=dev)


def forward(n, grad):
    h, o = hand[:n].clone().requires_grad_(grad), obj[:n].clone().requires_grad_(grad)
    return h, o, ops.interaction_loss(h, hand_f, o, obj_f, None, n_verts[:n], alpha=0.01)


def call(n, backward):
    h, o, vals = forward(n, backward)
    if backward:
        (vals[0] + vals[1] + vals[2]).sum().backward()


def window(n, backward):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.reps):
        call(n, backward)
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps, 1e3 * (t1 - t0) / a.reps


_, _, vals = forward(B, False)
say(f"# hand {hv.shape[0]} vertices / {hf.shape[0]} faces, object {ov.shape[0]} vertices (642 count) / {of.shape[0]} faces, alpha 10 mm; per call, ms: GPU time "
    f"by events around {a.reps} calls in a row / {a.reps}; {a.rounds} windows after {a.warmup} warm-up windows; every call clones both vertex arrays")
say(f"# per sample at B = {B}: rep_hand {1e3 * float(vals[0].mean()):.3f} mm, att {1e3 * float(vals[1].mean()):.3f} mm, rep_obj {1e3 * float(vals[2].mean()):.3f} mm; "
    f"{B * (hv.shape[0] * of.shape[0] + ov.shape[0] * hf.shape[0]):.2e} point-triangle pairs in the two vertex passes")
med = {}
for nb in (B, 1):
    for backward in (False, True):
        name = "forward + backward" if backward else "forward           "
        for _ in range(a.warmup):
            window(nb, backward)
        res = [window(nb, backward) for _ in range(a.rounds)]
        for i, (t, h) in enumerate(res):
            say(f"B = {nb:2d} {name} window {i} gpu {t:8.4f}  host {h:8.4f}")
        t, h = zip(*res)
        med[nb, backward] = statistics.median(t)
        say(f"B = {nb:2d} {name} median gpu {statistics.median(t):8.4f} ms per call (min {min(t):.4f} max {max(t):.4f})  "
            f"host {statistics.median(h):8.4f} (min {min(h):.4f} max {max(h):.4f})")
say(f"B = {B}: forward + backward {med[B, True]:.3f} ms = {100 * med[B, True] / 72.0:.1f} % of the 72 ms training step; forward {med[B, False]:.3f} ms "
    f"against the 1.07 ms of hoisdf_eval_interaction (B = 22, with its voxel pass)")

# the gradient's error against its bar, on the test's own three samples
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_interaction_loss as T

c, got = T.case(), T.result()
worst = 0.0
for b in range(3):
    tol_h, tol_o = L.grad_tolerance(c["ref"][b], T.BAR, 1e-9)
    for d, want, tol in ((got["d_hand"][b], c["ref"][b]["d_hand"], tol_h), (got["d_obj"][b], c["ref"][b]["d_obj"], tol_o)):
        worst = max(worst, float((np.abs(d.astype(np.float64) - want).max(1) / tol).max()))
    say(f"sample {b}: values off by " + ", ".join(f"{k} {abs(float(got[k][b]) - c['ref'][b][k]):.2e} m" for k in ("rep_hand", "att", "rep_obj")) + " (bar 5e-7 m)")
say(f"worst gradient error / bar over the three samples of tests/test_gpu_interaction_loss.py: {worst:.3f}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
