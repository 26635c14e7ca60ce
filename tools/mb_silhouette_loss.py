"""The silhouette loss at the training shape: the GPU time of ops.mask_edt (hoisdf_mask_edt: 2 launches) and of the pair of
ops.silhouette_loss calls a training step makes - the hand's 778 vertices and the object's 1000 (642 of them counting) against 128 x
128 masks - forward (hoisdf_silhouette_loss_fwd: 3 launches each) and forward + backward (hoisdf_silhouette_loss_bwd: 1 launch each), at
B = 32 and at B = 1.  GPU time by events around `--reps` calls in a row, per call (host = the time for those calls to return, per
call: where it equals the GPU time, the window measures how fast Python issues the call, not the kernels); the median of `--rounds`
such windows after `--warmup` of them.  There is no threshold on these numbers: they are recorded, next to the 72 ms of a training
step at B = 32 and the 0.83 ms of the interaction loss's forward + backward (profiles/interaction_loss_microbench.txt).
The scene: the ellipsoid hand (18 x 10 x 8 cm) and the ball (8 cm) of tools/mb_interaction_loss.py at 0.7 m, a focal length of 250
mask pixels; the masks are an ellipse and a disk of about their projected size, the hand's shifted by three pixels and cut by the
object's (modal masks); allow = the union.
  python tools/mb_silhouette_loss.py [--rounds 5] [--out profiles/silhouette_loss_microbench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np
import torch

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


v, _ = O.icosphere(3)
r = np.random.default_rng(0)
B, S, F = a.batch, 128, 250.0
centre = np.array([0.03, -0.02, 0.7])
hv = np.concatenate([v * [0.09, 0.05, 0.04], np.repeat(v[:1] * [0.09, 0.05, 0.04], 778 - len(v), 0)])
ov = np.concatenate([v * 0.04, np.repeat(v[:1] * 0.04, 1000 - len(v), 0)])
shift = np.array([0.03, 0.0, 0.06]) + r.uniform(-0.01, 0.01, (B, 3))
hand = torch.from_numpy((hv[None] + centre).astype(np.float32).repeat(B, 0)).to(dev)
obj = torch.from_numpy((ov[None] + centre + shift[:, None]).astype(np.float32)).to(dev)
n_verts = torch.full((B,), 642, dtype=torch.int32, device=dev)
K = torch.tensor([F, 0, S / 2 - F * centre[0] / centre[2], 0, F, S / 2 - F * centre[1] / centre[2]], dtype=torch.float32).repeat(B, 1).to(dev)
yy, xx = np.mgrid[0:S, 0:S]
hand_seg = ((((xx - S / 2 - 3) / (F * 0.09 / 0.7)) ** 2 + ((yy - S / 2) / (F * 0.05 / 0.7)) ** 2) <= 1).astype(np.float32)
obj_c = S / 2 + F * shift[:, :2] / (0.7 + shift[:, 2:3])
obj_seg = (((xx[None] - obj_c[:, 0, None, None]) ** 2 + (yy[None] - obj_c[:, 1, None, None]) ** 2) <= (F * 0.04 / 0.76) ** 2).astype(np.float32)
obj_seg = torch.from_numpy(obj_seg).to(dev)
hand_seg = torch.from_numpy(np.repeat(hand_seg[None], B, 0)).to(dev) * (1 - obj_seg)      # modal: the ball hides a part of the hand
allow = ops.mask_edt(hand_seg, obj_seg)


def pair(n, grad):
    h, o = hand[:n].clone().requires_grad_(grad), obj[:n].clone().requires_grad_(grad)
    vh = ops.silhouette_loss(h, K[:n], allow[:n], hand_seg[:n])
    vo = ops.silhouette_loss(o, K[:n], allow[:n], obj_seg[:n], n_verts=n_verts[:n])
    if grad:
        (vh[0] + vh[1] + vo[0] + vo[1]).sum().backward()
    return vh, vo


CALLS = {"edt               ": lambda n: ops.mask_edt(hand_seg[:n], obj_seg[:n]), "forward           ": lambda n: pair(n, False),
         "forward + backward": lambda n: pair(n, True)}


def window(n, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(a.reps):
        fn(n)
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / a.reps, 1e3 * (t1 - t0) / a.reps


vh, vo = pair(B, False)
say(f"# hand 778 vertices, object 1000 vertices (642 count), masks {S} x {S}; per call, ms: GPU time by events around {a.reps} calls in a row / "
    f"{a.reps}; {a.rounds} windows after {a.warmup} warm-up windows; forward = the hand's call and the object's; every call clones both vertex arrays")
say(f"# per sample at B = {B}: hand inside {float(vh[0].mean()):.3f} px, cover {float(vh[1].mean()):.3f} px; object inside {float(vo[0].mean()):.3f} px, "
    f"cover {float(vo[1].mean()):.3f} px; set pixels per sample: hand {float(hand_seg.sum()) / B:.0f}, object {float(obj_seg.sum()) / B:.0f}")
med = {}
for nb in (B, 1):
    for name, fn in CALLS.items():
        for _ in range(a.warmup):
            window(nb, fn)
        res = [window(nb, fn) for _ in range(a.rounds)]
        for i, (t, h) in enumerate(res):
            say(f"B = {nb:2d} {name} window {i} gpu {t:8.4f}  host {h:8.4f}")
        t, h = zip(*res)
        med[nb, name.strip()] = statistics.median(t)
        say(f"B = {nb:2d} {name} median gpu {statistics.median(t):8.4f} ms per call (min {min(t):.4f} max {max(t):.4f})  "
            f"host {statistics.median(h):8.4f} (min {min(h):.4f} max {max(h):.4f})")
for nb in (B, 1):
    both = med[nb, "edt"] + med[nb, "forward + backward"]
    say(f"B = {nb}: edt {med[nb, 'edt']:.3f} ms, forward {med[nb, 'forward']:.3f} ms, forward + backward {med[nb, 'forward + backward']:.3f} ms; edt + forward + "
        f"backward {both:.3f} ms" + (f" = {100 * both / 72.0:.1f} % of the 72 ms training step; the interaction loss's forward + backward: 0.83 ms" if nb == B else ""))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
