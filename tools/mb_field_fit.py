"""Rigid pose refinement against a sampled field at the evaluation shape: the GPU time of ops.field_fit (one hoisdf_field_fit call:
iters + 2 launches of one workgroup of 256 lanes per sample) and the host time to issue it, at n = 64 nodes per axis, V = 778 (the
MANO mesh) and V = 1000 points, iters = 32, for B = 22 and B = 1; next to it the time of the Model.field_values call that feeds it
(coarse grid -> field -> refined grid with cfg.refine_pad_cells -> field; the field queries dominate).  GPU time by events around
`--reps` calls in a row, per call (host = the time for those calls to return, per call); the median of `--rounds` such windows
after `--warmup` of them.  There is no threshold on these numbers: they are recorded.  Expect launch latency, not throughput.
The fit's field is the tanh of a rounded box's distance (the field of tests/test_field_fit_oracle.py on 64 nodes), its points are
points of the box's faces moved by 10 to 45 degrees and 0.05 to 0.2: the samples of a batch stop after different numbers of steps,
and the launches of a stopped sample return at once.  The model is the small deterministic one of the GPU tests (no trained weights
exist): ResNet-18 configuration without the encoder, synthetic pyramid with C = 992 channels, coarse grid of 32 nodes per axis.
  python tools/mb_field_fit.py [--rounds 5] [--out profiles/field_fit_microbench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from hoisdf_amd import field_fit_oracle as F
from hoisdf_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--model-reps", type=int, default=2)
ap.add_argument("--batch", type=int, default=22)
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--iters", type=int, default=32)
ap.add_argument("--out", type=str, default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
dev = torch.device("cuda", 0)
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def windows(fn, reps, label):
    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps, 1e3 * (t1 - t0) / reps

    for _ in range(a.warmup):
        window()
    res = [window() for _ in range(a.rounds)]
    t, h = zip(*res)
    say(f"{label}: median gpu {statistics.median(t):9.4f} ms per call (min {min(t):.4f} max {max(t):.4f})  host {statistics.median(h):9.4f} "
        f"(min {min(h):.4f} max {max(h):.4f})")
    return statistics.median(t)


n, B = a.n, a.batch
say(f"# n = {n} nodes per axis, iters = {a.iters} ({a.iters + 2} launches per call); per call, ms: GPU time by events around the calls of a "
    f"window / their number; {a.rounds} windows after {a.warmup} warm-up windows; {a.reps} calls per window")
# ---- the fit alone -------------------------------------------------------------------------------------------------------------------
g = F.BOX_GRID.copy()
g[3:6] = (np.float64(-2.0) * F.BOX_GRID[:3].astype(np.float64) / (n - 1)).astype(np.float32)
vals = torch.from_numpy(np.stack([F.box_field(g, n)] * B)).to(dev)
grid = torch.from_numpy(np.stack([g] * B)).to(dev)
for V in (778, 1000):
    pts = torch.from_numpy(np.stack([F.box_case(b % 4, count=V, seed=b)["points"] for b in range(B)])).to(dev)
    info = ops.field_fit(vals, grid, n, pts, iters=a.iters)["info"].cpu().numpy()
    say(f"# V = {V}: steps tried per sample min {info[:, 2].min()} max {info[:, 2].max()}, accepted min {info[:, 3].min()} max {info[:, 3].max()}, "
        f"points taking part at the end min {info[:, 1].min()}")
    for nb in (B, 1):
        windows(lambda: ops.field_fit(vals[:nb], grid[:nb], n, pts[:nb], iters=a.iters), a.reps, f"field_fit  V = {V:4d}  B = {nb:2d}")
say(f"# workspace of the call at B = {B}: {ops.lib().hoisdf_field_fit_workspace_bytes(B)} bytes")

# ---- the Model.field_values call that feeds it ---------------------------------------------------------------------------------------
from hoisdf_amd import testing as T
from hoisdf_amd.config import Config
from hoisdf_amd.model import get_model
from hoisdf_amd.nets import mano as MANO

c = Config()
c.resnet_type = 18
c.apply_setting("dexycb")
model = get_model("test", cfg=c, mano_layer=MANO.ManoLayer(MANO.synthetic_assets(0)), with_encoder=False)
sd = model.state_dict()
for k in sd:
    if not k.startswith("mano_head"):
        sd[k] = T.det_param(k, sd[k].shape)
model.load_state_dict(sd)
model = model.to(dev).eval()
pyr_cpu = T.synthetic_pyramid(B, seed=4)
levels = [v.to(dev).permute(0, 2, 3, 1).contiguous() for v in pyr_cpu.values()]
_, _, meta = T.synthetic_batch(B, 300, 8, seed=5)
meta = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in meta.items()}
pad = int(c.refine_pad_cells)
say(f"# Model.field_values(kind='hand', n={n}, coarse_n={n // 2}, pad_cells={pad}), pyramid of {sum(l.shape[-1] for l in levels)} channels, "
    f"chunks of {model.FIELD_CHUNK_ROWS} rows; {a.model_reps} calls per window")
for nb in (B, 1):
    pyr = ops.PyramidNHWC([l[:nb].contiguous() for l in levels])
    m = {k: (v[:nb] if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for k, v in meta.items()}
    windows(lambda: model.field_values(pyr, m, "hand", n, n // 2, pad_cells=pad), a.model_reps, f"Model.field_values  B = {nb:2d}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
