"""The mesh rasteriser at the training shape: the GPU time of ops.raster_meshes = one hoisdf_raster_meshes call (2 launches: setup
over the faces, raster over the pixels) for a MANO-sized hand (1538 faces) and a 2000-face object, a 256 x 256 raster folded to
128 x 128 masks, for B = 22 and B = 1; with all outputs and with the masks alone (what a training step asks for).  GPU time by
events around `--reps` calls in a row, per call (host = the time for those calls to return, per call); the median of `--rounds`
such windows after `--warmup` of them.  There is nothing to compare against - no other rasteriser is installed, and the numpy oracle
is a yardstick for bits, not a baseline - and no threshold on these numbers: they are recorded.
The two kernels apart come from a profiler run of its own (tracing slows the host, so it is not the run that is timed above):
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/mb_raster.py --rounds 1 --warmup 1
  python tools/mb_raster.py --kernel-stats DIR/*/*_kernel_stats.csv --out profiles/raster_microbench.txt      (appends; no GPU needed)
The scene: an icosphere of 1280 faces with 258 of them repeated (1538 rows) as the hand, 9 cm across at 0.7 m; a torus of 40 x 25
quads (2000 faces) as the object, 8 cm across, 3 cm nearer and beside it; K = 600 px focal length: what a DexYCB crop shows.
  python tools/mb_raster.py [--rounds 5] [--out profiles/raster_microbench.txt]"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--batch", type=int, default=22)
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--kernel-stats", type=str, default=None, help="a rocprofv3 *_kernel_stats.csv (or a glob) of a run of this tool")
a = ap.parse_args()
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def finish(mode):
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, mode) as fh:
            fh.write("\n".join(lines) + "\n")


if a.kernel_stats:
    paths = sorted(glob.glob(a.kernel_stats))
    assert paths, f"no file matches {a.kernel_stats}"
    say("# the two kernels apart, from a rocprofv3 --kernel-trace --stats run of this tool (all its calls: both batch sizes, both output sets)")
    for path in paths:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "raster" in r["Name"]:
                    say(f"{r['Name']}: {int(r['Calls'])} calls, average {float(r['AverageNs']) / 1e3:.1f} us "
                        f"(min {float(r['MinNs']) / 1e3:.1f} max {float(r['MaxNs']) / 1e3:.1f})")
    finish("a")
    sys.exit(0)

import numpy as np
import torch

from hoisdf_amd import ops
from hoisdf_amd.mesh_sdf_oracle import icosphere, torus

assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
dev = torch.device("cuda", 0)


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


B, W, H, HM = a.batch, 256, 256, 128
props = torch.cuda.get_device_properties(dev)
say(f"# measured on: {props.name} ({props.multi_processor_count} CUs), torch {torch.__version__}, HIP {torch.version.hip}")
say(f"# {W} x {H} raster, {HM} x {HM} masks; per call, ms: GPU time by events around the {a.reps} calls of a window / their number; "
    f"{a.rounds} windows after {a.warmup} warm-up windows")
hv, hf = icosphere(3)
hf = np.concatenate([hf, hf[:1538 - len(hf)]])
ov, of = torus(40, 25)
r = np.random.default_rng(0)
hand = np.stack([hv * 0.045 + [0, 0, 0.7] + r.uniform(-0.01, 0.01, 3) for _ in range(B)]).astype(np.float32)
obj = np.stack([ov * 0.04 + [0.04, 0.01, 0.67] + r.uniform(-0.01, 0.01, 3) for _ in range(B)]).astype(np.float32)
K = np.tile(np.float32([600, 0, 128, 0, 600, 128]), (B, 1))
d = lambda x, t=None: torch.from_numpy(np.ascontiguousarray(x)).to(dev) if t is None else torch.from_numpy(np.ascontiguousarray(x, t)).to(dev)
hand, hf, obj, of, K = d(hand), d(hf, np.int32), d(obj), d(of, np.int32), d(K)
res = ops.raster_meshes(hand, hf, obj, of, K, W, H, hm_shape=(HM, HM))
say(f"# {hf.shape[0]} + {of.shape[0]} faces; visible pixels per sample, hand / object: {res['counts'][0].tolist()} (sample 0), "
    f"mean {res['counts'].float().mean(0).tolist()}")
for nb in (B, 1):
    args = (hand[:nb], hf, obj[:nb], of, K[:nb], W, H)
    full = {k: v[:nb].contiguous() for k, v in res.items()}
    masks = {k: full[k] for k in ("hand_seg", "obj_seg")}
    t = windows(lambda: ops.raster_meshes(*args, hm_shape=(HM, HM), out=full), a.reps, f"raster_meshes, ids + depth + masks + counts  B = {nb:2d}")
    say(f"    = {nb * W * H / (t * 1e-3) / 1e9:.2f} G pixels / s, {nb * (hf.shape[0] + of.shape[0]) / (t * 1e-3) / 1e6:.1f} M faces / s")
    windows(lambda: ops.raster_meshes(*args, hm_shape=(HM, HM), want=(), out=masks), a.reps, f"raster_meshes, the two masks alone          B = {nb:2d}")
say(f"# workspace of the call at B = {B}: {ops.lib().hoisdf_raster_workspace_bytes(B, hf.shape[0], of.shape[0]) / 1e6:.2f} MB")
finish("w")
