"""The stage after the image encoder, eval: Model.hot_path (Python orchestration) next to Model.infer_native (ONE C-ABI call,
hoisdf_pose_infer) on the same pyramid - the BASELINE.json configs[3] shape (ho3d_render, B = 16, 3072 + 1024 points) and B = 1 of it.
The two are ALTERNATED in one process; per pair: GPU time by events around the call, host time per call by the host clock (time to
return = issue time), and the wall time to a device synchronise.  As in Model.forward, the survivor counts are queued ahead
(infer_counts_begin / infer_native_begin, where a real frame runs its image encoder) and have arrived when the timed call starts;
--counts-inside times the count and its host read with the call (the stand-alone use of either path).
  python tools/mb_pose_infer.py [--pairs 5] [--out profiles/pose_infer_native_vs_python.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from hoisdf_amd import ops, testing as T
from hoisdf_amd.config import Config
from hoisdf_amd.model import get_model
from hoisdf_amd.nets import mano as MANO

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--batches", type=str, default="16,1")
ap.add_argument("--out", type=str, default=None)
ap.add_argument("--counts-inside", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
dev = torch.device("cuda", 0)
nh, no = 3072, 1024


def setup(B):
    c = Config()
    c.resnet_type = 18
    c.apply_setting("ho3d_render")
    c.num_samp_hand, c.num_samp_obj, c.bins_n = nh, no, 64
    model = get_model("test", cfg=c, mano_layer=MANO.ManoLayer(MANO.synthetic_assets(0)), with_encoder=False)
    sd = model.state_dict()
    for k in sd:
        if not k.startswith("mano_head"):
            sd[k] = T.det_param(k, sd[k].shape)
    model.load_state_dict(sd)
    model = model.to(dev).eval()
    pyr = ops.PyramidNHWC([v.to(dev).permute(0, 2, 3, 1).contiguous() for v in T.synthetic_pyramid(B, seed=2).values()])
    inputs, targets, meta = (T.to_device(x, dev) for x in T.synthetic_batch(B, nh, no, seed=21))
    return model, pyr, inputs, targets, meta


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return out, e0.elapsed_time(e1), 1e3 * (t1 - t0), 1e3 * (t2 - t0)


lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


say(f"# eval, ho3d_render (IK variant), {nh} + {no} points, C = 992; {a.pairs} alternated pairs after {a.warmup} warm-up pairs; ms")
say("# gpu = events around the call; host = time for the call to return; wall = until the device is idle; survivor counts "
    + ("queued and read inside the timed call" if a.counts_inside else "queued ahead of the timed call"))
for B in [int(x) for x in a.batches.split(",")]:
    model, pyr, inputs, targets, meta = setup(B)

    def python_begin():
        return None if a.counts_inside else model.infer_counts_begin(meta)

    def python_path(ic=None):
        with torch.no_grad():
            return model.hot_path(pyr, inputs, targets, meta, "eval", infer_counts=ic)[1]

    def native_begin():
        return None if a.counts_inside else model.infer_native_begin(meta, pyr.C)

    def native_path(ic=None):
        return model.infer_native(pyr, meta, ic)

    for _ in range(a.warmup):
        python_path()
        native_path()
    rows = {"python": [], "native": []}
    for i in range(a.pairs):
        for name, begin, fn in (("python", python_begin, python_path), ("native", native_begin, native_path)):
            ic = begin()
            out, gpu, host, wall = timed(lambda: fn(ic))
            rows[name].append((gpu, host, wall))
            say(f"B={B:2d} pair {i} {name:6s} gpu {gpu:8.3f}  host {host:8.3f}  wall {wall:8.3f}")
    py, na = python_path(), native_path()
    torch.cuda.synchronize()
    diff = {k: float((py[k] - na[k]).abs().max()) for k in na if k in py}
    say(f"B={B:2d} max |native - python| per output: " + ", ".join(f"{k} {v:.2e}" for k, v in diff.items()))
    for name in ("python", "native"):
        cols = list(zip(*rows[name]))
        say(f"B={B:2d} {name:6s} median gpu {statistics.median(cols[0]):8.3f} (min {min(cols[0]):.3f} max {max(cols[0]):.3f})  "
            f"host {statistics.median(cols[1]):8.3f} (min {min(cols[1]):.3f} max {max(cols[1]):.3f})  "
            f"wall {statistics.median(cols[2]):8.3f} (min {min(cols[2]):.3f} max {max(cols[2]):.3f})")
    say()
    del model, pyr
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
