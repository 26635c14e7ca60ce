"""The IK variant's closed-form post-process (hand joints + shape -> MANO pose, joints, mesh): the batched torch restatement
hoisdf_amd/ik.py ik_solver_mano next to ONE HIP launch (ik_solver_mano_native -> hoisdf_ik_mano_fwd), on the same inputs - MANO
joints of random poses + 1e-3 noise in the layout of hand_joints_out (20 rows relative to the wrist), at B = 1 and B = 16.
The two are ALTERNATED in one process; per pair: GPU time by events around the call, host time per call by the host clock (time
to return = issue time), and the wall time to a device synchronise.  There is no threshold on these numbers: they are recorded.
  python tools/mb_ik.py [--pairs 7] [--out profiles/ik_native_vs_torch.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from hoisdf_amd.ik import ik_solver_mano, ik_solver_mano_native
from hoisdf_amd.nets import mano as MANO

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batches", type=str, default="1,16")
ap.add_argument("--out", type=str, default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
dev = torch.device("cuda", 0)


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


say(f"# IK post-process of the IK variant, synthetic MANO asset; {a.pairs} alternated pairs after {a.warmup} warm-up pairs; ms")
say("# gpu = events around the call; host = time for the call to return; wall = until the device is idle")
say("# torch = ik.ik_solver_mano (with the torch.cat that puts the zero wrist row in front); native = ik.ik_solver_mano_native (one launch)")
layer = MANO.ManoLayer(MANO.synthetic_assets(0)).to(dev)
for B in [int(x) for x in a.batches.split(",")]:
    g = torch.Generator().manual_seed(B)
    with torch.no_grad():
        betas = (torch.randn(B, 10, generator=g) * 0.5).to(dev)
        joints = layer((torch.randn(B, 48, generator=g) * 0.25).to(dev), betas)[1] / 1000.0
        joints = joints + 1e-3 * torch.randn(B, 21, 3, generator=g).to(dev)
        hand_joints_out = (joints - joints[:, :1])[:, 1:].contiguous()

    def torch_path():
        hj = torch.cat([torch.zeros_like(hand_joints_out[:, :1]), hand_joints_out], 1)
        return ik_solver_mano(layer, betas, hj)

    def native_path():
        return ik_solver_mano_native(layer, betas, hand_joints_out)

    for _ in range(a.warmup):
        torch_path()
        native_path()
    rows = {"torch": [], "native": []}
    for i in range(a.pairs):
        for name, fn in (("torch", torch_path), ("native", native_path)):
            out, gpu, host, wall = timed(fn)
            rows[name].append((gpu, host, wall))
            say(f"B={B:2d} pair {i} {name:6s} gpu {gpu:8.3f}  host {host:8.3f}  wall {wall:8.3f}")
    t, n = torch_path(), native_path()
    torch.cuda.synchronize()
    say(f"B={B:2d} max |native - torch|: " + ", ".join(f"{k} {float((t[k].float() - n[k].float()).abs().max()):.2e}" for k in ("pose", "joints", "verts", "vis")))
    for name in ("torch", "native"):
        cols = list(zip(*rows[name]))
        say(f"B={B:2d} {name:6s} median gpu {statistics.median(cols[0]):8.3f} (min {min(cols[0]):.3f} max {max(cols[0]):.3f})  "
            f"host {statistics.median(cols[1]):8.3f} (min {min(cols[1]):.3f} max {max(cols[1]):.3f})  "
            f"wall {statistics.median(cols[2]):8.3f} (min {min(cols[2]):.3f} max {max(cols[2]):.3f})")
    say()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
