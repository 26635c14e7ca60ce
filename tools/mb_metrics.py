"""One batch's full evaluation (object metrics + hand-joint metrics + mesh alignment, per-vertex errors into the two accumulators and
F-scores at 5 / 15 mm raw and aligned): metrics.Evaluator.feed over the batched torch functions next to the same call over the
hoisdf_eval_* entries (csrc/eval.hip), on the same synthetic batch - V = 1000 templates, a 778-vertex mesh, P = 200 per-point object
predictions - at B = 22 and B = 1.  The torch feed reads about ten scalars and the F-scores back per batch, the native feed reads nothing.
The two are ALTERNATED in one process; per pair: GPU time by events around the call, host time per call by the host clock (time to
return), and the wall time to a device synchronise.  There is no threshold on these numbers: they are recorded.
  python tools/mb_metrics.py [--pairs 7] [--out profiles/metrics_native_vs_torch.txt]"""
import argparse
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from hoisdf_amd import metrics as M
from hoisdf_amd.config import Config

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batches", type=str, default="22,1")
ap.add_argument("--out", type=str, default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
dev = torch.device("cuda", 0)
V, NV, P, T = 1000, 778, 200, 8


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


say(f"# one batch through metrics.Evaluator.feed (dexycb_full form), {V}-vertex templates, {NV}-vertex mesh, P = {P}; {a.pairs} alternated pairs "
    f"after {a.warmup} warm-up pairs; ms")
say("# gpu = events around the call; host = time for the call to return; wall = until the device is idle")
say("# torch = obj_metrics + eval_hand_joint + rigid_align + MeshEval.feed x 2 + fscore x 4 (reads its batch means back); native = "
    "hoisdf_eval_object + _hand_joints + _mesh + _accum_feed x 2 (8 library launches) + one stacked torch reduction into the running sums; nothing read back")
cfg = Config()
cfg.apply_setting("dexycb_full")                       # dexycb with the mesh block (cfg.eval_mesh)
for B in [int(x) for x in a.batches.split(",")]:
    g = torch.Generator().manual_seed(B)
    r = lambda *s: torch.randn(*s, generator=g)
    templates = (0.05 * r(T, V, 3)).to(dev)
    gt_v, gt_j = 0.05 * r(B, NV, 3), 0.05 * r(B, 21, 3)
    out = {"obj_rot_out": 0.3 * r(B, P, 3), "obj_trans_out": 0.05 * r(B, P, 3), "mano_joints_out": 1.05 * gt_j + 0.004 * r(B, 21, 3),
           "mano_joints_gt_out": gt_j, "mano_mesh_out": 1.05 * gt_v + 0.004 * r(B, NV, 3), "mano_mesh_gt_out": gt_v}
    out = {k: v.to(dev) for k, v in out.items()}
    targets = {"obj_rot": (0.3 * r(B, 3)).to(dev), "rel_obj_trans": (0.05 * r(B, 3)).to(dev)}
    meta = {"mano_root": torch.zeros(B, 3, device=dev)}
    obj_cls = (torch.arange(B) % T).to(dev)
    evs = {"torch": M.Evaluator(cfg, templates, native=False), "native": M.Evaluator(cfg, templates, native=True)}
    for _ in range(a.warmup):
        for ev in evs.values():
            ev.feed(out, targets, meta, obj_cls)
    rows = {"torch": [], "native": []}
    for i in range(a.pairs):
        for name, ev in evs.items():
            _, gpu, host, wall = timed(lambda: ev.feed(out, targets, meta, obj_cls))
            rows[name].append((gpu, host, wall))
            say(f"B={B:2d} pair {i} {name:6s} gpu {gpu:8.3f}  host {host:8.3f}  wall {wall:8.3f}")
    with tempfile.TemporaryDirectory() as d:                      # both saw the same batches: the files they write differ how much?
        txt = {k: open(ev.write(os.path.join(d, k))).read() for k, ev in evs.items()}
    vals = {k: [float(l.split(" :  ")[1]) for l in t.splitlines() if " :  " in l] for k, t in txt.items()}
    say(f"B={B:2d} max |native - torch| over the key : value lines of results.txt [cm]: "
        f"{max(abs(x - y) for x, y in zip(vals['torch'], vals['native'])):.2e}; the mesh and F-score blocks "
        f"{'agree' if txt['torch'].split('Evaluation', 1)[1] == txt['native'].split('Evaluation', 1)[1] else 'DIFFER'} as printed")
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
