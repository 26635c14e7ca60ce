"""SDF supervision from meshes at the training shape: the GPU time of the composite hoisdf_mesh_sdf_rows (ops.mesh_sdf_rows: 2 mesh
preparations + 2 samplers + 2 point x triangle passes) at B = 32, a hand of 1538 faces + an object of 2000 faces per sample,
4 x (600 + 200) candidate rows per sample (3.6e8 point-triangle pairs), and of the whole MeshSdfSource.make_inputs built on it -
next to SdfStore.make_inputs at the same B and 600 + 200 draws, the path it replaces (rows already in HBM: a draw, no geometry).
The three are ALTERNATED in one process; per round: GPU time by events around the call, host time for the call to return, wall time
to a device synchronise.  There is no threshold on these numbers: they are recorded.  The object is an icosphere with 3 subdivisions
(1280 faces) whose first 720 faces are repeated to reach 2000 rows: the work per pair does not depend on where a triangle lies.
  python tools/mb_mesh_sdf.py [--rounds 7] [--out profiles/mesh_sdf_microbench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from hoisdf_amd import mesh_sdf_oracle as O
from hoisdf_amd import ops
from hoisdf_amd import testing as T
from hoisdf_amd.config import Config
from hoisdf_amd.nets import mano as MANO
from hoisdf_amd.sdf_data import MeshSdfSource, pack_templates, synthetic_store

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--step-ms", type=float, default=72.0, help="the training step this is a share of")
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


B, nh, no = a.batch, 600, 200
c = Config()
c.num_samp_hand, c.num_samp_obj = nh, no
layer = MANO.ManoLayer(MANO.synthetic_assets(0)).to(dev)
v, f = O.icosphere(3)
f2000 = np.concatenate([f, f[:720]])
src = MeshSdfSource(layer, pack_templates([(v, f2000)], 0.05), c)
_, targets, meta = T.synthetic_batch(B, 1, 1, seed=3)
targets, meta = T.to_device(targets, dev), T.to_device(meta, dev)
meta["obj_cls"] = torch.zeros(B, dtype=torch.int64, device=dev)
hand, hf, obj, of, on = src.meshes(targets, meta)
store = synthetic_store(B, rows_hand=4 * nh, rows_obj=4 * no)
frames = list(range(B))
k = c.mesh_sdf_candidates
pairs = B * k * (nh + no) * (hf.shape[0] + of.shape[1])
say(f"# mesh SDF rows at B = {B}: hand {hf.shape[0]} faces, object {of.shape[1]} faces, {k} x ({nh} + {no}) candidates per sample = "
    f"{pairs:.2e} point-triangle pairs; {a.rounds} alternated rounds after {a.warmup} warm-up rounds; ms")
say("# gpu = events around the call; host = time for the call to return; wall = until the device is idle")
say("# rows = ops.mesh_sdf_rows (the composite, 6 launches); source = MeshSdfSource.make_inputs (MANO + object placement + rows + draw);")
say(f"# store = SdfStore.make_inputs on {4 * nh} + {4 * no} precomputed rows per frame (the path replaced: a draw only)")
seed = [0]


def rows_path():
    seed[0] += 1
    return ops.mesh_sdf_rows(hand, hf, obj, of, on, src.vert_label, k * nh, k * no, c.mesh_sdf_sigma, c.mesh_sdf_uniform_every,
                             c.mesh_sdf_pad, c.mesh_sdf_label_clamp, seed[0])


def source_path():
    seed[0] += 1
    return src.make_inputs(targets, meta, nh, no, c.points_filter_dist, c.hand_sdf_scale, c.obj_sdf_scale, train=True, seed=seed[0])


def store_path():
    seed[0] += 1
    return store.make_inputs(frames, meta["mano_root"], meta["obj_center_cam"], nh, no, 0.15, c.hand_sdf_scale, c.obj_sdf_scale,
                             train=True, seed=seed[0])


paths = (("rows", rows_path), ("source", source_path), ("store", store_path))
for _ in range(a.warmup):
    for _, fn in paths:
        fn()
res = {n: [] for n, _ in paths}
for i in range(a.rounds):
    for name, fn in paths:
        _, gpu, host, wall = timed(fn)
        res[name].append((gpu, host, wall))
        say(f"round {i} {name:6s} gpu {gpu:8.3f}  host {host:8.3f}  wall {wall:8.3f}")
med = {}
for name, _ in paths:
    cols = list(zip(*res[name]))
    med[name] = statistics.median(cols[0])
    say(f"{name:6s} median gpu {med[name]:8.3f} (min {min(cols[0]):.3f} max {max(cols[0]):.3f})  "
        f"host {statistics.median(cols[1]):8.3f} (min {min(cols[1]):.3f} max {max(cols[1]):.3f})  "
        f"wall {statistics.median(cols[2]):8.3f} (min {min(cols[2]):.3f} max {max(cols[2]):.3f})")
say(f"rows: {pairs / (med['rows'] * 1e-3) / 1e9:.1f} G point-triangle pairs / s; {100 * med['rows'] / a.step_ms:.1f} % of a {a.step_ms:g} ms step "
    f"(source: {100 * med['source'] / a.step_ms:.1f} %, store: {100 * med['store'] / a.step_ms:.1f} %)")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
