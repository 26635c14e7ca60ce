"""Surface from the learned field at the evaluation shape: the GPU time of the extraction alone (ops.iso_surface = one
hoisdf_iso_extract call with fixed capacities: count, scan, vertices, faces; and the count-only call) and of Model.field_surface as a
whole (coarse grid -> field -> refined grid -> field -> extraction; the field queries dominate), at n = 64 nodes per axis, for B = 1
and B = 22.  GPU time by events around `--reps` calls in a row, per call (host = the time for those calls to return, per call); the
median of `--rounds` such windows after `--warmup` of them.  There is no threshold on these numbers: they are recorded.
The extraction's field is a sphere that fills 80 % of the grid's width, a little different in every sample (about the vertex count
a hand gives over its own box).  The model is the small deterministic one of the GPU tests (no trained weights exist): ResNet-18
configuration without the encoder, synthetic pyramid with C = 992 channels, coarse grid of 32 nodes per axis.
  python tools/mb_iso_surface.py [--rounds 5] [--out profiles/iso_surface_microbench.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from hoisdf_amd import isosurf_oracle as iso
from hoisdf_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--model-reps", type=int, default=2)
ap.add_argument("--batch", type=int, default=22)
ap.add_argument("--n", type=int, default=64)
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
say(f"# n = {n} nodes per axis ({n ** 3} nodes per sample); per call, ms: GPU time by events around the calls of a window / their number; "
    f"{a.rounds} windows after {a.warmup} warm-up windows")
# ---- the extraction alone ------------------------------------------------------------------------------------------------------------
g = iso.cube_grid(-1.0, 1.0, n)
p = iso.grid_points(g, n, np.float64)
r = np.random.default_rng(0)
vals = torch.from_numpy(np.stack([iso.sphere_field(p, r.uniform(-0.05, 0.05, 3), 0.8 + 0.01 * r.uniform(-1, 1)) for _ in range(B)])).to(dev)
grid = torch.from_numpy(np.stack([g] * B)).to(dev)
_, _, nv, nf = ops.iso_surface(vals, grid, n)
mv, mf = int(nv.max()), int(nf.max())
say(f"# extraction: a sphere of 80 % of the grid's width; vertices per sample min {int(nv.min())} max {mv}, faces min {int(nf.min())} max {mf}; "
    f"{a.reps} calls per window")
nws = ops.lib().hoisdf_iso_extract_workspace_bytes(B, n)
for nb in (B, 1):
    t = windows(lambda: ops.iso_surface(vals[:nb], grid[:nb], n, 0.0, mv, mf), a.reps, f"iso_surface (4 launches + 2 output fills)  B = {nb:2d}")
    say(f"    = {nb * n ** 3 / (t * 1e-3) / 1e9:.2f} G nodes / s; the field is {nb * n ** 3 * 4 / 1e6:.1f} MB, read by 3 of the 4 kernels")
say(f"# workspace of the call at B = {B}: {nws / 1e6:.1f} MB")

# ---- Model.field_surface as a whole ----------------------------------------------------------------------------------------------------
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
cap = int(c.field_max_verts)
say(f"# Model.field_surface(kind='hand', n={n}, coarse_n={n // 2}) with capacities {cap} / {2 * cap} (no read-back), pyramid of "
    f"{sum(l.shape[-1] for l in levels)} channels, "
    f"chunks of {model.FIELD_CHUNK_ROWS} rows; {a.model_reps} calls per window")
for nb in (B, 1):
    pyr = ops.PyramidNHWC([l[:nb].contiguous() for l in levels])
    m = {k: (v[:nb] if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for k, v in meta.items()}
    out = model.field_surface(pyr, m, "hand", n, n // 2, max_verts=cap, max_faces=2 * cap)
    say(f"# B = {nb}: vertices needed per sample {out[2].tolist()[:4]}{' ...' if nb > 4 else ''}")
    windows(lambda: model.field_surface(pyr, m, "hand", n, n // 2, max_verts=cap, max_faces=2 * cap), a.model_reps,
            f"Model.field_surface  B = {nb:2d}")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
