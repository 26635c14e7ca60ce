"""Hand-object interaction metrics at the evaluation shape: the GPU time of one hoisdf_eval_interaction call (ops.eval_interaction: 2
mesh preparations + 2 vertex passes + the voxel pass + the reduction) at B = 22 and at B = 1, a hand of 778 vertices / 1538 faces and
an object of 1000 vertices / 2000 faces per sample, 5 mm voxels and 5 mm contact distance.  GPU time by events around `--reps` calls
in a row, per call (host = the time for those calls to return, per call: where it equals the GPU time, the window measures how
fast Python issues the call, not the kernels); the median of `--rounds` such windows after `--warmup` of them.  Also recorded: the cells per sample, the
point-triangle pairs that stand for, and the share of the voxel kernel's workgroups (64 cells each) that skipped the hand pass because
none of their cells was inside the object - taken from ops.mesh_sdf's winding numbers at the same cell centres.  There is no
threshold on these numbers: they are recorded.
The meshes: both are icospheres with 3 subdivisions (642 vertices, 1280 faces) brought to the stated counts with copies of vertex 0
and with faces added in cancelling pairs (a face and its mirror image: the same work per pair, no change of the winding number).  The
hand is an ellipsoid of 18 x 10 x 8 cm.  Two objects are measured: a ball of 8 cm (a grasp: the overlap of the bounding boxes is a
fraction of the hand's box) whose lowest point is 2 cm above the hand's centre, and a ball of 20 cm whose lowest point is 2 cm below
it (the overlap is most of the hand's box: the upper bound of the work); 3 cm off along x, a little different in every sample.
  python tools/mb_interaction.py [--rounds 5] [--out profiles/interaction_microbench.txt]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--batch", type=int, default=22)
ap.add_argument("--voxel", type=float, default=0.005)
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


def measure(radius, gap, label):
    ov, of = padded(v * radius, f, 1000, 2000)
    r = np.random.default_rng(0)
    B = a.batch
    centre = np.array([0.03, -0.02, 0.7])
    shift = np.array([0.03, 0.0, radius + gap]) + r.uniform(-0.01, 0.01, (B, 3))
    hand = torch.from_numpy((hv[None] + centre).astype(np.float32).repeat(B, 0)).to(dev)
    obj = torch.from_numpy((ov[None] + centre + shift[:, None]).astype(np.float32)).to(dev)
    hand_f, obj_f = torch.from_numpy(hf).to(dev), torch.from_numpy(of).to(dev)

    def call(n):
        return ops.eval_interaction(hand[:n], hand_f, obj[:n], obj_f, contact_dist=0.005, voxel=a.voxel)

    def window(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(a.reps):
            call(n)
        e1.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps, 1e3 * (t1 - t0) / a.reps

    out = call(B)
    grid = out["grid"].cpu().numpy()
    n = grid[:, 6].copy().view(np.int32)
    dims = np.stack([n & 255, (n >> 8) & 255, (n >> 16) & 255], 1)
    cells = dims.prod(1)
    pairs = int(cells.sum()) * (hf.shape[0] + of.shape[0])
    say(f"# {label}: object radius {1e2 * radius:g} cm; hand {hv.shape[0]} vertices / {hf.shape[0]} faces, object {ov.shape[0]} vertices / {of.shape[0]} faces, voxel "
        f"{1e3 * a.voxel:g} mm; per call, ms: GPU time by events around {a.reps} calls in a row / {a.reps}; {a.rounds} windows after {a.warmup} warm-up windows")
    say(f"# cells per sample at B = {B}: min {cells.min()} median {int(np.median(cells))} max {cells.max()} (grid of sample 0: {dims[0].tolist()}); "
        f"{cells.sum()} cells x ({hf.shape[0]} + {of.shape[0]}) faces = {pairs:.2e} point-triangle pairs before the skip, "
        f"+ {B * (hv.shape[0] * of.shape[0] + ov.shape[0] * hf.shape[0]):.2e} in the two vertex passes")
    say(f"# per sample: penetration {1e2 * float(torch.maximum(out['pen_hand'], out['pen_obj']).mean()):.2f} cm, volume "
        f"{1e6 * float(out['volume'].mean()):.1f} cm^3, in contact {float(out['in_contact'].float().mean()):.2f}, inside cells {float(out['inside_count'].float().mean()):.0f}")

    # the workgroups that skipped the hand pass: blocks of 64 consecutive cells none of which is inside the object
    blocks = skipped = 0
    for b in range(B):
        i = torch.arange(int(cells[b]), device=dev)
        nx, ny = int(dims[b, 0]), int(dims[b, 1])
        idx = torch.stack([i % nx, (i // nx) % ny, i // (nx * ny)], 1).float()
        g = torch.from_numpy(grid[b]).to(dev)
        pts = (g[:3] + (idx + 0.5) * g[3:6])[None]
        wind = ops.mesh_sdf(pts, obj[b:b + 1], obj_f, extras=True)["winding"][0]
        inside = torch.nn.functional.pad(wind > 0.5, (0, (-len(i)) % 64)).view(-1, 64).any(1)
        blocks += len(inside)
        skipped += int((~inside).sum())
    say(f"# workgroups of the voxel pass with cells: {blocks}; skipped the hand pass: {skipped} = {100 * skipped / max(blocks, 1):.1f} %")

    res = {}
    for nb in (B, 1):
        for _ in range(a.warmup):
            window(nb)
        res[nb] = [window(nb) for _ in range(a.rounds)]
        for i, (t, h) in enumerate(res[nb]):
            say(f"B = {nb:2d} window {i} gpu {t:8.4f}  host {h:8.4f}")
    for nb in (B, 1):
        t, h = zip(*res[nb])
        say(f"B = {nb:2d} median gpu {statistics.median(t):8.4f} ms per call (min {min(t):.4f} max {max(t):.4f})  "
            f"host {statistics.median(h):8.4f} (min {min(h):.4f} max {max(h):.4f})")
    tb = statistics.median([t for t, _ in res[B]])
    say(f"B = {B}: {pairs / (tb * 1e-3) / 1e9:.1f} G point-triangle pairs / s of the voxel pass's nominal work over the WHOLE call (6 launches)")


measure(0.04, 0.02, "a grasped ball, 2 cm deep in the hand")
measure(0.10, -0.02, "a large object, the hand 6 cm deep in it")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
