"""The image encoder in evaluation mode: the torch modules (MIOpen convolutions + the fused BatchNorm passes, what Model.forward runs
without the switch) next to Model.encode_native (ONE C-ABI call, hoisdf_encoder_infer: exact-f32 HIP implicit-GEMM convolutions,
BatchNorm folded).  ResNet-50 + the small decoder, 256 x 256, B = 1 and B = 16; the two are ALTERNATED in one process with the
committed MIOpen tuning db.  Per pair: GPU time by events around the call, host time for the call to return, wall time to a device
synchronise.  Then the convolution kernel alone, layer class by layer class (every convolution of the encoder at its own shape,
events around --reps launches): time, FLOP and TF/s per class.
  python tools/mb_encoder_native.py [--pairs 5] [--out profiles/encoder_native_vs_torch.txt]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from hoisdf_amd import _lib, miopen_tuning, ops
from hoisdf_amd.config import Config
from hoisdf_amd.model import _ENCODER_CACHE, get_model
from hoisdf_amd.nets import mano as MANO

ap = argparse.ArgumentParser()
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=str, default="1,16")
ap.add_argument("--resnet", type=int, default=50)
ap.add_argument("--out", type=str, default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs a GPU: a timing from anywhere else says nothing"
dev = torch.device("cuda", 0)
db = miopen_tuning.enable()
H = W = 256


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


def layer_class(m, transposed):
    if transposed:
        return "deconv 4x4 s2"
    k, s = m.kernel_size[0], m.stride[0]
    if m.out_channels == 1:
        return "1x1 -> 1 (aux)"
    return f"{k}x{k} s{s}"


say(f"# eval, ResNet-{a.resnet} + small decoder, {H} x {W}; {a.pairs} alternated pairs after {a.warmup} warm-up pairs; ms; MIOpen tuning db: {'hoisdf_amd/miopen_db (private copy)' if db else 'none'}")
say("# gpu = events around the call; host = time for the call to return; wall = until the device is idle")
for B in [int(x) for x in a.batches.split(",")]:
    c = Config()
    c.resnet_type = a.resnet
    c.apply_setting("dexycb")
    torch.manual_seed(0)
    model = get_model("test", cfg=c, mano_layer=MANO.ManoLayer(MANO.synthetic_assets(0)))
    for m in list(model.backbone_net.modules()) + list(model.decoder_net.modules()):
        if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d)):
            torch.nn.init.kaiming_normal_(m.weight)
    model = model.to(dev).eval()
    model.backbone_net.to(memory_format=torch.channels_last)
    model.decoder_net.to(memory_format=torch.channels_last)
    img = torch.rand(B, 3, H, W, device=dev).contiguous(memory_format=torch.channels_last)

    shapes = []          # (module, input shape) of every convolution, recorded from one torch forward
    hooks = [m.register_forward_hook(lambda m_, i, o: shapes.append((m_, tuple(i[0].shape))))
             for m in list(model.backbone_net.modules()) + list(model.decoder_net.modules())
             if isinstance(m, (torch.nn.Conv2d, torch.nn.ConvTranspose2d))]

    def torch_path():
        with torch.no_grad():
            feat, skips = model.backbone_net(img)
            return model.decoder_net(feat, skips)

    def native_path():
        return model.encode_native(img)

    torch_path()
    for h in hooks:
        h.remove()
    for _ in range(a.warmup):
        torch_path()
        native_path()
    rows = {"torch": [], "native": []}
    for i in range(a.pairs):
        for name, fn in (("torch", torch_path), ("native", native_path)):
            out, gpu, host, wall = timed(fn)
            rows[name].append((gpu, host, wall))
            say(f"B={B:2d} pair {i} {name:6s} gpu {gpu:8.3f}  host {host:8.3f}  wall {wall:8.3f}")
    (pt, auxt), (pn, auxn) = torch_path(), native_path()
    torch.cuda.synchronize()
    lv = ("stride2", "stride4", "stride8", "stride16", "stride32")
    say(f"B={B:2d} max |native - torch| / max |torch| per level: "
        + ", ".join(f"{k} {float((pn.levels[i].permute(0, 3, 1, 2) - pt[k]).abs().max() / pt[k].abs().max()):.2e}" for i, k in enumerate(lv)))
    desc = _ENCODER_CACHE[model]["prepared"].desc
    say(f"B={B:2d} native: {_lib.lib().hoisdf_encoder_launch_count(_lib.C.addressof(desc))} kernel launches per frame in one C call "
        f"({len(shapes)} convolutions + maxpool + split-K reduces); blob {_ENCODER_CACHE[model]['prepared'].blob.numel() / 2**20:.1f} MiB, "
        f"workspace {_ENCODER_CACHE[model]['prepared'].workspace.numel() / 2**20:.1f} MiB")
    for name in ("torch", "native"):
        cols = list(zip(*rows[name]))
        say(f"B={B:2d} {name:6s} median gpu {statistics.median(cols[0]):8.3f} (min {min(cols[0]):.3f} max {max(cols[0]):.3f})  "
            f"host {statistics.median(cols[1]):8.3f} (min {min(cols[1]):.3f} max {max(cols[1]):.3f})  "
            f"wall {statistics.median(cols[2]):8.3f} (min {min(cols[2]):.3f} max {max(cols[2]):.3f})")

    # the convolution kernel alone, per layer class
    per = {}
    for m, shp in shapes:
        tr = isinstance(m, torch.nn.ConvTranspose2d)
        cw = ops.ConvWeight(m.weight, m.bias, transposed=tr)
        x = torch.randn(shp[0], shp[2], shp[3], shp[1], device=dev)
        s, p = (1, 0) if tr else (m.stride[0], m.padding[0])
        y = ops.conv2d_nhwc(x, cw, s, p, "relu")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            ops.conv2d_nhwc(x, cw, s, p, "relu", out=y)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.reps
        taps = 4 if tr else m.kernel_size[0] * m.kernel_size[1]
        flop = 2.0 * y.shape[0] * y.shape[1] * y.shape[2] * m.out_channels * m.in_channels * taps
        ent = per.setdefault(layer_class(m, tr), [0, 0.0, 0.0])
        ent[0] += 1
        ent[1] += ms
        ent[2] += flop
    tot_ms, tot_fl = sum(v[1] for v in per.values()), sum(v[2] for v in per.values())
    for k in sorted(per):
        n, ms, fl = per[k]
        say(f"B={B:2d} conv kernel, class {k:16s}: {n:3d} layers  {ms:8.3f} ms  {fl / 1e9:9.2f} GFLOP  {fl / ms / 1e9:7.2f} TF/s")
    say(f"B={B:2d} conv kernel, all classes         : {sum(v[0] for v in per.values()):3d} layers  {tot_ms:8.3f} ms  {tot_fl / 1e9:9.2f} GFLOP  "
        f"{tot_fl / tot_ms / 1e9:7.2f} TF/s   (launched one by one from Python: includes the launch gaps)")
    say()
    del model
    torch.cuda.empty_cache()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
