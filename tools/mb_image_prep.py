#!/usr/bin/env python
"""Time of the image pipeline on one MI355X next to the PIL chain it replaces on one CPU core.

    python tools/mb_image_prep.py [--batch 32] [--out profiles/image_prep_native_vs_pil.txt]

GPU: hoisdf_image_crop and hoisdf_image_augment (csrc/imgprep.hip) at B = 32, 480 x 640 -> 256 / 128, frames resident in HBM.  Each
sample is 5 windows of ITERS back-to-back calls bracketed by device events, the two entries ALTERNATED window by window; the figure
is the median window / ITERS (and the spread of the 5).  Bytes are about what the algorithm needs (one source pixel read per output pixel,
the u8 crop written and read once per pass over it, the outputs written once), so the rate is a memory rate of the call, not a kernel's share of peak.  A run that finds no
GPU fails.
CPU: the same work as the PIL calls the reference's data_aug makes per sample (Image.transform AFFINE for the frame and both
masks, GaussianBlur, the four ImageEnhance / HSV operations torchvision's PIL backend uses, the NEAREST mask resize, the float
conversion), one process, one thread, median of 5 windows.  Label arithmetic (boxes, affines, joints) is not in either figure.
From the two: the cores a CPU loader needs to feed `--rate` samples/s (default 445, the training step's rate per GPU).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RES, HM, H, W = 256, 128, 480, 640
ITERS = 1000


def make_batch(B, seed=0):
    from hoisdf_amd import image_data as D
    r = np.random.default_rng(seed)
    frames = r.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    masks = (r.random((2, B, H, W)) < 0.5).astype(np.uint8)
    crops, draws = [], D.draw_aug(r, B)
    for b in range(B):
        j = (np.array([320.0, 240.0]) + 90 * r.uniform(-1, 1, (21, 2))).astype(np.float32)
        p = np.array([340.0, 250.0]) + 70 * r.uniform(-1, 1, (21, 2))
        K = np.array([[615.0, 0, 311.5], [0, 614.0, 242.25], [0, 0, 1]])
        d = draws[b]
        crops.append(D.aug_params(j, p, K, W, H, bool(b % 2), RES, HM, d["center_u"], d["scale_jitter"], d["rot"]))
    return frames, masks, crops, draws


def gpu_part(B, lines):
    import ctypes as C
    import torch
    from hoisdf_amd import _lib, image_data as D
    if not torch.cuda.is_available():
        raise SystemExit("mb_image_prep: no GPU")
    dev = torch.device("cuda", 0)
    frames, masks, crops, draws = make_batch(B)
    f, hm_, om_ = (torch.from_numpy(a).to(dev) for a in (frames, masks[0], masks[1]))
    photo = [D.make_photo(d["blur"], d["factors"], d["order"]) for d in draws]
    # the C entries with their arguments built once, as a C host calls them: the Python wrappers' per-call marshalling (a few hundred
    # microseconds of host time at B = 32) would otherwise be what the window measures
    fr, cr, ph = D._frames_array(f, hm_, om_, False), D._crops_array(crops), (_lib.Photo * B)(*photo)
    img, u8, hs, os_ = D._outputs(B, RES, HM, False, dev, True)
    lsum = torch.empty(B, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    A = C.addressof
    run = {"hoisdf_image_crop": lambda: _lib.call("hoisdf_image_crop", A(fr), A(cr), B, RES, HM, 0, img.data_ptr(), None, hs.data_ptr(),
                                                  os_.data_ptr(), st),
           "hoisdf_image_augment": lambda: _lib.call("hoisdf_image_augment", A(fr), A(cr), A(ph), B, RES, HM, 0, img.data_ptr(), u8.data_ptr(),
                                                     lsum.data_ptr(), hs.data_ptr(), os_.data_ptr(), st)}
    for fn in run.values():                                  # warm-up: code objects, the allocator's blocks
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in run}
    for _ in range(5):
        for k, fn in run.items():                            # alternated
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(ITERS):
                fn()
            b.record()
            b.synchronize()
            windows[k].append(a.elapsed_time(b) / ITERS)
    out_px = B * RES * RES
    bytes_ = {"hoisdf_image_crop": out_px * 3 + out_px * 12 + 2 * B * HM * HM * (1 + 4),
              "hoisdf_image_augment": out_px * 3 * 2 + 2 * out_px * 3 + out_px * 12 + 2 * B * HM * HM * (1 + 4)}
    res = {}
    for k, w in windows.items():
        med = float(np.median(w))
        res[k] = med
        lines.append(f"{k:22s} B={B}: median {med * 1e3:8.1f} us / call  (5 windows of {ITERS} calls: min {min(w) * 1e3:.1f} max {max(w) * 1e3:.1f} us)"
                     f"  = {med * 1e3 / B:6.2f} us / sample, {B / med * 1e3:10.0f} samples/s, {bytes_[k] / med / 1e6:7.1f} GB/s of needed bytes")
    return res


def pil_chain(frame, hand, obj, inverse, d):
    from PIL import Image, ImageEnhance, ImageFilter
    t = tuple(float(v) for v in np.asarray(inverse).reshape(6))
    img = Image.fromarray(frame).transform((RES, RES), Image.AFFINE, t)
    img = img.filter(ImageFilter.GaussianBlur(d["blur"]))
    for op in d["order"]:
        fac = d["factors"][op]
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(fac)
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(fac)
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(fac)
        else:
            h, s, v = img.convert("HSV").split()
            nh = np.array(h, dtype=np.uint8)
            nh += np.uint8(int(fac * 255) & 255)
            img = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    segs = [np.asarray(Image.fromarray(m).transform((RES, RES), Image.AFFINE, t).resize((HM, HM), Image.NEAREST)).astype(np.float32)
            for m in (hand, obj)]
    return np.asarray(img).astype(np.float32).transpose(2, 0, 1) / 255.0, segs


def cpu_part(lines, n=16):
    try:
        import PIL
    except ImportError:
        lines.append("PIL chain: not measured (PIL is not installed on this node)")
        return None
    from hoisdf_amd import image_data as D
    frames, masks, crops, draws = make_batch(n, seed=1)
    inv = [D.crop_to_dict(c)["inverse"] for c in crops]
    for b in range(2):
        pil_chain(frames[b], masks[0][b], masks[1][b], inv[b], draws[b])
    w = []
    for _ in range(5):
        t0 = time.perf_counter()
        for b in range(n):
            pil_chain(frames[b], masks[0][b], masks[1][b], inv[b], draws[b])
        w.append((time.perf_counter() - t0) / n)
    med = float(np.median(w))
    lines.append(f"PIL {PIL.__version__} chain, one core of this node: median {med * 1e3:.2f} ms / sample (5 windows of {n} samples: min {min(w) * 1e3:.2f} "
                 f"max {max(w) * 1e3:.2f} ms) = {1 / med:.0f} samples/s per core")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rate", type=float, default=445.0, help="samples/s per GPU the loader has to feed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu-only", action="store_true", help="the PIL chain alone (a node without a GPU)")
    a = ap.parse_args()
    lines = [f"image preparation, {H} x {W} -> {RES} / {HM}; {time.strftime('%Y-%m-%d')}"]
    gpu = None if a.cpu_only else gpu_part(a.batch, lines)
    cpu = cpu_part(lines)
    if cpu is not None:
        lines.append(f"cores the PIL chain needs for {a.rate:.0f} samples/s: {a.rate * cpu:.1f} (image work alone; decoding and labels come on top)")
        if gpu is not None:
            t = gpu["hoisdf_image_augment"] / a.batch * 1e-3
            lines.append(f"hoisdf_image_augment at that rate: {100 * a.rate * t:.2f} % of one GPU's time ({cpu / t:.0f} x one core's samples/s)")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
