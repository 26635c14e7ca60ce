"""Deterministic synthetic weights / inputs shared by tests, the golden-vector generator,
``bench.py`` and ``__graft_entry__.smoke()``.

Weights are a pure function of (parameter name, shape, seed) through numpy's PCG64 - they
are never stored in fixtures, both sides of every parity test regenerate them.  Input
distributions follow SURVEY.md section 8(d) (DexYCB / HO3D shaped synthetic batches).
No oracle import here (this module is part of the shipped package).
"""
from __future__ import annotations

import math
import zlib
from collections import OrderedDict
from typing import Dict, Tuple

import numpy as np
import torch

PYRAMID_SMALL = OrderedDict(stride2=(32, 128), stride4=(64, 64), stride8=(128, 32),
                            stride16=(256, 16), stride32=(512, 8))
PYRAMID_BIG = OrderedDict(stride2=(128, 128), stride4=(256, 64), stride8=(512, 32),
                          stride16=(1024, 16), stride32=(2048, 8))


def hot_path_param_shapes(C: int = 992, ik: bool = False, hidden: int = 256,
                          enc_layers: int = 6, dec_layers: int = 4,
                          ffn: int = 1024, pre_norm: bool = False,
                          classifier: bool = False) -> "OrderedDict[str, Tuple[int, ...]]":
    """State-dict schema of the hot path (reference
    main/model.py:49-90, common/nets/sdf_net.py:50-62, common/nets/transformer.py)."""
    S: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    D = hidden
    S["hand_sigmoid_beta"] = (1,)
    S["obj_sigmoid_beta"] = (1,)
    S["norm1.weight"] = (C,)
    S["norm1.bias"] = (C,)

    def mlp(prefix, dims):
        for i in range(len(dims) - 1):
            S[f"{prefix}.layers.{i}.weight"] = (dims[i + 1], dims[i])
            S[f"{prefix}.layers.{i}.bias"] = (dims[i + 1],)

    mlp("linear_transformerin", [C, 1024, 512, 256, D - 33])
    mlp("linear_sdfin", [C, 512, D])
    for kind in ("hand", "obj"):
        dims = [(512, D + 33), (D - 33, 512), (512, 512), (512, 512)]
        for i, (o, n) in enumerate(dims):
            S[f"{kind}_sdf_decoder.linh{i}.bias"] = (o,)
            S[f"{kind}_sdf_decoder.linh{i}.weight_g"] = (o, 1)
            S[f"{kind}_sdf_decoder.linh{i}.weight_v"] = (o, n)
        if classifier:                      # common/nets/sdf_net.py:73-75 (cfg.ClassifierBranch)
            S[f"{kind}_sdf_decoder.classifier_head.weight"] = (6, 512)
            S[f"{kind}_sdf_decoder.classifier_head.bias"] = (6,)
        S[f"{kind}_sdf_decoder.linh4.weight"] = (1, 512)
        S[f"{kind}_sdf_decoder.linh4.bias"] = (1,)

    def attn(prefix):
        S[prefix + ".in_proj_weight"] = (3 * D, D)
        S[prefix + ".in_proj_bias"] = (3 * D,)
        S[prefix + ".out_proj.weight"] = (D, D)
        S[prefix + ".out_proj.bias"] = (D,)

    def ln(prefix):
        S[prefix + ".weight"] = (D,)
        S[prefix + ".bias"] = (D,)

    def enc(prefix, n):
        for l in range(n):
            p = f"{prefix}.layers.{l}"
            attn(p + ".self_attn")
            S[p + ".linear1.weight"] = (ffn, D)
            S[p + ".linear1.bias"] = (ffn,)
            S[p + ".linear2.weight"] = (D, ffn)
            S[p + ".linear2.bias"] = (D,)
            ln(p + ".norm1")
            ln(p + ".norm2")
        if pre_norm:                        # common/nets/transformer.py:33,87: encoder.norm only with normalize_before
            ln(prefix + ".norm")
        ln(prefix + ".inter_norm")

    enc("hand_transformer.encoder", enc_layers)
    for l in range(dec_layers):
        p = f"hand_transformer.decoder.layers.{l}"
        attn(p + ".self_attn")
        attn(p + ".multihead_attn")
        S[p + ".linear1.weight"] = (ffn, D)
        S[p + ".linear1.bias"] = (ffn,)
        S[p + ".linear2.weight"] = (D, ffn)
        S[p + ".linear2.bias"] = (D,)
        ln(p + ".norm1")
        ln(p + ".norm2")
        ln(p + ".norm3")
    ln("hand_transformer.decoder.norm")
    enc("obj_transformer.encoder", enc_layers // 2)

    S["mano_query_embed.weight"] = (1 if ik else 17, D)
    if not ik:
        mlp("linear_pose", [D, D, D, 6])
    mlp("linear_shape", [D, D, D, 10])
    mlp("linear_handvote", [D, D, D, D, 60])
    mlp("linear_handcls", [D, D, D, 20])
    mlp("linear_objvote", [D, D, D, D, 24])
    mlp("linear_objcls", [D, D, D, 8])
    mlp("linear_obj_rel_trans", [D, D, D, 3])
    mlp("linear_obj_rot", [D, D, D, 3])
    return S


def _rng(name: str, seed: int) -> np.random.Generator:
    return np.random.default_rng([zlib.crc32(name.encode()), seed])


def det_param(name: str, shape, seed: int = 0) -> torch.Tensor:
    """One deterministic parameter.  Scales keep activations O(1) through the stack and the
    SDF head un-saturated (|sdf| mostly inside the +-0.15 clamp with some values outside)."""
    r = _rng(name, seed)
    shape = tuple(shape)
    if name.endswith("sigmoid_beta"):
        v = np.array([0.08 if name.startswith("hand") else 0.12], np.float32)
    elif name.endswith("weight_g"):
        v = (0.8 + 0.4 * r.random(shape)).astype(np.float32)
    elif name.endswith("weight_v"):
        v = r.standard_normal(shape).astype(np.float32) / np.sqrt(shape[1])
    elif name.endswith("linh4.weight"):     # zero-sum so the SDF head is roughly centred
        v = r.standard_normal(shape)
        v = (v - v.mean()) / np.sqrt(shape[1])
    elif name.endswith("linh4.bias"):
        v = np.array([-0.15 if name.startswith("hand") else -0.18])
    elif "norm" in name and name.endswith(".weight"):
        v = (1.0 + 0.1 * r.standard_normal(shape)).astype(np.float32)
    elif name.endswith("mano_query_embed.weight"):
        v = (0.5 * r.standard_normal(shape)).astype(np.float32)
    elif len(shape) == 2:
        gain = 1.4 if ("layers" in name or "linear1" in name) else 1.0
        v = r.standard_normal(shape).astype(np.float32) * (gain / np.sqrt(shape[1]))
    else:
        v = (0.05 * r.standard_normal(shape)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float32)))


def det_params(shapes: Dict[str, Tuple[int, ...]], seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    return OrderedDict((k, det_param(k, s, seed)) for k, s in shapes.items())


OUTLIER_CHANNELS = (3, 17, 40)          # (modulo a level's channel count)


def synthetic_pyramid(B: int, big: bool = False, seed: int = 0, scale: float = 1.0,
                      nonneg: bool = True, outliers: float = 1.0) -> "OrderedDict[str, torch.Tensor]":
    """Random NCHW feature maps shaped like the CNN decoder's pyramid (post-ReLU => >= 0).
    outliers != 1: channels OUTLIER_CHANNELS of every level are that many times louder (trained CNN features have such channels;
    the "_smallbeta" fixtures use x 100)."""
    spec = PYRAMID_BIG if big else PYRAMID_SMALL
    out = OrderedDict()
    for name, (c, hw) in spec.items():
        a = _rng("pyr." + name, seed).standard_normal((B, c, hw, hw)).astype(np.float32) * scale
        if nonneg:
            a = np.maximum(a, 0)
        if outliers != 1.0:
            a[:, [ch % c for ch in OUTLIER_CHANNELS]] *= np.float32(outliers)
        out[name] = torch.from_numpy(a)
    return out


SMALL_BETA = {"hand_sigmoid_beta": 2e-3, "obj_sigmoid_beta": 1e-2}     # a trained model's gates: sigma up to 500 (main/model.py:123-126)
# "_trainedlike" fixtures: SMALL_BETA + outlier channels + the FIRST encoder layer's query / key projections scaled down to the token
# magnitudes they then see (sigma-gated rows up to ~5e3 / 2.4e4), as a network trained on such inputs would have them: attention scores
# of O(10-100).  With det_param's unit-gain q / k weights the same tokens give scores of 7e6 (hand) / 2.4e8 (object) in the log2 domain:
# one fp32 ulp of such a score is 0.5 / 16 - softmax is then decided by rounding, in any fp32 implementation
TRAINED_LIKE_QK = {"hand_transformer.encoder.layers.0.self_attn": 3e-3, "obj_transformer.encoder.layers.0.self_attn": 7e-4}


def apply_trained_like(get, E: int = 256):
    """scale rows [0, 2E) (q and k) of the two first-layer in-projections in place; ``get(name)`` returns the tensor of a parameter name"""
    with torch.no_grad():
        for prefix, f in TRAINED_LIKE_QK.items():
            get(prefix + ".in_proj_weight")[:2 * E].mul_(f)
            get(prefix + ".in_proj_bias")[:2 * E].mul_(f)


def synthetic_batch(B: int, n_hand: int, n_obj: int, seed: int = 1234):
    """(inputs, targets, meta_info) with the dataset schema of data/dexycb.py:627-655 and the
    distributions of SURVEY.md section 8(d).  CPU float32 tensors."""
    r = _rng("batch", seed)

    def U(lo, hi, *s):
        return torch.from_numpy((lo + (hi - lo) * r.random(s)).astype(np.float32))

    def N(std, *s):
        return torch.from_numpy((std * r.standard_normal(s)).astype(np.float32))

    K = torch.tensor([[600.0, 0, 128], [0, 600.0, 128], [0, 0, 1]]).repeat(B, 1, 1)
    inputs = dict(
        img=U(0, 1, B, 3, 256, 256),
        hand_sdf_points=U(-1, 1, B, n_hand, 3), obj_sdf_points=U(-1, 1, B, n_obj, 3),
        hand_pre_points=U(-0.3, 0.3, B, n_hand, 3), obj_pre_points=U(-0.3, 0.3, B, n_obj, 3))
    targets = dict(
        hand_sdf=U(0, 0.1, B, n_hand), obj_sdf=U(0, 0.1, B, n_obj),
        joint_cam_no_trans=N(50.0, B, 21, 3), mano_param=N(0.1, B, 58), obj_rot=N(1.0, B, 3),
        rel_obj_trans=N(0.05, B, 3),
        hand_seg=(U(0, 1, B, 128, 128) > 0.5).float(), obj_seg=(U(0, 1, B, 128, 128) > 0.5).float(),
        joint_coord=U(20, 108, B, 21, 2))
    meta = dict(
        mano_root=torch.tensor([0.0, 0.0, 0.7]).repeat(B, 1) + N(0.01, B, 3),
        obj_center_cam=torch.tensor([0.03, 0.02, 0.72]).repeat(B, 1) + N(0.01, B, 3),
        cam_intr=K,
        bbox_hand=torch.tensor([40.0, 40, 220, 220]).repeat(B, 1),
        bbox_obj=torch.tensor([60.0, 60, 200, 200]).repeat(B, 1))
    return inputs, targets, meta


# ---- asymmetric geometry: every symmetry of synthetic_batch / synthetic_pyramid broken on purpose -------------------------------
# (C, H, W) per level.  "encoder-like": the CNN decoder's channels (sum 992) on a 192 x 320 image's strides - ragged 16 x 16 tiles at
# 24 x 40 and 12 x 20, both coarse LDS groups (240 and 60 pixels); x 4 channels: C / 4 > 256, the looping forward gather.
# "odd": H > W, odd sizes, a level of two float4 columns, a level whose channels are no multiple of 64 (stays on the atomic path).
PYRAMID_ENCODER_LIKE = ((32, 96, 160), (64, 48, 80), (128, 24, 40), (256, 12, 20), (512, 6, 10))
PYRAMID_ENCODER_LIKE_BIG = tuple((4 * c, h, w) for c, h, w in PYRAMID_ENCODER_LIKE)
PYRAMID_ODD = ((8, 37, 21), (64, 17, 33), (192, 5, 9))
LEVEL_NAMES = ("stride2", "stride4", "stride8", "stride16", "stride32")

_ASYM_THETA_DEG = (17.0, -31.0, 8.0, -12.0, 26.0, -5.0, 21.0, -23.0)
# boxes as fractions (x0, y0, x1, y1) of (W, H, W, H): [60, 30, 260, 150], [20, 50, 200, 180], [100, 10, 300, 120] on 192 x 320
_ASYM_BOX = ((0.1875, 0.15625, 0.8125, 0.78125), (0.0625, 0.2604167, 0.625, 0.9375), (0.3125, 0.0520833, 0.9375, 0.625),
             (0.125, 0.1, 0.7, 0.9))
_ASYM_CENTER = ((0.01, -0.02, 0.70), (-0.03, 0.01, 0.62), (0.02, 0.03, 0.81), (-0.01, -0.03, 0.66))


def transposed(spec):
    """the (C, H, W) levels of ``spec`` with H and W exchanged (the pyramid of the transposed image)"""
    return tuple((c, w, h) for c, h, w in spec)


def nonsquare_pyramid(B: int, spec=PYRAMID_ENCODER_LIKE, seed: int = 0, nonneg: bool = True) -> "OrderedDict[str, torch.Tensor]":
    """Random NCHW feature maps with the (C, H, W) of ``spec`` per level, named like the CNN decoder's (stride2 ...)."""
    out = OrderedDict()
    for name, (c, h, w) in zip(LEVEL_NAMES, spec):
        a = _rng("nspyr." + name, seed).standard_normal((B, c, h, w)).astype(np.float32)
        out[name] = torch.from_numpy(np.maximum(a, 0) if nonneg else a)
    return out


def asymmetric_geometry(B: int, img_hw=(192, 320), seed: int = 77):
    """``meta_info`` like synthetic_batch's, with nothing shared between samples or between the two image axes: per-sample
    cam_intr = T_c R(theta_b) T_c^-1 K_b (the in-plane augmentation of data/dexycb.py:295,384: K = post_rot_trans . K; fx_b != fy_b
    in 560-640, cx_b != cy_b, every K[0,1] and K[1,0] non-zero), per-sample boxes inside the H x W image, centres centimetres apart."""
    H, W = img_hw
    r = _rng("asym_geometry", seed)
    ctr = ((W - 1) / 2.0, (H - 1) / 2.0)
    K, boxes_h, boxes_o, root, ocen = [], [], [], [], []
    for b in range(B):
        lap = b // len(_ASYM_BOX)                               # samples beyond the tables: the tables again, shifted
        fx, fy = 560.0 + 80.0 * r.random(), 560.0 + 80.0 * r.random()
        if abs(fx - fy) < 8.0:
            fy = fx - 24.0 if fx > 600.0 else fx + 24.0
        cx, cy = ctr[0] + (0.02 + 0.03 * r.random()) * W, ctr[1] - (0.02 + 0.03 * r.random()) * H
        th = np.deg2rad(_ASYM_THETA_DEG[b % len(_ASYM_THETA_DEG)] + 1.5 * lap)
        Kb = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float64)
        R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], np.float64)
        Tc = np.array([[1, 0, ctr[0]], [0, 1, ctr[1]], [0, 0, 1]], np.float64)
        K.append(Tc @ R @ np.linalg.inv(Tc) @ Kb)
        x0, y0, x1, y1 = _ASYM_BOX[b % len(_ASYM_BOX)]
        sh = 0.02 * lap
        boxes_h.append([round((x0 + sh) * W), round((y0 + sh) * H), round((x1 - sh) * W), round((y1 - sh) * H)])
        x0, y0, x1, y1 = _ASYM_BOX[(b + 1) % len(_ASYM_BOX)]
        boxes_o.append([round((x0 + sh) * W) + 3, round((y0 + sh) * H) + 5, round((x1 - sh) * W) - 7, round((y1 - sh) * H) - 2])
        c = np.array(_ASYM_CENTER[b % len(_ASYM_CENTER)]) + 0.004 * lap
        root.append(c)
        ocen.append(c + np.array([0.03, 0.02, 0.02]) * (1 + 0.5 * b) * (-1 if b % 2 else 1))
    f32 = lambda a: torch.from_numpy(np.asarray(a, np.float64).astype(np.float32))
    return dict(mano_root=f32(root), obj_center_cam=f32(ocen), cam_intr=f32(K), bbox_hand=f32(boxes_h), bbox_obj=f32(boxes_o))


def synthetic_decoder_out(B: int, seed: int = 13):
    """a seeded stand-in for decoder_net's second output (B, 3, 128, 128): channel 0 = heat-map logits on the scale of the
    255-peaked target, channels 1 / 2 = segmentation probabilities in (0.01, 0.99) with a few saturated pixels (BCELoss
    clamps its logs at -100)."""
    r = _rng("decoder_out", seed)
    d = torch.from_numpy((0.01 + 0.98 * r.random((B, 3, 128, 128))).astype(np.float32))
    d[:, 0] = d[:, 0] * 300.0
    d[0, 1, 0, 0], d[0, 2, 0, 1], d[-1, 1, 5, 7], d[-1, 2, 9, 3] = 0.0, 1.0, 1.0, 0.0
    return d


def synthetic_sdf_frames(n_frames: int, seed: int = 14):
    """``sdf_processed``-shaped frames ((N_h + N_o, 6) float32 rows [x y z sdf_hand sdf_obj label], tool/pre_process_sdf.py:
    140-148) + their ``sdf_index`` rows [N_h, N_o]; about a third of the rows pass the |sdf| < 0.05 pre-filter."""
    r = _rng("sdf_frames", seed)
    frames, index = [], []
    for _ in range(n_frames):
        nh, no = int(r.integers(300, 500)), int(r.integers(200, 400))
        a = np.zeros((nh + no, 6), np.float32)
        a[:, :3] = (r.uniform(-0.1, 0.1, (nh + no, 3)) + np.array([0.0, 0.0, 0.7])).astype(np.float32)
        a[:, 3] = r.uniform(-0.15, 0.15, nh + no)
        a[:, 4] = r.uniform(-0.15, 0.15, nh + no)
        a[:, 5] = r.integers(0, 6, nh + no)
        frames.append(a)
        index.append([nh, no])
    return frames, np.asarray(index)


def to_device(tree, device):
    if isinstance(tree, dict):
        return type(tree)((k, to_device(v, device)) for k, v in tree.items())
    if isinstance(tree, (list, tuple)):
        return type(tree)(to_device(v, device) for v in tree)
    if torch.is_tensor(tree):
        return tree.to(device)
    return tree


# ---- attention dropout held to fp64: the kernels print their own mask, autograd in float64 is the truth ---------------------------
# A "kernel" here is a pair of callables on CPU tensors: fwd(q, k, v) -> o (B, Lq, E) and bwd(q, k, v, do) -> (dq, dk, dv), both under
# one fixed (p, seed).  The dropout mask does not depend on the operand values, so one-hot V / dO read it out of them element by
# element; nothing below knows the hash.  `valid` (broadcastable to (B, H, Lq, Lk), bool) marks the pairs that
# take part in the softmax: keys below kv_len, pairs the uint8 mask leaves.  Every check raises AssertionError("<its name>: ...").
ATTN_HEAD = 64


def _one_hot_chunk(B: int, L: int, H: int, c: int) -> torch.Tensor:
    """(B, L, H * 64) float32: 1 at [b, 64 c + d, h * 64 + d] for every b, h and d with 64 c + d < L, 0 elsewhere"""
    t = torch.zeros(B, L, H, ATTN_HEAD)
    d = torch.arange(min(ATTN_HEAD, L - ATTN_HEAD * c))
    t[:, ATTN_HEAD * c + d, :, d] = 1.0
    return t.view(B, L, H * ATTN_HEAD)


def _heads(t: torch.Tensor, H: int) -> torch.Tensor:
    return t.reshape(t.shape[0], t.shape[1], H, ATTN_HEAD).transpose(1, 2)


def probe_dropped_probs_forward(fwd, q, k, H: int) -> torch.Tensor:
    """Pd (B, H, Lq, Lk) float64 = the dropped, rescaled probability matrix of the forward: with V one-hot on chunk c of 64 keys,
    o[b, i, h * 64 + d] = Pd[b, h, i, 64 c + d] - one non-zero term per output, so nothing is rounded"""
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    pd = torch.zeros(B, H, Lq, Lk, dtype=torch.float64)
    for c in range((Lk + ATTN_HEAD - 1) // ATTN_HEAD):
        n = min(ATTN_HEAD, Lk - ATTN_HEAD * c)
        o = fwd(q, k, _one_hot_chunk(B, Lk, H, c).to(q.dtype))
        pd[..., ATTN_HEAD * c:ATTN_HEAD * c + n] = _heads(o.detach().cpu().double(), H)[..., :n]
    return pd


def probe_dropped_probs_backward(bwd, q, k, v, H: int) -> torch.Tensor:
    """Pd (B, H, Lq, Lk) float64 as the backward regenerates it: dV = Pd^T dO needs neither delta nor dS, and with dO one-hot on
    chunk c of 64 queries dv[b, j, h * 64 + d] = Pd[b, h, 64 c + d, j]"""
    B, Lq, Lk = q.shape[0], q.shape[1], k.shape[1]
    pd = torch.zeros(B, H, Lq, Lk, dtype=torch.float64)
    for c in range((Lq + ATTN_HEAD - 1) // ATTN_HEAD):
        n = min(ATTN_HEAD, Lq - ATTN_HEAD * c)
        dv = bwd(q, k, v, _one_hot_chunk(B, Lq, H, c).to(q.dtype))[2]
        pd[:, :, ATTN_HEAD * c:ATTN_HEAD * c + n, :] = _heads(dv.detach().cpu().double(), H).transpose(-1, -2)[:, :, :n, :]
    return pd


def reference_probs(q, k, H: int, valid) -> torch.Tensor:
    """float64 softmax(q k^T / 8) over the valid pairs, (B, H, Lq, Lk); differentiable in q and k"""
    s = (_heads(q.double(), H) @ _heads(k.double(), H).transpose(-1, -2)) / math.sqrt(ATTN_HEAD)
    return torch.softmax(s.masked_fill(~valid.expand(s.shape), float("-inf")), -1)


def reference_dropout_attention(q, k, v, do, H: int, valid, keep_mask, p: float):
    """the truth: float64 autograd of ((softmax(s) * M / (1 - p)) @ V) -> (o, dq, dk, dv)"""
    q64, k64, v64 = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    pd = reference_probs(q64, k64, H, valid) * keep_mask.double() / (1.0 - p)
    o = (pd @ _heads(v64, H)).transpose(1, 2).reshape(q.shape)
    o.backward(do.double())
    return o.detach(), q64.grad, k64.grad, v64.grad


def _rel_err(got, ref) -> float:
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def check_probe_validity(p64, valid) -> float:
    """a condition on the reference, not on the kernel: every float64 probability on a valid pair is >= 1e-6, far above where a
    float32 (or a scaled f16 piece of a) kept probability could vanish, so `Pd > 0` is a faithful mask"""
    smallest = float(p64[valid.expand(p64.shape)].min())
    assert smallest >= 1e-6, f"probe validity: smallest reference probability {smallest:.3e} < 1e-6"
    return smallest


def check_same_mask(pd_fwd, pd_bwd, valid) -> torch.Tensor:
    """the forward's mask is the backward's mask on every valid (b, h, i, j); other pairs give exactly 0 in both probes.
    Returns the mask (bool, False outside `valid`)."""
    vm = valid.expand(pd_fwd.shape)
    for name, pd in (("forward", pd_fwd), ("backward", pd_bwd)):
        stray = (pd != 0) & ~vm
        assert not bool(stray.any()), f"same mask: the {name} probe is non-zero on excluded pairs, first at (b, h, i, j) = " \
                                      f"{tuple(stray.nonzero()[0].tolist())}"
    mf, mb = (pd_fwd > 0) & vm, (pd_bwd > 0) & vm
    diff = mf != mb
    assert not bool(diff.any()), f"same mask: forward and backward differ on {int(diff.sum())} pairs, first at (b, h, i, j) = " \
                                 f"{tuple(diff.nonzero()[0].tolist())} (forward keeps: {bool(mf[tuple(diff.nonzero()[0].tolist())])})"
    return mf


def check_kept_values(pd_fwd, p64, keep_mask, p: float, rel: float = 2e-5) -> float:
    """the probed forward matrix is P64 * M / (1 - p) to the attention-output bar (the probe is an attention output)"""
    err = _rel_err(pd_fwd, p64.detach() * keep_mask.double() / (1.0 - p))
    assert err <= rel, f"kept values: dropped probabilities are {err:.3e} of their max from P64 * M / (1 - p) (bar {rel:.0e})"
    return err


def check_forward_and_gradients(fwd, bwd, q, k, v, do, H: int, valid, keep_mask, p: float, rel_o: float = 2e-5, rel_g: float = 5e-5):
    """o, dq, dk, dv with real V and dO against float64 autograd under the probed mask; keys no query may see get exactly zero
    gradients.  Returns the four relative errors (of the reference's max)."""
    ro, rq, rk, rv = reference_dropout_attention(q, k, v, do, H, valid, keep_mask, p)
    o = fwd(q, k, v)
    dq, dk, dv = bwd(q, k, v, do)
    errs = dict(o=_rel_err(o, ro), dq=_rel_err(dq, rq), dk=_rel_err(dk, rk), dv=_rel_err(dv, rv))
    for name, bar in (("o", rel_o), ("dq", rel_g), ("dk", rel_g), ("dv", rel_g)):
        assert errs[name] <= bar, f"forward and gradients: {name} is {errs[name]:.3e} of its max from fp64 (bar {bar:.0e}); all: {errs}"
    unseen = ~valid.expand(keep_mask.shape).any(2).any(1)                     # (B, Lk): keys outside every softmax
    for name, g in (("dk", dk), ("dv", dv)):
        g = g.detach().cpu()
        assert float(g[unseen].abs().max() if bool(unseen.any()) else 0.0) == 0.0, f"forward and gradients: {name} of an excluded key is not 0"
    return errs


def check_mask_statistics(keep_mask, kv_len: int, p: float, sigmas: float = 5.0):
    """keep_mask (B, H, Lq, Lk) bool, keys < kv_len valid.  The keep fraction against the binomial around 1 - floor(p 2^16) / 2^16
    (the 16-bit threshold, csrc/common.h), and the joint keep frequency of neighbours - columns (2 c, 2 c + 1), which share a hash,
    columns (2 c + 1, 2 c + 2), rows, heads, samples - against its square: independent decisions.  Pairs are disjoint, so each
    count is binomial and sigma comes from the element count alone.  Returns {name: (frequency, expectation, n, z)}."""
    m = keep_mask[..., :kv_len]
    pk = 1.0 - math.floor(p * 65536.0) / 65536.0
    out = {}

    def one(name, hits, prob):
        n = hits.numel()
        if n == 0:
            return
        f = float(hits.double().mean())
        out[name] = (f, prob, n, (f - prob) / math.sqrt(prob * (1.0 - prob) / n))

    one("keep", m, pk)
    for dim, what in ((3, "columns"), (2, "rows"), (1, "heads"), (0, "samples")):
        for off in (0, 1):
            n = (m.shape[dim] - off) // 2
            a = m.narrow(dim, off, 2 * n)
            ix0, ix1 = torch.arange(0, 2 * n, 2), torch.arange(1, 2 * n, 2)
            one(f"{what} {'2n, 2n+1' if off == 0 else '2n+1, 2n+2'}", a.index_select(dim, ix0) & a.index_select(dim, ix1), pk * pk)
    for name, (f, prob, n, z) in out.items():
        assert abs(z) <= sigmas, f"mask statistics: {name}: frequency {f:.5f} over {n} is {z:+.1f} sigma from {prob:.5f}"
    return out


# ---- the small hot-path kernels held to fp64: one plain-torch function per operation ------------------------------------------------
# Every function takes the float32 CPU inputs the kernel gets, evaluates in ``dtype`` (float64 = the truth; float32 = the same formula
# at the kernel's precision, the yardstick of the slice-wise bar below) and returns a dict of ``dtype`` tensors; gradients come from
# autograd and are present when the matching upstream gradient is given.  Nothing here knows how a kernel orders its sums.
TOKEN_BETA_MIN = float(np.float32(2e-3))       # main/model.py:123-126 clamps the gate's beta here; the float32 constant the kernels hold


def _leaf(t: torch.Tensor, dtype) -> torch.Tensor:
    return t.detach().to(dtype).clone().requires_grad_(True)


def reference_posenc_rows(pts, ld: int = 30, col0: int = 0, fill: float = 0.0, dtype=torch.float64) -> torch.Tensor:
    """(n, ld) buffer as hoisdf_posenc_fwd leaves a ``fill``-filled x0: columns [col0, col0 + 30) = [sin(2^k p), cos(2^k p)], k = 0..4
    (three coordinates each), [col0 + 30, col0 + 33) = p, [col0 + 33, min(col0 + 36, ld)) = 0, every other element ``fill``.
    ld = 30, col0 = 0 is the ``pe`` output."""
    p = pts.detach().reshape(-1, 3).to(dtype)
    cols = []
    for k in range(5):
        cols += [torch.sin(p * float(2 ** k)), torch.cos(p * float(2 ** k))]
    body = torch.cat(cols + [p, torch.zeros_like(p)], 1)                      # 36 columns
    out = torch.full((p.shape[0], ld), fill, dtype=dtype)
    n = min(36, ld - col0)
    out[:, col0:col0 + n] = body[:, :n]
    return out


def reference_weight_norm(v, g, dW=None, ldw=None, dtype=torch.float64):
    """W [out, ldw] = g * v / ||v||_row in columns [0, in), 0 in the pad; norms [out]; dv, dg for dW [out, ldw] (its pad is not read)"""
    out_, in_ = v.shape
    ldw = in_ if ldw is None else ldw
    v_, g_ = _leaf(v, dtype), _leaf(g.reshape(out_), dtype)
    norms = v_.pow(2).sum(1).sqrt()
    W = torch.cat([v_ * (g_ / norms)[:, None], torch.zeros(out_, ldw - in_, dtype=dtype)], 1)
    res = dict(W=W.detach(), norms=norms.detach())
    if dW is not None:
        W.backward(dW.detach().to(dtype))
        res.update(dv=v_.grad, dg=g_.grad)
    return res


def reference_sdf_head(h, w, b, clamp: float, dsdf=None, dtype=torch.float64):
    """pre = h w + b, raw = tanh(pre), sdf = clamp(raw, +-clamp) (torch.clamp: the gradient passes on |raw| <= clamp);
    dh [M, K], dw [K], db [1] for dsdf [M]"""
    h_, w_, b_ = _leaf(h, dtype), _leaf(w.reshape(-1), dtype), _leaf(b.reshape(1), dtype)
    pre = h_ @ w_ + b_
    raw = torch.tanh(pre)
    sdf = raw.clamp(-clamp, clamp)
    res = dict(pre=pre.detach(), raw=raw.detach(), sdf=sdf.detach())
    if dsdf is not None:
        sdf.backward(dsdf.detach().reshape(-1).to(dtype))
        res.update(dh=h_.grad, dw=w_.grad, db=b_.grad)
    return res


def reference_token_build(cam, center, pe, feat, sdf, beta, dtok=None, dtype=torch.float64):
    """tok [B, P, D] = [cam - center | pe | feat * sigmoid(sdf / beta_eff) / beta_eff], beta_eff = max(beta, 2e-3) as the reference
    model clamps it; dfeat [B, P, D - 33] and dbeta [1] - the gradient with respect to beta_eff - for dtok [B, P, D].
    cam (B, P, 3), center (B, 3), pe (B, P, 30), feat (B, P, D - 33), sdf (B, P)"""
    B, P = sdf.shape[0], sdf.shape[1]
    feat_ = _leaf(feat.reshape(B, P, -1), dtype)
    beta_eff = _leaf(torch.clamp(beta.detach().reshape(1).float(), min=TOKEN_BETA_MIN), dtype)
    sig = torch.sigmoid(sdf.detach().reshape(B, P, 1).to(dtype) / beta_eff) / beta_eff
    tok = torch.cat([cam.detach().reshape(B, P, 3).to(dtype) - center.detach().to(dtype)[:, None],
                     pe.detach().reshape(B, P, 30).to(dtype), feat_ * sig], 2)
    res = dict(tok=tok.detach(), beta_eff=beta_eff.detach())
    if dtok is not None:
        tok.backward(dtok.detach().to(dtype))
        res.update(dfeat=feat_.grad, dbeta=beta_eff.grad)
    return res


def reference_vote(off, cls, pts, dj=None, dtype=torch.float64):
    """joints [L, B, J, 3] = sum_p softmax_p(cls)[p] (pts[p] + off[p, j]); doff, dcls for dj.  off (L, B, P, J * 3), cls (L, B, P, J),
    pts (B, P, 3); any J"""
    L, B, P, J = cls.shape
    off_, cls_ = _leaf(off, dtype), _leaf(cls, dtype)
    vote = pts.detach().to(dtype)[None, :, :, None, :] + off_.view(L, B, P, J, 3)
    joints = (vote * torch.softmax(cls_, dim=2).unsqueeze(-1)).sum(2)
    res = dict(joints=joints.detach())
    if dj is not None:
        joints.backward(dj.detach().to(dtype))
        res.update(doff=off_.grad, dcls=cls_.grad)
    return res


def vote_near(pts, gt_mm, radius: float):
    """float64 distances ||p - gt / 1000|| (B, P, J) and the mask distance < radius, from the float32 inputs"""
    d = (pts.detach().double()[:, :, None, :] - gt_mm.detach().double()[:, None] / 1000.0).norm(dim=-1)
    return d, d < radius


def reference_vote_loss(off, cls, pts, gt_mm, radius: float, dj=None, dl3d=None, dbce=None, dtype=torch.float64):
    """reference_vote plus the JointvoteLoss sums (common/nets/loss.py:31-56) with near = ||p - gt / 1000|| < radius (always decided
    in float64): l3d_sum [L, B] = sum_{p, j, xyz} smooth_l1(1000 vote - gt) near, bce_sum [L, B] = sum_{p, j} bce_with_logits(cls,
    near), near_sum [B] = sum_{p, j} near.  doff, dcls for whichever of dj [L, B, J, 3], dl3d [L, B], dbce [L, B] are given."""
    L, B, P, J = cls.shape
    off_, cls_ = _leaf(off, dtype), _leaf(cls, dtype)
    gt = gt_mm.detach().to(dtype)
    near = vote_near(pts, gt_mm, radius)[1].to(dtype)                                      # (B, P, J)
    vote = pts.detach().to(dtype)[None, :, :, None, :] + off_.view(L, B, P, J, 3)
    joints = (vote * torch.softmax(cls_, dim=2).unsqueeze(-1)).sum(2)
    x = vote * 1000.0 - gt[None, :, None]
    sl1 = torch.where(x.abs() < 1.0, 0.5 * x * x, x.abs() - 0.5)
    l3d = (sl1 * near[None, ..., None]).sum((2, 3, 4))
    bce = (cls_.clamp(min=0) - cls_ * near[None] + torch.log1p(torch.exp(-cls_.abs()))).sum((2, 3))
    res = dict(joints=joints.detach(), l3d_sum=l3d.detach(), bce_sum=bce.detach(), near_sum=near.sum((1, 2)))
    if dj is not None or dl3d is not None or dbce is not None:
        total = sum((o * g.detach().to(dtype)).sum() for o, g in ((joints, dj), (l3d, dl3d), (bce, dbce)) if g is not None)
        total.backward()
        res.update(doff=off_.grad, dcls=cls_.grad)
    return res


def reference_add_layernorm(x, r, keep_mask, p: float, gamma, beta, eps: float = 1e-5, dy=None, dtype=torch.float64):
    """y = LN(x + r * keep_mask / (1 - p)) over the last dimension (biased variance), r / keep_mask None = plain LayerNorm;
    dx, dr (None without r), dgamma, dbeta for dy"""
    x_, g_, b_ = _leaf(x, dtype), _leaf(gamma, dtype), _leaf(beta, dtype)
    r_ = None if r is None else _leaf(r, dtype)
    a = x_
    if r_ is not None:
        a = x_ + (r_ if keep_mask is None else r_ * keep_mask.to(dtype) / (1.0 - p))
    mu = a.mean(-1, keepdim=True)
    var = (a - mu).pow(2).mean(-1, keepdim=True)
    y = (a - mu) * torch.rsqrt(var + eps) * g_ + b_
    res = dict(y=y.detach())
    if dy is not None:
        y.backward(dy.detach().to(dtype))
        res.update(dx=x_.grad, dr=None if r_ is None else r_.grad, dgamma=g_.grad, dbeta=b_.grad)
    return res


# ---- bars: the tensor-wide measure of tests/test_gpu_ops.py and a slice-wise one for tensors whose slices span decades ---------------
def rel_err(got, ref) -> float:
    """largest |got - ref| over the largest |ref| of the whole tensor"""
    return _rel_err(got, ref)


def slice_err(got, ref, slice_dims: int) -> float:
    """the largest, over slices, of (largest |got - ref| of the slice) / (largest |ref| of the slice).  A slice is one index of the
    first ``slice_dims`` dimensions (dcls (L, B, P, J) moved to (L, B, J, P) has slice_dims = 3: one slice per (l, b, j))."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    n = math.prod(ref.shape[:slice_dims])
    g, f = got.reshape(n, -1), ref.reshape(n, -1)
    return float(((g - f).abs().amax(1) / f.abs().amax(1).clamp(min=1e-30)).max())


def slice_bar(ref32, ref64, slice_dims: int, tensor_bar: float) -> Tuple[float, float]:
    """(bar, fp32 error): the slice-wise bar is the larger of the tensor-wide bar and four times the slice-wise error of the SAME formula
    evaluated in float32 on the CPU (ref32) against float64 - a measurement that does not involve the kernel; four allows for another
    summation order"""
    e32 = slice_err(ref32, ref64, slice_dims)
    return max(tensor_bar, 4.0 * e32), e32


# ---- conditions on the inputs: two comparisons flip on a last bit, so no input may sit on their threshold ---------------------------
def vote_points_margin(pts, gt_mm, radius: float) -> float:
    """smallest | ||p - gt / 1000|| - radius | over every (b, p, j), in float64"""
    return float((vote_near(pts, gt_mm, radius)[0] - radius).abs().min())


def condition_vote_points(pts, gt_mm, radius: float, draw, seed: int, margin: float = 1e-6, max_rounds: int = 64):
    """Re-draws (``draw(generator, n) -> (n, 3)`` float32, from a second stream seeded ``seed``) every point of pts (B, P, 3) that has
    any joint with | ||p - gt / 1000|| - radius | < margin, until none is left.  -> (points, number of re-drawn points)"""
    pts = pts.detach().clone()
    g = torch.Generator().manual_seed(seed)
    redrawn = 0
    for _ in range(max_rounds):
        bad = ((vote_near(pts, gt_mm, radius)[0] - radius).abs() < margin).any(-1)         # (B, P)
        n = int(bad.sum())
        if n == 0:
            return pts, redrawn
        pts[bad] = draw(g, n).to(pts.dtype)
        redrawn += n
    raise RuntimeError(f"condition_vote_points: points within {margin} of the radius after {max_rounds} rounds")


def head_rows_margin(h, w, b, clamp: float) -> float:
    """smallest | |tanh(h w + b)| - clamp | over the rows, in float64"""
    return float((reference_sdf_head(h, w, b, clamp)["raw"].abs() - clamp).abs().min())


def condition_head_rows(h, w, b, clamp: float, draw, seed: int, margin: float = 1e-5, max_rounds: int = 64):
    """Re-draws (``draw(generator, n) -> (n, K)`` float32) every row of h (M, K) with | |tanh(h w + b)| - clamp | < margin in float64,
    until none is left.  -> (h, number of re-drawn rows)"""
    h = h.detach().clone()
    g = torch.Generator().manual_seed(seed)
    redrawn = 0
    for _ in range(max_rounds):
        bad = (reference_sdf_head(h, w, b, clamp)["raw"].abs() - clamp).abs() < margin
        n = int(bad.sum())
        if n == 0:
            return h, redrawn
        h[bad] = draw(g, n).to(h.dtype)
        redrawn += n
    raise RuntimeError(f"condition_head_rows: rows within {margin} of the clamp after {max_rounds} rounds")


# ---- the seeded inputs of tests/test_gpu_small_kernels.py for the two conditioned operations (tests/test_small_kernel_refs.py shows,
# without a GPU, that the conditioners end and hold at every one of these shapes)
HEAD_CLAMP = 0.15
HEAD_KS = (4, 256, 260, 512, 1024)             # the forward's; the backward serves K <= 512
HEAD_MS = (1, 5, 4097, 9001)
VOTE_RADIUS = 0.04
VOTE_JS = (1, 20, 21, 64)
VOTE_LBPS = ((1, 1, 1), (3, 2, 5), (3, 2, 257), (1, 1, 1025))
VOTE_CASES = tuple((L, B, P, J) for (L, B, P) in VOTE_LBPS for J in VOTE_JS) + ((6, 86, 520, 4),)
VOTE_FAMILIES = ("randn", "equal", "spike")
VOTE_POINTS_SALT = 2            # (the stream of the point draws; the conditioner makes any stream fit)


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def head_saturated_rows(M: int):
    """rows of a head case put at pre-activation -+20: two of a handful of rows, four of many"""
    return sorted({r for r in ((1, M - 1) if M < 100 else (1, 3, M // 2, M - 1)) if 0 < r < M})


def head_case_inputs(M: int, K: int):
    """h (M, K), w (K), b (1), dsdf (M) of one SDF-head case, conditioned: pre-activations ~ N(-0.02, 0.156^2) - about a third of the
    rows beyond the 0.15 clamp - head_saturated_rows(M) at pre-activation -+20, where tanh is exactly -+1 in float32 and float64;
    no row within 1e-5 of the clamp.  -> (h, w, b, dsdf, rows re-drawn)"""
    g = _gen("head", M, K)
    h = torch.randn(M, K, generator=g)
    w = torch.randn(K, generator=g)
    w = w * (0.156 / float(w.norm()))
    b = torch.tensor([-0.02])
    dsdf = torch.randn(M, generator=g)
    for n, r in enumerate(head_saturated_rows(M)):
        h[r] = w * ((-20.0 if n % 2 else 20.0) / float(w.double().pow(2).sum()))
    h, redrawn = condition_head_rows(h, w, b, HEAD_CLAMP, lambda gg, n: torch.randn(n, K, generator=gg), zlib.crc32(b"head2") + M + K)
    return h, w, b, dsdf, redrawn


def vote_case_points(B: int, P: int, J: int, far_sample=None, salt=None):
    """pts (B, P, 3) ~ N(0, 0.05^2) m and gt (B, J, 3) mm = a point of the sample + N(0, 15^2) mm (so some points lie inside the 40 mm
    radius), ``far_sample``'s joints moved a metre away (none of its points is near); UNCONDITIONED -> (pts, gt, draw)"""
    g = _gen("vote-points", VOTE_POINTS_SALT if salt is None else salt, B, P, J)
    pts = torch.randn(B, P, 3, generator=g) * 0.05
    gt = pts[:, torch.arange(J) % P] * 1000.0 + torch.randn(B, J, 3, generator=g) * 15.0
    if far_sample is not None:
        gt[far_sample] += 1000.0
    return pts, gt, (lambda gg, n: torch.randn(n, 3, generator=gg) * 0.05)


def vote_case_inputs(L: int, B: int, P: int, J: int, family: str, far_sample=None, salt=None):
    """conditioned pts, gt and off (L, B, P, J * 3), cls (L, B, P, J) of the logit ``family``: "randn"; "equal" (every logit 0.75);
    "spike" (randn * 30 - 1e4 with one point per (l, b, j) at +100: exp(100) overflows float32, so a softmax that does not subtract the
    maximum gives Inf / NaN).  -> (off, cls, pts, gt, points re-drawn)"""
    pts, gt, draw = vote_case_points(B, P, J, far_sample, salt)
    pts, redrawn = condition_vote_points(pts, gt, VOTE_RADIUS, draw, zlib.crc32(b"vote2") + P + J)
    g = _gen("vote", L, B, P, J, family)
    off = torch.randn(L, B, P, J * 3, generator=g) * 0.02
    if family == "randn":
        cls = torch.randn(L, B, P, J, generator=g)
    elif family == "equal":
        cls = torch.full((L, B, P, J), 0.75)
    elif family == "spike":
        cls = torch.randn(L, B, P, J, generator=g) * 30.0 - 1e4
        cls.scatter_(2, torch.randint(0, P, (L, B, 1, J), generator=g), 100.0)
    else:
        raise ValueError(family)
    return off, cls, pts, gt, redrawn
