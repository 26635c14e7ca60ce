"""Inference behind single C entries (include/hoisdf.h): the whole post-encoder model (csrc/pose_infer.hip), the evaluation-mode
convolutions (csrc/conv.hip), the image encoder (csrc/encoder_infer.hip) and the IK launch of csrc/mano.hip.  Stateless: nothing
here reads the step's seeds, arena or emulation switches."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from ._lib import PoseOutputs, Pyramid, call, lib
from ._marshal import _PreparedBlob, _QueuedCounts, _after_prepared, _check_survivors, _chk, _p, _size, _st


# ---------------------------------------------------------------------------------------------
# whole-model inference behind one C entry (include/hoisdf.h hoisdf_pose_*; csrc/pose_infer.hip)
# ---------------------------------------------------------------------------------------------
class PosePrepared(_PreparedBlob):
    """The prepared blob of hoisdf_pose_prepare for one (descriptor, weights) pair: device memory + the descriptor it was built
    for.  ``version`` counts the builds of the owning model (tests pin that a second frame does not prepare again)."""

    def __init__(self, desc, weights, device, version: int = 0):
        nbytes = _size("hoisdf_pose_prepared_bytes", C.addressof(desc))
        super().__init__(desc, version, nbytes, device, lambda blob: call(
            "hoisdf_pose_prepare", C.addressof(desc), C.addressof(weights), _p(blob), nbytes, _st()))


class PoseInferCounts(_QueuedCounts):
    """hoisdf_pose_infer_begin: the queued survivor counts of both fields (2 B words: hand, object), their page-locked host copy and
    the event behind the copy - as SdfInferCounts, for the whole-model entry."""

    def __init__(self, desc, root, ocen, cam_intr, bbox_hand, bbox_obj):
        self.args = tuple(t.contiguous() for t in (root, ocen, cam_intr, bbox_hand, bbox_obj))
        _chk(*self.args)
        B = root.shape[0]
        self.B = B
        super().__init__(2 * B, root.device, lambda counts, host: call(
            "hoisdf_pose_infer_begin", C.addressof(desc), *(_p(t) for t in self.args), _p(counts), host, _st()))


@torch.no_grad()
def pose_infer(prepared: PosePrepared, pyr: "PyramidNHWC", root, ocen, cam_intr, bbox_hand, bbox_obj, counts: Optional[PoseInferCounts] = None,
               side_stream=None, debug: bool = False):
    """hoisdf_pose_infer: the eval forward of everything after the image encoder in ONE C-ABI call -> dict of the ``*_out`` tensors
    (with ``debug`` also the selected points and their SDF values; with the descriptor's ``ik_solve`` also ``ik_joints_out`` /
    ``ik_verts_out`` / ``ik_pose_out`` / ``ik_valid_out``, root-relative).  Raises ValueError when a sample has fewer lattice survivors
    than requested points (nothing is launched then)."""
    d = prepared.desc
    dev = root.device
    if counts is None:
        counts = PoseInferCounts(d, root, ocen, cam_intr, bbox_hand, bbox_obj)
    root, ocen, cam_intr, bbox_hand, bbox_obj = counts.args
    B, nh, no = d.B, d.num_samp_hand, d.num_samp_obj
    e = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
    out = {"hand_joints_out": e(B, 20, 3), "obj_rot_out": e(B, no, 3), "obj_trans_out": e(B, no, 3)}
    c_names = {}                 # this dict's key -> the field of hoisdf_pose_outputs, where they differ
    if d.use_inverse_kinematics:
        out["mano_shape_out"] = e(B, 10)
        if d.ik_solve:           # the IK post-process as the call's last launch, under the keys engine.Tester.predict uses
            out.update(ik_joints_out=e(B, 21, 3), ik_verts_out=e(B, 778, 3), ik_pose_out=e(B, 48),
                       ik_valid_out=torch.empty(B, device=dev, dtype=torch.int32))
            c_names = {"ik_joints_out": "mano_joints_out", "ik_verts_out": "mano_mesh_out", "ik_pose_out": "mano_pose_out"}
    else:
        out["mano_mesh_out"], out["mano_joints_out"] = e(B, 778, 3), e(B, 21, 3)
    if debug:
        out.update(hand_points_out=e(B, nh, 3), obj_points_out=e(B, no, 3), hand_sdf_out=e(B, nh), obj_sdf_out=e(B, no))
    cl = counts.wait()          # the one host read of the path: everything that does not need the counts is done
    counts_h = (C.c_int32 * (2 * B))(*cl)
    for kind, n, part in (("hand", nh, cl[:B]), ("obj", no, cl[B:])):
        _check_survivors(part, n, f"sdf_infer({kind})")
    nbytes = _size("hoisdf_pose_infer_workspace", C.addressof(d), C.addressof(counts_h))
    ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    o = PoseOutputs(**{c_names.get(k, k): v.data_ptr() for k, v in out.items()})
    _after_prepared(prepared, dev)
    s = pyr.struct()
    call("hoisdf_pose_infer", C.addressof(d), _p(prepared.blob), C.byref(s), _p(root), _p(ocen), _p(cam_intr), _p(bbox_hand), _p(bbox_obj),
         _p(counts.counts), C.addressof(counts_h), C.addressof(o), _p(ws), nbytes,
         None if side_stream is None else C.c_void_p(side_stream.cuda_stream), _st())
    return out          # (the call returns with the current stream ordered behind the side stream's work: no record_stream needed)


# ---------------------------------------------------------------------------------------------
# convolution forward on channels-last maps (include/hoisdf.h hoisdf_conv*; csrc/conv.hip): exact f32, evaluation only
# ---------------------------------------------------------------------------------------------
CONV_ACT = {None: 0, "none": 0, "relu": 1, "sigmoid": 2}


class ConvWeight:
    """A convolution's weight packed once for the implicit-GEMM kernel (hoisdf_conv_pack_weight), an evaluation-mode BatchNorm folded
    in when ``bn`` = (gamma, beta, running_mean, running_var, eps) is given.  ``w``: [C_out][C_in][KH][KW], or ConvTranspose2d's
    [C_in][C_out][4][4] with ``transposed``."""

    def __init__(self, w, bias=None, bn=None, transposed: bool = False):
        g, be, mu, var, eps = bn if bn is not None else (None, None, None, None, 0.0)
        ts = [t if t is None else t.detach().contiguous() for t in (w, bias, g, be, mu, var)]
        _chk(*ts)
        self.transposed = bool(transposed)
        self.C_out, self.C_in = (w.shape[1], w.shape[0]) if transposed else (w.shape[0], w.shape[1])
        self.KH, self.KW = w.shape[2], w.shape[3]
        n = lib().hoisdf_conv_packed_floats(self.C_out, self.C_in, self.KH, self.KW)
        self.packed = torch.empty(n, device=w.device, dtype=torch.float32)
        self.bias = torch.empty((self.C_out + 3) // 4 * 4, device=w.device, dtype=torch.float32)
        call("hoisdf_conv_pack_weight", *(_p(t) for t in ts), float(eps), self.C_out, self.C_in, self.KH, self.KW, int(self.transposed),
             _p(self.packed), _p(self.bias), _st())


def conv_plan(M: int, C_out: int, K: int, classes: int = 1):
    """(tile, splitk) the convolution takes for M output rows, C_out columns and a contraction of K (classes = 4: transposed)"""
    tile, splitk = C.c_int(0), C.c_int(0)
    call("hoisdf_conv_plan", M, C_out, K, classes, C.addressof(tile), C.addressof(splitk))
    return tile.value, splitk.value


def _conv_ws(M, C_out, K, classes, device):
    n = _size("hoisdf_conv_workspace_bytes", M, C_out, K, classes)
    return (torch.empty(n, device=device, dtype=torch.uint8) if n else None), n


def _nhwc_slice(x):
    """a channels-last map or a channel slice of one: [B][H][W][C] with unit channel stride and dense pixels -> row stride"""
    B, H, W, Cc = x.shape
    ld = x.stride(2)
    if x.stride(3) != 1 or ld < Cc or x.stride(1) != W * ld or x.stride(0) != H * W * ld:
        raise ValueError("expected an NHWC map (or a channel slice of one) with dense pixels")
    return ld


@torch.no_grad()
def conv2d_nhwc(x, w: ConvWeight, stride: int = 1, pad: int = 0, act=None, residual=None, out=None, c_off: int = 0):
    """y = act(conv(x) + bias (+ residual)) on NHWC maps; ``x`` / ``residual`` / ``out`` may be channel slices of wider maps, or
    ``out`` a wider map whose channels [c_off, c_off + C_out) are written.  ConvTranspose2d(4, 2, 1) when ``w`` was packed transposed."""
    _chk(x, residual, out)
    B, H, W, _ = x.shape
    ldx = _nhwc_slice(x)
    if w.transposed:
        OH, OW, M, K, classes = 2 * H, 2 * W, B * H * W, 4 * w.C_in, 4
    else:
        OH, OW = (H + 2 * pad - w.KH) // stride + 1, (W + 2 * pad - w.KW) // stride + 1
        M, K, classes = B * OH * OW, w.KH * w.KW * w.C_in, 1
    if out is None:
        out = torch.empty(B, OH, OW, w.C_out, device=x.device, dtype=torch.float32)
    if tuple(out.shape[:3]) != (B, OH, OW) or c_off < 0 or out.shape[3] < c_off + w.C_out or x.shape[3] != w.C_in:
        raise ValueError(f"conv2d_nhwc: x {tuple(x.shape)} / out {tuple(out.shape)} do not fit the weight")
    ldy = _nhwc_slice(out)
    ws, nws = _conv_ws(M, w.C_out, K, classes, x.device)
    if w.transposed:
        if residual is not None:
            raise ValueError("the transposed convolution takes no residual")
        call("hoisdf_conv_transpose2d_fwd", _p(x), ldx, _p(w.packed), _p(w.bias), _p(out), ldy, c_off, B, H, W, w.C_in, w.C_out, CONV_ACT[act],
             _p(ws), nws, _st())
    else:
        ldr = 0 if residual is None else _nhwc_slice(residual)
        call("hoisdf_conv2d_fwd", _p(x), ldx, _p(w.packed), _p(w.bias), _p(residual), ldr, _p(out), ldy, c_off, B, H, W, w.C_in, w.C_out, w.KH,
             w.KW, stride, pad, CONV_ACT[act], _p(ws), nws, _st())
    return out[..., c_off:c_off + w.C_out]


@torch.no_grad()
def maxpool2d_nhwc(x):
    """MaxPool2d(3, 2, 1) of an NHWC map"""
    _chk(x)
    B, H, W, Cc = x.shape
    y = torch.empty(B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc, device=x.device, dtype=torch.float32)
    call("hoisdf_maxpool2d_fwd", _p(x), _nhwc_slice(x), _p(y), Cc, B, H, W, Cc, _st())
    return y


# ---------------------------------------------------------------------------------------------
# the image encoder in evaluation mode behind one C entry (include/hoisdf.h hoisdf_encoder_*; csrc/encoder_infer.hip)
# ---------------------------------------------------------------------------------------------
def encoder_tensor_table(desc):
    """[(checkpoint key, numel)] in the order hoisdf_encoder_prepare takes the tensors"""
    L, d = lib(), C.addressof(desc)
    n = _size("hoisdf_encoder_tensor_count", d)
    return [(L.hoisdf_encoder_tensor_name(d, i).decode(), L.hoisdf_encoder_tensor_numel(d, i)) for i in range(n)]


class EncoderPrepared(_PreparedBlob):
    """The prepared blob of hoisdf_encoder_prepare (BatchNorm folds + packed weights) for one (descriptor, weights) pair and the
    workspace of its frames.  ``tensors``: checkpoint key -> tensor, for every key of the table."""

    def __init__(self, desc, tensors, device, version: int = 0):
        table = encoder_tensor_table(desc)
        keep = []
        for name, numel in table:
            t = tensors[name].detach().float().contiguous()
            if t.numel() != numel:
                raise ValueError(f"{name}: {t.numel()} elements, the table has {numel}")
            keep.append(t)
        _chk(*keep)
        nbytes = _size("hoisdf_encoder_prepared_bytes", C.addressof(desc))
        nws = _size("hoisdf_encoder_infer_workspace", C.addressof(desc))
        self.workspace = torch.empty(nws, device=device, dtype=torch.uint8)
        ptrs = (C.c_void_p * len(keep))(*(t.data_ptr() for t in keep))
        super().__init__(desc, version, nbytes, device, lambda blob: call(
            "hoisdf_encoder_prepare", C.addressof(desc), ptrs, len(keep), _p(blob), nbytes, _st()))
        shape = Pyramid()
        call("hoisdf_encoder_pyramid_shape", C.addressof(desc), C.byref(shape))
        self.level_shapes = [(desc.B, shape.H[i], shape.W[i], shape.C[i]) for i in range(shape.n_levels)]


@torch.no_grad()
def encoder_infer(prepared: EncoderPrepared, img, want_aux: bool = True):
    """hoisdf_encoder_infer: ``img`` (B, 3, H, W) as the dataset yields it (a channels_last tensor is passed without a copy, anything
    else through one permute-copy) -> (PyramidNHWC, aux NHWC [B][H / 2][W / 2][3] or None)"""
    d = prepared.desc
    if tuple(img.shape) != (d.B, 3, d.img_h, d.img_w):
        raise ValueError(f"encoder_infer: image {tuple(img.shape)}, prepared for {(d.B, 3, d.img_h, d.img_w)}")
    x = img.permute(0, 2, 3, 1)
    if not x.is_contiguous():
        x = x.contiguous()
    _chk(x)
    dev = x.device
    levels = [torch.empty(s, device=dev, dtype=torch.float32) for s in prepared.level_shapes]
    aux = torch.empty(d.B, d.img_h // 2, d.img_w // 2, 3, device=dev, dtype=torch.float32) if want_aux else None
    _after_prepared(prepared, dev)
    ptrs = (C.c_void_p * len(levels))(*(t.data_ptr() for t in levels))
    call("hoisdf_encoder_infer", C.addressof(d), _p(prepared.blob), _p(x), ptrs, _p(aux), _p(prepared.workspace), prepared.workspace.numel(), _st())
    from .ops import PyramidNHWC            # at call time: the class belongs to the step (shared_grad, the arena-backed accumulator)
    return PyramidNHWC(levels), aux


# ---------------------------------------------------------------------------------------------
# (f3) the closed-form inverse kinematics + the MANO layer on its result (csrc/mano.hip, hoisdf_ik_mano_fwd)
# ---------------------------------------------------------------------------------------------
@torch.no_grad()
def ik_mano(joints, betas, assets):
    """(f3) the closed-form inverse kinematics of the IK variant + the MANO layer on its result in ONE launch (hoisdf_ik_mano_fwd):
    joints (H,21,3) metres with the wrist in row 0, or (H,20,3) = joints 1..20 relative to a wrist at the origin; betas (H, >= 10)
    with unit inner stride (any row stride) or None = zeros; assets as mano_head takes them (hands_mean must be zero) ->
    pose (H,48) axis-angle, verts (H,778,3) and joints (H,21,3) in metres at the input wrist, valid (H,) int32 = 0 where the palm
    fit is a reflection (that hand keeps the zero pose)."""
    joints = joints.contiguous().float()
    H, nj = joints.shape[0], joints.shape[1]
    assert joints.dim() == 3 and nj in (20, 21) and joints.shape[2] == 3, tuple(joints.shape)
    ld = 0
    if betas is not None:
        betas = betas.float()
        assert betas.dim() == 2 and betas.shape[0] == H and betas.shape[1] >= 10, tuple(betas.shape)
        if betas.stride(1) != 1 or betas.stride(0) < 10:
            betas = betas[:, :10].contiguous()
        ld = betas.stride(0)
    _chk(joints, betas)
    dev = joints.device
    pose = torch.empty(H, 48, device=dev, dtype=torch.float32)
    verts = torch.empty(H, 778, 3, device=dev, dtype=torch.float32)
    out_joints = torch.empty(H, 21, 3, device=dev, dtype=torch.float32)
    valid = torch.empty(H, device=dev, dtype=torch.int32)
    image, tmpl, jreg, w = assets[:4]
    call("hoisdf_ik_mano_fwd", _p(joints), nj, _p(betas), ld, H, _p(image), _p(tmpl), _p(jreg), _p(w), _p(pose), _p(verts), _p(out_joints),
         _p(valid), _st())
    return pose, verts, out_joints, valid
