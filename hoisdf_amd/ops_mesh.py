"""Mesh entries (csrc/mesh_sdf.hip, interact.hip, interact_loss.hip, isosurf.hip, field_fit.hip, raster.hip, silhouette_loss.hip).  Stateless:
marshal, size, allocate, one C call (the two losses: one per direction)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import call
from ._marshal import _chk, _counts, _p, _st, _workspace


# ---------------------------------------------------------------------------------------------
# SDF supervision from meshes (csrc/mesh_sdf.hip, the hoisdf_mesh_* entries).  No gradient: these are labels.
# ---------------------------------------------------------------------------------------------
class _Mesh:
    """A batch of meshes as the C ABI takes it: verts (B, V, 3) -> float32; faces (F, 3) shared by the batch or (B, F, 3) per sample,
    any integer dtype -> int32; n_faces (B,) = the rows of each sample that count (None: all F) -> int32.  ``B`` given: the batch the
    mesh must match; ``what`` opens the messages.  ``desc`` is the hoisdf_mesh; the tensors it points to live with this object."""

    def __init__(self, verts, faces, n_faces, B: Optional[int], what: str):
        verts = verts.detach().contiguous().float()
        _chk(verts)
        if verts.dim() != 3 or verts.shape[2] != 3 or (B is not None and verts.shape[0] != B):
            raise ValueError(f"{what} vertices {tuple(verts.shape)}: one (V, 3) mesh per sample" + ("" if B is None else f" of {B}"))
        dev, B = verts.device, verts.shape[0]
        faces = faces.to(dev, torch.int32).contiguous()
        if faces.dim() not in (2, 3) or faces.shape[-1] != 3 or (faces.dim() == 3 and faces.shape[0] != B):
            raise ValueError(f"{what} faces {tuple(faces.shape)}: (F, 3) or ({B}, F, 3)")
        self.verts, self.faces, self.n_faces = verts, faces, _counts(n_faces, B, dev, f"{what} face counts")
        self.B, self.V, self.F = B, verts.shape[1], faces.shape[-2]
        self.stride = 0 if faces.dim() == 2 else 3 * self.F
        self.desc = _lib.Mesh(verts=verts.data_ptr(), faces=faces.data_ptr(), n_faces=None if self.n_faces is None else self.n_faces.data_ptr(),
                              face_batch_stride=self.stride, V=self.V, max_faces=self.F)


class PreparedMesh(_Mesh):
    """hoisdf_mesh_prepare on a batch of meshes: verts (B, V, 3); faces (F, 3) shared by the batch or (B, F, 3) per sample, any
    integer dtype; n_faces (B,) = the rows of each sample that count (None: all F).  Holds tris / area / cdf / box on the device."""

    def __init__(self, verts, faces, n_faces=None):
        super().__init__(verts, faces, n_faces, None, "mesh:")
        B, F, dev = self.B, self.F, self.verts.device
        self.tris = torch.empty(B, F, 12, device=dev, dtype=torch.float32)
        self.area = torch.empty(B, F, device=dev, dtype=torch.float32)
        self.cdf = torch.empty(B, F, device=dev, dtype=torch.float32)
        self.box = torch.empty(B, 8, device=dev, dtype=torch.float32)
        call("hoisdf_mesh_prepare", _p(self.verts), B, self.V, _p(self.faces), self.stride, _p(self.n_faces), F, _p(self.tris),
             _p(self.area), _p(self.cdf), _p(self.box), _st())


def _as_prepared(verts, faces, n_faces) -> PreparedMesh:
    return verts if isinstance(verts, PreparedMesh) else PreparedMesh(verts, faces, n_faces)


def _mesh_pair(what: str, hand_verts, hand_faces, hand_n_faces, obj_verts, obj_faces, obj_n_faces):
    """-> (hand mesh, object mesh of the hand's batch); a mesh whose vertices are None stays None (the rasteriser takes either alone)"""
    mh = None if hand_verts is None else _Mesh(hand_verts, hand_faces, hand_n_faces, None, f"{what}: hand")
    mo = None if obj_verts is None else _Mesh(obj_verts, obj_faces, obj_n_faces, mh and mh.B, f"{what}: object")
    return mh, mo


@torch.no_grad()
def mesh_sdf(points, verts, faces=None, n_faces=None, vert_label=None, out=None, extras: bool = False):
    """Exact signed distance of points (B, N, >= 3) (xyz first, unit inner stride) to the mesh of their sample; ``verts`` may be a
    PreparedMesh.  vert_label (V,) shared or (B, V) ints: also the label of the nearest vertex-corner.  ``out`` (B, N) float32 view
    with any element stride inside a row block (e.g. ``rows[..., 3]``) receives the distances in place.
    -> sdf (B, N) [, label (B, N) int32]; with extras a dict: sdf, face, bary, winding [, label]."""
    m = _as_prepared(verts, faces, n_faces)
    if points.dim() != 3 or points.shape[0] != m.B or points.shape[2] < 3:
        raise ValueError(f"mesh_sdf: points {tuple(points.shape)} for {m.B} meshes")
    if points.stride(2) != 1 or points.stride(0) != points.shape[1] * points.stride(1) or points.dtype != torch.float32:
        points = points.float().contiguous()
    _chk(points)
    B, N, dev = m.B, points.shape[1], points.device
    if out is None:
        out = torch.empty(B, N, device=dev, dtype=torch.float32)
    if out.shape != (B, N) or out.dtype != torch.float32 or (N and out.stride(0) != N * out.stride(1)) or out.stride(1) < 1:
        raise ValueError("mesh_sdf: out must be a (B, N) float32 view whose rows follow each other")
    _chk(out)
    lab = stride = None
    if vert_label is not None:
        lab = vert_label.to(dev, torch.int32).contiguous()
        if lab.shape not in ((m.V,), (B, m.V)):
            raise ValueError(f"mesh_sdf: vert_label {tuple(lab.shape)} for {m.V} vertices")
        stride = 0 if lab.dim() == 1 else m.V
    label = torch.empty(B, N, device=dev, dtype=torch.int32) if lab is not None else None
    face = torch.empty(B, N, device=dev, dtype=torch.int32) if extras else None
    bary = torch.empty(B, N, 3, device=dev, dtype=torch.float32) if extras else None
    wind = torch.empty(B, N, device=dev, dtype=torch.float32) if extras else None
    call("hoisdf_mesh_sdf", _p(points), points.stride(1), B, N, _p(m.tris), _p(m.box), _p(m.n_faces), m.F, _p(lab), stride or 0,
         _p(out), out.stride(1) if N else 1, _p(face), _p(bary), _p(wind), _p(label), _st())
    if extras:
        r = {"sdf": out, "face": face, "bary": bary, "winding": wind}
        if label is not None:
            r["label"] = label
        return r
    return out if label is None else (out, label)


@torch.no_grad()
def mesh_sample_points(verts, faces=None, n_faces=None, n_points: int = 0, sigma=(0.01, 0.003), uniform_every: int = 16,
                       pad: float = 0.05, seed: int = 0, with_faces: bool = False):
    """n_points query points per sample around the mesh (``verts`` may be a PreparedMesh): near-surface with sigma[0] / sigma[1],
    every ``uniform_every``-th uniform in the box padded by ``pad``; a pure function of (seed, sample, index).
    -> points (B, n_points, 3) [, face (B, n_points) int32: the face a near-surface point started from, -1 for a box point]"""
    m = _as_prepared(verts, faces, n_faces)
    dev = m.tris.device
    pts = torch.empty(m.B, n_points, 3, device=dev, dtype=torch.float32)
    face = torch.empty(m.B, n_points, device=dev, dtype=torch.int32) if with_faces else None
    call("hoisdf_mesh_sample_points", _p(m.tris), _p(m.cdf), _p(m.box), _p(m.n_faces), m.F, m.B, n_points, float(sigma[0]),
         float(sigma[1]), int(uniform_every), float(pad), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(pts), 3, _p(face), _st())
    return (pts, face) if with_faces else pts


@torch.no_grad()
def mesh_sdf_rows(hand_verts, hand_faces, obj_verts, obj_faces, obj_n_faces, hand_vert_label, n_hand: int, n_obj: int,
                  sigma=(0.01, 0.003), uniform_every: int = 16, pad: float = 0.05, clamp: float = 0.05, seed: int = 0):
    """hoisdf_mesh_sdf_rows: hand mesh (B, Vh, 3) with shared faces (Fh, 3), object mesh (B, Vo, 3) with faces (B, Fo, 3) (or
    shared (Fo, 3)) and face counts obj_n_faces (B,) or None -> rows (B, n_hand + n_obj, 6) = [x y z sdf_hand sdf_obj label]."""
    mh, mo = _mesh_pair("mesh_sdf_rows", hand_verts, hand_faces, None, obj_verts, obj_faces, obj_n_faces)
    dev, B = mh.verts.device, mh.B
    lab = hand_vert_label.to(dev, torch.int32).contiguous()
    if lab.shape != (mh.V,) or mh.faces.dim() != 2:
        raise ValueError("mesh_sdf_rows: hand faces (Fh, 3) shared by the batch, one label per hand vertex")
    ws, nws = _workspace("hoisdf_mesh_sdf_rows_workspace_bytes", B, mh.F, mo.F, dev)
    rows = torch.empty(B, n_hand + n_obj, 6, device=dev, dtype=torch.float32)
    call("hoisdf_mesh_sdf_rows", C.addressof(mh.desc), C.addressof(mo.desc), _p(lab), B, n_hand, n_obj, float(sigma[0]), float(sigma[1]),
         int(uniform_every), float(pad), float(clamp), int(seed) & 0x7FFFFFFFFFFFFFFF, _p(rows), 6, _p(ws), nws, _st())
    return rows


# ---------------------------------------------------------------------------------------------
# Hand-object interaction metrics (csrc/interact.hip, hoisdf_eval_interaction).  No gradient: these are evaluation numbers.
# ---------------------------------------------------------------------------------------------
@torch.no_grad()
def eval_interaction(hand_verts, hand_faces, obj_verts, obj_faces, obj_n_faces=None, obj_n_verts=None, contact_dist: float = 0.005,
                     voxel: float = 0.005, want_mask: bool = False, hand_n_faces=None):
    """hoisdf_eval_interaction: hand mesh (B, Vh, 3) with shared faces (Fh, 3) (per-sample (B, Fh, 3) with counts hand_n_faces (B,)
    is taken too), object mesh (B, Vo, 3) with faces (B, Fo, 3) (or
    shared (Fo, 3)), face counts obj_n_faces (B,) and vertex counts obj_n_verts (B,) or None; one frame, metres -> a dict of
    per-sample tensors: pen_hand, pen_obj, min_dist, volume float32 (B,); contact_verts, in_contact, inside_count int32 (B,);
    grid float32 (B, 8) = lo xyz, cell xyz, the bits of n_x | n_y << 8 | n_z << 16, 0; with want_mask also inside uint8
    (B, 64^3): 1 where cell ix + n_x (iy + n_y iz) lies in both meshes, zero from n_x n_y n_z on.  want_mask may be that tensor:
    it is written in place, and its bytes from n_x n_y n_z on are left as they are."""
    mh, mo = _mesh_pair("eval_interaction", hand_verts, hand_faces, hand_n_faces, obj_verts, obj_faces, obj_n_faces)
    dev, B = mh.verts.device, mh.B
    ov = _counts(obj_n_verts, B, dev, "eval_interaction: obj_n_verts")
    ws, nws = _workspace("hoisdf_eval_interaction_workspace_bytes", B, mh.V, mh.F, mo.V, mo.F, dev)
    f32 = dict(device=dev, dtype=torch.float32)
    i32 = dict(device=dev, dtype=torch.int32)
    out = {"pen_hand": torch.empty(B, **f32), "pen_obj": torch.empty(B, **f32), "min_dist": torch.empty(B, **f32),
           "contact_verts": torch.empty(B, **i32), "in_contact": torch.empty(B, **i32), "volume": torch.empty(B, **f32),
           "inside_count": torch.empty(B, **i32), "grid": torch.empty(B, 8, **f32)}
    cells = _lib.CONSTANTS["INTERACT_MAX_GRID"] ** 3
    mask = None
    if torch.is_tensor(want_mask):
        mask = want_mask
        if mask.shape != (B, cells) or mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.device != dev:
            raise ValueError(f"eval_interaction: the mask must be a contiguous uint8 tensor of shape ({B}, {cells}) on {dev}")
    elif want_mask:
        mask = torch.zeros(B, cells, device=dev, dtype=torch.uint8)
    call("hoisdf_eval_interaction", C.addressof(mh.desc), C.addressof(mo.desc), _p(ov), B, float(contact_dist), float(voxel), _p(out["pen_hand"]),
         _p(out["pen_obj"]), _p(out["min_dist"]), _p(out["contact_verts"]), _p(out["in_contact"]), _p(out["volume"]),
         _p(out["inside_count"]), _p(mask), _p(out["grid"]), _p(ws), nws, _st())
    if mask is not None:
        out["inside"] = mask
    return out


# ---------------------------------------------------------------------------------------------
# Hand-object interaction loss (csrc/interact_loss.hip, hoisdf_interaction_loss_fwd / _bwd): repulsion and attraction with gradients
# to both vertex arrays.
# ---------------------------------------------------------------------------------------------
def _loss_weight(w, B: int, V: int, dev, what: str):
    """a per-vertex weight array -> (tensor or None, batch stride in elements): (V,) shared by the batch, (B, V) per sample"""
    if w is None:
        return None, 0
    w = torch.as_tensor(w).detach().to(dev, torch.float32).contiguous()
    if w.shape not in ((V,), (B, V)):
        raise ValueError(f"interaction_loss: {what} {tuple(w.shape)}: ({V},) or ({B}, {V})")
    return w, (0 if w.dim() == 1 else V)


class _InteractionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hand_verts, obj_verts, mh, mo, ov, weights, alpha):
        # mh / mo: the two meshes marshalled from (detached copies of) hand_verts / obj_verts, which are here for the graph alone
        dev, B = mh.verts.device, mh.B
        ws, nws = _workspace("hoisdf_interaction_loss_workspace_bytes", B, mh.V, mh.F, mo.V, mo.F, dev)
        out = [torch.empty(B, device=dev, dtype=torch.float32) for _ in range(3)]
        (wr, sr), (wa, sa), (wo, so) = weights
        common = (C.addressof(mh.desc), C.addressof(mo.desc), _p(ov), B, _p(wr), sr, _p(wa), sa, _p(wo), so, float(alpha))
        call("hoisdf_interaction_loss_fwd", *common, _p(out[0]), _p(out[1]), _p(out[2]), _p(ws), nws, _st())
        # the backward reads the workspace and every input again: all of them (the meshes hold the tensors their descriptors point
        # to) stay alive, and unchanged, with the context
        ctx.keep = (mh, mo, ov, wr, wa, wo, ws)
        ctx.common, ctx.nws = common, nws
        ctx.set_materialize_grads(False)
        return tuple(out)

    @staticmethod
    def backward(ctx, g_rep_hand, g_att, g_rep_obj):
        mh, mo = ctx.keep[0], ctx.keep[1]
        gs = [None if g is None else g.contiguous().float() for g in (g_rep_hand, g_att, g_rep_obj)]
        _chk(*gs)
        d_hand, d_obj = torch.empty_like(mh.verts), torch.empty_like(mo.verts)
        call("hoisdf_interaction_loss_bwd", *ctx.common, _p(gs[0]), _p(gs[1]), _p(gs[2]), _p(d_hand), _p(d_obj), _p(ctx.keep[-1]), ctx.nws, _st())
        return d_hand, d_obj, None, None, None, None, None


def interaction_loss(hand_verts, hand_faces, obj_verts, obj_faces, obj_n_faces=None, obj_n_verts=None, rep_w_hand=None,
                     att_w_hand=None, rep_w_obj=None, alpha: float = 0.01, hand_n_faces=None):
    """hoisdf_interaction_loss_fwd / _bwd: the meshes as ``eval_interaction`` takes them (one frame, metres); rep_w_hand, att_w_hand
    (Vh,) or (B, Vh) and rep_w_obj (Vo,) or (B, Vo) per-vertex weights, None = ones; alpha: the length at which the attraction
    saturates -> (rep_hand, att, rep_obj), each (B,): the weighted means of max(0, -sdf_obj) and alpha tanh(max(0, sdf_obj) / alpha)
    over the hand vertices and of max(0, -sdf_hand) over the object's vertices that count.  Gradients flow to hand_verts and obj_verts
    only (the envelope rule of include/hoisdf.h "interaction loss"); order-fixed: two calls give the same bits."""
    mh, mo = _mesh_pair("interaction_loss", hand_verts, hand_faces, hand_n_faces, obj_verts, obj_faces, obj_n_faces)
    _chk(hand_verts, obj_verts)                              # the gradients go back as float32: no other dtype is taken
    dev, B = mh.verts.device, mh.B
    ov = _counts(obj_n_verts, B, dev, "interaction_loss: obj_n_verts")
    weights = (_loss_weight(rep_w_hand, B, mh.V, dev, "rep_w_hand"), _loss_weight(att_w_hand, B, mh.V, dev, "att_w_hand"),
               _loss_weight(rep_w_obj, B, mo.V, dev, "rep_w_obj"))
    return _InteractionLoss.apply(hand_verts, obj_verts, mh, mo, ov, weights, float(alpha))


# ---------------------------------------------------------------------------------------------
# Surface from a sampled field (csrc/isosurf.hip, the hoisdf_iso_* entries and hoisdf_eval_surface).  No gradient.
# ---------------------------------------------------------------------------------------------
def _iso_grid(grid, n: int):
    grid = grid.contiguous().float()
    _chk(grid)
    if grid.dim() != 2 or grid.shape[1] != 8:
        raise ValueError(f"iso: grid {tuple(grid.shape)} must be (B, 8) = lo xyz, cell xyz, 0, 0")
    if not 2 <= int(n) <= _lib.CONSTANTS["ISO_MAX_GRID"]:
        raise ValueError(f"iso: n={n} (2 .. {_lib.CONSTANTS['ISO_MAX_GRID']})")
    return grid, grid.shape[0], int(n) ** 3


def _iso_values(values, B: int, N: int, what: str):
    """(B, n^3) float32 view whose rows follow each other, any element stride (a column of a wider row block) -> (view, ld)"""
    if values.dim() != 2 or values.shape != (B, N) or values.dtype != torch.float32 or values.stride(1) < 1 or \
            (B > 1 and values.stride(0) != N * values.stride(1)):
        values = values.reshape(B, N).float().contiguous()
    _chk(values)
    return values, values.stride(1)


@torch.no_grad()
def iso_grid_points(grid, n: int, with_sample_idx: bool = True):
    """grid (B, 8) -> points (B n^3, 3) [, sample_idx (B n^3,) int32]: the node positions as rows for sdf_query"""
    grid, B, N = _iso_grid(grid, n)
    pts = torch.empty(B * N, 3, device=grid.device, dtype=torch.float32)
    idx = torch.empty(B * N, device=grid.device, dtype=torch.int32) if with_sample_idx else None
    call("hoisdf_iso_grid_points", _p(grid), int(n), B, _p(pts), _p(idx), _st())
    return (pts, idx) if with_sample_idx else pts


@torch.no_grad()
def iso_refine_grid(values, grid, n: int, iso: float = 0.0, pad_cells: int = 1, n_out: Optional[int] = None):
    """values (B, n^3) on grid (B, 8) -> the (B, 8) grid of n_out nodes over the index box of the nodes below iso, grown by
    pad_cells and clipped to the coarse grid (a sample without such a node: the coarse grid re-divided).  No host read."""
    grid, B, N = _iso_grid(grid, n)
    values, ld = _iso_values(values, B, N, "iso_refine_grid")
    out = torch.empty(B, 8, device=grid.device, dtype=torch.float32)
    call("hoisdf_iso_refine_grid", _p(values), ld, _p(grid), int(n), B, float(iso), int(pad_cells), int(n if n_out is None else n_out),
         _p(out), _st())
    return out


@torch.no_grad()
def iso_surface(values, grid, n: int, iso: float = 0.0, max_verts: Optional[int] = None, max_faces: Optional[int] = None,
                out_scale: Optional[float] = None, out_shift=None):
    """hoisdf_iso_extract: values (B, n^3) on grid (B, 8) -> (verts (B, max_verts, 3), faces (B, max_faces, 3) int32, n_verts (B,),
    n_faces (B,) int32): the counts NEEDED; rows beyond them are not written (zero here), and a sample whose count exceeds a
    capacity is overflowed - its written faces keep their true vertex ids.  With both capacities given nothing synchronises;
    a capacity left None is sized from one count-only call and one read of the counts (exact allocation).  out_scale /
    out_shift (B, 3): the stored vertex is x * out_scale + out_shift."""
    grid, B, N = _iso_grid(grid, n)
    values, ld = _iso_values(values, B, N, "iso_surface")
    dev = grid.device
    shift = None
    if out_shift is not None or out_scale is not None:
        shift = torch.zeros(B, 3, device=dev, dtype=torch.float32) if out_shift is None else out_shift.reshape(B, 3).contiguous().float()
        _chk(shift)
    scale = 1.0 if out_scale is None else float(out_scale)
    ws, nws = _workspace("hoisdf_iso_extract_workspace_bytes", B, int(n), dev)
    nv =torch.zeros(B, device=dev, dtype=torch.int32)
    nf = torch.zeros(B, device=dev, dtype=torch.int32)

    def run(verts, faces, mv, mf):
        call("hoisdf_iso_extract", _p(values), ld, _p(grid), int(n), B, float(iso), scale, _p(shift), _p(verts), mv, _p(faces), mf,
             _p(nv), _p(nf), _p(ws), nws, _st())

    if max_verts is None or max_faces is None:
        run(None, None, 0, 0)
        counts = torch.stack([nv, nf]).amax(1).tolist() if B else [0, 0]      # the one sized read-back
        max_verts = counts[0] if max_verts is None else max_verts
        max_faces = counts[1] if max_faces is None else max_faces
    verts = torch.zeros(B, int(max_verts), 3, device=dev, dtype=torch.float32)
    faces = torch.zeros(B, int(max_faces), 3, device=dev, dtype=torch.int32)
    run(verts, faces, int(max_verts), int(max_faces))
    return verts, faces, nv, nf


@torch.no_grad()
def field_fit(values, grid, n: int, points, n_points=None, pivot=None, iters: int = 32, huber: float = 0.1, lambda0: float = 1e-3,
              step_tol: float = 1e-7, min_used_percent: int = 50, want=()):
    """hoisdf_field_fit: the points (B, V, 3), in the frame of the field ``values`` (B, n^3) on ``grid`` (B, 8), moved as a rigid
    body onto the field's zero level set (include/hoisdf.h "field fit"; the rules: hoisdf_amd/field_fit_oracle.py).  n_points (B,)
    or None: the rows of each sample that count (rows beyond are not read; their rows of points_out stay zero); pivot (B, 3) or
    None = the mean of the sample's points.  iters + 2 launches, nothing synchronises; order-fixed: two calls give the same bits.
    -> a dict of device tensors: rot (B, 3, 3), trans (B, 3), points_out (B, V, 3) float32; cost (B, 2) float64 = start, end;
    info (B, 4) int32 = points taking part at the start, at the end, steps tried, steps accepted; and what ``want`` names of
    normal (B, 56) float64 = the start pose's 28 sums and their magnitude sums, pose64 (B, 12) float64 = R, t unrounded."""
    grid, B, N = _iso_grid(grid, n)
    if values.dim() != 2 or values.shape != (B, N) or values.dtype != torch.float32 or values.stride(1) != 1 or \
            (B > 1 and values.stride(0) < N):
        values = values.reshape(B, N).float().contiguous()
    points = points.contiguous().float()
    _chk(values, points)
    if points.dim() != 3 or points.shape[0] != B or points.shape[2] != 3:
        raise ValueError(f"field_fit: points {tuple(points.shape)}: (V, 3) per sample of {B}")
    unknown = set(want) - {"normal", "pose64"}
    if unknown:
        raise ValueError(f"field_fit: want names {sorted(unknown)}; 'normal' and 'pose64' exist")
    dev, V = grid.device, points.shape[1]
    ld = values.stride(0) if B > 1 else max(values.stride(0), N)
    nv = _counts(n_points, B, dev, "field_fit: n_points")
    if pivot is not None:
        pivot = pivot.reshape(B, 3).contiguous().float()
        _chk(pivot)
    ws, nws = _workspace("hoisdf_field_fit_workspace_bytes", B, dev)
    f64 = dict(device=dev, dtype=torch.float64)
    out = {"rot": torch.empty(B, 3, 3, device=dev, dtype=torch.float32), "trans": torch.empty(B, 3, device=dev, dtype=torch.float32),
           "points_out": torch.zeros(B, V, 3, device=dev, dtype=torch.float32), "cost": torch.empty(B, 2, **f64),
           "info": torch.empty(B, 4, device=dev, dtype=torch.int32)}
    normal = torch.empty(B, 56, **f64) if "normal" in want else None
    pose64 = torch.empty(B, 12, **f64) if "pose64" in want else None
    call("hoisdf_field_fit", _p(values), ld, _p(grid), int(n), _p(points), V, _p(nv), _p(pivot), B, int(iters), float(huber),
         float(lambda0), float(step_tol), int(min_used_percent), _p(out["rot"]), _p(out["trans"]), _p(out["points_out"]),
         _p(out["cost"]), _p(out["info"]), _p(normal), _p(pose64), _p(ws), nws, _st())
    if normal is not None:
        out["normal"] = normal
    if pose64 is not None:
        out["pose64"] = pose64
    return out


@torch.no_grad()
def eval_surface(pred_verts, pred_n_verts, gt_verts, gt_faces, gt_n_faces=None, n_samples: int = 2048, seed: int = 0,
                 extras: bool = False):
    """hoisdf_eval_surface: predicted vertices (B, max_verts, 3) with counts (B,) against the ground-truth mesh gt_verts (B, V, 3),
    gt_faces (F, 3) shared or (B, F, 3) with counts gt_n_faces -> a dict of (B,) tensors: pred_to_gt, gt_to_pred, chamfer (mean
    squared distances, square metres) and n_used int32 (0: the sample has no predicted vertex or no usable face, and zeros).
    With extras also samples (B, n_samples, 3), the points drawn on the ground-truth surface, and nearest (B, n_samples) int32."""
    pred_verts = pred_verts.contiguous().float()
    _chk(pred_verts)
    if pred_verts.dim() != 3 or pred_verts.shape[2] != 3:
        raise ValueError(f"eval_surface: predicted {tuple(pred_verts.shape)}: (B, max_verts, 3)")
    dev, B, mv = pred_verts.device, pred_verts.shape[0], pred_verts.shape[1]
    m = _Mesh(gt_verts, gt_faces, gt_n_faces, B, "eval_surface: ground-truth")
    pn = _counts(pred_n_verts, B, dev, "eval_surface: pred_n_verts")
    ws, nws = _workspace("hoisdf_eval_surface_workspace_bytes", B, mv, m.F, int(n_samples), dev)
    out ={"pred_to_gt": torch.empty(B, device=dev, dtype=torch.float32), "gt_to_pred": torch.empty(B, device=dev, dtype=torch.float32),
           "chamfer": torch.empty(B, device=dev, dtype=torch.float32), "n_used": torch.empty(B, device=dev, dtype=torch.int32)}
    samples = torch.empty(B, int(n_samples), 3, device=dev, dtype=torch.float32) if extras else None
    nearest = torch.empty(B, int(n_samples), device=dev, dtype=torch.int32) if extras else None
    call("hoisdf_eval_surface", _p(pred_verts), _p(pn), mv, C.addressof(m.desc), B, int(n_samples), int(seed) & 0xFFFFFFFFFFFFFFFF,
         _p(out["pred_to_gt"]), _p(out["gt_to_pred"]), _p(out["chamfer"]), _p(out["n_used"]), _p(samples), _p(nearest), _p(ws), nws, _st())
    if extras:
        out["samples"], out["nearest"] = samples, nearest
    return out


# ---------------------------------------------------------------------------------------------
# Mesh rasteriser (csrc/raster.hip: hoisdf_raster_meshes, hoisdf_raster_overlay, hoisdf_eval_silhouette).  No gradient.
# ---------------------------------------------------------------------------------------------
@torch.no_grad()
def raster_meshes(hand_verts, hand_faces, obj_verts, obj_faces, K, width: int, height: int, hand_n_faces=None, obj_n_faces=None,
                  half_pixel: bool = False, near: float = 0.01, hm_shape=None, want=("ids", "depth", "counts"), out=None):
    """hoisdf_raster_meshes: the hand mesh (B, Vh, 3) and the object mesh (B, Vo, 3), one camera frame, metres, faces (F, 3) shared
    or (B, F, 3) with counts (B,), either mesh None; K (B, 6) or (B, 2, 3) = the top two rows of the camera matrix -> a dict with
    what `want` names: ids int32 (B, height, width) (-1: background, else mesh << 16 | face row), depth float32 (0: background),
    counts int32 (B, 2) = visible pixels per mesh and, with hm_shape = (hm_h, hm_w), hand_seg / obj_seg float32 (B, hm_h, hm_w):
    the modal masks under the NEAREST fold of image_crop.  `out`: a dict of tensors to write into instead of new ones."""
    if hand_verts is None and obj_verts is None:
        raise ValueError("raster_meshes: one mesh at least")
    mh, mo = _mesh_pair("raster_meshes", hand_verts, hand_faces, hand_n_faces, obj_verts, obj_faces, obj_n_faces)
    dev, B = (mh or mo).verts.device, (mh or mo).B
    K = K.to(dev).float().reshape(B, 6).contiguous()
    _chk(K)
    names = list(want) + (["hand_seg", "obj_seg"] if hm_shape is not None else [])
    shapes = {"ids": ((B, int(height), int(width)), torch.int32), "depth": ((B, int(height), int(width)), torch.float32),
              "counts": ((B, 2), torch.int32)}
    if hm_shape is not None:
        shapes["hand_seg"] = shapes["obj_seg"] = ((B, int(hm_shape[0]), int(hm_shape[1])), torch.float32)
    res = {}
    for k in names:
        shape, dtype = shapes[k]
        t = None if out is None else out.get(k)
        if t is None:
            t = torch.empty(shape, device=dev, dtype=dtype)
        elif tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"raster_meshes: out[{k!r}] must be a contiguous {dtype} tensor of shape {shape} on {dev}")
        res[k] = t
    ws, nws = _workspace("hoisdf_raster_workspace_bytes", B, mh.F if mh else 0, mo.F if mo else 0, dev)
    hm_h, hm_w = (int(hm_shape[0]), int(hm_shape[1])) if hm_shape is not None else (0, 0)
    call("hoisdf_raster_meshes", mh and C.addressof(mh.desc), mo and C.addressof(mo.desc), _p(K), B, int(width),
         int(height), int(bool(half_pixel)), float(near), _p(res.get("ids")), _p(res.get("depth")), _p(res.get("hand_seg")),
         _p(res.get("obj_seg")), hm_w, hm_h, _p(res.get("counts")), _p(ws), nws, _st())
    return res


@torch.no_grad()
def raster_overlay(ids, image, colour=((70, 130, 255), (255, 160, 40)), alpha: int = 160, out=None):
    """hoisdf_raster_overlay: ids int32 (B, H, W) of raster_meshes over image uint8 (B, H, W, 3) -> uint8 (B, H, W, 3): a covered pixel
    is (alpha colour[mesh] + (256 - alpha) image + 128) >> 8 with colour = (hand rgb, object rgb), a background pixel is copied.
    out may be `image` itself (in place)."""
    ids = ids.contiguous()
    image = image.contiguous()
    if not ids.is_cuda or image.device != ids.device:
        raise RuntimeError("hoisdf_amd ops need CUDA/HIP tensors on one device (no CPU fallback)")
    if ids.dtype != torch.int32 or image.dtype != torch.uint8 or ids.dim() != 3 or tuple(image.shape) != tuple(ids.shape) + (3,):
        raise ValueError(f"raster_overlay: ids int32 (B, H, W) {tuple(ids.shape)} and image uint8 (B, H, W, 3) {tuple(image.shape)}")
    if out is None:
        out = torch.empty_like(image)
    elif out.shape != image.shape or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != image.device:
        raise ValueError("raster_overlay: out must be a contiguous uint8 tensor of the image's shape on its device")
    col = (C.c_uint8 * 6)(*[int(c) for m in colour for c in m])
    B, H, W = ids.shape
    call("hoisdf_raster_overlay", _p(ids), _p(image), _p(out), C.addressof(col), int(alpha), B, W, H, _st())
    return out


@torch.no_grad()
def eval_silhouette(pred_hand, pred_obj, gt_hand, gt_obj):
    """hoisdf_eval_silhouette: four masks (B, ...) float32, set where > 0.5 -> int32 (B, 4): hand intersection, hand union, object
    intersection, object union of predicted against ground truth (integer sums on the device)"""
    B = pred_hand.shape[0]
    masks = [m.reshape(B, -1).float().contiguous() for m in (pred_hand, pred_obj, gt_hand, gt_obj)]
    _chk(*masks)
    if any(m.shape != masks[0].shape for m in masks):
        raise ValueError(f"eval_silhouette: four masks of one shape, got {[tuple(m.shape) for m in masks]}")
    counts = torch.empty(B, 4, device=masks[0].device, dtype=torch.int32)
    call("hoisdf_eval_silhouette", *[_p(m) for m in masks], B, masks[0].shape[1], _p(counts), _st())
    return counts


# ---------------------------------------------------------------------------------------------
# Silhouette loss (csrc/silhouette_loss.hip: hoisdf_mask_edt, hoisdf_silhouette_loss_fwd / _bwd): a mask's exact distance transform,
# and one projected point set held to a pair of mask maps, with the gradient to the points.
# ---------------------------------------------------------------------------------------------
def _mask_maps(what: str, *masks):
    """float masks (B, h, w) of one shape (None stays None) -> contiguous float32 tensors, B, h, w"""
    ms = [None if m is None else m.detach().float().contiguous() for m in masks]
    _chk(*ms)
    first = next(m for m in ms if m is not None)
    if first.dim() != 3 or any(m is not None and m.shape != first.shape for m in ms):
        raise ValueError(f"{what}: masks of one shape (B, h, w), got {[None if m is None else tuple(m.shape) for m in ms]}")
    return ms, first.shape[0], first.shape[1], first.shape[2]


@torch.no_grad()
def mask_edt(mask, mask_or=None, want_nearest: bool = False):
    """hoisdf_mask_edt: mask (B, h, w) float32, set where > 0.5 (with mask_or: the union of the two) -> d2 int32 (B, h, w): the exact
    squared distance in pixels^2 to the nearest set pixel (0 at a set pixel, EDT_NONE = 2^30 in a sample without one); with
    want_nearest also nearest int32 (B, h, w): the index y' w + x' of a nearest set pixel, the lowest on a tie (-1 without one)."""
    if mask is None:
        raise ValueError("mask_edt: a mask")
    (mask, mask_or), B, h, w = _mask_maps("mask_edt", mask, mask_or)
    d2 = torch.empty(B, h, w, device=mask.device, dtype=torch.int32)
    nearest = torch.empty_like(d2) if want_nearest else None
    call("hoisdf_mask_edt", _p(mask), _p(mask_or), B, w, h, _p(d2), _p(nearest), _st())
    return (d2, nearest) if want_nearest else d2


def silhouette_workspace_views(ws, B: int, V: int, h: int, w: int):
    """the pieces of a hoisdf_silhouette_loss_fwd workspace (the layout include/hoisdf.h states: each piece rounded up to 256
    bytes) as tensors over it -> dict: u, v float64 (B, V), cell int32 (B, V), nearest int32 (B, h, w), den float64 (B, 2)"""
    up = lambda n: (n + 255) // 256 * 256
    out, off = {}, 0
    for name, dtype, shape in (("u", torch.float64, (B, V)), ("v", torch.float64, (B, V)), ("cell", torch.int32, (B, V)),
                               ("nearest", torch.int32, (B, h, w)), ("den", torch.float64, (B, 2))):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        out[name] = ws[off:off + n].view(dtype).view(shape)
        off += up(n)
    return out


class _SilhouetteLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, verts, K, allow_d2, cover, nv, weight, stride, near):
        dev, (B, V, _) = verts.device, verts.shape
        h, w = cover.shape[1:]
        v = verts.detach().contiguous()
        ws, nws = _workspace("hoisdf_silhouette_loss_workspace_bytes", B, V, w, h, dev)
        inside, cov = torch.empty(B, device=dev, dtype=torch.float32), torch.empty(B, device=dev, dtype=torch.float32)
        common = (_p(v), _p(nv), V, _p(K), B, _p(allow_d2), _p(cover), w, h, float(near), _p(weight), stride)
        call("hoisdf_silhouette_loss_fwd", *common, _p(inside), _p(cov), _p(ws), nws, _st())
        # the backward reads the workspace and every input again: they stay alive, and unchanged, with the context
        ctx.keep = (v, nv, K, allow_d2, cover, weight, ws)
        ctx.common, ctx.nws = common, nws
        ctx.set_materialize_grads(False)
        return inside, cov

    @staticmethod
    def backward(ctx, g_inside, g_cover):
        gs = [None if g is None else g.contiguous().float() for g in (g_inside, g_cover)]
        _chk(*gs)
        d_verts = torch.empty_like(ctx.keep[0])
        call("hoisdf_silhouette_loss_bwd", *ctx.common, _p(gs[0]), _p(gs[1]), _p(d_verts), _p(ctx.keep[-1]), ctx.nws, _st())
        return d_verts, None, None, None, None, None, None, None


def silhouette_loss(verts, K, allow_d2, cover, n_verts=None, weight=None, near: float = 0.01):
    """hoisdf_silhouette_loss_fwd / _bwd: verts (B, V, 3) camera frame, metres; K (B, 6) or (B, 2, 3) FOR THE MASK GRID (mask pixel
    (px, py) sits at (px, py): render.mask_camera_rows); allow_d2 int32 (B, h, w) of ``mask_edt``: where the projected vertices may
    lie; cover float32 (B, h, w), set where > 0.5: the pixels that want a projected vertex near them; n_verts (B,) or None: rows
    from there on are padding; weight (V,) or (B, V) or None = ones -> (inside, cover), each (B,), in mask pixels: the weighted mean
    over the vertices of the bilinear read of sqrt(allow_d2) plus the distance back onto the map, and the mean over cover's set
    pixels of the distance to the nearest projected vertex.  The gradient flows to verts only; order-fixed: two calls give the
    same bits."""
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise ValueError(f"silhouette_loss: verts {tuple(verts.shape)} must be (B, V, 3)")
    _chk(verts)
    dev, (B, V, _) = verts.device, verts.shape
    (cover,), Bm, h, w = _mask_maps("silhouette_loss", cover)
    allow_d2 = allow_d2.contiguous()
    if Bm != B or tuple(allow_d2.shape) != (B, h, w) or allow_d2.dtype != torch.int32 or allow_d2.device != dev or cover.device != dev:
        raise ValueError(f"silhouette_loss: allow_d2 int32 and cover float32, both ({B}, h, w) on {dev}; got {tuple(allow_d2.shape)} "
                         f"{allow_d2.dtype} and {tuple(cover.shape)}")
    K = K.detach().to(dev).float().reshape(B, 6).contiguous()
    nv = _counts(n_verts, B, dev, "silhouette_loss: n_verts")
    if weight is not None:
        weight = torch.as_tensor(weight).detach().to(dev, torch.float32).contiguous()
        if weight.shape not in ((V,), (B, V)):
            raise ValueError(f"silhouette_loss: weight {tuple(weight.shape)}: ({V},) or ({B}, {V})")
    stride = 0 if weight is None or weight.dim() == 1 else V
    return _SilhouetteLoss.apply(verts, K, allow_d2, cover, nv, weight, stride, float(near))
