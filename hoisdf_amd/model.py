"""``Model`` / ``get_model``: drop-in for the reference's main/model.py surface with the hot path
(everything after the CNN encoder/decoder) running on hand-written gfx950 kernels.

Same constructor-level module names (state-dict schema of SURVEY.md Appendix D), same
``forward(inputs, targets, meta_info, mode, epoch_cnt, batch_ratio)`` signature and the
``*_out`` key convention (main/train.py:111-112).  Differences, all internal:
  * tokens are batch-first (B,S,256) and the pyramid is consumed channels-last;
  * ``sdf_infer`` is batched on the device (lattice -> bbox compaction -> SDF -> exact top-K),
    one host read of B survivor counts per field instead of 2*B CPU<->GPU hops
    (reference main/model.py:285-352);
  * the dense-grid selection returns the same *set* in the same ascending-|sdf| order.
Reference line numbers are cited per method.
"""
from __future__ import annotations

import contextlib
import dataclasses
import os
import random
import weakref
from typing import Dict

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._marshal import _chk
from .config import cfg as _global_cfg
from .nets.blocks import MLP, SDFDecoder, Transformer, VoteTransformer
from .nets.encoder import BackboneNet, DecoderNet
from .nets.heads import JointvoteLoss, ManoHead, ManoLoss, ManoShapeLoss, SepSDFLoss
from .nets.mano import ManoLayer


def get_mano_tgt_mask(cfg=_global_cfg):
    """common/utils/misc.py:11-31 - True = masked."""
    n = cfg.mano_num_queries
    m = torch.ones(n, n, dtype=torch.bool)
    m[0, 0] = False
    for i in range(5):
        m[3 * i + 1:3 * i + 4, 3 * i + 1:3 * i + 4] = False
    m[cfg.mano_shape_indx, cfg.mano_shape_indx] = False
    return m


def get_mano_memory_mask(cfg=_global_cfg):
    """common/utils/misc.py:42-47."""
    m = torch.zeros(cfg.mano_num_queries, cfg.num_samp_hand + cfg.num_samp_obj, dtype=torch.bool)
    m[:, cfg.num_samp_hand:] = True
    return m


def get_manoshape_memory_mask(cfg=_global_cfg):
    """common/utils/misc.py:34-39."""
    m = torch.zeros(1, cfg.num_samp_hand + cfg.num_samp_obj, dtype=torch.bool)
    m[:, cfg.num_samp_hand:] = True
    return m


# per-model cache of the hoisdf_sdf_query_fwd weight descriptors (ctypes structs of raw device pointers): kept OUT of the
# module's __dict__ so that copy.deepcopy(model) / torch.save(model) never see them
_SDFQ_CACHE = weakref.WeakKeyDictionary()
# per-model cache of the prepared blob of the whole-model C entry (ops.PosePrepared), keyed like the folds above
_POSE_CACHE = weakref.WeakKeyDictionary()
# the same for the image encoder's blob (ops.EncoderPrepared); created only when the native encoder is asked for
_ENCODER_CACHE = weakref.WeakKeyDictionary()


@dataclasses.dataclass
class _Field:
    """One of the two point sets of a step.  Declared: what differs between the hand and the object copy of the per-field sequence
    (the decoder follows from ``kind``; the input / bbox keys are ``{kind}_pre_points``, ``{kind}_sdf_points``, ``bbox_{kind}``).
    Model._query_points, _field_step and _own_token_rows fill in the others: points (B,n,3) in the field's frame; sdf_pred (B,P,1)
    on the SDF-loss points; feat (B n,C) gathered pixels, with gradient; cam (B,n,3) camera points; sdf (B,n,1) / pe (B,n,30) of the
    points in their own field and x_sdf / x_pe re-centred in the other field, detached; fea (B,n,223) token-MLP output; tok (B,S,D)."""
    kind: str                           # "hand" | "obj"
    center: torch.Tensor                # (B,3) mano_root | obj_center_cam
    scale: float                        # cfg.hand_sdf_scale | cfg.obj_sdf_scale
    n: int                              # cfg.num_samp_hand | cfg.num_samp_obj
    beta: nn.Parameter                  # hand_sigmoid_beta | obj_sigmoid_beta
    points = sdf_pred = feat = cam = sdf = pe = x_sdf = x_pe = fea = tok = None


class _StreamPlan:
    """One- or two-stream issue of a step: THE decision (cfg.overlap_streams, HOISDF_TWO_STREAMS, single-stream in deterministic
    mode; ``allow``: the caller's own condition) and the model's second stream, made on first use.  ``fork``: the side stream waits
    for what the ambient one holds so far; ``join``: the ambient stream waits for the side stream; both take the tensors the
    waiting stream will read of the other (None entries skipped).  With one stream they do nothing and ``on_side`` runs its block
    in place.  Autograd replays every op's backward on its forward stream."""

    def __init__(self, model, device, allow=True):
        self.two = allow and bool(getattr(model.cfg, "overlap_streams", True)) and os.environ.get("HOISDF_TWO_STREAMS", "1") != "0" \
            and not ops.deterministic()
        if self.two and model._side_stream is None:
            # HIGH priority = a hardware queue of its own.  HIP maps normal-priority streams onto 4 hardware queues
            # round-robin: once a RCCL process group has created its streams, a normal-priority second stream lands on
            # the compute stream's queue and the two never overlap (measured with world 1 through RCCL: 95.6 vs 91.3
            # ms/step, zero concurrent kernels in the trace; GPU_MAX_HW_QUEUES=8 cures it as well).  Without a process
            # group the priority changes nothing (92.8 vs 92.9 ms/step).
            model._side_stream = torch.cuda.Stream(device=device, priority=-1)
        self.side, self.cur = (model._side_stream, torch.cuda.current_stream(device)) if self.two else (None, None)

    def on_side(self):
        return torch.cuda.stream(self.side) if self.two else contextlib.nullcontext()

    def fork(self, *made_on_cur):
        self._edge(self.side, self.cur, made_on_cur)

    def join(self, *made_on_side):
        self._edge(self.cur, self.side, made_on_side)

    def _edge(self, waiter, other, tensors):
        if self.two:
            waiter.wait_stream(other)
            for t in tensors:
                if t is not None:
                    t.record_stream(waiter)


class Model(nn.Module):
    def __init__(self, backbone_net, decoder_net, hand_sdf_decoder, obj_sdf_decoder, hand_transformer,
                 obj_transformer, mano_layer, cfg=_global_cfg):
        super().__init__()
        self.cfg = cfg
        self.backbone_net = backbone_net
        self.decoder_net = decoder_net
        self.hand_sdf_decoder = hand_sdf_decoder
        self.obj_sdf_decoder = obj_sdf_decoder
        self.hand_transformer = hand_transformer
        self.obj_transformer = obj_transformer
        self.hand_sigmoid_beta = nn.Parameter(0.1 * torch.ones(1))
        self.obj_sigmoid_beta = nn.Parameter(0.1 * torch.ones(1))
        D, C = cfg.hidden_dim, cfg.mutliscale_dim
        self.norm1 = nn.LayerNorm(C)                       # defined, never applied (reference :55)
        self.linear_transformerin = MLP(C, [1024, 512, 256], D - cfg.PointFeatSize, 4, True)
        self.linear_sdfin = MLP(C, [512], D, 2, True)
        coord_change_mat = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])
        if cfg.use_inverse_kinematics:
            self.mano_query_embed = nn.Embedding(1, D)
        else:
            self.mano_query_embed = nn.Embedding(cfg.mano_num_queries, D)
            self.mano_head = ManoHead(mano_layer, coord_change_mat=coord_change_mat)
            self.linear_pose = MLP(D, D, 6, 3)
        self.linear_shape = MLP(D, D, 10, 3)
        self.linear_handvote = MLP(D, D, 20 * 3, 4)
        self.linear_handcls = MLP(D, D, 20, 3)
        self.linear_objvote = MLP(D, D, 8 * 3, 4)          # unused in forward (reference :86-87)
        self.linear_objcls = MLP(D, D, 8, 3)
        self.linear_obj_rel_trans = MLP(D, D, 3, 3)
        self.linear_obj_rot = MLP(D, D, 3, 3)
        self.joints_vote_loss = JointvoteLoss(cfg.hand_cls_dist)
        self.sdf_loss = SepSDFLoss()
        if cfg.use_inverse_kinematics:
            self.mano_shape_loss = ManoShapeLoss(cfg.lambda_manoshape, cfg.mano_lambda_regulshape)
        else:
            self.mano_loss = ManoLoss(cfg.lambda_verts3d, cfg.lambda_joints3d, cfg.lambda_manopose,
                                      cfg.lambda_manoshape)
        self.freeze_stages()
        self._py_random = random            # the p < 0.4 branch draw (reference :426); injectable for tests
        self._jitter = None                 # test hook: callable(like, d) -> jitter tensor
        self._side_stream = None            # the second HIP stream, made by the first two-stream _stream_plan
        # the IK variant owns no MANO layer (its state_dict has no mano_head.*): the layer its native post-process solves with is a
        # plain attribute, NOT a registered submodule (the checkpoint schema stays as it is)
        self.set_ik_mano_layer(mano_layer if cfg.use_inverse_kinematics else None)
        self.set_interaction_source(None)
        if cfg.use_inverse_kinematics and self.interaction_loss_enabled():
            raise ValueError("cfg.interaction_loss needs the predicted hand mesh in training: the IK variant (cfg.use_inverse_kinematics) has none")
        if cfg.use_inverse_kinematics and self.silhouette_loss_enabled():
            raise ValueError("cfg.silhouette_loss needs the predicted hand mesh in training: the IK variant (cfg.use_inverse_kinematics) has none")

    def set_ik_mano_layer(self, mano_layer):
        object.__setattr__(self, "ik_mano_layer", mano_layer)

    def interaction_loss_enabled(self) -> bool:
        """cfg.interaction_loss (default False) or HOISDF_INTERACTION_LOSS=1: training adds interaction_rep / interaction_att"""
        return bool(getattr(self.cfg, "interaction_loss", False)) or os.environ.get("HOISDF_INTERACTION_LOSS", "") == "1"

    def silhouette_loss_enabled(self) -> bool:
        """cfg.silhouette_loss (default False) or HOISDF_SILHOUETTE_LOSS=1: training adds silhouette_in / silhouette_cover"""
        return bool(getattr(self.cfg, "silhouette_loss", False)) or os.environ.get("HOISDF_SILHOUETTE_LOSS", "") == "1"

    def set_interaction_source(self, source, att_w_hand=None, rep_w_hand=None, rep_w_obj=None):
        """the meshes of the interaction loss (and of the silhouette loss, which poses the same pair): a ``sdf_data.MeshSdfSource`` (object templates + the MANO layer's faces; the Trainer
        hands its own over) and the per-vertex weights - ``att_w_hand`` (778,) defaults to sdf_data.contact_zone_weights of the
        source's layer, the two repulsion weights to ones.  A plain attribute, no submodule: the checkpoint schema stays as it is"""
        if source is not None and att_w_hand is None:
            from .sdf_data import contact_zone_weights
            att_w_hand = contact_zone_weights(source.layer.th_weights)
        object.__setattr__(self, "_interaction", None if source is None else (source, att_w_hand, rep_w_hand, rep_w_obj))

    def _predicted_pair(self, hand_rel, obj_rot, obj_trans, meta_info, what):
        """The PREDICTED pair of a training step in the camera frame, the one place where the mesh losses pose it: hand = the MANO
        mesh + mano_root, object = the template obj_cls turned and moved in torch by the mean votes + obj_center_cam, so autograd
        carries a vertex gradient on to both vote heads.  -> hand (B, 778, 3), obj (B, V, 3), the packed templates gathered per
        sample (faces, n_faces, n_verts), used (B,) bool: obj_cls >= 0 (a sample that is not used borrows template 0: give it
        the counts 0)"""
        if self._interaction is None:
            raise RuntimeError(f"cfg.{what} needs the meshes: Model.set_interaction_source(MeshSdfSource) (the Trainer does it)")
        if "obj_cls" not in meta_info:
            raise KeyError(f"cfg.{what} needs meta_info['obj_cls']: the object template of every sample (-1: none)")
        from .metrics import batch_rodrigues
        src = self._interaction[0]
        dev = hand_rel.device
        tm = src.to(dev).templates
        cls = meta_info["obj_cls"].to(dev).long().view(-1)
        used, k = cls >= 0, cls.clamp_min(0)
        hand = hand_rel + meta_info["mano_root"][:, None]
        R = batch_rodrigues(obj_rot[-1].mean(1))
        obj = tm["verts"][k] @ R.transpose(1, 2) + (obj_trans[-1].mean(1) + meta_info["obj_center_cam"])[:, None]
        zero = torch.zeros_like(tm["n_faces"][k])
        return hand, obj, tm["faces"][k], torch.where(used, tm["n_faces"][k], zero), torch.where(used, tm["n_verts"][k], zero), used

    def _interaction_losses(self, hand_rel, obj_rot, obj_trans, meta_info, loss):
        """The predicted hand against the predicted object (hoisdf_interaction_loss_fwd / _bwd): loss["interaction_rep"] = the
        repulsion of both directions, loss["interaction_att"] = the attraction of the hand's contact zones, each (B,).  The object
        is posed in torch from the mean votes, so autograd carries the vertex gradient on to both vote heads; a sample without an
        evaluated object (obj_cls < 0) has face and vertex count 0 and adds 0."""
        hand, obj, obj_faces, obj_nf, obj_nv, _ = self._predicted_pair(hand_rel, obj_rot, obj_trans, meta_info, "interaction_loss")
        src, att_w, rep_wh, rep_wo = self._interaction
        rep_hand, att, rep_obj = ops.interaction_loss(
            hand, src.layer.th_faces, obj, obj_faces, obj_nf, obj_nv,
            rep_wh, att_w, rep_wo, float(self.cfg.interaction_alpha))
        loss["interaction_rep"] = rep_hand + rep_obj
        loss["interaction_att"] = att

    def _silhouette_losses(self, hand_rel, obj_rot, obj_trans, targets, meta_info, loss):
        """The predicted pair against the mask targets (hoisdf_mask_edt, hoisdf_silhouette_loss_fwd / _bwd, once per mesh):
        loss["silhouette_in"] = how far the projected vertices lie outside hand_seg OR obj_seg (the masks are modal: a hand vertex
        hidden behind the object is no error), loss["silhouette_cover"] = how far the pixels of each mesh's own mask lie from its
        nearest projected vertex; each (B,), the hand's plus the object's, in mask pixels divided by the mask width.  A sample
        without an evaluated object (obj_cls < 0) has object vertex count 0 and adds the hand's share alone."""
        from .render import mask_camera_rows
        hand, obj, _, _, obj_nv, _ = self._predicted_pair(hand_rel, obj_rot, obj_trans, meta_info, "silhouette_loss")
        B = hand.shape[0]
        hand_seg, obj_seg = (targets[k].reshape(B, *targets[k].shape[-2:]) for k in ("hand_seg", "obj_seg"))
        K = mask_camera_rows(meta_info["cam_intr"].to(hand.device), self.cfg)
        allow = ops.mask_edt(hand_seg, obj_seg)
        near = float(self.cfg.raster_near)
        in_h, cov_h = ops.silhouette_loss(hand, K, allow, hand_seg, near=near)
        in_o, cov_o = ops.silhouette_loss(obj, K, allow, obj_seg, n_verts=obj_nv, near=near)
        width = float(hand_seg.shape[-1])
        loss["silhouette_in"] = (in_h + in_o) / width
        loss["silhouette_cover"] = (cov_h + cov_o) / width

    def _ik_layer(self, device):
        """the IK solve's layer on ``device``: as no submodule it does not follow Model.to, so the first native call moves it (once)"""
        ml = self.ik_mano_layer
        if ml.th_shapedirs.device != torch.device(device):
            ml.to(device)
        return ml

    def freeze_stages(self):
        if self.backbone_net is None:
            return
        for name, p in self.backbone_net.named_parameters():
            if "bn" in name:
                p.requires_grad = False

    # ---- pieces ---------------------------------------------------------------------------
    def _pyramid(self, feature_pyramid) -> ops.PyramidNHWC:
        if isinstance(feature_pyramid, ops.PyramidNHWC):
            return feature_pyramid
        return ops.PyramidNHWC.from_nchw([feature_pyramid[k] for k in self.cfg.mutliscale_layers])

    def sdf_activation(self, input, beta):
        """reference :123-126 (sigma = sigmoid(sdf/beta)/beta, beta floored in place)."""
        beta.data.clamp_(min=2e-3)
        return torch.sigmoid(input / beta) / beta

    def _sdf_rows(self, pyr, points, center, cam_intr, scale, kind, sample_idx=None, want_class=False):
        """K1-K4 on a flat list of points: returns (sdf clamped (n,), sdf_raw (n,), pe (n,30), cam (n,3)) and, with ``want_class``
        (cfg.ClassifierBranch: the public sdf_forward / sdf_infer hand the decoder's class logits back, main/model.py:236-240 -
        nothing in Model.forward reads them, so the hot path never asks), the logits (n,6) as a fifth element."""
        c = self.cfg
        dec = self.hand_sdf_decoder if kind == "hand" else self.obj_sdf_decoder
        if (not want_class and sample_idx is None and torch.is_grad_enabled() and ops.sdf_query_train_ok()
                and pyr.C == self.linear_sdfin.layers[0].weight.shape[1]):
            # one C-ABI call per direction (hoisdf_sdf_query_train_fwd / hoisdf_sdf_query_bwd)
            lin = self.linear_sdfin.layers
            routed = [lin[0].weight, lin[0].bias, lin[1].weight, lin[1].bias]
            for i in range(4):
                l = getattr(dec, f"linh{i}")
                routed += [l.effective_weight(), l.bias]
            routed += [dec.linh4.weight, dec.linh4.bias]
            sdf, pe, cam = ops.sdf_query_train(self._query_weights(kind), pyr, points, center, cam_intr, scale, c.ClampingDistance,
                                               c.input_img_shape, dec.dropout_prob if dec.training else 0.0, routed)
            return sdf, None, pe, cam
        feat, cam = ops.project_gather(pyr, points, center, cam_intr, scale, c.input_img_shape, sample_idx)
        fea = self.linear_sdfin(feat)
        pts = points.reshape(-1, 3)
        pe = ops.posenc(pts)
        # decoder input rows [feat256 | pe30 | xyz3] in a 292-wide (16-byte aligned) buffer
        n = pts.shape[0]
        x0 = torch.cat([fea, pe, pts, pts.new_zeros(n, 3)], dim=1)[:, :c.hidden_dim + c.PointFeatSize]
        if want_class:
            sdf, raw, cls = dec.forward_clamped(x0, c.ClampingDistance, want_class=True)
            return sdf, raw, pe, cam, cls
        sdf, raw = dec.forward_clamped(x0, c.ClampingDistance)
        return sdf, raw, pe, cam

    def _query_weights(self, kind):
        q = _SDFQ_CACHE.get(self)
        if q is None:
            q = {"hand": ops.SdfQueryWeights(self.linear_sdfin, self.hand_sdf_decoder),
                 "obj": ops.SdfQueryWeights(self.linear_sdfin, self.obj_sdf_decoder)}
            _SDFQ_CACHE[self] = q
        return q[kind]

    def invalidate_sdf_query_weights(self):
        """drop the cached weight-norm folds (call after changing SDF-MLP weights in a way torch's version counters and
        FusedAdamW cannot see, e.g. a foreign kernel writing the parameters in place)"""
        _SDFQ_CACHE.pop(self, None)
        ent = _POSE_CACHE.get(self)
        if ent is not None:
            ent["key"] = None            # the next infer_native prepares again (the build counter keeps counting)
        ent = _ENCODER_CACHE.get(self)
        if ent is not None:
            ent["key"] = None

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.invalidate_sdf_query_weights()
        return r

    @torch.no_grad()
    def _sdf_query(self, pyr, points, center, cam_intr, scale, kind, sample_idx=None, feat=None, want_feat=False):
        """K1-K4 for the call sites whose results are only used detached (reference :483-484,:517-518,:540,:558) and for
        sdf_infer: one C-ABI call (hoisdf_sdf_query_fwd), optionally on rows already gathered for the same camera points.
        Dropout follows the decoder's train()/eval() mode like the reference's module calls do.
        -> (sdf clamped (n,), sdf_raw (n,), pe (n,30), feat (n,C) | None)"""
        c = self.cfg
        dec = self.hand_sdf_decoder if kind == "hand" else self.obj_sdf_decoder
        p = dec.dropout_prob if dec.training else 0.0
        sdf, raw, pe, _, f = ops.sdf_query(self._query_weights(kind), pyr, points, center, cam_intr, scale,
                                           c.ClampingDistance, c.input_img_shape, sample_idx, feat, want_feat, False, p)
        return sdf, raw, pe, f

    def sdf_forward(self, feature_pyramid, sdf_points, center_joint, cam_intr, sdf_scale, type="hand"):
        """reference :181-244 -> (pred_sdf (B,P,1), pred_class (B,P,6) with cfg.ClassifierBranch else None, pos_enc3d (B,P,30))."""
        B, P, _ = sdf_points.shape
        if self.cfg.ClassifierBranch:
            sdf, _, pe, _, cls = self._sdf_rows(self._pyramid(feature_pyramid), sdf_points, center_joint, cam_intr, sdf_scale, type,
                                                want_class=True)
            return sdf.view(B, P, 1), cls.view(B, P, -1), pe.view(B, P, -1)
        sdf, _, pe, _ = self._sdf_rows(self._pyramid(feature_pyramid), sdf_points, center_joint, cam_intr,
                                       sdf_scale, type)
        return sdf.view(B, P, 1), None, pe.view(B, P, -1)

    def get_input_transformer(self, feature_pyramid, sdf_points, center_joint, cam_intr, sdf_scale):
        """reference :145-179 -> (transformer_latent (B,P,223), cam_sdf_points (B,P,3))."""
        B, P, _ = sdf_points.shape
        feat, cam = ops.project_gather(self._pyramid(feature_pyramid), sdf_points, center_joint, cam_intr, sdf_scale,
                                       self.cfg.input_img_shape)
        return self.linear_transformerin(feat).view(B, P, -1), cam.view(B, P, 3)

    @torch.no_grad()
    def sdf_infer(self, feature_pyramid, center_joint, cam_intr, bbox, sdf_scale, num_points, type="hand", counts=None):
        """reference :246-355, batched on the device -> (points (B,K,3), sdf (B,K,1), posenc (B,K,30), class logits (B,K,6) | None).
        ``counts``: the lattice-survivor count queued earlier (``infer_counts_begin``), so that nothing drains here."""
        c = self.cfg
        pyr = self._pyramid(feature_pyramid)
        B = center_joint.shape[0]
        dec = self.hand_sdf_decoder if type == "hand" else self.obj_sdf_decoder
        try:
            pose_points, pose_sdf, pose_pe = ops.sdf_infer(self._query_weights(type), pyr, center_joint, cam_intr, bbox, sdf_scale,
                                                           c.bins_n, num_points, c.ClampingDistance, c.input_img_shape,
                                                           dec.dropout_prob if dec.training else 0.0, counts)
        except ValueError as e:
            raise ValueError(str(e).replace("sdf_infer:", f"sdf_infer({type}):")) from None
        pose_sdf = pose_sdf.unsqueeze(-1)
        pose_class = None
        if c.ClassifierBranch:          # :351-352: the logits of the selected points (the decoder re-evaluated on them)
            pose_class = self.sdf_forward(pyr, pose_points, center_joint, cam_intr, sdf_scale, type)[1]
        return pose_points, pose_sdf, pose_pe, pose_class

    FIELD_CHUNK_ROWS = 262144      # rows of one hoisdf_sdf_query_fwd call of field_surface: one 64^3 sample, 1 GB of gathered rows at C = 992

    @torch.no_grad()
    def field_surface(self, feature_pyramid, meta_info, kind="hand", n=64, coarse_n=32, box=None, return_values=False, *,
                      max_verts=None, max_faces=None, chunk_rows=None, pad_cells=1):
        """The zero level set of the learned hand / object field as an indexed triangle mesh in camera metres (include/hoisdf.h
        "iso-surface"; no reference counterpart).  Coarse grid of ``coarse_n`` nodes per axis over the lattice cube [-1, 1]^3 of
        the scaled frame (``box`` (B, 2, 3): that region per sample instead) -> the field on its nodes -> hoisdf_iso_refine_grid
        (``pad_cells`` = 1: the box of the inside nodes, no host read) -> the field on the ``n`` fine nodes per axis -> hoisdf_iso_extract at
        level 0 of sdf_raw (the unclamped tanh sdf_infer ranks on), vertices stored as x / scale + centre.
        Decoder dropout is off whatever the module's mode.  The queries go in chunks of at most FIELD_CHUNK_ROWS = 262144 rows with
        their sample index (``chunk_rows`` overrides it), of equal size up to a multiple of 256, so hoisdf_sdf_query_workspace stays
        bounded: a gathered row is 4 KB at C = 992, and 22 x 64^3 rows at once would be 23 GB.
        -> (verts (B, max_verts, 3), faces (B, max_faces, 3) int32, n_verts (B,), n_faces (B,) int32: the counts needed) as
        ops.iso_surface returns them: with both capacities given nothing synchronises.  With ``return_values`` a fifth element,
        a dict: values (B, n^3), grid (B, 8), coarse_values (B, coarse_n^3), coarse_grid (B, 8), all in the scaled frame."""
        if kind not in ("hand", "obj"):
            raise ValueError(f"field_surface: kind={kind!r} ('hand' or 'obj')")
        fv = self.field_values(feature_pyramid, meta_info, kind, n, coarse_n, box, chunk_rows=chunk_rows, pad_cells=pad_cells)
        res = ops.iso_surface(fv["values"], fv["grid"], n, 0.0, max_verts, max_faces, out_scale=1.0 / fv["scale"], out_shift=fv["centre"])
        if return_values:
            return res + ({k: fv[k] for k in ("values", "grid", "coarse_values", "coarse_grid")},)
        return res

    @torch.no_grad()
    def field_values(self, feature_pyramid, meta_info, kind="hand", n=64, coarse_n=32, box=None, *, chunk_rows=None, pad_cells=1):
        """The learned hand / object field sampled on its refined grid: the part of ``field_surface`` before the extraction, for
        whoever needs the values themselves (refine.fit_pair).  The grids, the chunking and the dropout rule are field_surface's.
        -> a dict: values (B, n^3), grid (B, 8), coarse_values (B, coarse_n^3), coarse_grid (B, 8), all in the scaled frame
        x_scaled = (x_cam - centre) * scale, and that frame's centre (B, 3) and scale (a float)."""
        c = self.cfg
        if kind not in ("hand", "obj"):
            raise ValueError(f"field_values: kind={kind!r} ('hand' or 'obj')")
        pyr = self._pyramid(feature_pyramid)
        center = (meta_info["mano_root"] if kind == "hand" else meta_info["obj_center_cam"]).reshape(-1, 3).contiguous().float()
        scale = c.hand_sdf_scale if kind == "hand" else c.obj_sdf_scale
        K, B, dev = meta_info["cam_intr"], center.shape[0], center.device
        weights = self._query_weights(kind)
        chunk = int(chunk_rows or self.FIELD_CHUNK_ROWS)

        def field(grid, nodes):
            pts, idx = ops.iso_grid_points(grid, nodes)
            rows = pts.shape[0]
            parts = max(1, -(-rows // chunk))
            per = -(-(-(-rows // parts)) // 256) * 256
            raw = torch.empty(rows, device=dev)
            for s in range(0, rows, per):
                raw[s:s + per] = ops.sdf_query(weights, pyr, pts[s:s + per], center, K, scale, c.ClampingDistance, c.input_img_shape,
                                               idx[s:s + per], drop_p=0.0)[1]
            return raw.view(B, nodes ** 3)

        lo = torch.full((B, 3), -1.0, device=dev) if box is None else box[:, 0].to(dev).float()
        hi = torch.full((B, 3), 1.0, device=dev) if box is None else box[:, 1].to(dev).float()
        coarse_grid = torch.cat([lo, (hi - lo) / float(coarse_n - 1), torch.zeros(B, 2, device=dev)], 1)
        coarse = field(coarse_grid, coarse_n)
        grid = ops.iso_refine_grid(coarse, coarse_grid, coarse_n, 0.0, int(pad_cells), n)
        values = field(grid, n)
        return {"values": values, "grid": grid, "coarse_values": coarse, "coarse_grid": coarse_grid, "centre": center, "scale": float(scale)}

    def field_enabled(self) -> bool:
        """cfg.eval_field (default False) or HOISDF_FIELD=1: the eval forward adds the two field surfaces to its outputs"""
        return bool(getattr(self.cfg, "eval_field", False)) or os.environ.get("HOISDF_FIELD", "") == "1"

    def _field_outputs(self, out, feature_pyramid, meta_info):
        """the opt-in outputs of the eval forward: field_{hand,obj}_{verts,faces,n_verts,n_faces} in fixed-capacity tensors
        (cfg.field_max_verts vertex rows, twice as many face rows; the counts are the needs: a count above its capacity marks an
        overflowed sample).  Nothing synchronises."""
        c = self.cfg
        mv = int(c.field_max_verts)
        for kind in ("hand", "obj"):
            v, f, nv, nf = self.field_surface(feature_pyramid, meta_info, kind, int(c.field_grid), max(int(c.field_grid) // 2, 2),
                                              max_verts=mv, max_faces=2 * mv)
            out.update({f"field_{kind}_verts": v, f"field_{kind}_faces": f, f"field_{kind}_n_verts": nv, f"field_{kind}_n_faces": nf})

    def refine_enabled(self) -> bool:
        """cfg.eval_refine (default False) or HOISDF_REFINE=1: the eval forward fits the predicted pair to the two learned fields"""
        from .refine import enabled
        return enabled(self.cfg)

    def set_refine_source(self, source):
        """what the refinement of the eval forward poses the predicted pair from: a render.PairSource (the templates as meshes and
        the hand's faces; render.predicted_pair takes it).  A plain attribute, no submodule: the checkpoint schema stays as it is"""
        object.__setattr__(self, "_refine_source", source)

    def _refine_outputs(self, out, feature_pyramid, meta_info):
        """the opt-in outputs of the eval forward: refined_{hand,obj}_verts (camera metres) and refine_{hand,obj}_{rot,trans,cost,
        info} of refine.fit_pair on the predicted pair.  Needs ``set_refine_source`` and meta_info["obj_cls"].  Nothing synchronises."""
        from .refine import fit_pair
        from .render import predicted_pair
        if getattr(self, "_refine_source", None) is None:
            raise RuntimeError("cfg.eval_refine needs the templates: Model.set_refine_source(render.PairSource(cfg, templates, template_faces, hand_faces))")
        if "obj_cls" not in meta_info:
            raise KeyError("cfg.eval_refine needs meta_info['obj_cls']: the object template of every sample (-1: none)")
        if self.cfg.use_inverse_kinematics:
            raise ValueError("cfg.eval_refine needs the predicted hand mesh in the forward: the IK variant has none there")
        pair = predicted_pair(out, meta_info, meta_info["obj_cls"], self._refine_source)
        res = fit_pair(self, feature_pyramid, meta_info, pair)
        out["refined_hand_verts"], out["refined_obj_verts"] = res["pair"][0], res["pair"][2]
        for kind in ("hand", "obj"):
            for k in ("rot", "trans", "cost", "info"):
                out[f"refine_{kind}_{k}"] = res[kind][k]

    def render_gaussian_heatmap(self, joint_coord):
        """reference :128-143 (encoder-side auxiliary target; plain torch)."""
        c = self.cfg
        x = torch.arange(c.output_hm_shape[2], device=joint_coord.device).float()
        y = torch.arange(c.output_hm_shape[1], device=joint_coord.device).float()
        yy, xx = torch.meshgrid(y, x, indexing="ij")
        jx, jy = joint_coord[:, :, 0, None, None], joint_coord[:, :, 1, None, None]
        hm = torch.exp(-(((xx[None, None] - jx) / c.sigma) ** 2) / 2 - (((yy[None, None] - jy) / c.sigma) ** 2) / 2)
        return hm.sum(1) * 255

    # ---- the point-branch draw and the early survivor counts -----------------------------------
    def draw_branch(self, mode, epoch_cnt=1e8) -> bool:
        """reference :426-427: the ONE python-random draw of a forward; True = pre-sampled points + jitter (branch A),
        False = query points from the dense-lattice sdf_infer (always in eval)."""
        p = self._py_random.uniform(0, 1)
        return (p < 0.4 or epoch_cnt < self.cfg.point_sampling_epoch) and mode == "train"

    def infer_counts_begin(self, meta_info):
        """queue the lattice-survivor counts of both fields (they depend on mano_root / obj_center_cam / cam_intr / bbox only,
        reference :286-302).  Model.forward calls this BEFORE the image encoder; sdf_infer then waits for an event that has
        long fired instead of draining the device twice per field (round 3: four pipeline drains per eval step)."""
        c = self.cfg
        K = meta_info["cam_intr"]
        return {"hand": ops.sdf_infer_count_begin(meta_info["mano_root"], K, meta_info["bbox_hand"], c.hand_sdf_scale, c.bins_n),
                "obj": ops.sdf_infer_count_begin(meta_info["obj_center_cam"], K, meta_info["bbox_obj"], c.obj_sdf_scale, c.bins_n)}

    # ---- the hot path ----------------------------------------------------------------------
    def _query_points(self, f: _Field, pyr, inputs, meta_info, branch_a, batch_ratio, counts):
        """f.points: pre-sampled points + jitter (branch A), or the dense lattice's selection together with f.sdf / f.pe"""
        if branch_a:
            d = self.cfg.random_move_dist[len([a for a in self.cfg.random_ratio if batch_ratio > a])]
            jit = self._jitter or (lambda like, dd: torch.empty_like(like).uniform_(-dd, dd))
            f.points = inputs[f"{f.kind}_pre_points"] + jit(inputs[f"{f.kind}_pre_points"], d)
        else:                                                                          # :462-481
            f.points, f.sdf, f.pe, _ = self.sdf_infer(pyr, f.center, meta_info["cam_intr"], meta_info[f"bbox_{f.kind}"], f.scale, f.n,
                                                      f.kind, (counts or {}).get(f.kind))

    def _field_step(self, pyr, f: _Field, other: _Field, inputs, K, want_sdf_loss):
        """The per-field sequence, on the stream the caller chose: SDF-loss prediction, gather, token MLP (op-by-op form), the
        points in their own field (unless sdf_infer made that already) and re-centred in the ``other`` field."""
        B = f.center.shape[0]
        if want_sdf_loss:
            f.sdf_pred, _, _ = self.sdf_forward(pyr, inputs[f"{f.kind}_sdf_points"], f.center, K, f.scale, f.kind)
        # ONE gather of the points' pixels feeds the token MLP (with gradient), the own field and - the camera points being the same -
        # the other field (the reference gathers them three times, :445/:486/:499; its detached queries run as single hoisdf_sdf_query_fwd calls)
        f.feat, cam = ops.project_gather(pyr, f.points, f.center, K, f.scale, self.cfg.input_img_shape)
        f.cam = cam.view(B, f.n, 3)
        if not ops.tokens_ok(f.feat):           # (fused: K7 + K8 as one C call per point set, _own_token_rows)
            f.fea = self.linear_transformerin(f.feat).view(B, f.n, -1)                                  # :486-493
        fd = f.feat.detach()
        if f.sdf is None:                       # the reference tracks these calls but only ever uses them detached
            sdf, _, pe, _ = self._sdf_query(pyr, f.points, f.center, K, f.scale, f.kind, feat=fd)
            f.sdf, f.pe = sdf.view(B, f.n, 1), pe.view(B, f.n, -1)
        x_pts = (f.cam - other.center[:, None, :]) * other.scale                                        # :495-518
        x_sdf, _, x_pe, _ = self._sdf_query(pyr, x_pts, other.center, K, other.scale, other.kind, feat=fd)
        f.x_sdf, f.x_pe = x_sdf.view(B, f.n, 1), x_pe.view(B, f.n, -1)

    def _own_token_rows(self, f: _Field):
        """rows [0, n) of f.tok = [cam - center | pe | MLP(feat) * sigma(sdf, beta)].  Fused (hoisdf_tokens_fwd): makes the buffer
        and f.fea (detached: for the other field's cross rows) as well; op-by-op: K8 into the existing buffer"""
        if ops.tokens_ok(f.feat):
            lin, c = self.linear_transformerin.layers, self.cfg
            tok = torch.empty(f.center.shape[0], c.num_samp_hand + c.num_samp_obj, c.hidden_dim, device=f.center.device)
            f.tok, fea = ops.tokens(tok, f.feat, f.cam, f.center, f.pe, f.sdf.detach(), f.beta, 0, [l.weight for l in lin], [l.bias for l in lin])
            f.fea = fea.view(f.center.shape[0], f.n, -1)
        else:
            f.tok = ops.token_build(f.tok, f.cam.reshape(-1, 3), f.center, f.pe, f.fea, f.sdf.detach(), f.beta, 0)

    def _assemble_tokens(self, hand: _Field, obj: _Field):
        """token streams (batch-first).  The appended cross-field tokens are detached (:540,:558) and use
        the *other* centre for xyz ("# bug" lines :498,:508 replicated)."""
        fused = ops.tokens_ok(hand.feat)
        if fused:
            self._own_token_rows(hand)                  # (the object's: made on its own stream, right after its _field_step)
        else:
            hand.tok, obj.tok = (torch.empty(hand.center.shape[0], hand.n + obj.n, self.cfg.hidden_dim, device=hand.center.device)
                                 for _ in range(2))
        with torch.no_grad():                           # the cross rows [n, nh+no): the OTHER field's points in this field
            for f, o in ((hand, obj), (obj, hand)):
                ops.token_build(f.tok, o.cam.reshape(-1, 3), f.center, o.x_pe, o.fea.detach(), o.x_sdf, f.beta.detach(), f.n)
        if not fused:
            self._own_token_rows(hand)
            self._own_token_rows(obj)

    def _object_stack(self, obj: _Field):
        """the object encoder stack and its two heads -> (obj_rot, obj_trans), each (L,B,no,3)"""
        _, obj_enc = self.obj_transformer.forward_batch_first(obj.tok, n_keep=obj.n)       # :582-584
        return self.linear_obj_rot(obj_enc), self.linear_obj_rel_trans(obj_enc)

    def _mano_and_object_pose(self, hs, obj_rot, obj_trans, targets, training, loss, out):
        """MANO head (two launches: ground truth, predictions + fused losses) + the object pose outputs and losses"""
        c = self.cfg
        if c.use_inverse_kinematics:                                               # :595-597
            mano_shape = self.linear_shape(hs[:, :, 0])
            out["mano_shape_out"] = mano_shape[-1]
        else:                                                                      # :599-620
            pose6d = self.linear_pose(hs[:, :, :c.mano_shape_indx])                # (L,B,16,6)
            mano_shape = self.linear_shape(hs[:, :, c.mano_shape_indx])            # (L,B,10)
            mp = targets["mano_param"] if (training or c.dataset == "dexycb") else None
            pred_m, gt_m = self.mano_head.forward_batch_first(pose6d, mano_shape, mp)
            out["mano_mesh_out"] = pred_m["verts3d"][-1]
            out["mano_joints_out"] = pred_m["joints3d"][-1]
            if c.dataset == "dexycb":
                out["mano_joints_gt_out"] = gt_m["joints3d"]
                out["mano_mesh_gt_out"] = gt_m["verts3d"]
        if not training:                                                           # :622-624
            out["obj_rot_out"] = obj_rot[-1].contiguous()
            out["obj_trans_out"] = obj_trans[-1].contiguous()
        if training or c.dataset == "dexycb":                                      # :640-654
            if c.use_inverse_kinematics:
                loss["shape_param_loss"], loss["shape_reg_loss"] = self.mano_shape_loss(mano_shape, targets["mano_param"][:, -10:])
            else:
                (loss["mano_mesh_loss"], loss["mano_joint_loss"], loss["pose_param_loss"],
                 loss["shape_param_loss"], _, _) = self.mano_loss(pred_m, gt_m)
        loss["obj_rot"] = ops.smooth_l1_loss_broadcast(obj_rot, targets["obj_rot"], c.num_samp_obj)            # :656-662 (a15: HIP reductions)
        loss["obj_trans"] = ops.smooth_l1_loss_broadcast(obj_trans, targets["rel_obj_trans"], c.num_samp_obj)

    def _hand_votes(self, hand_rel, hand_enc, targets, training, loss, out):
        """hand vote heads + vote aggregation / losses"""
        joints_gt = targets["joint_cam_no_trans"][:, 1:] if training or self.cfg.dataset == "dexycb" else \
            torch.zeros(hand_rel.shape[0], 20, 3, device=hand_rel.device)              # :626-638
        if ops.tokens_ok(hand_enc):             # K11 + K12 as one C call per direction (hoisdf_heads_vote_fwd / _bwd)
            res = self.joints_vote_loss.forward_fused(hand_rel, hand_enc, self.linear_handvote, self.linear_handcls, joints_gt)
        else:                                   # :587-593: the vote / cls MLPs (L,B,nh,60 / 20), then K12
            res = self.joints_vote_loss(hand_rel, self.linear_handvote(hand_enc), self.linear_handcls(hand_enc), joints_gt, batch_first=True)
        loss["loss_joint_3d"], loss["loss_joint_cls"], loss["loss_all_joint_3d"], joints = res
        out["hand_joints_out"] = joints[-1]

    def hot_path(self, pyr: ops.PyramidNHWC, inputs, targets, meta_info, mode, epoch_cnt=1e8, batch_ratio=0, branch_a=None,
                 infer_counts=None):
        """reference :370-402 and :424-662: everything after decoder_net except the aux image losses.  ``branch_a`` /
        ``infer_counts``: the draw and the queued survivor counts when the caller (Model.forward) made them ahead of the
        encoder; drawn / queued here otherwise."""
        c = self.cfg
        training = mode == "train"
        if training:
            pyr = pyr.shared_grad()          # the step's four gather backwards scatter into ONE set of level gradients
        loss, out = {}, {}
        root, K = meta_info["mano_root"], meta_info["cam_intr"]
        hand = _Field("hand", root, c.hand_sdf_scale, c.num_samp_hand, self.hand_sigmoid_beta)
        obj = _Field("obj", meta_info["obj_center_cam"], c.obj_sdf_scale, c.num_samp_obj, self.obj_sigmoid_beta)
        # Everything that starts from the OBJECT points (their SDF query, input MLP, evaluation in the hand field and,
        # below, the object encoder stack) is independent of the hand-point work until the tokens are assembled: it is
        # issued on a second HIP stream, so its small grids (16 384 rows) share the chip with the hand stream's kernels.
        plan = _StreamPlan(self, root.device, allow=root.is_cuda)
        want_sdf_loss = training or c.dataset == "dexycb"                                # :370-402
        if branch_a is None:
            branch_a = self.draw_branch(mode, epoch_cnt)                               # :426-427
        if not branch_a and infer_counts is None:
            infer_counts = self.infer_counts_begin(meta_info)      # both fields queued before anything else of this path
        log = getattr(self, "branch_log", None)
        if log is not None and training:
            log.append("A" if branch_a else "B")             # bench.py --branch-mix reports the mix it measured
        for f in (hand, obj):
            self._query_points(f, pyr, inputs, meta_info, branch_a, batch_ratio, infer_counts)
        for f in (hand, obj):
            f.beta.data.clamp_(min=2e-3)                                               # :124
        # both streams read the cached SDF-query weight descriptors: (re)build them HERE, on the ambient stream and
        # ahead of the fork, so neither stream can launch a query before the folded weights are written
        for f in (hand, obj):
            self._query_weights(f.kind).get()
        plan.fork()                                     # the points, the pyramid, the inputs and the query weights are ready
        with plan.on_side():                            # ---- object points ----
            self._field_step(pyr, obj, hand, inputs, K, want_sdf_loss)
            if ops.tokens_ok(obj.feat):         # fused: the object's own token rows here, the hand's after the join (_assemble_tokens)
                self._own_token_rows(obj)
        self._field_step(pyr, hand, obj, inputs, K, want_sdf_loss)                     # ---- hand points (ambient stream) ----
        hand_rel = hand.cam - root[:, None, :]
        plan.join(obj.sdf_pred, obj.sdf, obj.pe, obj.fea, obj.cam, obj.x_sdf, obj.x_pe, obj.tok)
        if want_sdf_loss:
            loss["sdfhand_loss"], loss["sdfobj_loss"] = self.sdf_loss(
                hand.sdf_pred, obj.sdf_pred, targets["hand_sdf"], targets["obj_sdf"], clamp=c.ClampingDistance)   # :393-402, clamp fused
        self._assemble_tokens(hand, obj)
        tgt_mask = None if c.use_inverse_kinematics else get_mano_tgt_mask(c)         # :564-569
        # Only rows < nh (hand stream) / < no (object stream) of the encoder outputs are ever read (:587-593 and
        # the memory mask), so the last layer of each stack skips the other query rows - same values, less work.
        # The object encoder stack (+ its heads) goes to the second stream as well (127.3 -> 126.0 ms/step on its own): with
        # two streams it is issued AHEAD of the hand stack, with one stream behind it (dropout seeds follow the issue order).
        plan.fork(obj.tok)
        if plan.two:
            with plan.on_side():
                obj_rot, obj_trans = self._object_stack(obj)
        hs, memory, hand_enc = self.hand_transformer.forward_batch_first(hand.tok, self.mano_query_embed.weight, tgt_mask, hand.n,
                                                                         n_keep=hand.n)          # :571-581
        plan.fork(hs)                                   # hs is ready; the side stream already holds the object stack
        if not plan.two:
            obj_rot, obj_trans = self._object_stack(obj)
        with plan.on_side():                            # ---- under the big vote-head GEMMs of the ambient stream
            self._mano_and_object_pose(hs, obj_rot, obj_trans, targets, training, loss, out)
            if training and self.interaction_loss_enabled():
                self._interaction_losses(out["mano_mesh_out"], obj_rot, obj_trans, meta_info, loss)
            if training and self.silhouette_loss_enabled():
                self._silhouette_losses(out["mano_mesh_out"], obj_rot, obj_trans, targets, meta_info, loss)
            side_made = [t for t in list(loss.values()) + list(out.values()) if torch.is_tensor(t)]
        self._hand_votes(hand_rel, hand_enc, targets, training, loss, out)             # ---- (ambient stream)
        plan.join(*side_made)
        return loss, out

    # ---- the same stage through ONE C-ABI call (include/hoisdf.h hoisdf_pose_infer; opt-in) ------------------------------
    def native_infer_enabled(self) -> bool:
        """cfg.native_infer (default False) or HOISDF_INFER=native: Model.forward in eval mode runs infer_native instead of hot_path"""
        return bool(getattr(self.cfg, "native_infer", False)) or os.environ.get("HOISDF_INFER", "") == "native"

    def native_ik_enabled(self) -> bool:
        """cfg.native_ik (default False) or HOISDF_IK=native, for the IK variant with a MANO layer to solve with: infer_native asks
        hoisdf_pose_infer for the closed-form IK post-process too (ik_solve = 1) -> ik_joints_out / ik_verts_out / ik_pose_out"""
        from .ik import native_ik_enabled
        return bool(self.cfg.use_inverse_kinematics) and self.ik_mano_layer is not None and native_ik_enabled(self.cfg)

    def _pose_desc(self, B, C_):
        from ._lib import PoseDesc
        c = self.cfg
        return PoseDesc(B=B, num_samp_hand=c.num_samp_hand, num_samp_obj=c.num_samp_obj, bins_n=c.bins_n, img_h=c.input_img_shape[0],
                        img_w=c.input_img_shape[1], hand_sdf_scale=c.hand_sdf_scale, obj_sdf_scale=c.obj_sdf_scale,
                        clamping_distance=c.ClampingDistance, hidden_dim=c.hidden_dim, nheads=c.nheads, dim_feedforward=c.dim_feedforward,
                        enc_layers=c.enc_layers, dec_layers=c.dec_layers, C=C_, use_inverse_kinematics=int(c.use_inverse_kinematics),
                        pre_norm=int(c.pre_norm), classifier_branch=int(c.ClassifierBranch), attention=2 if ops.attention_emu() else 0,
                        ik_solve=int(self.native_ik_enabled()))

    def _pose_weights(self):
        """hoisdf_pose_weights from the module's own parameters -> (struct, the tensors it points to)"""
        from ._lib import PoseWeights
        w, keep = PoseWeights(), []

        def t(x):
            x = x.detach().float().contiguous()
            keep.append(x)
            return x.data_ptr()

        def mlp(dst, m, act_last):
            dst.n_layers, dst.act_last = len(m.layers), int(act_last)
            dst.dims[0] = m.layers[0].weight.shape[1]
            for i, l in enumerate(m.layers):
                dst.dims[i + 1] = l.weight.shape[0]
                dst.w[i], dst.b[i] = t(l.weight), t(l.bias)

        def sdf_dec(dst, dec):
            for i in range(4):
                l = getattr(dec, f"linh{i}")
                dst.weight_v[i], dst.weight_g[i], dst.bias[i] = t(l.weight_v), t(l.weight_g), t(l.bias)
            dst.linh4_weight, dst.linh4_bias = t(dec.linh4.weight), t(dec.linh4.bias)

        def enc(dst, stack):
            n = stack.inter_norm
            for i, l in enumerate(stack.layers):
                a, d = l.self_attn, dst[i]
                d.w_in, d.b_in, d.w_out, d.b_out = t(a.in_proj_weight), t(a.in_proj_bias), t(a.out_proj.weight), t(a.out_proj.bias)
                d.g1, d.be1, d.w1, d.b1 = t(l.norm1.weight), t(l.norm1.bias), t(l.linear1.weight), t(l.linear1.bias)
                d.w2, d.b2, d.g2, d.be2 = t(l.linear2.weight), t(l.linear2.bias), t(l.norm2.weight), t(l.norm2.bias)
                d.g3, d.be3 = t(n.weight), t(n.bias)

        mlp(w.linear_sdfin, self.linear_sdfin, True)
        sdf_dec(w.hand_sdf_decoder, self.hand_sdf_decoder)
        sdf_dec(w.obj_sdf_decoder, self.obj_sdf_decoder)
        mlp(w.linear_transformerin, self.linear_transformerin, True)
        w.hand_sigmoid_beta, w.obj_sigmoid_beta = t(self.hand_sigmoid_beta), t(self.obj_sigmoid_beta)
        enc(w.hand_encoder, self.hand_transformer.encoder)
        enc(w.obj_encoder, self.obj_transformer.encoder)
        dn = self.hand_transformer.decoder.norm
        for i, l in enumerate(self.hand_transformer.decoder.layers):
            sa, ca, d = l.self_attn, l.multihead_attn, w.hand_decoder[i]
            d.sa_w_in, d.sa_b_in, d.sa_w_out, d.sa_b_out = t(sa.in_proj_weight), t(sa.in_proj_bias), t(sa.out_proj.weight), t(sa.out_proj.bias)
            d.ca_w_in, d.ca_b_in, d.ca_w_out, d.ca_b_out = t(ca.in_proj_weight), t(ca.in_proj_bias), t(ca.out_proj.weight), t(ca.out_proj.bias)
            d.w1, d.b1, d.w2, d.b2 = t(l.linear1.weight), t(l.linear1.bias), t(l.linear2.weight), t(l.linear2.bias)
            d.g1, d.be1, d.g2, d.be2, d.g3, d.be3 = (t(x) for x in (l.norm1.weight, l.norm1.bias, l.norm2.weight, l.norm2.bias,
                                                                      l.norm3.weight, l.norm3.bias))
            d.g4, d.be4 = t(dn.weight), t(dn.bias)
        w.mano_query_embed = t(self.mano_query_embed.weight)
        mlp(w.linear_shape, self.linear_shape, False)
        mlp(w.linear_handvote, self.linear_handvote, False)
        mlp(w.linear_handcls, self.linear_handcls, False)
        mlp(w.linear_obj_rot, self.linear_obj_rot, False)
        mlp(w.linear_obj_rel_trans, self.linear_obj_rel_trans, False)
        iks = self.native_ik_enabled()
        if not self.cfg.use_inverse_kinematics or iks:
            if iks:
                ml = self._ik_layer(self.hand_sigmoid_beta.device)
            else:
                mlp(w.linear_pose, self.linear_pose, False)
                ml = self.mano_head.mano_layer
            if ml.kernel_assets() is None:
                raise RuntimeError("infer_native needs this package's ManoLayer on the GPU, centred on the wrist, with a zero hand mean "
                                   "(the configuration of the reference, main/model.py:735-742)")
            w.mano_shapedirs, w.mano_posedirs, w.mano_weights = t(ml.th_shapedirs), t(ml.th_posedirs), t(ml.th_weights)
            w.mano_v_template, w.mano_j_regressor, w.mano_hands_mean = t(ml.th_v_template), t(ml.th_J_regressor), t(ml.th_hands_mean)
        return w, keep

    def _pose_prepared(self, B, C_, device):
        """the prepared blob (weight copies, weight-norm folds, weight images, MANO image, floored betas, target mask), rebuilt only
        when a parameter, the batch size or an arithmetic switch changed - the key of the SDF-query folds, over every parameter"""
        ps = [p for n, p in self.named_parameters() if not n.startswith(("backbone_net", "decoder_net"))] + \
             [b for n, b in self.named_buffers() if n.startswith("mano_head")]
        iks = self.native_ik_enabled()
        if iks:                         # the layer the IK solve reads is no submodule: its asset tensors join the key by hand
            ps += [b for n, b in self._ik_layer(device).named_buffers() if n.startswith("th_")]
        key = (B, C_, str(device), ops._WEIGHT_GEN[0], ops.gemm_emu(), ops.attention_emu(), iks) + tuple((p.data_ptr(), p._version) for p in ps)
        ent = _POSE_CACHE.get(self)
        if ent is None:
            ent = _POSE_CACHE[self] = {"key": None, "prepared": None, "builds": 0}
        if ent["key"] != key:
            w, keep = self._pose_weights()
            ent["builds"] += 1
            ent["prepared"] = ops.PosePrepared(self._pose_desc(B, C_), w, device, ent["builds"])
            ent["key"] = key
            del keep            # (the blob holds its own copies; the copies above are ordered on the current stream)
        return ent["prepared"]

    @torch.no_grad()
    def infer_native(self, pyr, meta_info, counts=None, debug=False) -> Dict[str, torch.Tensor]:
        """The eval forward of hot_path through ONE C-ABI call (hoisdf_pose_infer): pyramid + camera inputs + boxes ->
        hand_joints_out, obj_rot_out, obj_trans_out and mano_mesh_out + mano_joints_out (or mano_shape_out for the IK variant; with
        native_ik_enabled() also that variant's post-process: ik_joints_out / ik_verts_out / ik_pose_out / ik_valid_out),
        same keys and shapes as hot_path(..., "eval")'s outputs.  No losses, no ground-truth MANO outputs.  ``counts``: what
        infer_native_begin queued ahead of the encoder.  The default arithmetic only (cfg.attention_f16_eval is not offered)."""
        pyr = self._pyramid(pyr)
        root = meta_info["mano_root"]
        _chk(root, self.hand_sigmoid_beta)         # GPU tensors only: there is no CPU form of this path
        prepared = self._pose_prepared(root.shape[0], pyr.C, root.device)
        return ops.pose_infer(prepared, pyr, root, meta_info["obj_center_cam"], meta_info["cam_intr"], meta_info["bbox_hand"],
                              meta_info["bbox_obj"], counts, _StreamPlan(self, root.device).side, debug)

    def infer_native_begin(self, meta_info, C_=None):
        """queue both survivor counts of infer_native (hoisdf_pose_infer_begin) - ahead of the image encoder, as infer_counts_begin"""
        root = meta_info["mano_root"]
        prepared = self._pose_prepared(root.shape[0], self.cfg.mutliscale_dim if C_ is None else C_, root.device)
        return ops.PoseInferCounts(prepared.desc, root, meta_info["obj_center_cam"], meta_info["cam_intr"], meta_info["bbox_hand"],
                                   meta_info["bbox_obj"])

    # ---- the image encoder through the C ABI (include/hoisdf.h hoisdf_encoder_infer; opt-in, evaluation only) -------------------
    def native_encoder_enabled(self) -> bool:
        """cfg.native_encoder (default False) or HOISDF_ENCODER=native; honoured only where _forward_native runs"""
        return bool(getattr(self.cfg, "native_encoder", False)) or os.environ.get("HOISDF_ENCODER", "") == "native"

    def _encoder_prepared(self, B, H, W, device):
        """the encoder's prepared blob (BatchNorm folds from the running statistics, packed weights), rebuilt only when an encoder
        parameter or BatchNorm buffer, the batch size or the image size changed"""
        if self.backbone_net is None or self.decoder_net is None:
            raise RuntimeError("encode_native needs a model built with its image encoder")
        sd = {}
        for prefix, net in (("backbone_net.", self.backbone_net), ("decoder_net.", self.decoder_net)):
            for n, t in list(net.named_parameters()) + list(net.named_buffers()):
                if t.is_floating_point():
                    sd[prefix + n] = t
        key = (B, H, W, str(device), ops._WEIGHT_GEN[0]) + tuple((t.data_ptr(), t._version) for t in sd.values())
        ent = _ENCODER_CACHE.get(self)
        if ent is None:
            ent = _ENCODER_CACHE[self] = {"key": None, "prepared": None, "builds": 0}
        if ent["key"] != key:
            from ._lib import EncoderDesc
            for m in list(self.backbone_net.modules()) + list(self.decoder_net.modules()):
                if isinstance(m, nn.BatchNorm2d) and (m.eps != 1e-5 or m.running_mean is None):
                    raise RuntimeError("encode_native folds BatchNorm2d with running statistics and eps = 1e-5")
            desc = EncoderDesc(B=B, img_h=H, img_w=W, resnet_type=self.cfg.resnet_type, big_decoder=int(self.cfg.use_big_decoder))
            ent["builds"] += 1
            ent["prepared"] = ops.EncoderPrepared(desc, sd, device, ent["builds"])
            ent["key"] = key
        return ent["prepared"]

    @torch.no_grad()
    def encode_native(self, img, want_aux=True):
        """backbone_net + decoder_net in evaluation mode through ONE C-ABI call (hoisdf_encoder_infer: exact-f32 HIP convolutions,
        BatchNorm folded): ``img`` (B, 3, H, W) -> (PyramidNHWC, aux NHWC [B][H / 2][W / 2][3] or None).  Running statistics only."""
        _chk(img)
        prepared = self._encoder_prepared(img.shape[0], img.shape[2], img.shape[3], img.device)
        return ops.encoder_infer(prepared, img, want_aux)

    def _set_arithmetic(self, f16_eval=None):
        """the configuration's arithmetic switches -> ops (``f16_eval`` None: that one is left alone - infer_native does not offer it)"""
        c = self.cfg
        if f16_eval is not None:
            ops.set_attention_f16_eval(bool(getattr(c, "attention_f16_eval", False)) and f16_eval)
        if getattr(c, "gemm_emu", None) is not None:
            ops.set_gemm_emu(bool(c.gemm_emu))
        if getattr(c, "attention_emu", None) is not None:
            ops.set_attention_emu(bool(c.attention_emu))

    @staticmethod
    def _aux_outputs(out, targets, decoder_out):            # heat-map and segmentation maps next to their targets
        out.update(joint_heatmap_out=decoder_out[:, 0], hand_seg_gt_out=targets["hand_seg"], hand_seg_pred_out=decoder_out[:, 1],
                   obj_seg_gt_out=targets["obj_seg"], obj_seg_pred_out=decoder_out[:, 2])

    def _forward_native(self, inputs, targets, meta_info):
        """eval forward with the switch on: the encoder in PyTorch (or, with cfg.native_encoder, through hoisdf_encoder_infer), then
        infer_native; dexycb keeps its ground-truth MANO outputs"""
        c = self.cfg
        if self.refine_enabled():
            raise ValueError("cfg.eval_refine is not offered on the one-call path (cfg.native_infer): run the eval forward without it")
        self._set_arithmetic()
        with torch.no_grad():
            counts = self.infer_native_begin(meta_info, self.linear_sdfin.layers[0].weight.shape[1])
            if self.native_encoder_enabled():
                feature_pyramid, aux = self.encode_native(inputs["img"], want_aux=c.dataset == "dexycb")
                decoder_out = None if aux is None else aux.permute(0, 3, 1, 2)
            else:
                img_feat, skips = self.backbone_net(inputs["img"])
                feature_pyramid, decoder_out = self.decoder_net(img_feat, skips)
            pyr = self._pyramid(feature_pyramid)
            out = self.infer_native(pyr, meta_info, counts)
            if self.field_enabled():
                self._field_outputs(out, pyr, meta_info)
            if c.dataset == "dexycb":
                if not c.use_inverse_kinematics:
                    gv, gj, _ = ops.mano_gt(targets["mano_param"], self.mano_head.mano_layer.kernel_assets())
                    out["mano_joints_gt_out"], out["mano_mesh_gt_out"] = gj, gv
                self._aux_outputs(out, targets, decoder_out)
        return out

    def forward(self, inputs, targets, meta_info, mode, epoch_cnt=1e8, batch_ratio=0):
        """reference :357-665."""
        c = self.cfg
        if mode != "train" and not self.training and self.native_infer_enabled():
            return self._forward_native(inputs, targets, meta_info)
        branch_a = self.draw_branch(mode, epoch_cnt)                                  # :426-427, drawn ahead of the encoder
        infer_counts = None if branch_a else self.infer_counts_begin(meta_info)       # read back under the encoder's kernels
        img_feat, skips = self.backbone_net(inputs["img"])                            # :367-368 (PyTorch / MIOpen)
        feature_pyramid, decoder_out = self.decoder_net(img_feat, skips)
        pyr = self._pyramid(feature_pyramid)
        self._set_arithmetic(f16_eval=mode != "train")
        loss, out = self.hot_path(pyr, inputs, targets, meta_info, mode, epoch_cnt, batch_ratio, branch_a, infer_counts)
        if mode != "train" and not self.training and self.field_enabled():
            self._field_outputs(out, pyr, meta_info)
        if mode != "train" and not self.training and self.refine_enabled():
            self._refine_outputs(out, pyr, meta_info)
        if mode == "train" or c.dataset == "dexycb":                                   # :404-422 aux image losses
            self._aux_outputs(out, targets, decoder_out)
            # (f4) one HIP pass: Gaussian heat-map target + MSE + the two BCE maps
            loss["joint_heatmap"], loss["obj_seg"], loss["hand_seg"], _ = ops.aux_image_losses(
                decoder_out, targets["joint_coord"], targets["hand_seg"], targets["obj_seg"], c.sigma)
        return {**loss, **out}


def init_weights(m):
    """reference :668-679."""
    if isinstance(m, (nn.ConvTranspose2d,)):
        nn.init.normal_(m.weight, std=0.001)
    elif isinstance(m, nn.Conv2d):
        nn.init.normal_(m.weight, std=0.001)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)
    elif isinstance(m, nn.BatchNorm2d):
        nn.init.constant_(m.weight, 1)
        nn.init.constant_(m.bias, 0)
    elif type(m) is nn.Linear:
        nn.init.normal_(m.weight, std=0.01)
        nn.init.constant_(m.bias, 0)


def get_model(mode, cfg=_global_cfg, mano_layer=None, with_encoder=True):
    """reference :682-766.  ``mano_layer``: a module with manopth's ManoLayer interface; defaults to
    the synthetic MANO-shaped asset (the licensed MANO_RIGHT.pkl is not redistributable)."""
    backbone = BackboneNet(cfg.resnet_type) if with_encoder else None
    decoder = DecoderNet(cfg.resnet_type, big=cfg.use_big_decoder) if with_encoder else None
    mk = lambda: SDFDecoder(cfg.hidden_dim, cfg.PointFeatSize, use_classifier=cfg.ClassifierBranch)
    hand_dec, obj_dec = mk(), mk()
    hand_tr = Transformer(d_model=cfg.hidden_dim, dropout=cfg.dropout, nhead=cfg.nheads,
                          dim_feedforward=cfg.dim_feedforward, num_encoder_layers=cfg.enc_layers,
                          num_decoder_layers=cfg.dec_layers, normalize_before=cfg.pre_norm,
                          return_intermediate_dec=True)
    obj_tr = VoteTransformer(d_model=cfg.hidden_dim, dropout=cfg.dropout, nhead=cfg.nheads,
                             dim_feedforward=cfg.dim_feedforward, num_encoder_layers=cfg.enc_layers // 2,
                             normalize_before=cfg.pre_norm, return_intermediate_dec=True)
    if mano_layer is None:
        mano_layer = ManoLayer()
    if mode == "train":
        if decoder is not None:
            decoder.apply(init_weights)
        for m in (hand_tr, obj_tr, hand_dec, obj_dec):
            m.apply(init_weights)
        for dec in (hand_dec, obj_dec):      # weight-normed layers: only the bias is re-initialised
            for i in range(4):
                nn.init.constant_(getattr(dec, f"linh{i}").bias, 0)
    return Model(backbone, decoder, hand_dec, obj_dec, hand_tr, obj_tr, mano_layer, cfg=cfg)
