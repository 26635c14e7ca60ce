#!/usr/bin/env python3
"""Inference driver with the reference's CLI (main/test.py:51-74): --gpu_ids --ckpt_path.
Loads a reference-format checkpoint (strict), runs the eval forward (dense-grid sdf_infer branch) and writes, next to
the checkpoint (main/test.py:88-90) or under --out_dir,
  * results.txt in the reference's layout (main/test.py:229-261): ``key :  value`` lines - ADDS_error, and for dexycb
    mano_mje / mano_pamje / OCE_error / MCE_error (cm) + the 3D-mesh AUC block and the F-scores, for ho3d MME_error;
  * pred_mano.json for ho3d (main/test.py:263-265, the HO3D submission format), IK post-process included for the IK
    variant (main/test.py:139-160).
Datasets and the YCB object models are licence-gated and absent offline: without them the driver evaluates DexYCB /
HO3D-shaped synthetic samples against synthetic object templates (the numbers are then a plumbing check only)."""
import argparse
import os

import torch

from hoisdf_amd import metrics as M
from hoisdf_amd.config import cfg
from hoisdf_amd.engine import SyntheticDataset, Tester, native_image_enabled
from hoisdf_amd.refine import enabled as refine_enabled

JOINTS_SIMPLE_TO_MANO = M.JOINTS_SIMPLE_TO_MANO            # the order of the HO3D submission file


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu_ids", type=str, default="0")
    ap.add_argument("--ckpt_path", type=str, default=None, help="Full path to the checkpoint file")
    ap.add_argument("--setting", type=str, default="dexycb", help="the reference edits Config.setting in config.py")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--n_batches", type=int, default=2)
    ap.add_argument("--out_dir", type=str, default=None, help="default: the checkpoint's directory, else outputs/result")
    ap.add_argument("--native-infer", action="store_true",
                    help="run everything after the image encoder through the one C entry hoisdf_pose_infer (cfg.native_infer)")
    ap.add_argument("--native-encoder", action="store_true",
                    help="with --native-infer: the image encoder too through the C ABI (hoisdf_encoder_infer, cfg.native_encoder)")
    ap.add_argument("--native-image", action="store_true",
                    help="raw synthetic camera frames, cropped on the device (hoisdf_image_crop, cfg.native_image)")
    ap.add_argument("--native-ik", action="store_true",
                    help="the IK variant's closed-form post-process as one HIP launch (hoisdf_ik_mano_fwd, cfg.native_ik)")
    ap.add_argument("--native-metrics", action="store_true",
                    help="the evaluation metrics through the hoisdf_eval_* entries, running sums on the device (cfg.native_metrics)")
    ap.add_argument("--interaction", action="store_true",
                    help="also report penetration depth, contact ratio and intersection volume of the predicted hand and object "
                         "(hoisdf_eval_interaction, cfg.eval_interaction); the stand-in templates are then procedural MESHES")
    ap.add_argument("--field-surface", action="store_true",
                    help="also extract the zero level set of the two learned fields (Model.field_surface, hoisdf_iso_extract) and report "
                         "their Chamfer distance to the ground-truth meshes (cfg.eval_field); procedural MESHES as templates")
    ap.add_argument("--refine", action="store_true",
                    help="also move the predicted hand and object, each as a rigid body, onto the zero level set of the field the network "
                         "predicts (hoisdf_field_fit, cfg.eval_refine) and report the vertex errors before and after; procedural MESHES "
                         "as templates")
    ap.add_argument("--silhouette", action="store_true",
                    help="also report the IoU of the predicted hand's and object's rendered silhouettes against the mask targets "
                         "(hoisdf_raster_meshes, cfg.eval_silhouette); procedural MESHES as templates")
    ap.add_argument("--overlay", type=str, default="", metavar="DIR",
                    help="write one image per sample into DIR: the predicted hand and object blended over the input crop "
                         "(hoisdf_raster_overlay, cfg.overlay_dir; PNG where PIL imports, else binary PPM); procedural MESHES as templates")
    a = ap.parse_args()
    assert a.gpu_ids, "Please set propoer gpu ids"
    if "-" in a.gpu_ids:                                   # "0-3" -> "0,1,2,3" (main/test.py:66-70)
        lo, hi = a.gpu_ids.split("-")
        a.gpu_ids = ",".join(str(i) for i in range(int(lo), int(hi) + 1))
    return a


def main():
    a = parse_args()
    cfg.apply_setting(a.setting)
    cfg.native_infer = bool(a.native_infer)
    cfg.native_encoder = bool(a.native_encoder)
    cfg.native_ik = bool(a.native_ik)
    cfg.native_image = bool(a.native_image)
    cfg.native_metrics = bool(a.native_metrics)
    cfg.eval_interaction = bool(a.interaction)
    cfg.eval_field = bool(a.field_surface)
    cfg.eval_silhouette = bool(a.silhouette)
    cfg.eval_refine = bool(a.refine)
    cfg.overlay_dir = a.overlay or ""
    # one process drives one GPU: the first id of --gpu_ids (the reference wraps the model in DataParallel over all of them)
    dev = torch.device("cuda", int(a.gpu_ids.split(",")[0]))
    torch.cuda.set_device(dev)
    tester = Tester(cfg, dev, a.ckpt_path)
    mano_layer = getattr(getattr(tester.model, "mano_head", None), "mano_layer", None)
    if mano_layer is None:
        from hoisdf_amd.nets.mano import ManoLayer
        mano_layer = ManoLayer().to(dev)
    loader = torch.utils.data.DataLoader(SyntheticDataset(cfg, a.batch * a.n_batches, seed=1, raw_frames=native_image_enabled(cfg)), batch_size=a.batch)
    g = torch.Generator().manual_seed(0)
    templates = (0.05 * torch.randn(4, 500, 3, generator=g)).to(dev)         # stand-ins for the YCB models
    ho3d = cfg.dataset == "ho3d"
    faces = None
    refine = refine_enabled(cfg)
    if M.interaction_enabled(cfg) or M.field_enabled(cfg) or M.silhouette_enabled(cfg) or refine or cfg.overlay_dir:   # point clouds have no inside and no surface: closed procedural meshes instead
        from hoisdf_amd.sdf_data import procedural_templates
        faces = procedural_templates(device=dev)
        templates = faces["verts"]
    ev = M.Evaluator(cfg, templates, native=M.native_metrics_enabled(cfg), template_faces=faces,
                     hand_faces=mano_layer.th_faces if faces is not None else None)
    if refine:                                             # the eval forward poses the predicted pair from the same templates
        from hoisdf_amd.render import PairSource
        tester.model.set_refine_source(PairSource(cfg, templates, faces, mano_layer.th_faces))
    for it, (inputs, targets, meta) in enumerate(loader):
        B = meta["mano_root"].shape[0]
        obj_cls = (torch.arange(B) + it) % templates.shape[0]
        if refine:
            meta["obj_cls"] = obj_cls
        out = tester.predict(inputs, targets, meta, mano_layer=mano_layer)
        ev.feed(out, targets, meta, obj_cls)
        if cfg.overlay_dir:
            from hoisdf_amd.render import write_overlays
            write_overlays(cfg.overlay_dir, it * a.batch, inputs, out, meta, obj_cls, ev, cfg)
    out_dir = a.out_dir or (os.path.dirname(a.ckpt_path) if a.ckpt_path else "outputs/result")
    path = ev.write(out_dir)
    if ho3d:
        print(f"Dumped {ev.n_dumped[0]} joints and {ev.n_dumped[1]} verts predictions to {out_dir}/pred_mano.json")
    print(open(path).read())


if __name__ == "__main__":
    main()
