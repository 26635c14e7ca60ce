"""Configuration surface, attribute-compatible with the reference's global ``cfg``
(/root/reference/main/config.py:38-189) for everything the model reads.  Unlike the
reference, importing this module has no side effects (no sys.path edits, no mkdir).
"""
from __future__ import annotations

import os.path as osp


class Config:
    setting = "dexycb"  # ho3d, ho3d_render, dexycb, dexycb_full
    dataset = "dexycb"

    train_batch_size = 22
    test_batch_size = 22
    eval_batch_size = 22

    num_samp_hand = 600
    num_samp_obj = 200
    points_filter_dist = 0.05
    random_ratio = [0.3, 0.7]
    random_move_dist = [0.03, 0.05, 0.07]
    hand_sdf_scale = 3.1
    obj_sdf_scale = 3.1
    hand_cls_dist = 0.04
    obj_cls_dist = 0.05

    # SDF config
    bins_n = 64
    num_class = 6
    PointFeatSize = 33
    ClassifierBranch = False
    ClampingDistance = 0.15

    # model
    use_big_decoder = False
    use_inverse_kinematics = False
    # not in the reference: BASELINE.json configs[4] ("fp16 MFMA attention"): f16-operand attention kernel for
    # gradient-free forward passes (mode != "train"); off = exact f32 everywhere (the parity configuration)
    attention_f16_eval = False
    gemm_emu = None              # None: follow the library default (on; HOISDF_GEMM=f32 turns it off).  True / False: linear layers as fp32 emulated on the bf16 MFMA pipe (exact 3-way bf16 splits, 6 products; csrc/gemm_emu*.hip) / the exact-f32 MFMA GEMM
    attention_emu = None         # the same for the attention forward (csrc/attention_emu.hip); HOISDF_ATTENTION=f32 turns the default off
    # not in the reference: eval forwards run the stage after the image encoder through ONE C-ABI call (hoisdf_pose_infer) instead of
    # Model.hot_path's Python orchestration; same kernels, no losses in the output (HOISDF_INFER=native does the same)
    native_infer = False
    # not in the reference: the IK variant's closed-form post-process (hoisdf_amd/ik.py) as one HIP launch (hoisdf_ik_mano_fwd;
    # with native_infer on, as the last launch of hoisdf_pose_infer).  Also HOISDF_IK=native / test.py --native-ik
    native_ik = False
    # not in the reference: the evaluation metrics of test.py (hoisdf_amd/metrics.py Evaluator) through the hoisdf_eval_* entries
    # (csrc/eval.hip) instead of batched torch; the running sums stay on the device until results.txt is written.  Also
    # HOISDF_METRICS=native / test.py --native-metrics
    native_metrics = False
    # not in the reference: on that path (eval, no gradient, native_infer on) the image encoder too runs through the C ABI
    # (hoisdf_encoder_infer: BatchNorm folded, exact-f32 HIP convolutions) instead of torch / MIOpen (HOISDF_ENCODER=native does the same)
    native_encoder = False
    # not in the reference: batches that carry raw camera frames (uint8 frame, two masks, 2D labels) are cropped / augmented on the
    # device (hoisdf_amd/image_data.py ImagePipeline: hoisdf_image_crop / hoisdf_image_augment) instead of arriving as ready
    # tensors from a CPU loader.  Also HOISDF_IMAGE=native / test.py --native-image
    native_image = False
    # not in the reference: "mesh" = the SDF query points and their two distances are computed on the device each step from the
    # step's own hand and object meshes (hoisdf_amd/sdf_data.py MeshSdfSource: hoisdf_mesh_sdf_rows) instead of being read from
    # precomputed sdf_processed rows.  "" = off.  Also HOISDF_SDF=mesh.  The sampling recipe is DeepSDF's near-surface one scaled to a
    # hand (two Gaussian shells + a uniform share in the padded box); it is NOT fitted to the precomputed files' distribution
    sdf_source = ""
    mesh_sdf_sigma = (0.01, 0.003)       # metres: the two near-surface shells
    mesh_sdf_uniform_every = 16          # every 16th candidate is uniform in the box (share 1/16)
    mesh_sdf_pad = 0.05                  # metres around the mesh's bounding box
    mesh_sdf_candidates = 4              # candidate rows per sample = this x num_samp_hand (num_samp_obj)
    mesh_sdf_label_clamp = 0.05          # metres: a hand row keeps its part label where |sdf_hand| <= this
    # not in the reference: test.py's Evaluator also reports whether the PREDICTED hand and the PREDICTED object are physically
    # compatible - penetration depth, contact ratio, intersection volume (hoisdf_eval_interaction, csrc/interact.hip) - in a block
    # appended to results.txt.  Also HOISDF_INTERACTION=1 / test.py --interaction.  5 mm voxels are ObMan's; 5 mm contact is a
    # definition, not a measurement
    eval_interaction = False
    contact_dist = 0.005                 # metres: a hand vertex this close to the object (or inside it) is in contact
    interaction_voxel = 0.005            # metres: the cell of the intersection-volume grid (at most 64 cells per axis)
    # not in the reference: training adds a hand-object interaction loss on the PREDICTED hand mesh and the PREDICTED object (the
    # template posed by the mean rotation and translation votes): loss["interaction_rep"] = ObMan's repulsion of the vertices of
    # either mesh that lie inside the other, loss["interaction_att"] = its saturating attraction of the hand's contact zones
    # (vertices of the distal finger joints) onto the object (hoisdf_interaction_loss_fwd / _bwd, csrc/interact_loss.hip).  Also
    # HOISDF_INTERACTION_LOSS=1.  Needs meta_info["obj_cls"]; not offered for the IK variant.  The two weights are UNTUNED starting
    # values (no dataset and no trained weights here to tune them on); alpha is the length at which the attraction saturates
    interaction_loss = False
    interaction_rep_weight = 100.0
    interaction_att_weight = 10.0
    interaction_alpha = 0.01             # metres
    # not in the reference: training holds the PREDICTED hand mesh and the PREDICTED object (posed as for the interaction loss) to
    # the mask targets hand_seg / obj_seg, which otherwise supervise only the CNN decoder: loss["silhouette_in"] = the projected
    # vertices' distance to hand_seg OR obj_seg (the bilinear read of the masks' exact distance transform; the masks are modal, so
    # the union is what a vertex may hide behind), loss["silhouette_cover"] = the distance of every pixel of a mesh's own mask to its
    # nearest projected vertex; hand plus object, in mask pixels divided by the mask width (hoisdf_mask_edt,
    # hoisdf_silhouette_loss_fwd / _bwd, csrc/silhouette_loss.hip).  Also HOISDF_SILHOUETTE_LOSS=1.  Needs meta_info["obj_cls"]
    # and the templates as meshes, like the interaction loss; not offered for the IK variant.  The two weights are UNTUNED
    # starting values (no dataset and no trained weights here to tune them on)
    silhouette_loss = False
    silhouette_in_weight = 10.0
    silhouette_cover_weight = 10.0
    # not in the reference: the eval forward also extracts the zero level set of the two learned fields as triangle meshes
    # (Model.field_surface: hoisdf_iso_extract, csrc/isosurf.hip) and test.py's Evaluator reports their Chamfer distance to the
    # ground-truth MANO mesh and to the posed ground-truth template in a block appended to results.txt.  Also HOISDF_FIELD=1 /
    # test.py --field-surface
    eval_field = False
    field_grid = 64                      # nodes per axis of the fine grid (the coarse one has half as many)
    field_max_verts = 131072             # vertex rows per sample of the fixed-capacity outputs; twice as many face rows
    field_samples = 4096                 # points drawn on the ground-truth surface for the gt -> prediction half
    # not in the reference: the eval forward moves the predicted hand mesh and the predicted object, each as a rigid body, onto the
    # zero level set of the field the same network predicts (refine.fit_pair: Model.field_values + hoisdf_field_fit,
    # csrc/field_fit.hip) and adds refined_{hand,obj}_verts / refine_{hand,obj}_{rot,trans,cost,info} to its outputs; the Evaluator
    # appends a Refined: block to results.txt.  Also HOISDF_REFINE=1 / Evaluator(refine=True) / test.py --refine.  Needs
    # Model.set_refine_source and meta_info["obj_cls"]; not offered on the one-call path (native_infer) or for the IK variant
    eval_refine = False
    refine_grid = None                   # nodes per axis of the field the fit reads; None: field_grid
    refine_pad_cells = 4                 # coarse cells around the inside nodes: a fit starts OFF the surface
    refine_iters = 32                    # tried steps at the most (<= HOISDF_FIELD_FIT_MAX_ITERS)
    refine_huber = 0.1                   # field units: the residual beyond which the cost is linear (the field is tanh-shaped)
    # not in the reference: the mesh rasteriser (hoisdf_raster_meshes, csrc/raster.hip; hoisdf_amd/render.py), three uses, all off:
    #   seg_source = "mesh" (also HOISDF_SEG=mesh / Trainer(seg_source=...)): the trainer renders targets["hand_seg"] / ["obj_seg"] each
    #     step from the step's own label meshes through meta["cam_intr"] - the modal silhouettes, mutual occlusion included - instead
    #     of taking them from per-frame mask files; with sdf_source = "mesh" both share one MeshSdfSource.  "" = off
    #   eval_silhouette (also HOISDF_SILHOUETTE=1 / Evaluator(silhouette=True) / test.py --silhouette): results.txt gains a block
    #     with the mean IoU of the predicted hand's and the predicted object's rendered silhouettes against the mask targets
    #   overlay_dir (test.py --overlay DIR): one image per sample, the predicted pair blended over the input crop
    seg_source = ""
    eval_silhouette = False
    overlay_dir = ""
    raster_half_pixel = False            # False: pixel (px, py) is sampled at (px, py), the OpenCV convention of the 2D labels
    raster_near = 0.01                   # metres: a face with a corner nearer than this is dropped (no clipping)
    overlay_alpha = 160                  # of 256: the weight of the mesh colour over the image
    # not in the reference: run the object transformer stack on a second HIP stream next to the hand stack
    overlap_streams = True
    resnet_type = 50
    mutliscale_layers = ["stride2", "stride4", "stride8", "stride16", "stride32"]
    mutliscale_dim = 32 + 64 + 128 + 256 + 512

    input_img_shape = (256, 256)
    output_hm_shape = (128, 128, 128)
    sigma = 2.5 / 2

    hidden_dim = 256
    dropout = 0.1
    nheads = 4
    dim_feedforward = 1024
    enc_layers = 6
    dec_layers = 4
    pre_norm = False

    mano_num_queries = 15 + 1 + 1
    mano_shape_indx = 16

    end_epoch = 70
    point_sampling_epoch = 40
    lr = 1e-4
    lr_decay_gamma = 0.7
    lr_drop = 9

    sdf_hand_weight = 50
    sdf_obj_weight = 25
    sdf_cls_weight = 10
    hm_weight = 100 / 100000
    joint_weight = 1 / 10
    cls_weight = 1 / 1
    obj_hm_weight = 1
    obj_rot_weight = 0.7
    obj_trans_weight = 100 / 1

    lambda_verts3d = 1e4
    lambda_joints3d = 1e4
    lambda_manopose = 10
    lambda_manoshape = 0.1
    mano_lambda_regulshape = 0.000001

    eval_mesh = False
    output_dir = "outputs"
    num_thread = 15
    gpu_ids = "0"
    num_gpus = 1
    continue_train = True

    def apply_setting(self, setting: str) -> None:
        """What editing ``setting`` in the reference's config.py does (config.py:39-44,96-97,154)."""
        self.setting = setting
        self.dataset = "ho3d" if "ho3d" in setting else "dexycb"
        self.use_big_decoder = setting == "ho3d"
        self.use_inverse_kinematics = setting == "ho3d_render"
        self.eval_mesh = setting == "dexycb_full"
        self.calc_mutliscale_dim(self.use_big_decoder, self.resnet_type)

    def calc_mutliscale_dim(self, use_big_decoder_l, resnet_type_l):
        if use_big_decoder_l:
            self.mutliscale_dim = 128 + 256 + 512 + 1024 + 2048
        else:
            self.mutliscale_dim = 32 + 64 + 128 + 256 + 512

    def setup_out_dirs(self, model_dir_name):
        self.log_dir = osp.join(self.output_dir, "log", model_dir_name)
        self.model_dir = osp.join(self.output_dir, "model_dump", model_dir_name)
        self.tensorboard_dir = osp.join(self.output_dir, "tensorboard", model_dir_name)

    def set_args(self, gpu_ids, model_dir_name, continue_train=False):
        self.gpu_ids = gpu_ids
        self.num_gpus = len(self.gpu_ids.split(","))
        self.continue_train = continue_train
        self.model_dir_name = model_dir_name
        self.setup_out_dirs(model_dir_name)


cfg = Config()
