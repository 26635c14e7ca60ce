"""The layout of the binding modules: _lib <- _marshal <- ops_eval / ops_mesh / ops_infer <- ops.  The family modules import without
ops (each in a fresh interpreter), and ops still answers to every name it had as one file - a moved name as the very object of its
new home."""
import os
import subprocess
import sys

import pytest

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

# what moved out of ops.py, by new home
MOVED = {
    "_marshal": ["_p", "_st", "_chk", "_workspace", "_counts", "_rows", "_PINNED_I32"],
    "ops_eval": ["_eval_workspace", "eval_thresholds", "eval_object", "eval_hand_joints", "eval_mesh", "eval_accum_init", "eval_accumulate",
                 "eval_accum_finish"],
    "ops_mesh": ["_Mesh", "PreparedMesh", "_as_prepared", "mesh_sdf", "mesh_sample_points", "mesh_sdf_rows", "eval_interaction",
                 "_loss_weight", "_InteractionLoss", "interaction_loss", "_iso_grid", "_iso_values", "iso_grid_points", "iso_refine_grid",
                 "iso_surface", "eval_surface", "raster_meshes", "raster_overlay", "eval_silhouette", "_mask_maps", "mask_edt",
                 "silhouette_workspace_views", "_SilhouetteLoss", "silhouette_loss"],
    "ops_infer": ["PosePrepared", "PoseInferCounts", "pose_infer", "CONV_ACT", "ConvWeight", "conv_plan", "_conv_ws", "_nhwc_slice",
                  "conv2d_nhwc", "maxpool2d_nhwc", "encoder_tensor_table", "EncoderPrepared", "encoder_infer", "ik_mano"],
}

# every non-dunder attribute of ops that is not an imported module, as of the last commit at which ops.py was one file (the private
# names that bench.py, tests/, tools/ and the package reach for are among them), and the one module tests reach through it
OPS_NAMES = """
CONV_ACT ConvWeight DecoderLayerDesc DecoderLayerGrads DecoderLayerWeights EncoderLayerDesc EncoderLayerGrads EncoderLayerWeights
EncoderPrepared MLP_MAX_LAYERS Mlp MlpGrads Optional PoseInferCounts PoseOutputs PosePrepared PreparedMesh Pyramid PyramidNHWC
SdfInferCounts SdfQueryWeights SdfWeightGrads SdfWeights Sequence WeightImageCache _ARENA _ATTENTION_EMU _ATTENTION_F16_EVAL
_ATTN_BWD_EMU _ATTN_FORM_H2 _AddLayerNorm _AttentionCross _AttentionSelf _AttentionSmall _AuxImageLosses _BN_WS _BnAct
_DECODER_LAYER_C _DecoderLayerC _EMU_CACHE _EMU_PLANES _EMU_SMALL_MAX _ENCODER_LAYER_C _EncoderLayer _EncoderLayerC _GEMM_EMU
_GEMM_EMU_DW_MIN_ROWS _GEMM_EMU_DW_MIN_WIDTH _GEMM_EMU_MIN_ROWS _H2 _HeadsVote _InteractionLoss _Linear _ManoHead _Mesh _PINNED_I32
_PointLoss _ProjectGather _PyrAcc _PyrSink _ResidualDropout _SDF_QUERY_TRAIN_C _SEED _SdfHead _SdfQueryTrain _SilhouetteLoss _TOKENS_C
_TokenBuild _Tokens _Vote _VoteLoss _WEIGHT_GEN _WeightNorm _ZeroArena _as_prepared _attn_bwd _attn_bwd_emu _attn_bwd_mode
_attn_emulated _attn_fwd _attn_fwd_emu _attn_fwd_f16 _attn_fwd_mode _attn_h2 _attn_out _bn_workspace_floats _chk _coarse_layer_ok
_conv_ws _counts _emu_bwd _emu_image _emu_ok _emu_small_max_rows _emu_small_ok _eval_workspace _gemm_bwd_input _gemm_bwd_weight
_gemm_fwd _h2 _head_measure _iso_grid _iso_values _lin_bwd_input _lin_bwd_weight _lin_fwd _loss_weight _mag_known _mag_measure
_mano_gt_args _mask_maps _mlp_grads _mlp_struct _nhwc_slice _p _planes_key _pyramid_struct _rows _rows_cl _st _use_f16 _workspace
_zero_views _zeros add_layernorm annotations attention_cross attention_emu attention_self attention_small aux_image_losses bn_act
bn_act_supported bump_weight_generation call conv2d_nhwc conv_plan decoder_layer decoder_layer_ok deterministic encoder_infer
encoder_layer encoder_tensor_table eval_accum_finish eval_accum_init eval_accumulate eval_hand_joints eval_interaction eval_mesh
eval_object eval_silhouette eval_surface eval_thresholds gather_rows gemm_emu heads_vote ik_mano interaction_loss iso_grid_points
iso_refine_grid iso_surface l1_loss_clamped_target lattice_candidates lib linear mano_dirs_image mano_gt mano_head manual_seed
mask_edt maxpool2d_nhwc mesh_sample_points mesh_sdf mesh_sdf_rows next_seed pose_infer posenc prepare_batch_table project_gather
raster_meshes raster_overlay residual_dropout sdf_head sdf_infer sdf_infer_count_begin sdf_query sdf_query_train sdf_query_train_ok
select_smallest_abs set_attention_emu set_attention_f16_eval set_deterministic set_gemm_emu silhouette_loss
silhouette_workspace_views smooth_l1_loss_broadcast token_build tokens tokens_ok vote_aggregate vote_loss weight_norm
zero_arena_begin_step zero_arena_end_step
_lib
""".split()


@pytest.mark.parametrize("module", sorted(MOVED))
def test_family_module_imports_without_ops(module):
    code = (f"import sys, hoisdf_amd.{module}\n"
            "print('ops loaded' if 'hoisdf_amd.ops' in sys.modules else 'ops not loaded')\n")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[-2] == "ops not loaded", r.stdout


def test_ops_answers_to_every_name_it_had():
    from hoisdf_amd import ops
    assert len(OPS_NAMES) == 205 and len(set(OPS_NAMES)) == 205
    missing = [n for n in OPS_NAMES if not hasattr(ops, n)]
    assert not missing, missing
    for names in MOVED.values():
        assert set(names) <= set(OPS_NAMES)


def test_moved_names_are_the_objects_of_their_new_home():
    import importlib
    from hoisdf_amd import ops
    for module, names in MOVED.items():
        home = importlib.import_module("hoisdf_amd." + module)
        for n in names:
            assert getattr(ops, n) is getattr(home, n), (module, n)


def test_one_pool_of_pinned_count_buffers():
    from hoisdf_amd import _marshal, ops, ops_infer
    for cls in (ops.SdfInferCounts, ops_infer.PoseInferCounts):
        assert issubclass(cls, _marshal._QueuedCounts) and "wait" not in vars(cls)
        assert cls.wait.__globals__["_PINNED_I32"] is _marshal._PINNED_I32
    assert ops._PINNED_I32 is _marshal._PINNED_I32 and not hasattr(ops_infer, "_PINNED_I32")
