"""-m gpu: the companion test of tests/test_gpu_fullsize.py at the reference's default point counts: 600 hand + 200 object points, so
the encoder sees S = 800 tokens and n_query = 600 - neither a multiple of the emulated GEMM's 128-row wave sub-tile, so the rows of two
samples share sub-tiles.  B = 3 is the smallest batch that puts the B S = 2400 rows on the emulated route (>= 2048 rows), where the
attention operands take one f16x2 scale per (sample, head): sample 0's outputs must be bit-identical whatever samples 1 and 2 are."""
import pytest
import torch

from hoisdf_amd import testing as T
from hoisdf_amd.config import Config

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, NH, NO = 3, 600, 200


@pytest.fixture(scope="module")
def setup():
    from hoisdf_amd import ops
    from hoisdf_amd.model import get_model
    from hoisdf_amd.nets import mano as MANO
    c = Config()
    c.resnet_type = 50
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj, c.bins_n = NH, NO, 64
    torch.manual_seed(0)
    model = get_model("train", cfg=c, mano_layer=MANO.ManoLayer(MANO.synthetic_assets(0)), with_encoder=False).to(DEV)
    model.eval()                                                     # dropout off; mode="train" still selects branch A
    model._jitter = lambda like, d: torch.zeros_like(like)
    pyr = ops.PyramidNHWC([v.to(DEV).permute(0, 2, 3, 1).contiguous() for v in T.synthetic_pyramid(B, seed=3).values()])
    batch = tuple(T.to_device(x, DEV) for x in T.synthetic_batch(B, NH, NO, seed=31))
    return model, pyr, batch


def run(model, pyr, batch, mode):
    with torch.no_grad():
        loss, out = model.hot_path(pyr, *batch, mode, 0, 0.1)
    return {**loss, **out}


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_sample_0_does_not_depend_on_its_companions_at_600_plus_200_points(setup, mode):
    """"train" = branch A on the given points (dropout off), "eval" = the dense-lattice sdf_infer path.  Samples 1 and 2 are replaced
    by other pyramids, points and cameras, at x 1 and with a x 300 louder pyramid: every `*_out` of sample 0 stays bit for bit, sample
    1's really change."""
    from hoisdf_amd import ops
    assert (B * (NH + NO)) >= ops._GEMM_EMU_MIN_ROWS and (NH + NO) % 128 and NH % 128
    model, pyr, batch = setup
    ref = run(model, pyr, batch, mode)
    other = tuple(T.to_device(x, DEV) for x in T.synthetic_batch(B, NH, NO, seed=977))
    pyr_o = [v.to(DEV).permute(0, 2, 3, 1).contiguous() for v in T.synthetic_pyramid(B, seed=55).values()]
    for loud in (1.0, 300.0):
        levels = [torch.cat([l[:1], lo[1:] * loud]) for l, lo in zip(pyr.levels, pyr_o)]
        mixed = tuple({k: (torch.cat([v[:1], other[i][k][1:]]) if torch.is_tensor(v) and v.shape[:1] == (B,) else v) for k, v in d.items()}
                      for i, d in enumerate(batch))
        got = run(model, ops.PyramidNHWC(levels), mixed, mode)
        n = 0
        for k, v in ref.items():
            if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == B and k.endswith("_out"):
                assert float((got[k][1] - v[1]).abs().max()) > 0, k                        # the companions really changed
                assert torch.equal(got[k][0], v[0]), (mode, loud, k, float((got[k][0] - v[0]).abs().max()))
                n += 1
        assert n >= 3
