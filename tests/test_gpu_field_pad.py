"""GPU: Model.field_surface(pad_cells=...) - the margin, in coarse cells, that hoisdf_iso_refine_grid keeps around the inside nodes.
The default (1) is today's behaviour bit for bit; a wider margin gives a fine grid that contains the default one (a consumer that
starts OFF the surface, such as a fit of the predicted mesh to the field, needs the field some way around it).  The small untrained
model of tests/test_gpu_isosurf.py: this tests plumbing, not accuracy."""
import inspect

import numpy as np
import pytest
import torch

from hoisdf_amd import isosurf_oracle as iso
from hoisdf_amd import ops

pytestmark = pytest.mark.gpu
N, COARSE = 17, 9                    # the sizes of tests/test_gpu_isosurf.py's field_surface tests


@pytest.fixture(scope="module")
def small_model():
    from hoisdf_amd import testing as T
    from hoisdf_amd.config import Config
    from hoisdf_amd.model import get_model
    from hoisdf_amd.nets import mano as MANO
    c = Config()
    c.resnet_type = 18
    c.apply_setting("dexycb")
    c.num_samp_hand, c.num_samp_obj = 300, 100
    model = get_model("test", cfg=c, mano_layer=MANO.ManoLayer(MANO.synthetic_assets(0)), with_encoder=False)
    sd = model.state_dict()
    for k in sd:
        if not k.startswith("mano_head"):
            sd[k] = T.det_param(k, sd[k].shape)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    pyr_cpu = T.synthetic_pyramid(2, seed=4)
    pyr = ops.PyramidNHWC([v.cuda().permute(0, 2, 3, 1).contiguous() for v in pyr_cpu.values()])
    _, _, meta = T.synthetic_batch(2, 300, 8, seed=5)
    dm = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in meta.items()}
    return model, pyr, dm


@pytest.mark.parametrize("kind", ["hand", "obj"])
def test_pad_cells_default_keeps_the_bits_and_a_wider_margin_contains_it(small_model, kind):
    from hoisdf_amd.model import Model
    sig = inspect.signature(Model.field_surface).parameters
    assert sig["pad_cells"].default == 1 and sig["pad_cells"].kind is inspect.Parameter.KEYWORD_ONLY
    model, pyr, dm = small_model
    a = model.field_surface(pyr, dm, kind, n=N, coarse_n=COARSE, return_values=True)
    b = model.field_surface(pyr, dm, kind, n=N, coarse_n=COARSE, return_values=True, pad_cells=1)
    assert all(torch.equal(x, y) for x, y in zip(a[:4], b[:4])) and all(torch.equal(a[4][k], b[4][k]) for k in a[4])
    for pad in (0, 3):
        w = model.field_surface(pyr, dm, kind, n=N, coarse_n=COARSE, return_values=True, pad_cells=pad)[4]
        assert torch.equal(w["coarse_values"], a[4]["coarse_values"]) and torch.equal(w["coarse_grid"], a[4]["coarse_grid"])
        coarse, cgrid = w["coarse_values"].cpu().numpy(), w["coarse_grid"].cpu().numpy()
        for s in range(2):                                            # the refined grid is the oracle's for that margin
            want = iso.refine_grid(coarse[s], cgrid[s], COARSE, 0.0, pad, N)
            assert np.array_equal(w["grid"][s].cpu().numpy().view(np.uint32), want.view(np.uint32)), (kind, pad, s)
        lo, hi = w["grid"][:, :3], w["grid"][:, :3] + w["grid"][:, 3:6] * (N - 1)
        lo1, hi1 = a[4]["grid"][:, :3], a[4]["grid"][:, :3] + a[4]["grid"][:, 3:6] * (N - 1)
        if pad == 3:
            assert (lo <= lo1).all() and (hi >= hi1 - 1e-6).all() and (w["grid"][:, 3:6] >= a[4]["grid"][:, 3:6]).all()
        else:
            assert (lo >= lo1).all() and (hi <= hi1 + 1e-6).all()
