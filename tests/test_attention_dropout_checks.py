"""The checks of tests/test_gpu_attention_dropout.py (hoisdf_amd/testing.py: mask probes + float64 truth) can fail: a float64
torch "kernel" with a known random mask passes all of them and its probes return that mask; five deliberately wrong variants - the
mistakes a dropout backward can make without the "linear in V" identity noticing - are each rejected by the check that is there for
them.  Runs on the CPU; nothing here touches a GPU."""
import math
import re

import pytest
import torch

from hoisdf_amd import testing as T

B, H, LQ, LK, KV, E = 3, 4, 100, 200, 149, 256                  # case A of the GPU file


class ToyKernel:
    """softmax attention with dropout on P, forward and hand-written backward in float64 (the algebra of csrc/attention.hip:
    delta = rowsum(dO * O), dS = P (dP * M / (1 - p) - delta)), with switches for the mistakes"""

    def __init__(self, mask_fwd, p, valid, mask_bwd=None, delta_from_undropped_o=False, no_inv_keep_in_dp=False):
        self.mf, self.mb = mask_fwd.double(), (mask_fwd if mask_bwd is None else mask_bwd).double()
        self.p, self.valid = p, valid
        self.delta_from_undropped_o, self.no_inv_keep_in_dp = delta_from_undropped_o, no_inv_keep_in_dp

    def _merge(self, x):
        return x.transpose(1, 2).reshape(x.shape[0], x.shape[2], -1)

    def fwd(self, q, k, v, dropped=True):
        P = T.reference_probs(q, k, H, self.valid)
        return self._merge((P * self.mf / (1.0 - self.p) if dropped else P) @ T._heads(v.double(), H))

    def bwd(self, q, k, v, do):
        P = T.reference_probs(q, k, H, self.valid)
        qh, kh, vh, doh = (T._heads(t.double(), H) for t in (q, k, v, do))
        inv_keep = 1.0 / (1.0 - self.p)
        dv = (P * self.mb * inv_keep).transpose(-1, -2) @ doh
        dP = (doh @ vh.transpose(-1, -2)) * self.mb * (1.0 if self.no_inv_keep_in_dp else inv_keep)
        delta = (doh * T._heads(self.fwd(q, k, v, dropped=not self.delta_from_undropped_o), H)).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        return self._merge(dS @ kh) / 8.0, self._merge(dS.transpose(-1, -2) @ qh) / 8.0, self._merge(dv)


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(5)
    q, do = torch.randn(B, LQ, E, generator=g), torch.randn(B, LQ, E, generator=g)
    k, v = torch.randn(B, LK, E, generator=g), torch.randn(B, LK, E, generator=g)
    valid = (torch.arange(LK) < KV).view(1, 1, 1, LK)
    p = 0.1
    mask = (torch.randint(0, 65536, (B, H, LQ, LK), generator=g) >= math.floor(p * 65536)) & valid
    return dict(q=q, k=k, v=v, do=do, valid=valid, p=p, mask=mask, p64=T.reference_probs(q, k, H, valid))


def _run_all(kern, c):
    """every check of the GPU file in its order; returns the probed mask"""
    T.check_probe_validity(c["p64"], c["valid"])
    pdf = T.probe_dropped_probs_forward(kern.fwd, c["q"], c["k"], H)
    pdb = T.probe_dropped_probs_backward(kern.bwd, c["q"], c["k"], c["v"], H)
    m = T.check_same_mask(pdf, pdb, c["valid"])
    T.check_kept_values(pdf, c["p64"], m, c["p"])
    T.check_forward_and_gradients(kern.fwd, kern.bwd, c["q"], c["k"], c["v"], c["do"], H, c["valid"], m, c["p"])
    T.check_mask_statistics(m, KV, c["p"])
    return m


def test_a_right_kernel_passes_and_the_probes_return_its_mask(case):
    c = case
    m = _run_all(ToyKernel(c["mask"], c["p"], c["valid"]), c)
    assert torch.equal(m, c["mask"])
    # the probes read the dropped matrix itself, not only its support
    pdf = T.probe_dropped_probs_forward(ToyKernel(c["mask"], c["p"], c["valid"]).fwd, c["q"], c["k"], H)
    assert torch.equal(pdf, c["p64"] * c["mask"] / (1.0 - c["p"]))


def test_the_hand_written_backward_is_autograd(case):
    """the toy's own algebra against autograd, so that the wrong variants below differ from the truth by their mistake alone"""
    c = case
    kern = ToyKernel(c["mask"], c["p"], c["valid"])
    errs = T.check_forward_and_gradients(kern.fwd, kern.bwd, c["q"], c["k"], c["v"], c["do"], H, c["valid"], c["mask"], c["p"],
                                         rel_o=1e-12, rel_g=1e-12)
    assert max(errs.values()) <= 1e-12


@pytest.mark.parametrize("variant,check", [("delta from the undropped output", "forward and gradients: dq"),
                                           ("backward mask shifted by one key", "same mask"),
                                           ("backward mask of every head taken from head 0", "same mask"),
                                           ("inv_keep missing in dP", "forward and gradients: dq"),
                                           ("the pair partner's decision on odd columns", "mask statistics: columns 2n, 2n+1")])
def test_a_wrong_kernel_is_rejected_by_the_check_that_is_there_for_it(case, variant, check):
    c = case
    mask = c["mask"]
    if variant == "delta from the undropped output":
        kern = ToyKernel(mask, c["p"], c["valid"], delta_from_undropped_o=True)
    elif variant == "backward mask shifted by one key":
        kern = ToyKernel(mask, c["p"], c["valid"], mask_bwd=torch.roll(mask, 1, -1) & c["valid"])
    elif variant == "backward mask of every head taken from head 0":
        kern = ToyKernel(mask, c["p"], c["valid"], mask_bwd=mask[:, :1].expand_as(mask))
    elif variant == "inv_keep missing in dP":
        kern = ToyKernel(mask, c["p"], c["valid"], no_inv_keep_in_dp=True)
    else:                                                       # forward and backward agree - only the statistics can see it
        paired = mask.clone()
        paired[..., 1::2] = mask[..., 0::2]
        kern = ToyKernel(paired & c["valid"], c["p"], c["valid"])
    with pytest.raises(AssertionError, match="^" + re.escape(check)):
        _run_all(kern, c)


def test_the_wrong_gradients_leave_dv_and_the_forward_right(case):
    """what made these mistakes invisible so far: with a wrong delta or a missing inv_keep in dP the forward and dV - all that the
    "linear in V" identity sees - stay exact; dq and dk alone are wrong, and by far more than the bar"""
    c = case
    for kw in (dict(delta_from_undropped_o=True), dict(no_inv_keep_in_dp=True)):
        kern = ToyKernel(c["mask"], c["p"], c["valid"], **kw)
        ro, rq, rk, rv = T.reference_dropout_attention(c["q"], c["k"], c["v"], c["do"], H, c["valid"], c["mask"], c["p"])
        dq, dk, dv = kern.bwd(c["q"], c["k"], c["v"], c["do"])
        assert T._rel_err(kern.fwd(c["q"], c["k"], c["v"]), ro) <= 1e-12 and T._rel_err(dv, rv) <= 1e-12
        assert T._rel_err(dq, rq) > 1e-3 and T._rel_err(dk, rk) > 1e-3, kw
