"""The audit of tests/test_kernel_audit.py for csrc/attention_emu_bwd4g.hip, the f16x2 attention backward with two dS pieces (60 MFMAs per
query tile, issued through inline asm like the other two units of csrc/attention_emu_bwd4.inc): exactly the two instantiations the
library launches, no spills, no scratch, no VALU write of an MFMA operand within two instructions ahead of the MFMA, every non-MFMA
reader of an accumulator at least two MFMAs behind the chain's last product; and the committed schedule is what its generator prints.
hipcc cross-compiles for gfx950 without a GPU (about ten seconds)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOL = "_ZN6hoisdf21emu_attn_bwd4g_kernel"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_two_piece_attention_backward_asm_mfma_hazard_audit(tmp_path):
    src = os.path.join(ROOT, "hoisdf_amd", "csrc", "attention_emu_bwd4g.hip")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "-Wno-nonnull", "-c", src, "-o", str(tmp_path / "b4g.o"),
           "-save-temps=obj"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    path = str(tmp_path / asm[0])
    text = open(path).read()
    kernels = re.findall(r"\.name:\s+(" + SYMBOL + r"\S+)", text)
    assert len(set(kernels)) == 2, kernels                       # <DROP> x 2: every instantiation the library launches
    spills = re.findall(r"\.name:\s+" + SYMBOL + r".*?\.vgpr_spill_count:\s+(\d+)", text, re.S)
    scratch = re.findall(r"\.name:\s+" + SYMBOL + r".*?\.private_segment_fixed_size:\s+(\d+)", text, re.S)
    assert len(spills) == 2 and len(scratch) == 2 and all(int(x) == 0 for x in spills + scratch), (spills, scratch)
    a = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_mfma.py"), path, "bwd4g_kernel"], capture_output=True, text=True)
    assert a.returncode == 0, a.stdout[-3000:]
    assert a.stdout.count("MFMAs 60 findings 0") == 2, a.stdout


def test_two_piece_schedule_is_current():
    """the committed attn_bwd4g_phase.inc is what tools/gen/attn_bwd4g_phase.py prints"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen", "attn_bwd4g_phase.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    have = open(os.path.join(ROOT, "hoisdf_amd", "csrc", "attn_bwd4g_phase.inc")).read()
    assert out.stdout.strip() == have.strip()
