#!/usr/bin/env python3
"""Kernel-by-kernel comparison of gfx950 assembly before and after a change that must not touch code generation:
`python tools/cmp_kernel_asm.py before.s after.s [after2.s ...]` over the `*-hip-amdgcn-*.s` files that `hipcc -save-temps=obj`
leaves.  Kernels are matched by their demangled name without the parameter list.  Per kernel: the descriptor (registers, LDS, scratch,
spills) must be equal; the body (symbol to .Lfunc_end, `;` comments dropped, .LBB labels renumbered) is `same`, `prologue-only` (equal
from the first v_mfma to the end; differing lines and the instruction counts ahead of that MFMA are listed) or `differs`."""
import difflib
import re
import subprocess
import sys

DESC = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    spills = dict(re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)", text))
    vspills = dict(re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", text))
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
        body = text[text.index(f"\n{sym}:") + 1:]
        body = body[:body.index(".Lfunc_end")]
        lines = [l.split(";")[0].strip().replace(sym, "KERNEL") for l in body.split("\n")[1:]]
        lines = [l for l in lines if l]
        labels = {}
        for l in lines:
            for lb in re.findall(r"\.LBB\d+_\d+", l): labels.setdefault(lb, f".L{len(labels)}")
        lines = [re.sub(r"\.LBB\d+_\d+", lambda m: labels[m.group(0)], l) for l in lines]
        d = text[text.index(f".amdhsa_kernel {sym}"):]
        d = d[:d.index(".end_amdhsa_kernel")]
        desc = tuple(re.search(rf"\.amdhsa_{k} (\S+)", d).group(1) for k in DESC) + (spills.get(sym, "?"), vspills.get(sym, "?"))
        name = subprocess.run(["c++filt", sym], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
        out[re.match(r"(?:void )?([\w:]+(?:<[^()]*>)?)", name).group(1)] = (lines, desc)
    return out


before, after = kernels(sys.argv[1]), {}
for p in sys.argv[2:]: after.update(kernels(p))
count = {"same": 0, "prologue-only": 0, "differs": 0}
print(f"{'kernel':46s} {'instr':>6s}  verdict   descriptor (vgpr accum_offset sgpr lds scratch sgpr-spill vgpr-spill)")
for name in sorted(before):
    (a, da), (b, db) = before[name], after.get(name, ([], ()))
    isn = lambda ls: [l for l in ls if not l.endswith(":") and not l.startswith(".")]
    mf = lambda ls: next((i for i, l in enumerate(ls) if l.startswith("v_mfma")), len(ls))
    note = ""
    if a == b: verdict = "same"
    elif da == db and a[mf(a):] == b[mf(b):] and mf(a) < len(a):
        verdict = "prologue-only"
        nd = sum(1 for l in difflib.ndiff(a[:mf(a)], b[:mf(b)]) if l[0] in "+-")
        note = f"   {nd} lines differ ahead of the first MFMA; instructions there {len(isn(a[:mf(a)]))} -> {len(isn(b[:mf(b)]))}"
    else: verdict = "differs"
    if da != db: verdict, note = "differs", f"   descriptor after: {' '.join(db)}"
    count[verdict] += 1
    print(f"{name:46s} {len(isn(a)):6d}  {verdict:9s} {' '.join(da)}{note}")
print(f"{len(before)} kernels: " + ", ".join(f"{v} {k}" for k, v in count.items()) + f"; kernels only after: {sorted(set(after) - set(before))}")
sys.exit(1 if count["differs"] else 0)
