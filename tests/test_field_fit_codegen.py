"""CPU: csrc/field_fit.hip compiled to gfx950 assembly (hipcc cross-compiles without a GPU, as tests/test_kernel_audit.py obtains
assembly): in every kernel of the file no workgroup barrier lies between a label and a later branch back to that label - no barrier
inside any loop.  A one-launch form of this fit once hung on its first run: `if (lane == 0)` blocks at both ends of the step loop were
threaded across the back edge by the compiler, and the barrier landed in a loop that lanes 1 - 63 of wave 0 ran while lane 0 waited
outside it.  The kernels here iterate on the host instead; this test keeps it so.  It reads labels, branches and barriers only, twice:
by the span from a label to a later branch back to it (strict: a cold block laid out behind a barrier with a jump back counts, loop
or not), and on the control-flow graph (a barrier whose block can reach itself, wherever the blocks were laid out)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("ff_init_kernel", "ff_round_kernel", "ff_finish_kernel")


def barriers_in_loops(lines):
    """lines of one function -> [(label, label line, branch line, barrier line)] for every barrier inside a backward branch's span"""
    label_at = {}
    for i, ln in enumerate(lines):
        m = re.match(r"(\.?\w+):", ln)
        if m:
            label_at[m[1]] = i
    barriers = [i for i, ln in enumerate(lines) if re.match(r"\s*s_barrier\b", ln)]
    found = []
    for j, ln in enumerate(lines):
        m = re.match(r"\s*s_c?branch\w*\s+(\.?\w+)", ln)
        if m and m[1] in label_at and label_at[m[1]] <= j:
            found += [(m[1], label_at[m[1]], j, b) for b in barriers if label_at[m[1]] <= b <= j]
    return found


def barriers_on_cycles(lines):
    """the same question on the control-flow graph, which block layout cannot fool either way: lines of one function -> the line
    numbers of barriers whose basic block can reach itself.  Blocks start at labels and after branches; a conditional branch
    falls through as well, s_branch and s_endpgm do not"""
    starts = {0}
    for i, ln in enumerate(lines):
        if re.match(r"(\.?\w+):", ln):
            starts.add(i)
        if re.match(r"\s*(s_c?branch|s_endpgm|s_setpc)", ln):
            starts.add(i + 1)
    starts = sorted(x for x in starts if x < len(lines))
    block_of = {}
    for b, st in enumerate(starts):
        for i in range(st, starts[b + 1] if b + 1 < len(starts) else len(lines)):
            block_of[i] = b
    label_block = {m[1]: block_of[i] for i, ln in enumerate(lines) for m in [re.match(r"(\.?\w+):", ln)] if m}
    succ = {b: set() for b in range(len(starts))}
    for b, st in enumerate(starts):
        end = (starts[b + 1] if b + 1 < len(starts) else len(lines)) - 1
        last = next((lines[i] for i in range(end, st - 1, -1) if lines[i].strip() and not lines[i].lstrip().startswith(";")), "")
        m = re.match(r"\s*s_c?branch\w*\s+(\.?\w+)", last)
        if m and m[1] in label_block:
            succ[b].add(label_block[m[1]])
        if not re.match(r"\s*(s_branch|s_endpgm|s_setpc)", last) and b + 1 < len(starts):
            succ[b].add(b + 1)
    found = []
    for i, ln in enumerate(lines):
        if re.match(r"\s*s_barrier\b", ln):
            seen, todo = set(), list(succ[block_of[i]])
            while todo:
                x = todo.pop()
                if x not in seen:
                    seen.add(x)
                    todo += succ[x]
            if block_of[i] in seen:
                found.append(i)
    return found


def test_the_reader_finds_a_barrier_in_a_loop_and_passes_one_outside():
    loop = ["f:", ".LBB0_1:", "  v_add_f64 v[0:1], v[0:1], v[2:3]", "  s_barrier", "  s_cbranch_execnz .LBB0_1", "  s_endpgm"]
    assert barriers_in_loops(loop) == [(".LBB0_1", 1, 4, 3)]
    straight = ["f:", "  s_cbranch_scc1 .LBB0_2", ".LBB0_1:", "  v_nop", "  s_cbranch_execnz .LBB0_1", ".LBB0_2:", "  s_barrier", "  s_endpgm"]
    assert barriers_in_loops(straight) == []
    assert barriers_on_cycles(loop) == [3] and barriers_on_cycles(straight) == []
    # a loop whose barrier block is laid out behind the exit, outside the label-to-branch span: only the graph sees it
    far = ["f:", ".LBB0_1:", "  v_nop", "  s_cbranch_scc1 .LBB0_3", ".LBB0_2:", "  s_endpgm", ".LBB0_3:", "  s_barrier", "  s_branch .LBB0_1"]
    assert barriers_on_cycles(far) == [7]
    # a cold block behind a barrier that jumps back to code before it is no loop: the span flags it, the graph does not
    cold = ["f:", "  s_cbranch_scc1 .LBB0_3", ".LBB0_1:", "  v_nop", "  s_barrier", "  s_endpgm", ".LBB0_3:", "  v_nop", "  s_branch .LBB0_1"]
    assert barriers_on_cycles(cold) == [] and barriers_in_loops(cold) == [(".LBB0_1", 2, 8, 4)]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_no_field_fit_kernel_has_a_barrier_inside_a_loop(tmp_path):
    csrc = os.path.join(ROOT, "hoisdf_amd", "csrc")
    flags = re.search(r"^CXXFLAGS\s*=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), re.M)[1].replace("$(ARCH)", "gfx950").split()
    r = subprocess.run([HIPCC] + flags + ["-c", os.path.join(csrc, "field_fit.hip"), "-o", str(tmp_path / "ff.o"), "-save-temps=obj"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(str(tmp_path / asm[0])).read()
    names = sorted(set(re.findall(r"\.name:\s+(_Z\S+)", text)))
    assert len(names) == len(KERNELS) and all(any(k in n for n in names) for k in KERNELS), names
    for name in names:
        body = re.search(r"^" + re.escape(name) + r":.*?^\.Lfunc_end\d+:", text, re.S | re.M)
        assert body, name
        lines = body[0].splitlines()
        n_barrier = sum(bool(re.match(r"\s*s_barrier\b", ln)) for ln in lines)
        back = sum(1 for _ in re.finditer(r"s_c?branch", body[0]))
        found = barriers_in_loops(lines)
        assert barriers_on_cycles(lines) == [], (name, barriers_on_cycles(lines))
        print(f"{name}: {len(lines)} lines, {n_barrier} barriers, {back} branches, barriers inside a loop: {found}")
        assert not found, (name, found)
        # what the source says: two barriers in init, one per round, none in finish - and the loops are there to be looked at
        want = 2 if "init" in name else 1 if "round" in name else 0
        assert n_barrier == want, (name, n_barrier)
        assert any(re.match(r"\s*s_c?branch\w*\s+(\.?\w+)", ln) for ln in lines)
