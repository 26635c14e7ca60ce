#!/usr/bin/env python3
"""Emits HPHASE (wave tile 128 x 128, 4 x 4 MFMA blocks: the 256 x 256 tile, one workgroup per CU) and HPHASE2 (wave tile 128 x 64,
4 x 2 blocks: the 256 x 128 tile, two workgroups per CU), the pinned bodies of one slab phase of emu_h2_kernel
(hoisdf_amd/csrc/gemm_emu_h2.hip): three groups of 4 NJ v_mfma_f32_32x32x16_f16 (three products per slab), each MFMA followed by the
fragment reads / staging units pinned behind it.

  group 0  hi hi of slab s - 1   A = aH, B = bC      (fragments read before the barrier)
  group 1  lo hi of slab s       A = aL, B = bN      aL / bN read during group 0
  group 2  hi lo of slab s       A = aH, B = bL      aH re-read at the start of group 1 (its last use is the end of group 0), then bL
On exit aH / bN hold slab s: the next phase is called with bC and bN exchanged.  Staging of slab s + 1 (per thread four quads of
the activation tile -> scale, hi plane, residual, lo plane -> two 8-byte LDS writes each; NJ 16-byte pieces of the weight image)
and the loads of slab s + 2 are spread over the MFMAs.
    python tools/gen/h2_phase.py > hoisdf_amd/csrc/h2_phase.inc"""
from phase_emit import header, macro


def table(nj):
    g = 4 * nj                      # MFMAs per group
    n = 3 * g
    t = {}
    add = lambda s, w: t.setdefault(s, []).append(w)
    for i in range(4): add(i, f"aL[{i}] = HLA(cur, 1, {i})")
    for j in range(nj): add(4 + j, f"bN[{j}] = HLB(cur, 0, {j})")
    for i in range(4): add(g + i, f"aH[{i}] = HLA(cur, 0, {i})")          # aH[3]'s last use: MFMA g - 1
    for j in range(nj): add(g + 4 + j, f"bL[{j}] = HLB(cur, 1, {j})")
    # weight image pieces: stage write, then the reload of the same register for slab s + 2
    for q in range(nj):
        add((8 if nj == 4 else 6) + q, f"HSTB(nxt, {q})")
        add((12 if nj == 4 else 8) + q, f"HLDGB({q}, (s) + 2)")
    # activation quads: item i = UI + two pairs x (C1, C2), two LDS writes, the reload
    for i in range(4):
        s0 = (9 + 9 * i) if nj == 4 else (1 + 6 * i - (i > 0))
        units = [f"HUI({i}, (s) + 1); HC1({2 * i})", f"HC2({2 * i})", f"HC1({2 * i + 1})", f"HC2({2 * i + 1})"]
        if nj == 4:
            for k, w in enumerate(units): add(s0 + k, w)
            add(s0 + 4, f"HSTA(nxt, {i}, t0, 0); HLDGA({i}, (s) + 2)")
            add(s0 + 5, f"HSTA(nxt, {i}, t1, 1)")
        else:                       # 24 slots: a pair (C1, C2) per slot is too much VALU behind one MFMA; one unit per slot, items back to back
            s0 = 6 * i
            for k, w in enumerate(units): add(s0 + k, w)
            add(s0 + 4, f"HSTA(nxt, {i}, t0, 0); HLDGA({i}, (s) + 2)")
            add(s0 + 5, f"HSTA(nxt, {i}, t1, 1)")
    assert max(t) < n, max(t)
    return t


def emit(nj, name):
    t = table(nj)
    g = 4 * nj
    groups = [("aH", "bC"), ("aL", "bN"), ("aH", "bL")]
    note = {0: "hi hi of slab s - 1", g: "lo hi of slab s", 2 * g: "hi lo of slab s"}
    lines = [f"#define {name}(cur, nxt, s, bC, bN)", "  do {"]
    for m in range(3 * g):
        ax, bx = groups[m // g]
        i, j = (m % g) // nj, m % nj
        w = "; ".join(t.get(m, [])) or "NOP_"
        l = f"    HM1({ax}, {bx}, {i}, {j}, {w});"
        if m in note: l += f"   /* {note[m]} */"
        lines.append(l)
    lines.append("  } while (0)")
    return macro(lines)


if __name__ == "__main__":
    print(header("h2_phase.py", "the slot tables of emu_h2_kernel's phase (one MFMA + the units pinned behind it)"))
    print(emit(4, "HPHASE"))
    print(emit(2, "HPHASE2"))
