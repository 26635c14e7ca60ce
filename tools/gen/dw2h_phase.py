#!/usr/bin/env python3
"""Emits the DHPHASE macro of emu_dw2h_kernel (hoisdf_amd/csrc/gemm_emu_dw.hip, the f16x2 grad-weight): the 48 MFMAs of a phase
(hi hi of slab s - 1 | lo hi, hi lo of slab s; 4 x 4 blocks each), each followed by the units pinned behind it: the 16 fragment
reads of slab s, the conversion + LDS writes of slab s + 1 (four columns x (four row pairs x (DU1, DU2) + two 16-byte writes)) and
the reload of the patch registers for slab s + 2.

  slots  0-15  hi hi of slab s - 1   A = aH, B = bC      (fragments read before the barrier)
  slots 16-31  lo hi of slab s       A = aL, B = bN      aL read at 0-3, bN at 4-7
  slots 32-47  hi lo of slab s       A = aH, B = bL      aH re-read at 16-19 (last used by MFMA 15), bL at 20-23
On exit aH / bN hold the hi pieces of slab s: the next phase is called with bC and bN exchanged.
    python tools/gen/dw2h_phase.py > hoisdf_amd/csrc/dw2h_phase.inc"""
from phase_emit import header, macro


def table():
    t = {}
    add = lambda s, w: t.setdefault(s, []).append(w)
    for i in range(4): add(i, f"aL[{i}] = DLA(cur, 1, {i})")
    for j in range(4): add(4 + j, f"bN[{j}] = DLB(cur, 0, {j})")
    for i in range(4): add(16 + i, f"aH[{i}] = DLA(cur, 0, {i})")
    for j in range(4): add(20 + j, f"bL[{j}] = DLB(cur, 1, {j})")
    # column j of the patch: four row pairs x (DU1, DU2), then its two planes' LDS writes
    for j in range(4):
        s0 = 2 + 10 * j
        k = 0
        for pr in range(4):
            for u in (1, 2):
                add(s0 + k, f"DU{u}({j}, {pr})")
                k += 1
        add(s0 + 8, f"DSTA(nxt, {j}, 0)")
        add(s0 + 9, f"DSTA(nxt, {j}, 1)")
    # the patch lives in two half sets (columns 0-1 / 2-3 of every row): a half is requested again for slab s + 2 as soon as its
    # two columns of slab s + 1 are converted; the bitmap words once column 0 has packed them
    for e in range(8): add(10 + e, f"DLDM({e}, (s) + 2)")
    for e in range(8): add(22 + e, f"DLDG(0, {e}, (s) + 2)")
    for e in range(8): add(40 + e, f"DLDG(1, {e}, (s) + 2)")
    assert max(t) < 48, max(t)
    return t


def emit():
    t = table()
    groups = [("aH", "bC"), ("aL", "bN"), ("aH", "bL")]
    note = {0: "hi hi of slab s - 1", 16: "lo hi of slab s", 32: "hi lo of slab s"}
    lines = ["#define DHPHASE(cur, nxt, s, bC, bN)", "  do {"]
    for m in range(48):
        ax, bx = groups[m // 16]
        i, j = (m % 16) // 4, m % 4
        w = "; ".join(t.get(m, [])) or "NOP_"
        l = f"    M1({ax}, {bx}, {i}, {j}, {w});"
        if m in note: l += f"   /* {note[m]} */"
        lines.append(l)
    lines.append("  } while (0)")
    return macro(lines)


if __name__ == "__main__":
    print(header("dw2h_phase.py", "the slot table of emu_dw2h_kernel's phase (one MFMA + the units pinned behind it)"))
    print(emit())
