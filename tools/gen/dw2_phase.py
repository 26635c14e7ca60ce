#!/usr/bin/env python3
"""Emits the DPHASE macro of emu_dw2_kernel (hoisdf_amd/csrc/gemm_emu_dw.hip): the 96 MFMAs of a phase (second half of slab s - 1:
a1 b1, a1 b0, a2 b0 | first half of slab s: a0 b2, a0 b1, a0 b0; 4 x 4 blocks each), each followed by the units pinned behind it:
the 24 fragment reads of slab s, the reload of the other patch register set (slab s + 2) and the conversion + LDS writes of slab
s + 1 (four columns x (four row pairs x U1..U4 + three 16-byte writes)).  `python tools/gen/dw2_phase.py` prints the macro."""
from phase_emit import header, macro
import sys

# B fragment sets: bP = y1 of slab s - 1, then y2 of slab s; bQ = y0 of slab s - 1, then y0 of slab s; bR = y1 of slab s (the next
# phase is called with bP and bR exchanged)
GROUPS = [("aX", "bP"), ("aX", "bQ"), ("aY", "bQ"), ("aZ", "bP"), ("aZ", "bR"), ("aZ", "bQ")]
NOTE = {0: "x1 y1 of slab s - 1", 16: "x1 y0", 32: "x2 y0", 48: "x0 y2 of slab s", 64: "x0 y1", 80: "x0 y0"}


def table():
    t = {}
    add = lambda s, w: t.setdefault(s, []).append(w)
    for i in range(4): add(i, f"aZ[{i}] = DLA(cur, 0, {i})")
    for j in range(4): add(16 + j, f"bP[{j}] = DLB(cur, 2, {j})")        # bP (y1 of slab s - 1) was last used by MFMA 15
    for j in range(4): add(20 + j, f"bR[{j}] = DLB(cur, 1, {j})")
    for j in range(4): add(48 + j, f"bQ[{j}] = DLB(cur, 0, {j})")        # bQ (y0 of slab s - 1) was last used by MFMA 47
    for i in range(4): add(32 + i, f"aX[{i}] = DLA(cur, 1, {i})")        # aX last used by MFMA 31
    for i in range(4): add(52 + i, f"aY[{i}] = DLA(cur, 2, {i})")        # aY last used by MFMA 47
    # the patch lives in two half sets (columns 0-1 / 2-3 of every row): a half is requested again for slab s + 2 as soon as its two
    # columns of slab s + 1 are converted - >= 56 MFMAs before its next use, without a second patch set
    for e in range(8): add(45 + e, f"DLDG(0, {e}, (s) + 2)")
    for e in range(8): add(85 + e, f"DLDG(1, {e}, (s) + 2)")
    for e in range(8): add(26 + e, f"DLDM({e}, (s) + 2)")                 # bitmap words: their registers are free once column 0 is through
    for j in range(4):
        s0 = 12 + 20 * j
        k = 0
        for pr in range(4):
            for u in (1, 2, 3, 4):
                add(s0 + k, f"DU{u}({j}, {pr})")
                k += 1
        for pl in range(3): add(s0 + 16 + pl, f"DSTA(nxt, {j}, {pl})")
    assert max(t) < 96, max(t)
    return t


def emit():
    t = table()
    lines = ["#define DPHASE(cur, nxt, s, aX, aY, aZ, bP, bQ, bR)", "  do {"]
    for m in range(96):
        ax, bx = GROUPS[m // 16]
        i, j = (m % 16) // 4, m % 4
        w = "; ".join(t.get(m, [])) or "NOP_"
        l = f"    M1({ax}, {bx}, {i}, {j}, {w});"
        if m in NOTE: l += f"   /* {NOTE[m]} */"
        lines.append(l)
    lines.append("  } while (0)")
    return macro(lines)


if __name__ == "__main__":
    print(header("dw2_phase.py", "the slot table of emu_dw2_kernel's phase (one MFMA + the units pinned behind it)"))
    print(emit())
