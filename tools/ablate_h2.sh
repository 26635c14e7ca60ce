#!/bin/bash
# the f16x2 forward GEMM with its HBM round trips ablated (compile-time hooks of emu_h2_kernel, off in the product build; the source to recompile is gemm_emu_h2.hip:
# tools/build_variant.sh nostore gemm_emu_h2.hip -DH2_ABL_NOSTORE, likewise noloada / both): run from the
# repo root on the GPU box AFTER tools/build_variant.sh built ab/lib_{nostore,noloada,both}.so here (hipcc cross-compiles)
for v in "" nostore noloada both; do
  if [ -z "$v" ]; then python tools/mb_h2_ablate.py 2>/dev/null | tail -1; else HOISDF_LIB=$PWD/ab/lib_$v.so python tools/mb_h2_ablate.py 2>/dev/null | tail -1; fi
done
