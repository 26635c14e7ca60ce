#!/usr/bin/env python3
"""add + LayerNorm forward + backward at the encoder's shape (65536 x 256, dropout 0.1):  python tools/mb_ln.py
(variants of the kernels: tools/build_variant.sh + HOISDF_LIB)"""
import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def main():
    import time, torch
    from hoisdf_amd import ops as O
    M, D = 65536, 256
    x = torch.randn(M, D, device="cuda", requires_grad=True)
    r = torch.randn(M, D, device="cuda", requires_grad=True)
    g = torch.ones(D, device="cuda", requires_grad=True)
    b = torch.zeros(D, device="cuda", requires_grad=True)
    gy = torch.randn(M, D, device="cuda")

    def run():
        O.add_layernorm(x, r, g, b, 1e-5, 0.1).backward(gy)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        run()
    torch.cuda.synchronize()
    print("RESULT %.1f us per fwd+bwd" % ((time.perf_counter() - t0) / 50 * 1e6))


if __name__ == "__main__":
    main()
