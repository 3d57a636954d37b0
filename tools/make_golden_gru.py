#!/usr/bin/env python
"""Writes tests/golden/gru_tiny.pt from the UNMODIFIED reference module rave.blocks.GRU (rave/blocks.py:295-319) on the CPU.

    python tools/make_golden_gru.py            # needs the reference tree (oracle/ref_import.py: RAVE_REFERENCE_ROOT)

Recorded data only: for (B, H, T, L) = (3, 48, 7, 2) under a fixed seed the module's state_dict, an input, the output, a
cotangent, dx and every parameter gradient; and the sorted state_dict keys and shapes of the module at (H, L) = (128, 2).
The input differs along every axis (a layout mix-up cannot pass).
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

SHAPE = (3, 48, 7, 2)        # B, H, T, L
SEED = 20


def main() -> None:
    from ref_import import import_reference
    rave = import_reference()
    from rave import blocks
    b, h, t, n_layers = SHAPE
    torch.manual_seed(SEED)
    m = blocks.GRU(h, n_layers)
    gen = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(b, h, t, generator=gen)
    dy = torch.randn(b, h, t, generator=gen)
    xr = x.clone().requires_grad_(True)
    y = m(xr)
    y.backward(dy)
    big = blocks.GRU(128, 2)
    out = dict(shape=SHAPE, seed=SEED,
               state_dict={k: v.detach().clone() for k, v in m.state_dict().items()},
               x=x, y=y.detach().clone(), dy=dy, dx=xr.grad.clone(),
               grads={k: p.grad.clone() for k, p in m.named_parameters()},
               keys_128_2=sorted((k, tuple(v.shape)) for k, v in big.state_dict().items()))
    path = os.path.join(ROOT, "tests", "golden", "gru_tiny.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
