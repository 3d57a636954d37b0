#!/usr/bin/env python
"""Writes tests/golden/pqmf_bands.pt from the UNMODIFIED reference on the CPU: ``rave.pqmf.CachedPQMF(attenuation=100,
n_band=M)`` for M in {2, 4, 8, 32}, the band counts ``N_BAND`` of configs/v1.gin can be rebound to besides the shipped 16
(whose fixture is tests/golden/pqmf.pt, written by oracle/make_golden.py).

    python tools/make_golden_pqmf_bands.py      # needs the reference tree (oracle/ref_import.py: RAVE_REFERENCE_ROOT)

Recorded data only, one dict per M under ``out[M]``: the buffers ``h`` and ``hk``, the two conv weights ``w_fwd`` /
``w_inv``, a seeded input ``x`` (3, 1, 64 M), its analysis ``y`` and the synthesis ``x_rec`` of that, the cotangents
``cot_y`` / ``cot_x`` with the input gradients ``grad_x`` / ``grad_y`` they give, and the same four results under the causal
overlay (configs/causal.gin: pads (32 M, 0) and (32, 0)) as ``y_causal``, ``x_rec_causal``, ``grad_x_causal``,
``grad_y_causal``.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

BANDS = (2, 4, 8, 32)
SEED = 40


def t(x):
    return x.detach().clone().contiguous()


def run(pq, x, cy, cx):
    """analysis, synthesis of the analysis, and the two input gradients of one reference module."""
    xa = x.clone().requires_grad_(True)
    y = pq(xa)
    (y * cy).sum().backward()
    ya = y.detach().clone().requires_grad_(True)
    xr = pq.inverse(ya)
    (xr * cx).sum().backward()
    return t(y), t(xr), t(xa.grad), t(ya.grad)


def main() -> None:
    from ref_import import import_reference, set_causal
    rave = import_reference()
    from rave import pqmf
    import rave_oracle as O
    out = {}
    for m in BANDS:
        set_causal(False)
        pq = pqmf.CachedPQMF(attenuation=100, n_band=m)
        x = O.synthetic_batch(3, 1, 64 * m, seed=SEED + m)
        g = torch.Generator().manual_seed(SEED + 100 + m)
        cy = torch.randn(3, m, 64, generator=g)
        cx = torch.randn(3, 1, 64 * m, generator=g)
        y, xr, gx, gy = run(pq, x, cy, cx)
        assert y.shape == cy.shape and xr.shape == cx.shape
        d = dict(h=t(pq.h), hk=t(pq.hk), w_fwd=t(pq.forward_conv.weight), w_inv=t(pq.inverse_conv.weight), x=t(x), y=y,
                 x_rec=xr, cot_y=cy, cot_x=cx, grad_x=gx, grad_y=gy)
        set_causal(True)                             # the padding mode is read when the convolutions are built
        pc = pqmf.CachedPQMF(attenuation=100, n_band=m)
        set_causal(False)
        assert torch.equal(pc.forward_conv.weight, pq.forward_conv.weight)
        yc, xc, gxc, gyc = run(pc, x, cy, cx)
        d.update(y_causal=yc, x_rec_causal=xc, grad_x_causal=gxc, grad_y_causal=gyc)
        out[m] = d
        print(m, {k: tuple(v.shape) for k, v in d.items()})
    path = os.path.join(ROOT, "tests", "golden", "pqmf_bands.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
