#!/usr/bin/env python
"""Writes tests/golden/gan_loss_tiny.pt from the UNMODIFIED reference on the CPU: ``rave.core.hinge_gan``, ``ls_gan`` and
``nonsaturating_gan`` (rave/core.py:151-170) and their autograd gradients, in float32 and in float64.

    python tools/make_golden_gan_loss.py       # needs the reference tree (oracle/ref_import.py: RAVE_REFERENCE_ROOT)

Recorded data only (tensors, a few KB): per objective the scores of one head of 37 scores per half (tests/gan_loss_reference.py:
N(0, 2^2), the hinge gates at equality planted, +-12 planted for the non-saturating objective), the two losses, and the gradients
of GRAD_OUT[0] * loss_dis + GRAD_OUT[1] * loss_adv with respect to both halves.  No score reaches the clamp of the non-saturating
objective: the reference takes the clamp bounds in the dtype it runs in, so its float64 run saturates elsewhere than a float32 run
(tests/gan_loss_reference.py); the saturated regime is tested against the restatement instead.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 37
SEED = 50
GRAD_OUT = (1.0, 0.5)


def main() -> None:
    from ref_import import import_reference
    import gan_loss_reference as R
    import_reference()
    import rave.core as core
    fns = {"hinge": core.hinge_gan, "ls": core.ls_gan, "nonsaturating": core.nonsaturating_gan}
    out = {"grad_out": torch.tensor(GRAD_OUT, dtype=torch.float64)}
    for i, mode in enumerate(R.MODES):
        r64, f64 = R.scores(N, SEED + i, mode)
        if mode == "nonsaturating":                    # keep +-12, drop the saturated plants (see above)
            r64[N // 2], r64[N - 1], f64[N // 2], f64[N - 1] = 0.75, -2.5, -0.25, 3.5
        rec = {"real": r64.float().reshape(1, 1, N), "fake": f64.float().reshape(1, 1, N)}
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            r = rec["real"].to(dtype).clone().requires_grad_(True)
            f = rec["fake"].to(dtype).clone().requires_grad_(True)
            dis, adv = fns[mode](r, f)
            (GRAD_OUT[0] * dis + GRAD_OUT[1] * adv).backward()
            rec[tag] = {"loss_dis": dis.detach().clone(), "loss_adv": adv.detach().clone(), "d_real": r.grad.clone(),
                        "d_fake": f.grad.clone()}
        out[mode] = rec
    path = os.path.join(ROOT, "tests", "golden", "gan_loss_tiny.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
