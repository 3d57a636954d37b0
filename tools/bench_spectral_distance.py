"""Cost of the plain ``SpectralDistance`` on its HIP kernels (rave_amd/csrc/spec_dist.hip) behind ``losses.EncodecAudioDistance`` on
one MI355X, in one process: forward plus backward with respect to ``y`` of the whole distance over five scales (five launches +
one finalize forward, five launches backward, one autograd node) against the torch composition on the same device with the same
buffers -- ``unfold``, the window product, rocFFT, ``abs``, the ATen reductions of ``mean_difference`` and autograd through all of
it, which is what ``RH_SPEC_DIST=0`` runs.  Loss shapes: rows 32 and 64, T 65536, scales 2048 ... 128, L1 + L2, power 1,
normalised (rave_amd/configs/mi355x_encodec.gin).  The two legs alternate, HIP events around every repetition of REPEAT
back-to-back calls (launch overhead included).  Also prints the error of either leg's grad_y against float64 on one small input.

    python tools/bench_spectral_distance.py [--reps 30] [--out FILE]        (the report is profiles/spectral_distance.txt)
"""
import argparse
import os
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rave_amd.losses import EncodecAudioDistance, SpectralDistance

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each leg (alternated)")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
T, SCALES, REPEAT = 65536, [2048, 1024, 512, 256, 128], 3
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[len(ts) // 4], ts[(3 * len(ts)) // 4], ts[-1]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm())


def leg(m, switch, x, y):
    """forward + backward w.r.t. y of the spectral distance with RH_SPEC_DIST = switch (read per call)."""
    def once():
        os.environ["RH_SPEC_DIST"] = switch
        out = m(x, y)["spectral_distance"]
        return out, torch.autograd.grad(out, y)[0]
    return once


m = EncodecAudioDistance(SCALES, partial(SpectralDistance, sampling_rate=44100, norm=("L1", "L2"), power=1, normalized=True)).to(dev)
say(f"EncodecAudioDistance over the plain SpectralDistance, T {T}, scales {SCALES}, L1 + L2, power 1, normalised; times per forward + "
    f"backward (grad_y) of the spectral distance over all scales")

# accuracy of either leg against float64 on a small input
g = torch.Generator().manual_seed(3)
xs, ys = torch.randn(3, 1, 8192, generator=g), torch.randn(3, 1, 8192, generator=g)
m64 = EncodecAudioDistance(SCALES, partial(SpectralDistance, sampling_rate=44100, norm=("L1", "L2"), power=1, normalized=True)).double()
y64 = ys.double().requires_grad_(True)
d64 = m64(xs.double(), y64)["spectral_distance"]
(g64,) = torch.autograd.grad(d64, y64)
for name, switch in (("HIP kernels", "1"), ("torch composition, float32", "0")):
    out, gy = leg(m, switch, xs.to(dev), ys.to(dev).requires_grad_(True))()
    say(f"{name} ({type(out.grad_fn).__name__}) against the float64 composition (white noise, (3, 1, 8192)): value off by "
        f"{abs(float(out) - float(d64)) / float(d64):.2e}, grad_y rel L2 {rel(gy, g64):.2e}")

for rows in (32, 64):
    x = (0.1 * torch.randn(rows, 1, T, generator=torch.Generator().manual_seed(1))).clamp(-1, 1).to(dev)
    y = (0.1 * torch.randn(rows, 1, T, generator=torch.Generator().manual_seed(2))).clamp(-1, 1).to(dev).requires_grad_(True)
    legs = [("HIP   one node: 5 + 1 launches forward, 5 backward", leg(m, "1", x, y)),
            ("torch unfold + rocFFT + abs + ATen reductions + autograd", leg(m, "0", x, y))]
    assert "SpecDist" in type(legs[0][1]()[0].grad_fn).__name__ and "SpecDist" not in type(legs[1][1]()[0].grad_fn).__name__

    def run(fn):
        def go():
            for _ in range(REPEAT):
                fn()
        return go
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[], []]
    for _ in range(max(args.reps, 10)):
        for i, (_, fn) in enumerate(legs):
            ts[i].append(timed(run(fn)) / REPEAT)
    for (name, _), t in zip(legs, ts):
        med, lo, q1, q3, hi = stats(t)
        say(f"rows {rows}: {name}: {1e3 * med:.1f} us (median of {len(t)} alternated repetitions of {REPEAT} back-to-back calls; "
            f"quartiles {1e3 * q1:.1f} .. {1e3 * q3:.1f}, range {1e3 * lo:.1f} .. {1e3 * hi:.1f} us)")
    say(f"rows {rows}: HIP / composition = {stats(ts[0])[0] / stats(ts[1])[0]:.2f}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
