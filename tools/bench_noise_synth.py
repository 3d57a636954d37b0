"""Cost of the noise generators' tail -- everything behind the branch's last convolution: mod_sigmoid, amp_to_impulse_response,
fft_convolve, the two permutes (rave_amd/blocks.py) -- forward + backward on one MI355X, in one process: the HIP kernels of
rave_amd/csrc/noise_synth.hip against the torch composition (``RH_NOISE_SYNTH=0``: ATen + rocFFT) at the three shipped sizes,
batch 32 of 65 536 samples on 16 PQMF bands.  The modules themselves run, with their convolutions replaced by a pass-through (the
input IS the last convolution's output) and the U(-1, 1) draw injected (both paths draw it with the same three ATen launches);
the two legs alternate, HIP events around every repetition.  Then the GPU kernels each leg launches are counted under
torch.profiler, in a pass of its own.

    python tools/bench_noise_synth.py [--reps 30] [--out FILE]          (the report is the "Time" part of profiles/noise_synth.txt)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
from rave_amd import blocks

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each leg (alternated)")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
B, SAMPLES, BANDS = 32, 65536, 16
REPEAT = 10          # passes inside one event bracket (a single pass is of the order of the event resolution)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


class Pass(nn.Module):
    def forward(self, x, act=0, slope=0.2):
        return x


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
    return float((a.double() - b.double()).norm() / b.double().norm())


CONFIGS = [("v1.gin        NoiseGenerator   5 bands, ratios 4 4 4", lambda: blocks.NoiseGenerator(8, BANDS, (4, 4, 4), 5), 5, 64),
           ("v2_small.gin  NoiseGeneratorV2 32 bands, ratios 2 2 2", lambda: blocks.NoiseGeneratorV2(8, 64, BANDS, [2, 2, 2], 32), 32, 8),
           ("noise.gin     NoiseGeneratorV2 5 bands, ratios 2 2 2", lambda: blocks.NoiseGeneratorV2(8, 64, BANDS, [2, 2, 2], 5), 5, 8)]

say(f"noise generators' tail, forward + backward, batch {B} x {SAMPLES} samples on {BANDS} bands; per pass, median of {max(args.reps, 20)} "
    f"alternated repetitions of {REPEAT} back-to-back passes (quartiles; range), HIP events around the host loop, launch overhead included")
for name, make, nb, n in CONFIGS:
    m = make().to(dev)
    m.net = nn.Sequential(Pass())
    t = SAMPLES // BANDS // n
    gen = torch.Generator().manual_seed(nb * 100 + n)
    h = (3 * torch.randn(B, BANDS * nb, t, generator=gen)).to(dev).requires_grad_(True)
    noise = (torch.rand(B, t, BANDS, n, generator=gen) * 2 - 1).to(dev)
    gout = torch.randn(B, BANDS, t * n, generator=gen).to(dev)

    def one_pass():
        out = m(h, noise=noise)
        return out, torch.autograd.grad(out, h, gout)[0]

    def leg(switch):
        def run():
            os.environ["RH_NOISE_SYNTH"] = switch
            for _ in range(REPEAT):
                one_pass()
        return run

    legs = [("HIP kernels (rave_amd/csrc/noise_synth.hip)", leg("1")), ("torch composition (RH_NOISE_SYNTH=0)", leg("0"))]
    os.environ["RH_NOISE_SYNTH"] = "1"
    a = [v.detach().clone() for v in one_pass()]
    os.environ["RH_NOISE_SYNTH"] = "0"
    b = [v.detach().clone() for v in one_pass()]
    say(f"\n{name}: h {tuple(h.shape)}, noise {tuple(noise.shape)} -> {tuple(a[0].shape)}; kernels vs composition on the device: "
        f"out rel L2 {rel(a[0], b[0]):.2e}, gh rel L2 {rel(a[1], b[1]):.2e}")
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = [[], []]
    for _ in range(max(args.reps, 20)):
        for i, (_, fn) in enumerate(legs):
            ts[i].append(timed(fn) / REPEAT)
    from torch.profiler import ProfilerActivity, profile
    for (leg_name, fn), tl in zip(legs, ts):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        launches = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
        med, lo, q1, q3, hi = stats(tl)
        say(f"  {leg_name}: {1e3 * med:.1f} us per pass ({1e3 * q1:.1f} .. {1e3 * q3:.1f}; {1e3 * lo:.1f} .. {1e3 * hi:.1f}), "
            f"{launches / REPEAT:.1f} GPU kernels and copies per pass")
        if args.out:                                  # kept up to date: a later leg that fails leaves the earlier lines
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    say(f"  composition / kernels: {stats(ts[1])[0] / stats(ts[0])[0]:.2f} x")
os.environ.pop("RH_NOISE_SYNTH", None)
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
