"""Cost of the instantaneous-frequency (phase) distance, forward + backward, on one MI355X in one process:
rave_amd.losses.WeightedInstantaneousSpectralDistance on the HIP kernels of rave_amd/csrc/inst_freq_loss.hip against the torch
composition (``RH_INST_FREQ=0``: rocFFT + ATen + autograd) on the same device, at the training shape -- batch 32 of 65 536 samples,
the five scales of rave_amd/configs/mi355x_phase.gin, normalized -- for both ``weighted`` values.  The two legs alternate, HIP
events around every repetition; medians after warm-up.  Then the GPU kernels each leg launches are counted under
torch.profiler, in a pass of its own.

    python tools/bench_inst_freq.py [--reps 20] [--out FILE]          (the report is the "Time" part of profiles/inst_freq_distance.txt)
"""
import argparse
import os
import sys
from functools import partial

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rave_amd import losses

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20, help="timed repetitions of each leg (alternated)")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
B, SAMPLES, SCALES = 32, 65536, [2048, 1024, 512, 256, 128]
REPEAT = 3           # passes inside one event bracket
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:                                      # kept up to date: a later leg that fails leaves the earlier lines
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


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


gen = torch.Generator().manual_seed(0)
x = (0.3 * torch.randn(B, 1, SAMPLES, generator=gen)).to(dev).requires_grad_(True)
y = (0.5 * x.detach().cpu() + 0.2 * torch.randn(B, 1, SAMPLES, generator=gen)).to(dev).requires_grad_(True)
say(f"WeightedInstantaneousSpectralDistance, forward + backward (gradients of spectral_distance + phase_distance w.r.t. both "
    f"signals), batch {B} x {SAMPLES}, scales {SCALES}, normalized; per pass, median of {args.reps} alternated repetitions of "
    f"{REPEAT} back-to-back passes (quartiles; range), HIP events around the host loop, launch overhead included")
for weighted in (False, True):
    dist = losses.WeightedInstantaneousSpectralDistance(
        partial(losses.MultiScaleSTFT, scales=SCALES, sample_rate=44100, magnitude=False, normalized=True), weighted=weighted).to(dev)

    def one_pass():
        out = dist(x, y)
        return (out["spectral_distance"], out["phase_distance"]) + torch.autograd.grad(out["spectral_distance"] + out["phase_distance"], (x, y))

    def leg(switch):
        def run():
            os.environ["RH_INST_FREQ"] = switch
            for _ in range(REPEAT):
                one_pass()
        return run

    legs = [("HIP kernels (rave_amd/csrc/inst_freq_loss.hip)", leg("1")), ("torch composition (RH_INST_FREQ=0)", leg("0"))]
    os.environ["RH_INST_FREQ"] = "1"
    a = [v.detach().clone() for v in one_pass()]
    os.environ["RH_INST_FREQ"] = "0"
    b = [v.detach().clone() for v in one_pass()]
    say(f"\nweighted = {weighted}: kernels vs composition on the device: spectral_distance {float(a[0]):.6f} / {float(b[0]):.6f}, "
        f"phase_distance {float(a[1]):.6f} / {float(b[1]):.6f}, dx rel L2 {rel(a[2], b[2]):.2e}, dy rel L2 {rel(a[3], b[3]):.2e}")
    for _, fn in legs:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ts = [[], []]
    for _ in range(args.reps):
        for i, (_, fn) in enumerate(legs):
            ts[i].append(timed(fn) / REPEAT)
    from torch.profiler import ProfilerActivity, profile
    for (leg_name, fn), tl in zip(legs, ts):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA]
        med, lo, q1, q3, hi = stats(tl)
        say(f"  {leg_name}: {med:.3f} ms per pass ({q1:.3f} .. {q3:.3f}; {lo:.3f} .. {hi:.3f}), "
            f"{sum(e.count for e in evs) / REPEAT:.1f} GPU kernels and copies per pass")
        if leg_name.startswith("HIP"):
            dt = lambda e: getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
            for e in sorted(evs, key=lambda e: -dt(e))[:12]:
                say(f"      {dt(e) / e.count:9.1f} us x {e.count / REPEAT:4.1f}  {e.key[:110]}")
    say(f"  composition / kernels: {stats(ts[1])[0] / stats(ts[0])[0]:.2f} x")
os.environ.pop("RH_INST_FREQ", None)
