"""Cost of the differentiable mel spectrogram (rave_amd/csrc/mel.hip: rh_mel_diff_fwd_f32 / rh_mel_diff_bwd_f32) behind
``losses.SpectralDistance(mel=n)`` on one MI355X, in one process: forward plus backward of ``DifferentiableMelSpectrogram`` (two
HIP launches) against the torch composition on the same device with the same buffers -- ``torch.stft`` (rocFFT), ``|.|^power``,
the filterbank matmul, and autograd through all of it -- which is what torchaudio itself would launch.  Loss shapes: rows 32 and
64, T 65536, n_fft 512 / 1024 / 2048 with hop n_fft / 4, 64 mels, power 1, normalised, uncentred.  The two legs alternate, HIP
events around every repetition of REPEAT back-to-back calls (launch overhead included).  Also prints the error of either leg
against float64 on one small input per size (the figures the power-1 bound of tests/test_gpu_mel_distance.py would fall back on).

    python tools/bench_mel_distance.py [--reps 30] [--out FILE]        (the report is profiles/mel_distance.txt)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rave_amd import ops
from rave_amd.mel import DifferentiableMelSpectrogram

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each leg (alternated)")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
T, N_MELS, POWER, REPEAT = 65536, 64, 1, 5
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


def legs_of(mel, x, g):
    def compose(xx):
        return ops.mel_diff_compose(xx, mel.spectrogram.window, mel.mel_scale.fb, mel.n_fft, mel.hop_length, mel._host_scale(), mel.power,
                                    mel.center)

    def run(f):
        def go():
            for _ in range(REPEAT):
                torch.autograd.grad(f(x), x, g)
        return go
    return compose, [("HIP   DifferentiableMelSpectrogram forward + backward (2 launches)", run(mel)),
                     ("torch.stft + |.| + matmul + autograd (rocFFT, ATen)", run(compose))]


say(f"differentiable mel spectrogram, T {T}, {N_MELS} mels, power {POWER}, normalised, uncentred, hop n_fft / 4; times per forward + "
    f"backward of ONE signal (a loss runs two per scale)")
for n_fft in (512, 1024, 2048):
    mel = DifferentiableMelSpectrogram(44100, n_fft, hop_length=n_fft // 4, n_mels=N_MELS, power=POWER, normalized=True, center=False).to(dev)
    # accuracy of either leg against float64 on a small input
    xs = torch.randn(3, 3 * n_fft + 5, generator=torch.Generator().manual_seed(n_fft), dtype=torch.float64)
    m64 = DifferentiableMelSpectrogram(44100, n_fft, hop_length=n_fft // 4, n_mels=N_MELS, power=POWER, normalized=True, center=False).double()
    x64 = xs.clone().requires_grad_(True)
    y64 = m64(x64)
    gs = torch.randn(y64.shape, generator=torch.Generator().manual_seed(n_fft + 1), dtype=torch.float64)
    (d64,) = torch.autograd.grad(y64, x64, gs)
    x32 = xs.float().to(dev).requires_grad_(True)
    compose, _ = legs_of(mel, x32, gs.float().to(dev))
    for name, f in (("HIP kernels", mel), ("torch composition, float32", compose)):
        y = f(x32)
        (d,) = torch.autograd.grad(y, x32, gs.float().to(dev))
        say(f"n_fft {n_fft}: {name} against the float64 composition (white noise, (3, {3 * n_fft + 5})): forward rel L2 {rel(y, y64):.2e}, "
            f"backward {rel(d, d64):.2e}")
    for rows in (32, 64):
        x = (0.1 * torch.randn(rows, 1, T, generator=torch.Generator().manual_seed(1))).clamp(-1, 1).to(dev).requires_grad_(True)
        with torch.no_grad():
            g = torch.randn_like(mel(x))
        _, legs = legs_of(mel, x, g)
        for _, fn in legs:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ts = [[], []]
        for _ in range(max(args.reps, 10)):
            for i, (_, fn) in enumerate(legs):
                ts[i].append(timed(fn) / REPEAT)
        for (name, _), t in zip(legs, ts):
            med, lo, q1, q3, hi = stats(t)
            say(f"n_fft {n_fft} rows {rows}: {name}: {1e3 * med:.1f} us (median of {len(t)} alternated repetitions of {REPEAT} "
                f"back-to-back calls; quartiles {1e3 * q1:.1f} .. {1e3 * q3:.1f}, range {1e3 * lo:.1f} .. {1e3 * hi:.1f} us)")
        say(f"n_fft {n_fft} rows {rows}: HIP / composition = {stats(ts[0])[0] / stats(ts[1])[0]:.2f}")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
