"""Cost of the complex spectrogram in front of the spectral discriminators (rave_amd/csrc/spectrogram.hip, rave_amd.Spectrogram)
on one MI355X, in one process:

(a) per reference scale (n_fft 4096 .. 256, hop n_fft / 4), forward and forward + backward, the HIP kernels against the torch
    composition that runs without ``hip_frontend`` on the same device with the same buffers -- for the Encodec nets
    (64 x 1 x 65536, center=False, normalized: ``torch.stft`` + ``cat([real, imag], 1)`` and autograd through rocFFT) and for the
    descript MRD (32 x 2 x 65536, centred: the framing kernel + ``torch.fft.rfft`` + the permuted view); the two alternated, HIP
    events around every repetition;
(b) the replayed GAN-phase steps of ``build_discrete()`` at batch 32 x 65536 with and without ``hip_frontend``, in alternating
    windows of discriminator + generator step pairs.

    python tools/bench_spectrogram.py [--reps 30] [--no-step] [--out FILE]      (the report is the "Time" part of
                                                                                  profiles/spectrogram.txt)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rave_amd import descript_discriminator as DD, discriminator as D, model as M

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each leg (alternated)")
ap.add_argument("--windows", type=int, default=15, help="timed windows of 5 step pairs per step leg (alternated)")
ap.add_argument("--no-step", action="store_true", help="skip (b), the training-step legs")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
N = 65536
SCALES = [4096, 2048, 1024, 512, 256]
REPEAT = 5           # calls inside one event bracket
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


def median(ts):
    return sorted(ts)[len(ts) // 2]


def encodec_legs(n):
    spec = D.spectrogram(n).to(dev)

    def torch_front(xx):
        s = spec(xx)
        return torch.cat([s.real, s.imag], 1)
    return spec.real_imag, torch_front


def descript_legs(n):
    stft = DD._Stft(n, n // 4).to(dev)

    def hip(xx):
        s = stft.planes(xx)
        return s.reshape(s.shape[0], -1, s.shape[-2], s.shape[-1]).transpose(-1, -2)

    def torch_front(xx):
        s = torch.view_as_real(stft(xx))
        b, c, t, f, p = s.shape
        return s.permute(0, 1, 4, 2, 3).reshape(b, c * p, t, f)
    return hip, torch_front


def bench_front(tag, shape, legs_of):
    x = (0.1 * torch.randn(*shape, generator=torch.Generator().manual_seed(1))).clamp(-1, 1).to(dev)
    say(f"(a) {tag}: x {tuple(shape)}; us per call, median of {max(args.reps, 10)} alternated repetitions of {REPEAT} back-to-back calls "
        "(HIP events around the host loop, launch overhead included)")
    say(f"    {'n_fft':>6} {'frames':>7} | {'fwd HIP':>9} {'fwd torch':>10} {'ratio':>6} | {'fwd+bwd HIP':>12} {'fwd+bwd torch':>14} {'ratio':>6} | "
        f"{'out rel L2':>10} {'dx rel L2':>10}")
    for n in SCALES:
        hip, ref = legs_of(n)
        xg = x.clone().requires_grad_(True)
        a, b = hip(xg), ref(xg)
        g = torch.randn(a.shape, generator=torch.Generator().manual_seed(2)).to(dev)
        (da,), (db,) = torch.autograd.grad(a, xg, g), torch.autograd.grad(b, xg, g)
        e_out, e_dx = float((a - b).detach().norm() / b.detach().norm()), float((da - db).norm() / db.norm())
        frames = a.shape[-1] if tag.startswith("Encodec") else a.shape[-2]

        def fwd(f):
            def run():
                with torch.no_grad():
                    for _ in range(REPEAT):
                        f(x)
            return run

        def both(f):
            def run():
                for _ in range(REPEAT):
                    torch.autograd.grad(f(xg), xg, g)
            return run

        legs = [fwd(hip), fwd(ref), both(hip), both(ref)]
        for f in legs:
            f()
            f()
        torch.cuda.synchronize()
        ts = [[] for _ in legs]
        for _ in range(max(args.reps, 10)):
            for i, f in enumerate(legs):
                ts[i].append(1e3 * timed(f) / REPEAT)
        m = [median(t) for t in ts]
        say(f"    {n:>6} {frames:>7} | {m[0]:>9.1f} {m[1]:>10.1f} {m[1] / m[0]:>5.2f}x | {m[2]:>12.1f} {m[3]:>14.1f} {m[3] / m[2]:>5.2f}x | "
            f"{e_out:>10.2e} {e_dx:>10.2e}")
        del a, b, g, da, db, xg


bench_front("Encodec front end (rave/discriminator.py:12-20,147-152; center=False, normalized)", (64, 1, N), encodec_legs)
bench_front("descript MRD front end (rave/descript_discriminator.py:153-160; centred, reflect)", (32, 2, N), descript_legs)
say("    ratio = torch / HIP: above 1 the kernel is faster")

# ---- (b) the replayed GAN-phase steps of the discrete config, with and without the flag
if not args.no_step:
    B = 32
    g = torch.Generator().manual_seed(20250509)
    x = (0.1 * torch.randn(B, 1, N, generator=g)).clamp(-1, 1).to(dev)
    steps = {}
    for hip in (False, True):
        torch.manual_seed(0)
        m = M.build_discrete(hip_frontend=hip).to(dev).train()
        m.encoder.enabled.fill_(1)
        m.configure_optimizers(capturable=True)
        m.warmed_up = True
        pre = torch.cuda.Stream()
        pre.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(pre):          # one eager step of each kind on a side stream: every codebook initialised
            for i in range(2):
                m.training_step(x.detach().clone(), i, capture_safe=True)
                m.on_train_batch_end(None, None, i)
        torch.cuda.current_stream().wait_stream(pre)
        torch.cuda.synchronize()
        st = M.GraphedTrainingStep(m, x)
        st(x, 0)
        st(x, 1)
        torch.cuda.synchronize()
        steps[hip] = (m, st)
    count = [1]

    def window(hip, pairs=5):
        m, st = steps[hip]

        def run():
            for _ in range(2 * pairs):
                i = count[0] = count[0] + 1
                st(x, i)
                m.on_train_batch_end(None, x, i)
        return timed(run) / (2 * pairs)

    for hip in (False, True):
        count[0] = 1
        window(hip, 2)
    tw = {False: [], True: []}
    for _ in range(args.windows):
        for hip in (False, True):
            count[0] = 1
            tw[hip].append(window(hip))
    for hip in (False, True):
        t = sorted(tw[hip])
        say(f"(b) replayed discrete GAN-phase step (mean of a discriminator and a generator step), batch {B} x {N}, hip_frontend={hip}: "
            f"{median(t):.3f} ms per step (median of {len(t)} alternated windows of 5 step pairs, {t[0]:.3f} .. {t[-1]:.3f} ms)")
    say(f"(b) hip_frontend on instead of off: {median(tw[True]) - median(tw[False]):+.3f} ms per step")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
