"""Cost of the mel-spectrogram encoder input (rave_amd/csrc/mel.hip, rave_amd.mel.MelSpectrogram) on one MI355X, in one process:

(a) ``log_mel`` (one HIP launch: framing, window, FFT, power, mel sums, log1p, last frame dropped) at (32, 1, 65536) against the
    torch composition on the same device with the same buffers -- ``torch.stft`` (rocFFT), |.|^2, the (1025 x 128) matmul,
    ``log1p`` -- which is what torchaudio itself would launch; the two alternated, HIP events around every repetition;
(b) the replayed VAE-phase step at batch 32 x 65536 of ``build_v2(mel_input=True, gru_layers=2)`` next to ``build_v2(gru_layers=2)``
    (the parent's hybrid generator half on the PQMF encoder), in alternating windows.

    python tools/bench_mel.py [--reps 50] [--no-step] [--out FILE]      (the report is the "Time" part of profiles/mel.txt)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rave_amd import model as M
from rave_amd.mel import MelSpectrogram

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50, help="timed repetitions of each leg (alternated)")
ap.add_argument("--windows", type=int, default=5, help="timed windows of 10 steps per step leg (alternated)")
ap.add_argument("--no-step", action="store_true", help="skip (b), the training-step legs")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
B, N = 32, 65536
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


# ---- (a) the front-end alone
mel = MelSpectrogram(sample_rate=44100, n_fft=2048, win_length=2048, hop_length=256, normalized=True, n_mels=128).to(dev)
x = (0.1 * torch.randn(B, 1, N, generator=torch.Generator().manual_seed(1))).clamp(-1, 1).to(dev)
REPEAT = 10          # calls inside one event bracket (a single call is of the order of the event resolution)


def hip():
    for _ in range(REPEAT):
        mel.log_mel(x)


def composition():
    with torch.no_grad():
        for _ in range(REPEAT):
            torch.log1p(mel.compose(x)[..., :-1])


with torch.no_grad():
    ya, yb = mel.log_mel(x), torch.log1p(mel.compose(x)[..., :-1])
say(f"mel input, x {tuple(x.shape)} -> {tuple(ya.shape)}; HIP kernel vs the torch composition on the device: rel L2 "
    f"{float((ya - yb).norm() / yb.norm()):.2e}")
legs = [("HIP   rave_amd.MelSpectrogram.log_mel (1 launch)", hip), ("torch.stft + |.|^2 + matmul + log1p (rocFFT, ATen)", composition)]
for _, fn in legs:
    for _ in range(3):
        fn()
torch.cuda.synchronize()
ts = [[], []]
for _ in range(max(args.reps, 20)):
    for i, (_, fn) in enumerate(legs):
        ts[i].append(timed(fn) / REPEAT)
for (name, _), t in zip(legs, ts):
    med, lo, q1, q3, hi = stats(t)
    say(f"(a) {name}: {1e3 * med:.1f} us per call (median of {len(t)} alternated repetitions of {REPEAT} back-to-back calls; "
        f"quartiles {1e3 * q1:.1f} .. {1e3 * q3:.1f}, range {1e3 * lo:.1f} .. {1e3 * hi:.1f} us; HIP events around the host loop, "
        f"launch overhead included)")

# ---- (b) the replayed VAE-phase step with the mel encoder and with the PQMF encoder
if not args.no_step:
    steps = {}
    for mel_input in (False, True):
        torch.manual_seed(0)
        m = M.build_v2(gru_layers=2, mel_input=mel_input).to(dev).train()
        m.configure_optimizers(capturable=True)
        m.warmed_up = False
        st = M.GraphedTrainingStep(m, x)
        st(x, 0)
        steps[mel_input] = (m, st)
    torch.cuda.synchronize()
    count = [0]

    def window(mel_input, n=10):
        m, st = steps[mel_input]

        def run():
            for _ in range(n):
                i = count[0] = count[0] + 1
                st(x, i)
                m.on_train_batch_end(None, x, i)
        return timed(run) / n

    window(False, 3)
    window(True, 3)
    tw = {False: [], True: []}
    for _ in range(args.windows):
        for mel_input in (False, True):
            tw[mel_input].append(window(mel_input))
    for mel_input in (False, True):
        med, lo, _, _, hi = stats(tw[mel_input])
        say(f"(b) replayed v2 VAE-phase step, batch {B} x {N}, gru_layers=2, mel_input={mel_input}: {med:.3f} ms per step "
            f"(median of {len(tw[mel_input])} alternated windows of 10 steps, {lo:.3f} .. {hi:.3f} ms)")
    say(f"(b) mel encoder instead of the PQMF encoder: {stats(tw[True])[0] - stats(tw[False])[0]:+.3f} ms per step")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
