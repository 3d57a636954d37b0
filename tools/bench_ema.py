"""Cost of the weight average (rave_amd/ema.py, `rave train --ema`) on one MI355X, two readings in one process:

(a) the update over the full v2 model (build_v2() defaults) through ``EMA.on_train_batch_end`` against the torch
    restatement of the reference loop (scripts/train.py:88-96: ``w * f + p * (1 - f)`` per tensor), the two alternated,
    HIP events around every repetition; ms and achieved GB/s against the 12 bytes per parameter the work needs;
(b) the replayed v2 VAE-phase step at batch 32 x 65536 followed by ``on_train_batch_end``, with and without the EMA
    object, in alternating windows; ms per step.

    python tools/bench_ema.py [--reps 30] [--out profiles/ema_update.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rave_amd import model as M
from rave_amd.ema import EMA

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each update leg (alternated)")
ap.add_argument("--windows", type=int, default=5, help="timed windows of 10 steps per step leg (alternated)")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
FACTOR = .999
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
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


torch.manual_seed(0)
m = M.build_v2().to(dev).train()
named = list(m.named_parameters())
n_par = sum(p.numel() for _, p in named)
say(f"v2 model: {len(named)} parameter tensors, {n_par / 1e6:.2f} M f32 parameters; factor {FACTOR}")

# ---- (a) the update alone
ema = EMA(FACTOR)
ema.on_train_batch_end(None, m, None, None, 0)            # clones
ref = {n: p.data.clone() for n, p in named}


def hip_update():
    ema.on_train_batch_end(None, m, None, None, 1)


def torch_update():
    for n, p in named:
        ref[n] = ref[n] * FACTOR + p.data * (1 - FACTOR)


for _ in range(3):
    hip_update()
    torch_update()
torch.cuda.synchronize()
t_hip, t_torch = [], []
for _ in range(max(args.reps, 20)):
    t_hip.append(timed(hip_update))
    t_torch.append(timed(torch_update))
same = all(torch.equal(ema.weights[n], ref[n]) for n, _ in named)
for name, ts in (("HIP   rh_ema_update_f32", t_hip), ("torch w * f + p * (1 - f) per tensor", t_torch)):
    ms, lo, hi = median(ts)
    say(f"(a) {name}: {ms:.3f} ms per update = {12 * n_par / ms / 1e6:.0f} GB/s of the 12 bytes per parameter "
        f"(median of {len(ts)} alternated repetitions, {lo:.3f} .. {hi:.3f} ms, HIP events around the host loop)")
say(f"(a) averages of both legs bit-identical after {len(t_hip) + 3} updates: {same}")
del ref

# ---- (b) the replayed VAE-phase step with and without the callback
B, T = 32, 65536
g = torch.Generator().manual_seed(1)
x = (0.1 * torch.randn(B, 1, T, generator=g)).clamp(-1, 1).to(dev)
m.configure_optimizers(capturable=True)
m.warmed_up = False
step = M.GraphedTrainingStep(m, x)
step(x, 0)
torch.cuda.synchronize()
ema = EMA(FACTOR)
count = [0]


def window(with_ema, n=10):
    def run():
        for _ in range(n):
            i = count[0] = count[0] + 1
            step(x, i)
            m.on_train_batch_end(None, x, i)
            if with_ema:
                ema.on_train_batch_end(None, m, None, x, i)
    return timed(run) / n


window(True, 3)
window(False, 3)
t_with, t_without = [], []
for _ in range(args.windows):
    t_without.append(window(False))
    t_with.append(window(True))
for name, ts in (("without EMA", t_without), ("with EMA   ", t_with)):
    ms, lo, hi = median(ts)
    say(f"(b) replayed v2 VAE-phase step, batch {B} x {T}, + on_train_batch_end, {name}: {ms:.3f} ms per step "
        f"(median of {len(ts)} alternated windows of 10 steps, {lo:.3f} .. {hi:.3f} ms)")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
