"""Cost of the recurrent latent layer (rave_amd/csrc/gru.hip, blocks.GRU) on one MI355X, in one process:

(a) forward (under no_grad) and forward + backward of ``rave_amd.blocks.GRU`` at B = 32, H = 128, T = 32, L = 2 (T = 32 is
    what 65536 samples become at the v2 latent rate) against ``torch.nn.GRU`` (MIOpen) between the reference's two permutes
    on the same device with the same weights, the two alternated, HIP events around every repetition;
(b) the replayed v2 VAE-phase step at batch 32 x 65536 with ``gru_layers=2`` and without, in alternating windows.

    python tools/bench_gru.py [--reps 50] [--no-step] [--out FILE]      (the report is the "Time" part of profiles/gru.txt)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rave_amd import blocks
from rave_amd import model as M

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50, help="timed repetitions of each leg (alternated)")
ap.add_argument("--windows", type=int, default=5, help="timed windows of 10 steps per step leg (alternated)")
ap.add_argument("--no-step", action="store_true", help="skip (b), the training-step legs")
ap.add_argument("--out", default=None, help="also write the report to this file")
args = ap.parse_args()

dev = torch.device("cuda:0")
B, H, T, NL = 32, 128, 32, 2
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


# ---- (a) the layer alone
torch.manual_seed(0)
ours = blocks.GRU(H, NL).to(dev)
stock = torch.nn.GRU(input_size=H, hidden_size=H, num_layers=NL, batch_first=True).to(dev)
stock.load_state_dict({k[len("gru."):]: v for k, v in ours.state_dict().items() if k.startswith("gru.")})
gen = torch.Generator().manual_seed(1)
x = torch.randn(B, H, T, generator=gen).to(dev)
dy = torch.randn(B, H, T, generator=gen).to(dev)
REPEAT = 10          # calls inside one event bracket (a single call is of the order of the event resolution)


def fwd_of(mod, is_stock):
    def run():
        with torch.no_grad():
            for _ in range(REPEAT):
                if is_stock:
                    mod(x.permute(0, 2, 1))[0].permute(0, 2, 1)
                else:
                    mod(x)
    return run


def fwd_bwd_of(mod, is_stock):
    xg = x.clone().requires_grad_(True)

    def run():
        for _ in range(REPEAT):
            y = mod(xg.permute(0, 2, 1))[0].permute(0, 2, 1) if is_stock else mod(xg)
            torch.autograd.backward(y, dy, inputs=[xg] + list(mod.parameters()))
            xg.grad = None
            for p in mod.parameters():
                p.grad = None
    return run


with torch.no_grad():
    ya, yb = ours(x), stock(x.permute(0, 2, 1))[0].permute(0, 2, 1)
say(f"GRU B {B} x H {H} x T {T}, {NL} layers; HIP output vs torch.nn.GRU on the device: rel L2 "
    f"{float((ya - yb).norm() / yb.norm()):.2e}")
for what, make in (("forward (no_grad)", fwd_of), ("forward + backward", fwd_bwd_of)):
    legs = [("HIP   rave_amd.blocks.GRU", make(ours, False)), ("torch.nn.GRU (MIOpen) + permutes", make(stock, True))]
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
        say(f"(a) {what}, {name}: {1e3 * med:.1f} us per call (median of {len(t)} alternated repetitions of {REPEAT} "
            f"back-to-back calls; quartiles {1e3 * q1:.1f} .. {1e3 * q3:.1f}, range {1e3 * lo:.1f} .. {1e3 * hi:.1f} us; HIP "
            f"events around the host loop, launch overhead included)")

# ---- (b) the replayed VAE-phase step with and without the layer
if not args.no_step:
    N = 65536
    g = torch.Generator().manual_seed(1)
    xs = (0.1 * torch.randn(B, 1, N, generator=g)).clamp(-1, 1).to(dev)
    steps = {}
    for layers in (0, 2):
        torch.manual_seed(0)
        m = M.build_v2(gru_layers=layers).to(dev).train()
        m.configure_optimizers(capturable=True)
        m.warmed_up = False
        st = M.GraphedTrainingStep(m, xs)
        st(xs, 0)
        steps[layers] = (m, st)
    torch.cuda.synchronize()
    count = [0]

    def window(layers, n=10):
        m, st = steps[layers]

        def run():
            for _ in range(n):
                i = count[0] = count[0] + 1
                st(xs, i)
                m.on_train_batch_end(None, xs, i)
        return timed(run) / n

    window(0, 3)
    window(2, 3)
    tw = {0: [], 2: []}
    for _ in range(args.windows):
        for layers in (0, 2):
            tw[layers].append(window(layers))
    for layers in (0, 2):
        med, lo, _, _, hi = stats(tw[layers])
        say(f"(b) replayed v2 VAE-phase step, batch {B} x {N}, gru_layers={layers}: {med:.3f} ms per step "
            f"(median of {len(tw[layers])} alternated windows of 10 steps, {lo:.3f} .. {hi:.3f} ms)")
    say(f"(b) added by the two-layer GRU: {stats(tw[2])[0] - stats(tw[0])[0]:+.3f} ms per step")
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
