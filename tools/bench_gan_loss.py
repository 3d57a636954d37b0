"""Cost of the GAN-objective tail of a GAN-phase step on one MI355X, in one process: rave_amd.ops.gan_losses (the HIP kernels of
rave_amd/csrc/gan_loss.hip, ONE call over all heads) against the float32 ATen composition (the per-head loop of
RAVE.training_step under ``RH_GAN_LOSS=0``: the objective, the two logged means and the four scalar accumulations per head) on
the score maps of the benchmarked v2 discriminator (5 period + 3 scale heads, batch 32 x 65 536 samples), for the three
objectives, forward alone and forward + backward.  Two timings per leg: the eager host loop (launch overhead included, HIP
events around 10 back-to-back passes, legs alternated) and the same pass recorded into a hipGraph and replayed (what a recorded
training step pays).  GPU kernels per pass are counted under torch.profiler in a pass of their own.

    python tools/bench_gan_loss.py [--reps 30] [--out FILE]        (the "Time" part of profiles/gan_loss.txt)
    python tools/bench_gan_loss.py --replay N [--root DIR]          records the two GAN-phase step kinds of the v2 model at the
                                                                    benchmarked size (GraphedTrainingStep) and replays each N
                                                                    times, with the package imported from DIR (another checkout):
                                                                    run under a kernel trace at two values of N, the difference
                                                                    of the dispatch totals is the count of the replayed steps
"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30, help="timed repetitions of each leg (alternated)")
ap.add_argument("--out", default=None, help="also write the report to this file")
ap.add_argument("--replay", type=int, default=0)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

import torch  # noqa: E402
from rave_amd import model as M  # noqa: E402

dev = torch.device("cuda:0")
B, SAMPLES = 32, 65536
REPEAT = 10
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def kernels_of(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)


if args.replay:
    torch.manual_seed(0)
    m = M.build_v2().to(dev).train()
    m.configure_optimizers(capturable=True)
    m.warmed_up = True
    x = (0.1 * torch.randn(B, 1, SAMPLES)).clamp(-1, 1).to(dev)
    step = M.GraphedTrainingStep(m, x)
    every = m.update_discriminator_every
    for i in range(args.replay):
        for idx in (every * (i + 1), every * (i + 1) + 1):        # one discriminator step, one generator step
            step(x, idx)
            m.on_train_batch_end(None, None, idx)
    torch.cuda.synchronize()
    print(f"replayed {args.replay} recorded discriminator steps and {args.replay} recorded generator steps", flush=True)
    sys.exit(0)

from rave_amd import losses, ops  # noqa: E402


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


torch.manual_seed(0)
model = M.build_v2().to(dev).train()
with torch.no_grad():
    ops.range_reset(dev)
    model.prepare_weights(with_discriminator=True)
    feats = model.discriminator((0.1 * torch.randn(2 * B, 1, SAMPLES)).clamp(-1, 1).to(dev))
    model.release_weights()
heads = [(3.0 * s[-1].detach() / s[-1].detach().std()).requires_grad_(True) for s in feats]       # scores of a few units, as trained
del model, feats
say(f"GAN objectives over the {len(heads)} heads of build_v2()'s discriminator, batch {B} x {SAMPLES}: score maps "
    + ", ".join(f"{tuple(h.shape)}{'' if h.is_contiguous() else ' permuted'}" for h in heads)
    + f"; per pass, median of {max(args.reps, 20)} alternated repetitions of {REPEAT} back-to-back passes (quartiles; range)")
cot = torch.ones((), device=dev)


def composition(fn):
    os.environ["RH_GAN_LOSS"] = "0"
    dis = adv = pr = pf = 0
    for h in heads:
        r, f = torch.split(h, h.shape[0] // 2, 0)
        d, a = fn(r, f)
        pr = pr + r.detach().mean()
        pf = pf + f.detach().mean()
        dis = dis + d
        adv = adv + a
    return dis, adv, pr, pf


for name, fn in losses.GAN_LOSSES.items():
    def fused():
        os.environ["RH_GAN_LOSS"] = "1"
        return ops.gan_losses(heads, name)

    legs = {"HIP kernels, one call": fused, "ATen composition, per head": lambda: composition(fn)}
    a = [v.detach().clone() for v in fused()]
    b = [v.detach().clone() for v in composition(fn)]
    ga = torch.autograd.grad(fused()[0], heads, cot)
    gb = torch.autograd.grad(composition(fn)[0], heads, cot)
    # (a head whose scores are all saturated has a zero gradient on both paths: the absolute difference stands in there)
    gerr = max(float((x.double() - y.double()).norm() / (y.double().norm() if float(y.double().norm()) > 0 else 1.0)) for x, y in zip(ga, gb))
    say(f"\n{name}: kernels vs composition on the device: " + ", ".join(f"{k} {float(x):.6f} / {float(y):.6f}" for k, x, y in
        zip(("loss_dis", "loss_adv", "pred_real", "pred_fake"), a, b)) + f"; d loss_dis / d scores rel L2 {gerr:.2e} (worst head)")
    for way in ("forward", "forward + backward (d loss_dis)"):
        def one(leg):
            out = leg()
            if way != "forward":
                torch.autograd.grad(out[0], heads, cot)

        runs = {k: (lambda leg=leg: [one(leg) for _ in range(REPEAT)]) for k, leg in legs.items()}
        graphs = {}
        for k, leg in legs.items():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    one(leg)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                one(leg)
            graphs[k] = g
        replays = {k: (lambda g=g: [g.replay() for _ in range(REPEAT)]) for k, g in graphs.items()}
        for fnr in list(runs.values()) + list(replays.values()):
            fnr()
        torch.cuda.synchronize()
        te, tg = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(max(args.reps, 20)):
            for k in legs:
                te[k].append(timed(runs[k]) / REPEAT)
            for k in legs:
                tg[k].append(timed(replays[k]) / REPEAT)
        say(f"  {way}")
        for k in legs:
            n = kernels_of(runs[k]) / REPEAT
            me, _, q1, q3, _ = stats(te[k])
            mg, _, g1, g3, _ = stats(tg[k])
            say(f"    {k}: eager {1e3 * me:.1f} us per pass ({1e3 * q1:.1f} .. {1e3 * q3:.1f}), replayed graph {1e3 * mg:.1f} us "
                f"({1e3 * g1:.1f} .. {1e3 * g3:.1f}), {n:.1f} GPU kernels and copies per pass")
        ks = list(legs)
        say(f"    composition / kernels: eager {stats(te[ks[1]])[0] / stats(te[ks[0]])[0]:.2f} x, replayed "
            f"{stats(tg[ks[1]])[0] / stats(tg[ks[0]])[0]:.2f} x")
        del graphs, replays
os.environ.pop("RH_GAN_LOSS", None)
