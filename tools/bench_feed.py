"""Throughput of the GPU data feed (rave_amd/data.py): batches of 32 x 65536 from 64 resident items.
``--rand-pitch lo,hi`` adds a leg with RandomPitch on (about half the items resampled), ``--post`` a leg with ``normalize``
and ``derivative`` on (the launches of rh_feed_batch_post_i16_f32: the chain kernel plus the gain / difference kernel), ``--freq_mask P`` two
legs with FrequencyMasking on (rh_feed_freq_mask_f32 behind the chain: every item masked, and a share P of them),
``--resample ORIG,NEW`` a leg with Resample(ORIG, NEW) behind Dequantize (rh_feed_batch_resample_i16_f32: the chain kernel plus the
resampling kernel; with ``--post`` a second one with ``normalize`` and ``derivative`` behind it, three launches), ``--step`` the
replayed v2 training step (bench.py's default workload) the feed has to hide under on a side stream -- all timed in the same
process, with HIP events, in alternating windows.  The "feed" leg is the chain launch alone."""
import argparse
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rave_amd import data as D

ap = argparse.ArgumentParser()
ap.add_argument("--rand-pitch", default=None, help="lo,hi: also time the feed with RandomPitch in this range")
ap.add_argument("--p-pitch", type=float, default=.5, help="share of the items that are resampled (reference: 0.5)")
ap.add_argument("--post", action="store_true", help="also time the feed with normalize=True, derivative=True")
ap.add_argument("--freq_mask", type=float, default=None, metavar="P",
                help="also time the feed with FrequencyMasking: all items masked, and with probability P")
ap.add_argument("--resample", default=None, metavar="ORIG,NEW",
                help="also time the feed of a dataset stored at ORIG Hz resampled to NEW Hz (with --post: also with both steps)")
ap.add_argument("--step", action="store_true", help="also time the replayed v2 training step at batch 32 x 65536")
ap.add_argument("--reps", type=int, default=3, help="timed windows per leg, alternating between the legs")
args = ap.parse_args()

dev = torch.device("cuda:0")
pcm = torch.randint(-20000, 20000, (64, 1, 4 * 65536), dtype=torch.int16, device=dev)
legs = [("feed", D.GpuBatchFeed(pcm, seed=0))]
if args.rand_pitch:
    lo, hi = map(float, args.rand_pitch.split(","))
    legs.append((f"feed --rand-pitch {lo:g},{hi:g} (p = {args.p_pitch:g})", D.GpuBatchFeed(pcm, seed=0, rand_pitch=(lo, hi), p_pitch=args.p_pitch)))
if args.post:
    legs.append(("feed normalize + derivative", D.GpuBatchFeed(pcm, seed=0, normalize=True, derivative=True)))
if args.freq_mask is not None:
    legs.append(("feed + freq_mask, all rows masked", D.GpuBatchFeed(pcm, seed=0, freq_mask=1.)))
    legs.append((f"feed + freq_mask (p = {args.freq_mask:g})", D.GpuBatchFeed(pcm, seed=0, freq_mask=args.freq_mask)))
if args.resample:
    orig, new = map(int, args.resample.split(","))
    legs.append((f"feed + resample {orig} -> {new}", D.GpuBatchFeed(pcm, sr=orig, seed=0, resample_to=new)))
    if args.post:
        legs.append((f"feed + resample {orig} -> {new}, normalize + derivative",
                     D.GpuBatchFeed(pcm, sr=orig, seed=0, resample_to=new, normalize=True, derivative=True)))


class Step:
    """The v2 step as bench.py runs it: one captured graph, replayed."""

    def __init__(self):
        from rave_amd import model as M
        torch.manual_seed(0)
        self.m = M.build_v2().to(dev).train()
        self.m.configure_optimizers(capturable=True)
        self.m.warmed_up = False
        self.x = (0.1 * torch.randn(32, 1, 65536)).clamp(-1, 1).to(dev)
        self.graphed = M.GraphedTrainingStep(self.m, self.x)
        self.i = 0

    def sample(self, batch, n_signal):
        self.graphed(self.x, self.i)
        self.m.on_train_batch_end(None, None, self.i)
        self.i += 1


if args.step:
    legs.append(("v2 training step (graph replay)", Step()))


def window(feed, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        feed.sample(32, 65536)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


for _, feed in legs:
    for _ in range(3):
        feed.sample(32, 65536)
torch.cuda.synchronize()
times = {name: [] for name, _ in legs}
for _ in range(args.reps):
    for name, feed in legs:
        times[name].append(window(feed))
for name, _ in legs:
    t = sorted(times[name])
    ms = t[len(t) // 2]
    if name.startswith("feed"):
        print(f"{name}: {ms:.3f} ms per batch of 32 x 65536 = {32 * 65536 / ms / 1e3:.1f} M samples/s (noise draw included; "
              f"median of {len(t)} windows of 10 batches, {t[0]:.3f} .. {t[-1]:.3f} ms)")
    else:
        print(f"{name}: {ms:.3f} ms per step of 32 x 65536 (median of {len(t)} windows of 10 steps, {t[0]:.3f} .. {t[-1]:.3f} ms)")
