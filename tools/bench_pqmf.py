"""PQMF kernels at the BASELINE size (32 x 65536): direct-form MFMA kernels, folded form generation 1 (pqmf_fold.hip)
and generation 2 (pqmf_fold2.hip); module-level timings (autograd call, eager) and kernel-level ones (the C ABI called
back to back: launch-to-launch time of the kernel alone, warm waveform), against the 8 B/sample HBM roofline.

    python tools/bench_pqmf.py                      # the 16-band forms, as above
    python tools/bench_pqmf.py --bands 2,4,8,32     # the other band counts (pqmf_bands.hip) next to the 16-band direct form

``--bands``: the four C entry points per band count, called back to back at 32 x 65536 between HIP events, in the same
process as the 16-band direct form (the MFMA kernels of pqmf.hip, what RH_PQMF_FOLD=0 runs) and alternating with it over
several rounds; microseconds (median of the rounds, with their spread) and achieved GB/s at the 8 B/sample all of them
move.  The output is committed as profiles/pqmf_bands.txt."""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from rave_amd import pqmf, _lib as L
ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--bands", default=None, help="comma-separated band counts to time against the 16-band direct form")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=200, help="back-to-back launches per timed window")
args = ap.parse_args()
dev = torch.device("cuda:0")
ROWS, T = 32, 65536


def bench_bands(bands):
    """Kernel level, every transform of every band count: {M: {transform: [us per round]}}."""
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn(ROWS, 1, T, device=dev)
    calls = {}
    for M in bands:
        q = pqmf.CachedPQMF(100, M).to(dev)
        wf, wi = q.forward_conv.weight, q.inverse_conv.weight
        kf, ki = wf.shape[-1], wi.shape[-1]
        pf, pi = q.forward_conv._pad[0], q.inverse_conv._pad[0]
        n = T // M
        y = torch.randn(ROWS, M, n, device=dev)
        yo, xo = torch.empty_like(y), torch.empty_like(x)
        keep = (q, y, yo, xo)                     # the lambdas hold raw pointers
        calls[M] = (keep, {
            "analysis": lambda wf=wf, kf=kf, pf=pf, n=n, M=M, yo=yo: L.check(L.lib.rh_pqmf_analysis_fwd_f32(
                x.data_ptr(), wf.data_ptr(), ROWS, T, M, kf, pf, n, yo.data_ptr(), st)),
            "analysis-bwd": lambda wf=wf, kf=kf, pf=pf, n=n, M=M, y=y, xo=xo: L.check(L.lib.rh_pqmf_analysis_bwd_f32(
                y.data_ptr(), wf.data_ptr(), ROWS, T, M, kf, pf, n, xo.data_ptr(), st)),
            "synthesis": lambda wi=wi, ki=ki, pi=pi, n=n, M=M, y=y, xo=xo: L.check(L.lib.rh_pqmf_synthesis_fwd_f32(
                y.data_ptr(), wi.data_ptr(), ROWS, n, M, ki, pi, n, xo.data_ptr(), st)),
            "synthesis-bwd": lambda wi=wi, ki=ki, pi=pi, n=n, M=M, yo=yo: L.check(L.lib.rh_pqmf_synthesis_bwd_f32(
                x.data_ptr(), wi.data_ptr(), ROWS, n, M, ki, pi, n, yo.data_ptr(), st)),
        })
    out = {M: {k: [] for k in calls[M][1]} for M in bands}
    for _ in range(args.rounds):                  # the band counts alternate inside a round
        for M in bands:
            for name, f in calls[M][1].items():
                out[M][name].append(t(f, args.iters))
    return out


def report_bands(bands):
    res = bench_bands(sorted(set(bands) | {16}))
    mb = 2 * ROWS * T * 4 / 1e6                   # algorithmic bytes: 8 B / sample, every band count
    med = lambda v: sorted(v)[len(v) // 2]
    print("PQMF direct-form kernels at %d x %d, C entry points back to back (%d launches per window, median of %d rounds "
          "[min .. max]); GB/s = 8 B/sample / time; 'vs 16' = bytes/s relative to the 16-band direct form (pqmf.hip, the "
          "kernels RH_PQMF_FOLD=0 runs) of the same process" % (ROWS, T, args.iters, args.rounds))
    print("device: %s" % torch.cuda.get_device_name(0))
    for M in sorted(res):
        for name, v in res[M].items():
            us, ref = med(v), med(res[16][name])
            print("M=%-2d %-14s %8.1f us [%7.1f .. %7.1f]  %8.1f GB/s  vs 16: %5.2f x   (%d MAC/sample)"
                  % (M, name, us, min(v), max(v), mb / us * 1e3, ref / us, 33 * M))


m = pqmf.CachedPQMF(100, 16).to(dev)
x = torch.randn(32, 1, 65536, device=dev)


def t(f, n=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


if args.bands:
    report_bands([int(b) for b in args.bands.split(",")])
    sys.exit(0)

mb = 2 * 32 * 65536 * 4 / 1e6                     # algorithmic bytes: 8 B / sample
for fold, v2 in (("1", "1"), ("1", "0"), ("0", "0")):
    os.environ["RH_PQMF_FOLD"] = fold
    os.environ["RH_PQMF_V2"] = v2
    xa = x.clone().requires_grad_(True)
    y = m(xa); cy = torch.randn_like(y)
    ya = y.detach().clone().requires_grad_(True)
    xr = m.inverse(ya); cx = torch.randn_like(xr)
    with torch.no_grad():
        a = t(lambda: m(x)); s = t(lambda: m.inverse(y))
    ab = t(lambda: torch.autograd.grad(y, xa, cy, retain_graph=True))
    sb = t(lambda: torch.autograd.grad(xr, ya, cx, retain_graph=True))
    print("fold=%s v2=%s  module: analysis %.1f us (%.2f TB/s)  synthesis %.1f us (%.2f TB/s)  analysis-bwd %.1f us  synthesis-bwd %.1f us"
          % (fold, v2, a, mb / a, s, mb / s, ab, sb))      # MB / us = TB/s (HIP events around the autograd call)

# kernel level: the folded-form entry points themselves
os.environ["RH_PQMF_FOLD"] = "1"
ft = m._fold(m.forward_conv.weight)
tab, lpad = ft
st = torch.cuda.current_stream().cuda_stream
yb = torch.empty(32, 16, 4096, device=dev)
xo = torch.empty(32, 1, 65536, device=dev)
pad = m.forward_conv._pad
ipad = m.inverse_conv._pad
for v2 in ("1", "0"):
    os.environ["RH_PQMF_V2"] = v2
    k1 = t(lambda: L.check(L.lib.rh_pqmf_fold_k1_f32(x.data_ptr(), tab.data_ptr(), 32, 65536, 4096, lpad - pad[0], 1.0, yb.data_ptr(), st)), 50)
    k2 = t(lambda: L.check(L.lib.rh_pqmf_fold_k2_f32(yb.data_ptr(), tab.data_ptr(), 32, 4096, 65536, 496 - 16 * ipad[0] - lpad, 16.0, xo.data_ptr(), st)), 50)
    print("kernel level v2=%s: fold->matrix (analysis fwd / synthesis bwd) %.1f us = %.2f TB/s = %.1f %% of 8 TB/s;  "
          "matrix->overlap-add (synthesis fwd / analysis bwd) %.1f us = %.2f TB/s = %.1f %%"
          % (v2, k1, mb / k1, 100 * mb / k1 / 8.0, k2, mb / k2, 100 * mb / k2 / 8.0))
