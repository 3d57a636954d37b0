"""The three GAN objectives of the training step (hinge, least squares, non-saturating) restated in torch, in any float dtype,
with their gradients through autograd -- the yardstick of tests/test_gan_loss_host.py and tests/test_gpu_gan_loss.py (a plain
helper module, no fixtures; importing it needs no GPU).

With r a real and f a fake score, means over the n scores of one head:
    hinge           dis = mean(relu(1 - r) + relu(1 + f))             adv = mean(-f)
    ls              dis = mean((r - 1)^2 + f^2)                       adv = mean((f - 1)^2)
    nonsaturating   p = clamp(sigmoid(s), LO, HI)
                    dis = mean(-(log p_r + log(1 - p_f)))             adv = mean(-log p_f)
LO, HI are 1e-7 and 1 - 1e-7 ROUNDED TO FLOAT32, in every dtype: a float32 run takes them so (HI = 1 - 2^-23), and a float64
yardstick for a float32 run has to saturate at the same two values (log(1 - HI) differs from log(1e-7) by 0.17).
Gates are autograd's: relu passes its gradient where its argument is > 0, clamp where LO <= p <= HI.
"""
import numpy as np
import torch

MODES = ("hinge", "ls", "nonsaturating")
LO = float(np.float32(1e-7))
HI = float(np.float32(1.0 - 1e-7))
U = 2.0 ** -24                      # unit roundoff of float32


def terms(mode, r, f):
    """The per-score summands (dis, adv): dis over pairs (r_k, f_k), adv over f_k."""
    if mode == "hinge":
        return torch.relu(1 - r) + torch.relu(1 + f), -f
    if mode == "ls":
        return (r - 1).pow(2) + f.pow(2), (f - 1).pow(2)
    if mode == "nonsaturating":
        pr = torch.clamp(torch.sigmoid(r), LO, HI)
        pf = torch.clamp(torch.sigmoid(f), LO, HI)
        return -(torch.log(pr) + torch.log(1 - pf)), -torch.log(pf)
    raise ValueError(mode)


def objective(mode, r, f):
    """(loss_dis, loss_adv) of one head."""
    d, a = terms(mode, r.reshape(-1), f.reshape(-1))
    return d.mean(), a.mean()


def totals(mode, heads, dtype, grad_out=(1.0, 1.0)):
    """``heads``: (real, fake) pairs.  Returns (out, grads, mean_abs, head_means): out = [loss_dis, loss_adv, pred_real,
    pred_fake] summed over the heads in ``dtype`` (0-d tensors), grads = [(d_real, d_fake)] of
    grad_out[0] * loss_dis + grad_out[1] * loss_adv, mean_abs = per head the mean |summand| of each of the four sums, head_means =
    per head its four means."""
    dev = heads[0][0].device
    out = [torch.zeros((), dtype=dtype, device=dev) for _ in range(4)]
    leaves, mean_abs, head_means = [], [], []
    for r, f in heads:
        r = r.detach().to(dtype).clone().requires_grad_(True)
        f = f.detach().to(dtype).clone().requires_grad_(True)
        leaves.append((r, f))
        d, a = terms(mode, r.reshape(-1), f.reshape(-1))
        vals = (d.mean(), a.mean(), r.mean(), f.mean())
        for k in range(4):
            out[k] = out[k] + vals[k]
        mean_abs.append(tuple(float(v.detach().abs().double().mean()) for v in (d, a, r, f)))
        head_means.append(tuple(float(v.detach()) for v in vals))
    (grad_out[0] * out[0] + grad_out[1] * out[1]).backward()
    grads = [(r.grad, f.grad) for r, f in leaves]
    return [v.detach() for v in out], grads, mean_abs, head_means


def derived_bound(mean_abs, head_means, k):
    """The float32 error allowed on total k (0 dis, 1 adv, 2 pred_real, 3 pred_fake) of a call, from the number format alone:
    per head 16 u (1 + mean |summand|) -- a few ulp for the expf / logf / division chain, whose absolute error near p -> 1 is
    capped by ulp(1), the 16 sequential additions of a thread, the 6 + 2 levels of the workgroup's tree, the ordered finalize and
    the division by n --, and for the ordered sum over H heads the worst case of H - 1 sequential float32 additions,
    (H - 1) u sum_h |mean_h|."""
    per_head = sum(16 * U * (1 + m[k]) for m in mean_abs)
    return per_head + (len(mean_abs) - 1) * U * sum(abs(h[k]) for h in head_means)


def scores(n, seed, mode=None, plant=True):
    """(real, fake) float64 scores of one head from N(0, 2^2), no |s| beyond 13 (the float32 sigmoid reaches the clamp bounds
    near |s| = 16: nothing may sit in [14, 18], where two libraries' sigmoids can fall on either side).  ``plant`` (n >= 5):
    non-saturating -- +-12 (inside the clamp) and +-20 (outside: the gradient is exactly 0) in both halves; hinge -- r == 1 and
    f == -1 exactly (the gates are closed at equality)."""
    g = torch.Generator().manual_seed(seed)
    r = (2 * torch.randn(n, generator=g, dtype=torch.float64)).clamp(-13, 13)
    f = (2 * torch.randn(n, generator=g, dtype=torch.float64)).clamp(-13, 13)
    r, f = r.float().double(), f.float().double()          # exactly representable in float32
    if plant and n >= 5:
        if mode == "nonsaturating":
            for t in (r, f):
                t[0], t[1], t[n // 2], t[n - 1] = 12.0, -12.0, 20.0, -20.0
        elif mode == "hinge":
            r[n // 2], f[n - 1] = 1.0, -1.0
    return r, f


def planted(mode, n):
    """Indices (into a half) where the gradient must be exactly 0: {"real": [...], "fake_dis": [...]} -- for the fake half of the
    hinge objective only the dis part is gated (adv = -f always passes), so callers test it with grad_out = (g, 0)."""
    if n < 5:
        return dict(real=[], fake_dis=[], fake_all=[])
    if mode == "nonsaturating":
        return dict(real=[n // 2, n - 1], fake_dis=[n // 2, n - 1], fake_all=[n // 2, n - 1])
    if mode == "hinge":
        return dict(real=[n // 2], fake_dis=[n - 1], fake_all=[])
    return dict(real=[], fake_dis=[], fake_all=[])
