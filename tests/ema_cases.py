"""Inputs of the multi-tensor EMA / swap kernel tests (tests/test_gpu_ema.py), shared with the host test that shows these
very inputs can tell the three-rounding form from every plausible wrong one (tests/test_ema_host.py)."""
import torch

# 70 tensors: the table chunks at 64, and with the two empty ones (which take no slot) the first chunk spans 66 items.
# Sizes around the 2048 elements of a workgroup and the 4 of a 16-byte access, one beyond 32 workgroups.
SIZES = [1, 5, 0, 2047, 2048, 2049, 4099, 65536 + 3, 3001, 2500] + [3 + 37 * i for i in range(29)] + [0] + \
        [4 + 8 * i for i in range(30)]
W_MISALIGNED = 8          # w starts one float past a 16-byte boundary, p is aligned
P_MISALIGNED = 9          # the other way round
GUARD = 4                 # floats kept in front of and behind every tensor
FACTORS = (0.999, 0.5, 0.0, 1.0)
assert len(SIZES) == 70 and SIZES.count(0) == 2


def ema_inputs(seed: int = 0):
    """[(w, p)]: independent standard normal draws, CPU f32."""
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=gen), torch.randn(n, generator=gen)) for n in SIZES]
