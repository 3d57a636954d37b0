"""Host side of the weight average (rave_amd/csrc/ema.hip, rave_amd/ema.py): what rh_ema_update_f32 / rh_swap_f32 refuse
before they launch anything, the resources of their kernels, and that the inputs of the GPU kernel test can tell the
arithmetic of scripts/train.py:95-96 from its plausible misreadings.  No GPU."""
import ctypes as C
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from ema_cases import SIZES, ema_inputs


def _table(n, a, b, count):
    from rave_amd import _lib as L
    it = (L.PairItem * n)()
    for i in range(n):
        it[i].a, it[i].b, it[i].n = a, b, count
    return it


def test_pair_entry_points_validate_their_host_tables_without_a_gpu():
    from rave_amd import _lib as L
    buf = (C.c_float * 64)()
    a, b = C.addressof(buf), C.addressof(buf) + 128
    update = lambda items, n, factor=0.999: L.lib.rh_ema_update_f32(items, n, factor, None)     # noqa: E731
    swap = lambda items, n, factor=None: L.lib.rh_swap_f32(items, n, None)                     # noqa: E731
    err = L.lib.rh_last_error
    for fn, who in ((update, b"ema_update"), (swap, b"swap")):
        assert fn(None, 0) == 0                                          # empty tables: nothing launched
        assert fn(_table(1, a, b, 8), 0) == 0
        assert fn(_table(3, None, None, 0), 3) == 0                      # only empty tensors (their pointers may be null)
        assert fn(_table(1, a, b, 8), -1) != 0 and who in err() and b"negative item count" in err()
        assert fn(None, 2) != 0 and who in err() and b"null table" in err()
        assert fn(_table(2, None, b, 8), 2) != 0 and b"null pointer" in err()
        assert fn(_table(2, a, None, 8), 2) != 0 and b"null pointer" in err()
        assert fn(_table(1, a, b, -1), 1) != 0 and b"bad element count" in err()
        assert fn(_table(1, a, b, 2 ** 31 - 1), 1) != 0 and b"bad element count" in err()
        assert fn(_table(1, a, b, 2 ** 40), 1) != 0 and b"bad element count" in err()
        assert fn(_table(1, a, a, 8), 1) != 0 and who in err() and b"same tensor" in err()
        bad_last = _table(70, a, b, 0)                                   # the WHOLE table is checked before the first launch
        bad_last[69].a, bad_last[69].b, bad_last[69].n = None, b, 4
        assert fn(bad_last, 70) != 0 and b"item 69" in err()
    for factor in (-0.001, 1.001, math.nan, math.inf, -math.inf):
        assert update(_table(1, a, b, 8), 1, factor) != 0 and b"factor" in err(), factor


def test_ema_kernels_use_no_scratch():
    spec = importlib.util.spec_from_file_location(
        "kernel_resources", Path(__file__).resolve().parents[1] / "tools" / "kernel_resources.py")
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    ks = [k for k in kr.kernels() if "ema_update_kernel" in k["name"] or "swap_kernel" in k["name"]]
    assert len(ks) == 2, ks
    for k in ks:
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0 and k["lds"] == 0, k


def _fma32(a, b, c):
    """fmaf on f32 arrays: the product of two f32 is exact in f64, so the sum is rounded once in f64 and once to f32 (the
    double rounding moves a result only where the f64 sum sits within 2^-29 relative of an f32 tie)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def test_the_gpu_test_inputs_tell_the_three_rounding_form_from_its_variants():
    """The expression the kernel must reproduce bit for bit is torch's ``w * factor + p * (1 - factor)``: two tensor-by-
    Python-scalar products (the scalar rounded to f32, the subtraction done in double before that) and one sum, each rounded.
    On the inputs of tests/test_gpu_ema.py that form equals torch's CPU result exactly and every other reading of the
    line differs from it in at least 100 elements -- a kernel that contracts into an FMA, derives 1 - factor in f32 or uses
    the lerp form cannot pass the GPU test."""
    assert max(SIZES) >= 65536
    pairs = ema_inputs()
    factor = 0.999
    want = np.concatenate([(w * factor + p * (1 - factor)).numpy() for w, p in pairs])
    w = np.concatenate([w.numpy() for w, _ in pairs])
    p = np.concatenate([p.numpy() for _, p in pairs])
    assert w.dtype == np.float32 and w.size == sum(SIZES)
    f, g = np.float32(factor), np.float32(1.0 - factor)
    three = w * f + p * g
    assert three.dtype == np.float32
    assert np.array_equal(three, want)
    variants = {
        "fma(w, f, p*g)": _fma32(w, f, p * g),
        "fma(p, g, w*f)": _fma32(p, g, w * f),
        "g = 1.f - (float)factor": w * f + p * (np.float32(1.0) - f),
        "lerp w + (p - w) * g": w + (p - w) * g,
    }
    for name, got in variants.items():
        assert got.dtype == np.float32
        differing = int(np.count_nonzero(got != want))
        print(f"{name}: {differing} of {want.size} elements differ")
        assert differing >= 100, (name, differing)


def test_cpu_parameters_are_refused():
    """No CPU fallback (tests/test_abi_and_host.py::test_no_cpu_fallback): the callback refuses a module it cannot serve."""
    from rave_amd.ema import EMA
    ema = EMA()
    with pytest.raises(RuntimeError, match="GPU"):
        ema.on_train_batch_end(None, torch.nn.Linear(3, 2), None, None, 0)
    assert ema.weights == {}
