"""CPU tests of the plain ``SpectralDistance`` (rave/core.py:446-490 without ``mel``) and of what carries its HIP path: the five C
entry points and their host answers, the loss and both gradients on the CPU (the torch composition) against the float64
restatement of tests/spectral_distance_reference.py at the 1e-5 of tests/test_oracle.py, the ``RH_SPEC_DIST`` switch, the gin
overlay and ``build_v2(encodec_distance=True)``."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from functools import partial

import pytest
import torch

import spectral_distance_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RH_ERR_INVALID, RH_ERR_UNSUPPORTED = -1, -2
TOL = 1e-5           # tests/test_oracle.py's bar for this class
ENTRY_POINTS = ("rh_spec_dist_supported", "rh_spec_dist_workspace_bytes", "rh_spec_dist_fwd_f32", "rh_spec_dist_finalize_all_f32",
                "rh_spec_dist_bwd_f32")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def test_header_declares_the_five_entry_points():
    from rave_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "rave_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(L.lib, name), name
    assert "rave/core.py:446-490" in hdr and "rave/core.py:415-433" in hdr


def test_supported_answers():
    from rave_amd import _lib as L, ops
    sup = L.lib.rh_spec_dist_supported
    for n in (128, 256, 512, 1024, 2048):
        assert sup(n, n // 4, n, 1, 1) == 1 and sup(n, n // 4, n, 65535, 2) == 1, n
        assert sup(n, n // 4, n - 1, 1, 1) == 0, n
        assert sup(n, n // 4, 2 ** 30, 1, 1) == 1 and sup(n, n // 4, 2 ** 30 + 1, 1, 1) == 0, n
    for args in ((64, 16, 4096, 1, 1), (4096, 1024, 65536, 1, 1), (1000, 250, 4096, 1, 1), (512, 100, 4096, 1, 1), (512, 512, 4096, 1, 1),
                 (512, 128, 511, 1, 1), (512, 128, 4096, 0, 1), (512, 128, 4096, 65536, 1), (512, 128, 4096, 1, 0), (512, 128, 4096, 1, 3)):
        assert sup(*args) == 0, args
    assert ops.spec_dist_supported([2048, 1024, 512, 256, 128], 65536, 32, 1)
    assert not ops.spec_dist_supported([512, 64], 4096, 2, 1) and not ops.spec_dist_supported([512], 4096, 2, None)
    assert not ops.spec_dist_supported([512], 4096, 2, 1.5) and not ops.spec_dist_supported([], 4096, 2, 1)
    assert L.lib.rh_spec_dist_workspace_bytes(64, 4096, 1) == 0
    assert L.lib.rh_spec_dist_workspace_bytes(512, 4096, 2) >= 2 * 2 * 4


def test_backward_plan_stays_within_the_stft_kernel_s_lds():
    """The backward kernel's dynamic LDS never exceeds what rh_stft_loss_bwd_f32 takes at n_fft = 2048 (its plan's 150 KiB cap),
    and every span tiles the row."""
    from rave_amd import _lib as L
    cap = 150 * 1024
    out, ref = (C.c_int64 * 6)(), (C.c_int64 * 6)()
    worst = 0
    for t, rows in ((65536, 32), (65536, 1), (2 ** 20, 1), (12288, 1)):
        assert L.lib.rh_stft_loss_plan_info(2048, t, rows, ref) == 0
        worst = max(worst, ref[5])
    assert worst <= cap
    for n in (128, 256, 512, 1024, 2048):
        for t, rows in ((n, 1), (3 * n + 5, 3), (5000, 3),(65536, 32), (65536, 64), (2 ** 20, 1)):
            assert L.lib.rh_spec_dist_plan_info(n, t, rows, out) == 0
            fpw, fwgs, cb, nch, last, lds = list(out)
            frames, blocks = (t - n) // (n // 4) + 1, (t + n // 4 - 1) // (n // 4)
            assert fpw * fwgs >= frames > fpw * (fwgs - 1)
            assert (nch - 1) * cb + last == blocks and last >= 1
            assert lds <= cap, (n, t, rows, lds)
    assert L.lib.rh_spec_dist_plan_info(64, 4096, 1, out) == RH_ERR_UNSUPPORTED


def test_entry_points_refuse_before_a_launch():
    from rave_amd import _lib as L
    lib = L.lib
    p, q = 1 << 20, 1 << 24          # never dereferenced: every call below is refused before a launch

    def fwd(x=p, y=q, win=64, tw=64, rows=2, t=4096, n_fft=512, power=1, scale=1.0, ws=64, nbytes=1 << 20):
        return lib.rh_spec_dist_fwd_f32(x, y, win, tw, rows, t, n_fft, power, scale, ws, nbytes, None)

    def bwd(x=p, y=q, win=64, tw=64, rows=2, t=4096, n_fft=512, power=1, scale=1.0, l1=1, l2=1, g=64, dx=64, dy=64):
        return lib.rh_spec_dist_bwd_f32(x, y, win, tw, rows, t, n_fft, power, scale, l1, l2, g, dx, dy, 0, None)

    for call, names in ((fwd, ("x", "y", "win", "tw", "ws")), (bwd, ("x", "y", "win", "tw", "g"))):
        for name in names:
            assert call(**{name: None}) == RH_ERR_INVALID, name
            assert b"null" in lib.rh_last_error()
        for bad in (dict(n_fft=4096), dict(n_fft=64), dict(n_fft=1000), dict(t=511), dict(t=2 ** 30 + 1), dict(rows=0), dict(rows=65536),
                    dict(power=0), dict(power=3)):
            assert call(**bad) == RH_ERR_UNSUPPORTED, bad
            assert lib.rh_last_error()
        assert call(tw=68) == RH_ERR_INVALID and b"aligned" in lib.rh_last_error()
        for s in (0.0, float("nan"), float("inf"), -1.0):
            assert call(scale=s) == RH_ERR_INVALID, s
        assert call(y=p) == RH_ERR_INVALID and b"overlap" in lib.rh_last_error()
        assert call(y=p + 4 * (2 * 4096 - 1)) == RH_ERR_INVALID and call(x=q + 4 * (2 * 4096 - 1)) == RH_ERR_INVALID
    assert fwd(nbytes=4) != 0
    assert bwd(l1=0, l2=0) == RH_ERR_UNSUPPORTED
    assert bwd(dx=None, dy=None) == 0                                   # nothing to do, nothing launched
    parts, nb = (C.c_void_p * 1)(64), (C.c_int64 * 1)(16)
    fin = lib.rh_spec_dist_finalize_all_f32
    assert fin(parts, nb, 1, 64, 0, 0, 64, 64, None) == RH_ERR_UNSUPPORTED
    assert fin(parts, nb, 0, 64, 1, 1, 64, 64, None) == RH_ERR_INVALID and fin(parts, nb, 9, 64, 1, 1, 64, 64, None) == RH_ERR_INVALID
    assert fin(parts, nb, 1, None, 1, 1, 64, 64, None) == RH_ERR_INVALID
    assert fin(parts, (C.c_int64 * 1)(12), 1, 64, 1, 1, 64, 64, None) == RH_ERR_INVALID


@pytest.mark.parametrize("norms", ["L1", "L2", ("L1", "L2")], ids=str)
@pytest.mark.parametrize("power", [1, 2])
def test_cpu_value_and_gradients_against_float64(power, norms):
    """The composition, unchanged."""
    from rave_amd.losses import SpectralDistance
    d = SpectralDistance(256, 44100, norms, power, True)
    x, y = R.white_noise((2, 1, 2048), 1).requires_grad_(True), R.white_noise((2, 1, 2048), 2).requires_grad_(True)
    got = d(x, y)
    gx, gy = torch.autograd.grad(got, (x, y))
    x64, y64 = x.detach().double().requires_grad_(True), y.detach().double().requires_grad_(True)
    want = R.spectral_distance(x64, y64, 256, norms, power, True)
    gx64, gy64 = torch.autograd.grad(want, (x64, y64))
    assert got.dtype == torch.float32 and got.dim() == 0
    assert "SpecDist" not in type(got.grad_fn).__name__
    assert abs(float(got.detach()) - float(want.detach())) <= TOL * abs(float(want.detach())), (float(got.detach()), float(want.detach()))
    assert _rel(gx, gx64) <= TOL and _rel(gy, gy64) <= TOL, (_rel(gx, gx64), _rel(gy, gy64))
    assert tuple(d.spec(x).shape) == (2, 1, 129, (2048 - 256) // 64 + 1)


def test_encodec_distance_on_the_cpu():
    from rave_amd.losses import EncodecAudioDistance, SpectralDistance
    m = EncodecAudioDistance([512, 128, 64], partial(SpectralDistance, sampling_rate=44100, norm=("L1", "L2"), power=1, normalized=True))
    x, y = R.white_noise((2, 1, 4096), 3), R.white_noise((2, 1, 4096), 4)
    got = m(x, y)
    want = R.encodec_audio_distance(x.double(), y.double(), [512, 128, 64], ("L1", "L2"), 1, True)
    assert sorted(got) == ["spectral_distance", "waveform_distance"]
    for k in got:
        assert abs(float(got[k]) - float(want[k])) <= TOL * abs(float(want[k])), k
    assert list(m.state_dict()) == []


def test_the_reference_helpers():
    x, y = R.white_noise((2, 1024), 5, torch.float64), R.white_noise((2, 1024), 6, torch.float64)
    assert R.smallest_gap(x, x, 256, True) == 0.0
    g = R.smallest_gap(x, y, 256, True)
    assert 0.0 < g < 1.0
    a, b = R.power_spectrum(y, 256, 1, True), R.power_spectrum(x, 256, 1, True)
    assert tuple(a.shape) == (2, (1024 - 256) // 64 + 1, 129)
    assert g == float(((a - b).abs() / torch.maximum(a, b)).min())
    assert torch.allclose(R.power_spectrum(x, 256, 2, True), b * b)
    assert R.kink_clear(x, y, 256, True) == (g > 1e-5 and R.smallest_relative_bin(x, 256, 64, True, False) > 1e-6
                                             and R.smallest_relative_bin(y, 256, 64, True, False) > 1e-6)


def test_switch():
    from rave_amd import ops
    old = os.environ.get("RH_SPEC_DIST")
    try:
        os.environ["RH_SPEC_DIST"] = "0"
        assert not ops.spec_dist_on()
        os.environ["RH_SPEC_DIST"] = "1"
        assert ops.spec_dist_on()
    finally:
        if old is None:
            os.environ.pop("RH_SPEC_DIST", None)
        else:
            os.environ["RH_SPEC_DIST"] = old


def test_compose_is_the_module_s_expression():
    from rave_amd import ops
    from rave_amd.losses import SpectralDistance
    x, y = R.white_noise((2, 1, 2048), 7), R.white_noise((2, 1, 2048), 8)
    for power in (1, 2, None):
        d = SpectralDistance(256, 44100, ("L1",) if power is None else ("L1", "L2"), power, True)
        got = ops.spec_dist_compose(x, y, d.window, 256, d.norm, power, True)
        sx, sy = d.spec(x), d.spec(y)
        want = sum(((sy - sx).abs().mean() if n == "L1" else ((sy - sx) * (sy - sx)).mean()) for n in d.norm)
        assert torch.equal(got, want) and torch.equal(d(x, y), want), power


_GIN_SCRIPT = r"""
import json, os, re, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "oracle", "shims"))
sys.dont_write_bytecode = True
import gin
text = open(os.path.join(root, "rave_amd", "configs", "mi355x_encodec.gin")).read()
# upstream's package is no part of this repository: its import and its one block are taken out (the caller checks the block)
text = re.sub(r"^import rave\n", "", text, flags=re.M)
text = re.sub(r"^rave\.RAVE:\n(?:[ \t]+.*\n?)+", "", text, flags=re.M)
assert "rave.RAVE" not in "\n".join(l for l in text.splitlines() if not l.startswith("#"))
gin.clear_config()
gin.parse_config("SAMPLING_RATE = 48000")            # what v1.gin defines ahead of the overlay
gin.parse_config(text)
import rave_amd.losses
m = gin._make_ref(rave_amd.losses.EncodecAudioDistance, "")()
ds = list(m.spectral_distances)
print("RESULT" + json.dumps(dict(cls=type(m).__module__ + "." + type(m).__name__,
                                 kinds=sorted({type(d).__module__ + "." + type(d).__name__ for d in ds}),
                                 plain=[d.is_plain() and not hasattr(d, "mel_spec") for d in ds],
                                 geo=[[d.n_fft, d.hop, d.power, d.normalized] for d in ds],
                                 norm=[list(d.norm) for d in ds], keys=list(m.state_dict()))))
"""


def test_gin_overlay_builds_the_loss_on_the_drop_in_classes():
    """rave_amd/configs/mi355x_encodec.gin through the repository's own gin parser (oracle/shims/gin): the bindings build
    ``EncodecAudioDistance`` over plain ``SpectralDistance`` members, and ``rave.RAVE`` is handed that class."""
    text = open(os.path.join(ROOT, "rave_amd", "configs", "mi355x_encodec.gin")).read()
    code = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    assert code.lstrip().startswith("from __gin__ import dynamic_registration")
    assert re.search(r"^rave\.RAVE:\s*\n\s+audio_distance = @rave_amd\.losses\.EncodecAudioDistance\s*(\n|$)", code, re.M)
    assert "import rave_amd.losses" in code and "mel" not in code
    r = subprocess.run([sys.executable, "-c", _GIN_SCRIPT, ROOT], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert got["cls"] == "rave_amd.losses.EncodecAudioDistance"
    assert got["kinds"] == ["rave_amd.losses.SpectralDistance"] and got["plain"] == [True] * 5
    assert got["geo"] == [[n, n // 4, 1, True] for n in (2048, 1024, 512, 256, 128)]
    assert got["norm"] == [["L1", "L2"]] * 5 and got["keys"] == []


def test_build_v2_option():
    from rave_amd import losses, model as M
    kw = dict(capacity=16, latent_size=16, disc_capacity=16)
    torch.manual_seed(0)
    base = M.build_v2(**kw)
    torch.manual_seed(0)
    off = M.build_v2(encodec_distance=False, **kw)
    torch.manual_seed(0)
    on = M.build_v2(encodec_distance=True, **kw)
    assert isinstance(base.audio_distance, losses.AudioDistanceV1) and isinstance(off.audio_distance, losses.AudioDistanceV1)
    assert list(base.state_dict()) == list(off.state_dict()) == list(on.state_dict())
    assert all(torch.equal(a, b) for a, b in zip(base.state_dict().values(), off.state_dict().values()))
    ad = on.audio_distance
    assert isinstance(ad, losses.EncodecAudioDistance) and isinstance(on.multiband_audio_distance, losses.AudioDistanceV1)
    assert [type(d) for d in ad.spectral_distances] == [losses.SpectralDistance] * 5
    assert [(d.n_fft, d.power, d.normalized, d.norm, d.is_plain()) for d in ad.spectral_distances] == \
        [(n, 1, True, ("L1", "L2"), True) for n in (2048, 1024, 512, 256, 128)]
    assert list(ad.state_dict()) == []
    with pytest.raises(ValueError, match="choose one"):
        M.build_v2(encodec_distance=True, phase_distance=True, **kw)
