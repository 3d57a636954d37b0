"""CPU tests of the mel variant of ``SpectralDistance`` (rave/core.py:446-490) and of what carries it: the loss and its gradient
against the float64 restatement of tests/mel_distance_reference.py at the 1e-5 of tests/test_oracle.py, the module tree and
buffers of ``rave_amd.mel.DifferentiableMelSpectrogram``, what stays refused, the untouched plain variant, the host answers of
the C entry points, and the gin overlay."""
import os
import re
import subprocess
import sys
from functools import partial

import pytest
import torch

import mel_distance_reference as R

RH_ERR_INVALID, RH_ERR_UNSUPPORTED = -1, -2
TOL = 1e-5           # tests/test_oracle.py's bar for the non-mel class


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("power", [1, 2])
def test_cpu_value_and_gradient_against_float64(power):
    from rave_amd.losses import SpectralDistance
    d = SpectralDistance(256, 44100, ("L1", "L2"), power, True, mel=16)
    x, y = R.white_noise((2, 1, 2048), 1), R.white_noise((2, 1, 2048), 2).requires_grad_(True)
    got = d(x, y)
    (gy,) = torch.autograd.grad(got, y)
    y64 = y.detach().double().requires_grad_(True)
    want = R.spectral_distance(x.double(), y64, 256, 44100, ("L1", "L2"), power, True, 16)
    (gy64,) = torch.autograd.grad(want, y64)
    assert got.dtype == torch.float32 and got.dim() == 0
    assert abs(float(got.detach()) - float(want.detach())) <= TOL * abs(float(want.detach())), (float(got.detach()), float(want.detach()))
    assert _rel(gy, gy64) <= TOL, _rel(gy, gy64)
    assert tuple(d.spec(x).shape) == (2, 1, 16, (2048 - 256) // 64 + 1)


def test_encodec_distance_on_the_cpu():
    from rave_amd.losses import EncodecAudioDistance, SpectralDistance
    m = EncodecAudioDistance([256, 512], partial(SpectralDistance, sampling_rate=44100, norm=("L1", "L2"), power=1, normalized=True, mel=16))
    x, y = R.white_noise((2, 1, 4096), 3), R.white_noise((2, 1, 4096), 4)
    got = m(x, y)
    want = R.encodec_audio_distance(x.double(), y.double(), [256, 512], 44100, ("L1", "L2"), 1, True, 16)
    assert sorted(got) == ["spectral_distance", "waveform_distance"]
    for k in got:
        assert abs(float(got[k]) - float(want[k])) <= TOL * abs(float(want[k])), k
    assert sorted(m.state_dict()) == [f"spectral_distances.{i}.mel_spec.{k}" for i in (0, 1) for k in ("mel_scale.fb", "spectrogram.window")]


def test_module_tree_and_buffers():
    import rave_amd
    from rave_amd.losses import SpectralDistance
    from rave_amd.mel import DifferentiableMelSpectrogram, melscale_fbanks
    assert rave_amd.DifferentiableMelSpectrogram is DifferentiableMelSpectrogram
    d = SpectralDistance(256, 44100, ("L1", "L2"), 1, True, mel=16)
    mel = d.mel_spec
    assert isinstance(mel, DifferentiableMelSpectrogram)
    assert sorted(mel.state_dict()) == ["mel_scale.fb", "spectrogram.window"]
    assert torch.equal(mel.mel_scale.fb, melscale_fbanks(129, 0.0, 22050.0, 16, 44100))
    assert torch.equal(mel.spectrogram.window, torch.hann_window(256))
    assert (mel.n_fft, mel.hop_length, mel.n_mels, mel.power, mel.normalized, mel.center) == (256, 64, 16, 1, True, False)
    assert callable(d.spec) and not isinstance(d.spec, torch.nn.Module)          # still the method
    assert hasattr(mel, "refresh_host_caches")
    mel.refresh_host_caches()                                                     # host buffers: nothing to build, no error
    # a loaded filterbank is what the module computes with
    fb = torch.rand(129, 16)
    mel.load_state_dict({"mel_scale.fb": fb, "spectrogram.window": torch.hamming_window(256)})
    x = R.white_noise((3, 1000), 5)
    want = R.mel_spectrogram(x.double(), 44100, 256, 64, 16, 1, True, False, fb=fb, window=torch.hamming_window(256))
    assert _rel(mel(x), want) <= TOL


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("power", [1, 2])
def test_module_on_the_cpu_against_float64(power, center):
    from rave_amd.mel import DifferentiableMelSpectrogram
    m = DifferentiableMelSpectrogram(44100, 512, hop_length=100, n_mels=40, power=power, normalized=power == 2, center=center)
    x = R.white_noise((2, 3, 1777), 6).requires_grad_(True)
    got = m(x)
    x64 = x.detach().double().requires_grad_(True)
    want = R.mel_spectrogram(x64, 44100, 512, 100, 40, power, power == 2, center)
    assert tuple(got.shape) == tuple(want.shape) == (2, 3, 40, 1777 // 100 + 1 if center else (1777 - 512) // 100 + 1)
    g = R.white_noise(tuple(want.shape), 7, torch.float64)
    (dx,) = torch.autograd.grad(got, x, g.float())
    (dx64,) = torch.autograd.grad(want, x64, g)
    assert _rel(got, want) <= TOL and _rel(dx, dx64) <= TOL


def test_what_stays_refused():
    from rave_amd.losses import SpectralDistance
    from rave_amd.mel import DifferentiableMelSpectrogram, MelSpectrogram
    hybrid = dict(sample_rate=44100, n_fft=2048, win_length=2048, hop_length=256, normalized=True, n_mels=128)
    for bad in (dict(power=1.0), dict(center=False)):                             # the encoder input is what it was
        with pytest.raises(NotImplementedError):
            MelSpectrogram(**{**hybrid, **bad})
    for bad, word in ((dict(mel_scale="slaney"), "slaney"), (dict(norm="slaney"), "norm"), (dict(win_length=1024), "win_length"),
                      (dict(pad=8), "pad"), (dict(window_fn=torch.hamming_window), "window_fn"), (dict(onesided=False), "onesided"),
                      (dict(power=None), "power"), (dict(power=3.0), "power"), (dict(pad_mode="constant"), "pad_mode")):
        with pytest.raises(NotImplementedError, match=word):
            DifferentiableMelSpectrogram(**{**hybrid, **bad})
    DifferentiableMelSpectrogram(**{**hybrid, "power": 1.0, "center": False, "pad_mode": None})
    with pytest.raises(ValueError, match="power"):
        SpectralDistance(256, 44100, "L1", None, True, mel=16)


def test_plain_variant_is_what_it_was():
    from rave_amd.losses import SpectralDistance
    d = SpectralDistance(256, 44100, ("L1", "L2"), 1, True)
    assert list(d.state_dict()) == []
    assert [k for k, _ in d.named_buffers()] == ["window"] and [k for k, _ in d.named_modules()] == [""]
    assert not hasattr(d, "mel_spec")
    x, y = R.white_noise((2, 1, 2048), 8), R.white_noise((2, 1, 2048), 9)
    re, im = R.spectrum(x.double(), 256, 64, True, False)
    assert _rel(d.spec(x), (re * re + im * im).sqrt().transpose(-1, -2)) <= TOL
    assert torch.isfinite(d(x, y))
    assert torch.is_complex(SpectralDistance(256, 44100, "L1", None, True).spec(x))


def test_entry_points_answer_for_built_and_unbuilt_sizes():
    from rave_amd import _lib as L, ops
    lib = L.lib
    for n_fft, hop, n_mels, t, rows, center, power, want in (
            (2048, 512, 64, 65536, 64, 0, 1, 1), (128, 32, 128, 128, 1, 0, 2, 1), (128, 128, 1, 128, 1, 1, 1, 1),
            (256, 1, 16, 300, 3, 0, 2, 1), (512, 100, 80, 1000, 3, 1, 2, 1), (1024, 256, 128, 4096, 65535, 0, 1, 1),
            (2048, 512, 64, 1025, 1, 1, 1, 1), (2048, 512, 64, 2 ** 30, 1, 0, 1, 1),
            (2048, 512, 64, 2047, 1, 0, 1, 0),        # uncentred: at least one whole frame
            (2048, 512, 64, 1024, 1, 1, 1, 0),        # centred: T must exceed n_fft / 2 (reflect padding)
            (4096, 1024, 64, 65536, 1, 0, 1, 0), (64, 16, 16, 4096, 1, 0, 1, 0), (1000, 250, 64, 4096, 1, 0, 1, 0),
            (2048, 0, 64, 4096, 1, 0, 1, 0), (2048, -512, 64, 4096, 1, 0, 1, 0), (2048, 2049, 64, 8192, 1, 0, 1, 0),
            (2048, 512, 129, 4096, 1, 0, 1, 0), (2048, 512, 0, 4096, 1, 0, 1, 0), (2048, 512, 64, 4096, 0, 0, 1, 0),
            (2048, 512, 64, 4096, 65536, 0, 1, 0), (2048, 512, 64, 2 ** 30 + 1, 1, 0, 1, 0), (2048, 512, 64, 4096, 1, 0, 0, 0),
            (2048, 512, 64, 4096, 1, 0, 3, 0), (2048, 512, 64, 4096, 1, 2, 1, 0), (2048, 512, 64, 4096, 1, -1, 1, 0)):
        assert lib.rh_mel_diff_supported(n_fft, hop, n_mels, t, rows, center, power) == want, (n_fft, hop, n_mels, t, rows, center, power)
    assert ops.mel_diff_supported(512, 128, 64, 4096, 2, False, 1) and not ops.mel_diff_supported(512, 128, 64, 4096, 2, False, None)
    assert not ops.mel_diff_supported(512, 128, 64, 4096, 2, False, 1.5)

    p = 64               # never dereferenced: every call below is refused before a launch

    def fwd(x=p, win=p, tw=p, fb=p, bins=p, rows=2, t=4096, n_fft=2048, hop=512, n_mels=64, center=0, power=1, scale=1.0, y=p):
        return lib.rh_mel_diff_fwd_f32(x, win, tw, fb, bins, rows, t, n_fft, hop, n_mels, center, power, scale, y, None)

    def bwd(dmel=p, x=p, win=p, tw=p, fb=p, bins=p, rows=2, t=4096, n_fft=2048, hop=512, n_mels=64, center=0, power=1, scale=1.0, dx=p):
        return lib.rh_mel_diff_bwd_f32(dmel, x, win, tw, fb, bins, rows, t, n_fft, hop, n_mels, center, power, scale, dx, None)

    for call, names in ((fwd, ("x", "win", "tw", "fb", "bins", "y")), (bwd, ("dmel", "x", "win", "tw", "fb", "bins", "dx"))):
        for name in names:
            assert call(**{name: None}) == RH_ERR_INVALID, name
            assert b"null" in lib.rh_last_error()
        for bad in (dict(n_fft=4096), dict(n_fft=1000), dict(hop=0), dict(hop=4096), dict(n_mels=129), dict(n_mels=0), dict(t=2047),
                    dict(rows=0), dict(rows=65536), dict(power=0), dict(power=3), dict(center=2)):
            assert call(**bad) == RH_ERR_UNSUPPORTED, bad
            assert lib.rh_last_error()
        assert call(tw=68) == RH_ERR_INVALID and b"aligned" in lib.rh_last_error()
        for s in (0.0, float("nan"), float("inf"), -1.0):
            assert call(scale=s) == RH_ERR_INVALID, s


_GIN_SCRIPT = r"""
import json, os, re, sys
root = sys.argv[1]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "oracle", "shims"))
sys.dont_write_bytecode = True
import gin
text = open(os.path.join(root, "rave_amd", "configs", "mi355x_encodec_mel.gin")).read()
# upstream's package is no part of this repository: its import and its one block are taken out (the caller checks the block)
text = re.sub(r"^import rave\n", "", text, flags=re.M)
text = re.sub(r"^rave\.RAVE:\n(?:[ \t]+.*\n?)+", "", text, flags=re.M)
assert "rave.RAVE" not in "\n".join(l for l in text.splitlines() if not l.startswith("#"))
gin.clear_config()
gin.parse_config("SAMPLING_RATE = 48000")            # what v1.gin defines ahead of the overlay
gin.parse_config(text)
import rave_amd.losses, rave_amd.mel
m = gin._make_ref(rave_amd.losses.EncodecAudioDistance, "")()
mels = [d.mel_spec for d in m.spectral_distances]
print("RESULT" + json.dumps(dict(cls=type(m).__module__ + "." + type(m).__name__,
                                 kinds=sorted({type(d).__module__ + "." + type(d).__name__ for d in m.spectral_distances}),
                                 mel=sorted({type(s).__module__ + "." + type(s).__name__ for s in mels}),
                                 geo=[[s.sample_rate, s.n_fft, s.hop_length, s.n_mels, s.power, s.normalized, s.center] for s in mels],
                                 norm=[list(d.norm) for d in m.spectral_distances])))
"""


def test_gin_overlay_builds_the_loss_on_the_drop_in_classes():
    """rave_amd/configs/mi355x_encodec_mel.gin through the repository's own gin parser (oracle/shims/gin): the bindings build
    ``EncodecAudioDistance`` over ``SpectralDistance(mel=64)`` on ``DifferentiableMelSpectrogram``, and ``rave.RAVE`` is handed
    that class."""
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "rave_amd", "configs", "mi355x_encodec_mel.gin")).read()
    code = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    assert code.lstrip().startswith("from __gin__ import dynamic_registration")
    assert re.search(r"^rave\.RAVE:\s*\n\s+audio_distance = @rave_amd\.losses\.EncodecAudioDistance\s*(\n|$)", code, re.M)
    assert "import rave_amd.losses" in code
    r = subprocess.run([sys.executable, "-c", _GIN_SCRIPT, root], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])
    assert got["cls"] == "rave_amd.losses.EncodecAudioDistance"
    assert got["kinds"] == ["rave_amd.losses.SpectralDistance"] and got["mel"] == ["rave_amd.mel.DifferentiableMelSpectrogram"]
    assert got["geo"] == [[48000, n, n // 4, 64, 1, True, False] for n in (2048, 1024, 512, 256, 128)]
    assert got["norm"] == [["L1", "L2"]] * 5
