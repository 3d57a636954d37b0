"""Host-side tests of the complex spectrogram (rave_amd.Spectrogram, rave_amd.ops.spectrogram, the ``hip_frontend`` flag of the
two spectral discriminators): no GPU needed.  CPU tensors take the torch composition; the float64 restatement of
tests/spectrogram_reference.py is itself pinned against torch.stft (and torchaudio, where installed)."""
import importlib
import inspect
import os
import re
from functools import partial

import pytest
import torch
import torch.nn as nn

import spectrogram_reference as R
from conftest import rel_l2

F32 = 2e-6        # float32 rounding of an n_fft <= 1024 point transform against float64 (eps 6e-8 x a few passes)


def test_reference_helper_is_torch_stft_in_float64():
    for n_fft, hop, t, center, normalized in ((128, 32, 1000, False, True), (256, 64, 777, True, True), (512, 100, 2048, True, False),
                                              (128, 128, 128, False, False), (128, 1, 65, True, True)):
        x = R.white_noise((2, 3, t), 1, torch.float64)
        win = torch.hamming_window(n_fft, dtype=torch.float64)
        got = R.spectrogram(x, win, n_fft, hop, normalized, center)
        want = torch.stft(x.reshape(-1, t), n_fft, hop_length=hop, win_length=n_fft, window=win, center=center, pad_mode="reflect",
                          normalized=False, onesided=True, return_complex=True).reshape(2, 3, n_fft // 2 + 1, -1)
        if normalized:
            want = want / win.pow(2).sum().sqrt()
        assert got.shape == want.shape and got.shape[-1] == R.frames_of(n_fft, hop, t, center)
        assert rel_l2(torch.view_as_real(got), torch.view_as_real(want)) < 1e-14


def test_reference_helper_is_torchaudio():
    ta = pytest.importorskip("torchaudio")
    shims = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "shims")
    if os.path.abspath(ta.__file__).startswith(shims + os.sep):
        pytest.skip("oracle/shims/torchaudio is on the path: the oracle's stand-in, not torchaudio")
    for power in (None, 1, 2):
        x = R.white_noise((2, 1, 3000), 2, torch.float64)
        mod = ta.transforms.Spectrogram(512, hop_length=128, power=power, normalized=True, center=power is not None).double()
        want = mod(x)
        got = R.spectrogram(x, mod.window, 512, 128, True, power is not None, power)
        assert rel_l2(torch.view_as_real(got) if power is None else got, torch.view_as_real(want) if power is None else want) < 1e-13


def test_module_has_torchaudios_signature_and_one_buffer():
    import rave_amd
    S = rave_amd.Spectrogram
    names = list(inspect.signature(S.__init__).parameters)[1:]
    assert names == ["n_fft", "win_length", "hop_length", "pad", "window_fn", "power", "normalized", "wkwargs", "center", "pad_mode",
                     "onesided"]
    d = {k: p.default for k, p in inspect.signature(S.__init__).parameters.items()}
    assert (d["n_fft"], d["win_length"], d["hop_length"], d["pad"], d["power"], d["normalized"], d["center"], d["pad_mode"],
            d["onesided"]) == (400, None, None, 0, 2.0, False, True, "reflect", True) and d["window_fn"] is torch.hann_window
    m = S(512)
    assert [k for k, _ in m.named_buffers()] == ["window"] and list(m.state_dict()) == ["window"] and not list(m.parameters())
    assert m.window.shape == (512,) and torch.equal(m.window, torch.hann_window(512)) and m.hop_length == 256
    assert torch.equal(S(128, window_fn=torch.hamming_window, wkwargs=dict(periodic=False)).window,
                       torch.hamming_window(128, periodic=False))


@pytest.mark.parametrize("power", [None, 1, 2])
@pytest.mark.parametrize("center", [False, True])
def test_cpu_tensors_equal_the_reference(power, center):
    import rave_amd
    x = R.white_noise((2, 3, 3000), 3)
    m = rave_amd.Spectrogram(512, hop_length=128, power=power, normalized=True, center=center)
    got = m(x)
    want = R.spectrogram(x.double(), m.window.double(), 512, 128, True, center, power)
    assert got.shape == want.shape and got.is_complex() == (power is None)
    assert got.dtype == (torch.complex64 if power is None else torch.float32)
    frames = want.shape[-1]
    if power is None:
        got, want = torch.view_as_real(got), torch.view_as_real(want)
    assert rel_l2(got, want) < F32
    ri = m.real_imag(x)
    assert ri.shape == (2, 6, 257, frames) and rel_l2(ri, R.real_imag(x.double(), m.window.double(), 512, 128, True, center)) < F32
    pl = m.planes(x)
    assert pl.shape == (2, 3, 2, 257, frames) and rel_l2(pl, R.planes(x.double(), m.window.double(), 512, 128, True, center)) < F32


def test_cpu_gradient_flows_through_the_composition():
    from rave_amd import ops
    x = R.white_noise((1, 2, 1000), 4).requires_grad_(True)
    win = torch.hann_window(256)
    g = R.white_noise((1, 4, 129, 12), 5)
    ops.spectrogram(x, win, 256, 64, True, False, cat_channels=True).backward(g)
    x64 = x.detach().double().requires_grad_(True)
    R.real_imag(x64, win.double(), 256, 64, True, False).backward(g.double())
    assert rel_l2(x.grad, x64.grad) < F32


def test_refused_arguments_name_themselves():
    import rave_amd
    S = rave_amd.Spectrogram
    for kw, word in ((dict(pad=1), "pad"), (dict(onesided=False), "onesided"), (dict(win_length=256), "win_length"),
                     (dict(center=True, pad_mode="constant"), "pad_mode"), (dict(power=3), "power")):
        with pytest.raises(NotImplementedError, match=word):
            S(512, **kw)
    S(512, center=False, pad_mode="constant")          # unused when not centred, as in torchaudio


def test_supported_query_answers_on_the_host():
    from rave_amd import _lib as L, ops
    q = L.lib.rh_spectrogram_supported
    for n in (128, 256, 512, 1024, 2048, 4096):
        for hop in (1, n // 4, n):
            assert q(n, hop, n, 3, 0) == 1 and q(n, hop, n // 2 + 1, 3, 1) == 1, (n, hop)
        assert q(n, 0, 4 * n, 3, 0) == 0 and q(n, n + 1, 4 * n, 3, 0) == 0                # hop outside 1 .. n_fft
        assert q(n, n // 4, n - 1, 3, 0) == 0 and q(n, n // 4, n // 2, 3, 1) == 0         # too short to frame / to reflect
        assert q(n, n // 4, n - 1, 3, 1) == 1
        for c in (0, 1):                                                                  # the kernels' index math is int
            assert q(n, n // 4, 1 << 30, 3, c) == 1 and q(n, n // 4, (1 << 30) + 1, 3, c) == 0
        assert q(n, n // 4, 4 * n, 0, 0) == 0 and q(n, n // 4, 4 * n, 65536, 0) == 0 and q(n, n // 4, 4 * n, 65535, 0) == 1
    for n in (64, 8192, 1000, 384, 0, -128):
        assert q(n, max(n // 4, 1), 65536, 3, 0) == 0, n
    assert ops.spectrogram_supported(512, 128, 65536, 64, False) and not ops.spectrogram_supported(8192, 2048, 65536, 64, False)


def test_entry_points_refuse_on_the_host():
    from rave_amd import _lib as L
    p = 64            # a non-null address nothing dereferences: every case below returns before a launch

    def call(fn, a=p, win=p, tw=p, rows=4, channels=2, t=4096, n_fft=512, hop=128, center=0, scale=1.0, b=p):
        return fn(a, win, tw, rows, channels, t, n_fft, hop, center, scale, b, None)

    for fn in (L.lib.rh_spectrogram_fwd_f32, L.lib.rh_spectrogram_bwd_f32):
        for name in ("a", "win", "tw", "b"):
            assert call(fn, **{name: None}) == -1 and b"null" in L.lib.rh_last_error(), name
        for bad in (dict(n_fft=8192), dict(n_fft=64), dict(n_fft=1000), dict(hop=0), dict(hop=513), dict(t=511), dict(rows=0),
                    dict(rows=65536), dict(t=256, center=1)):
            assert call(fn, **bad) == -2, bad
        assert call(fn, channels=3) == -1 and call(fn, channels=0) == -1
        assert call(fn, tw=68) == -1 and b"aligned" in L.lib.rh_last_error()
        assert call(fn, scale=0.0) == -1 and call(fn, scale=float("nan")) == -1 and call(fn, scale=float("inf")) == -1


def _encodec(hip):
    from rave_amd import discriminator as D
    return D.MultiScaleSpectralDiscriminator([512, 128], partial(D.EncodecConvNet, capacity=8), n_channels=2, hip_frontend=hip)


def _descript(hip):
    from rave_amd import descript_discriminator as DD
    return DD.DescriptDiscriminator(periods=[3], fft_sizes=[256], n_channels=2, hip_frontend=hip)


@pytest.mark.parametrize("make", [_encodec, _descript])
def test_flag_changes_neither_modules_nor_keys(make):
    on, off = make(True), make(False)
    assert list(on.state_dict()) == list(off.state_dict())
    assert [(k, type(m)) for k, m in on.named_modules()] == [(k, type(m)) for k, m in off.named_modules()]
    windows = [k for k in on.state_dict() if k.endswith(".window")]
    assert windows and all(torch.equal(on.state_dict()[k], off.state_dict()[k]) for k in windows)


def test_default_is_off():
    from rave_amd import descript_discriminator as DD, discriminator as D, model as M
    for f in (D.MultiScaleSpectralDiscriminator.__init__, DD.MRD.__init__, DD.DescriptDiscriminator.__init__, M.build_v2):
        assert inspect.signature(f).parameters["hip_frontend"].default is False


def test_on_cpu_both_front_ends_are_the_same_composition():
    """The convolutions behind the front ends have no CPU path, so the nets are replaced by the identity: what is compared is
    everything ``hip_frontend`` switches."""
    from rave_amd import descript_discriminator as DD, discriminator as D
    x = R.white_noise((2, 2, 3000), 6)
    on, off = (D.MultiScaleSpectralDiscriminator([512, 128], lambda n_channels: nn.Identity(), n_channels=2, hip_frontend=h)
               for h in (True, False))
    for a, b in zip(on(x), off(x)):
        assert a.shape == b.shape and torch.equal(a, b)
    # the descript front end of today runs its framing on the GPU only: the flag's CPU result against upstream's statements
    mrd = DD.MRD(256, n_channels=2, hip_frontend=True)
    s = torch.stft(x.reshape(-1, 3000), 256, hop_length=64, win_length=256, window=mrd.stft.window, center=True, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True).reshape(2, 2, 129, -1)
    want = torch.view_as_real(s).permute(0, 1, 4, 3, 2).reshape(2, 4, s.shape[-1], 129)       # "b c f t p -> b (c p) t f"
    got = mrd.spectrogram(x)
    assert [tuple(b.shape[-1:]) for b in got] == [(hi - lo,) for lo, hi in mrd.bands]
    assert torch.equal(torch.cat(got, -1), want[..., mrd.bands[0][0]:mrd.bands[-1][1]])


def test_builders_forward_the_flag():
    from rave_amd import descript_discriminator as DD, discriminator as D, model as M
    kw = dict(capacity=16, latent_size=16, disc_capacity=16, spectral_capacity=8)
    for hip in (False, True):
        m = M.build_discrete(hip_frontend=hip, **kw)
        flags = [d.hip_frontend for d in m.discriminator.modules() if isinstance(d, D.MultiScaleSpectralDiscriminator)]
        assert flags == [hip]
        m = M.build_v3(hip_frontend=hip, **kw)
        flags = [d.hip_frontend for d in m.discriminator.modules() if isinstance(d, DD.MRD)]
        assert flags == [hip] * 3


_OVERLAYS = {"mi355x_spectrogram.gin": {"rave_amd.discriminator.MultiScaleSpectralDiscriminator", "rave_amd.discriminator.EncodecConvNet",
                                        "rave_amd.discriminator.CombineDiscriminators", "rave.RAVE"},
             "mi355x_spectrogram_descript.gin": {"rave_amd.descript_discriminator.DescriptDiscriminator", "rave.RAVE"}}


@pytest.mark.parametrize("name", sorted(_OVERLAYS))
def test_overlay_parses_and_binds_existing_names(name):
    """Every binding of the overlay names a constructor argument of an importable class (``rave`` itself is the upstream
    package, not importable here: its one binding is ``discriminator``, checked by the test below where upstream is present)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "rave_amd", "configs", name)).read()
    code = [ln for ln in text.splitlines() if ln.strip() and not ln.lstrip().startswith("#")]
    assert code[0] == "from __gin__ import dynamic_registration"
    imports = [ln.split()[1] for ln in code[1:] if ln.startswith("import ")]
    assert imports and all(importlib.import_module(m) for m in imports if m != "rave")
    bound, target = [], None
    for ln in code[1:]:
        if ln.startswith("import "):
            continue
        head = re.fullmatch(r"([\w.]+):", ln)
        if head:
            target = head.group(1)
            continue
        m = re.fullmatch(r"\s+(\w+) = (.+)", ln)
        if m:
            assert target, ln
            bound.append((target, m.group(1), m.group(2)))
        else:
            assert re.fullmatch(r"\s+(@[\w.]+,|\])", ln), ln          # the lines of a bracketed list
    for target, name_, value in bound:
        mod, cls = target.rsplit(".", 1)
        assert mod in imports
        if mod == "rave":
            assert (cls, name_) == ("RAVE", "discriminator")
        else:
            assert name_ in inspect.signature(getattr(importlib.import_module(mod), cls).__init__).parameters, (target, name_)
    for ref in re.findall(r"@([\w.]+)", "\n".join(code)):
        mod, cls = ref.rsplit(".", 1)
        assert isinstance(getattr(importlib.import_module(mod), cls), type), ref
    assert {t for t, _, _ in bound} == _OVERLAYS[name]
    assert sum((n, v) == ("hip_frontend", "True") for _, n, v in bound) == 1


_GIN_SCRIPT = r"""
import json, os, sys
root, overlay = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "oracle"))
sys.dont_write_bytecode = True
from ref_import import import_reference
rave = import_reference()
import gin, torch
gin.clear_config()
cfg = os.path.join(root, "rave_amd", "configs")
files = ["configs/v2.gin", os.path.join(cfg, "mi355x.gin")] + ([os.path.join(cfg, overlay)] if overlay != "-" else [])
gin.parse_config_files_and_bindings(files, ["CAPACITY = 8", "LATENT_SIZE = 16"])
model = rave.RAVE()                       # upstream's own class, every argument from the parsed .gin files
from rave_amd import descript_discriminator as DD, discriminator as D, spectrogram as S
front = [(type(m).__name__, bool(m.hip_frontend), [s.n_fft for s in m.modules() if isinstance(s, S.Spectrogram)])
         for m in model.discriminator.modules() if isinstance(m, (D.MultiScaleSpectralDiscriminator, DD.MRD))]
conv = sorted({type(m).__module__.split(".")[0] for m in model.discriminator.modules()
               if type(m).__name__ in ("Conv1d", "Conv2d", "Conv2dK1", "PlainConv1d")})
print("RESULT" + json.dumps(dict(cls=type(model).__module__, disc=type(model.discriminator).__module__ + "." +
                                 type(model.discriminator).__name__, front=front, conv_roots=conv,
                                 parts=[type(d).__name__ for d in model.discriminator.discriminators],
                                 sd={k: list(v.shape) for k, v in model.discriminator.state_dict().items()})))
"""


def _build_through_gin(overlay):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _GIN_SCRIPT, root, overlay], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1][6:])


def test_overlays_build_upstreams_model_with_the_flag_on():
    """The documented command lines (v2 + mi355x.gin + an overlay), parsed as tests/test_abi_and_host.py parses mi355x.gin: the
    unmodified ``rave.RAVE`` constructs the drop-in spectral discriminators with ``hip_frontend`` True on every spectral module,
    with the state_dict the builders of rave_amd.model give the same discriminators.  Without an overlay nothing spectral is
    built, which is why binding the flag alone would do nothing.  (Construction only; needs upstream's package.)"""
    from rave_amd import descript_discriminator as DD, discriminator as D
    if not os.path.isdir("/root/reference/rave"):
        pytest.skip("reference tree not present (GPU box)")
    shapes = lambda m: {k: list(v.shape) for k, v in m.state_dict().items()}
    base = _build_through_gin("-")
    assert base["cls"] == "rave.model" and base["front"] == [] and base["parts"] == ["MultiPeriodDiscriminator", "MultiScaleDiscriminator"]

    enc = _build_through_gin("mi355x_spectrogram.gin")
    assert enc["cls"] == "rave.model" and enc["disc"] == "rave_amd.discriminator.CombineDiscriminators"
    assert enc["parts"] == ["MultiScaleDiscriminator", "MultiScaleSpectralDiscriminator"]
    assert enc["front"] == [["MultiScaleSpectralDiscriminator", True, [4096, 2048, 1024, 512, 256]]]
    assert enc["conv_roots"] == ["rave_amd"]
    msd = partial(D.MultiScaleDiscriminator, n_discriminators=3,
                  convnet=partial(D.ConvNet, out_size=1, capacity=8, n_layers=4, stride=4, conv=nn.Conv1d, kernel_size=15))
    mssd = partial(D.MultiScaleSpectralDiscriminator, scales=[4096, 2048, 1024, 512, 256], convnet=partial(D.EncodecConvNet, capacity=32))
    assert enc["sd"] == shapes(D.CombineDiscriminators([msd, mssd], n_channels=1))

    des = _build_through_gin("mi355x_spectrogram_descript.gin")
    assert des["cls"] == "rave.model" and des["disc"] == "rave_amd.descript_discriminator.DescriptDiscriminator"
    assert des["front"] == [["MRD", True, [n]] for n in (2048, 1024, 512)]
    assert des["conv_roots"] == ["rave_amd"]
    assert des["sd"] == shapes(DD.DescriptDiscriminator(n_channels=1))
