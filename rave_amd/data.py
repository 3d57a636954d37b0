"""GPU-side training data feed (SURVEY.md section 8f "next" #4): the default transform chain of
``rave.dataset.get_dataset`` (rave/dataset.py:218-229,246) -- int16 -> float32, RandomCrop, RandomApply(random
all-pass "phase mangle", p = .8), Dequantize(16) -- for a whole minibatch in one HIP launch (rh_feed_batch_i16_f32)
on PCM that is already resident in HBM (288 GB hold ~900 h of 44.1 kHz mono int16).

The random draws follow the reference's distributions (uniform item / crop point, log-uniform pole frequency in
[20, 2000] Hz at radius .99, U[0,1) dequantisation noise) but not its RNG streams; ``draws`` can be injected, which is
how the parity test compares with scipy.signal.lfilter.  ``load_lmdb_dataset`` reads the reference's on-disk container (the
lmdb / ``AudioExample`` store of scripts/preprocess.py, rave_amd/lmdb_reader.py) into the int16 tensor this class samples from.

``rand_pitch=(lo, hi)`` adds the ``RandomPitch`` that ``rave train --rand_pitch lo,hi`` inserts in front of the crop
(scripts/train.py:67,169, rave/dataset.py:233-236, rave/transforms.py:56-89: scipy.signal.resample_poly of the whole item by
a random ratio up / down, padtype='mean') and ``p_mute`` the ``RandomMute`` of rave/configs/augmentations/mute.gin
(rave/transforms.py:168-177), both in the same launch (feed_pitch_kernel): the polyphase filter is evaluated only
for the samples inside the crop window.  ``RandomGain`` (gain.gin) needs nothing: it returns its input unchanged
(rave/transforms.py:163).  The draws are host logic (``pitch_factors``, ``PitchTable``, ``draw_batch``) and need no GPU.

``normalize=True`` and ``derivative=True`` are the two steps ``rave train --normalize`` / ``--derivative`` put between
Dequantize and the augmentations (scripts/train.py:61-63,160-167): ``normalize_signal`` (rave/dataset.py:196-204,241-242: one
gain per item from the peak over all its channels, capped at ``max_gain_db`` = 30 dB) and the derivator (rave/dataset.py:24-29,
244-245: ``lfilter([.5, -.5], [1], x)``).  They run in a launch pair (feed_pitch_kernel, feed_post_kernel): the chain kernel keeps its
float64 rows and one peak per row in a workspace cached on the feed, a second kernel applies gain and difference in float64 and
rounds once to float32.

``freq_mask=prob`` adds ``FrequencyMasking(prob, max_size)`` (rave/transforms.py:180-195; named, commented out, in
configs/v2_with_augs.gin and reachable through ``dataset.get_dataset.augmentations``): per item, with probability ``prob``, a band
of ``randrange(1, max_size)`` bins at ``randrange(0, 2049 - mask_size)`` is zeroed in scipy.signal.stft(x, nperseg=4096) and the
item rebuilt by scipy.signal.istft.  It is a launch of its own behind the chain (rh_feed_freq_mask_f32, csrc/feed_mask.hip): the
chain writes a float32 buffer cached on the feed, the mask kernel writes the batch; a batch in which no item is masked takes
neither.  The reference masks its float64 item before the final float32 rounding, and RandomMute runs after the mask or before
it, in config order; muting multiplies by 0 or 1 and commutes with the (linear) mask, so masking the chain's float32 output is the
same transform up to one float32 rounding of the mask's input.  ``n_signal`` must be a multiple of 2048 of at least 4096: for any
other length scipy pads the item (10000 samples become 10240) or shortens the window, and the feed refuses.

``resample_to=rate`` adds the ``Resample(sr_dataset, sr)`` that ``get_dataset`` appends right behind Dequantize when the stored
dataset's ``metadata.yaml`` rate (``load_lmdb_dataset``: ``info["sr"]``, the ``sr`` of this class) differs from the run's
(rave/dataset.py:238-239, rave/transforms.py:31-40: torchaudio.functional.resample(x.float(), orig, new) with its defaults).
torchaudio's filter table is built on the host in float32 as torchaudio builds it (``sinc_resample_kernel``) and kept on the
device; a launch between the chain kernel and the normalize / derivative kernel (feed_resample_kernel) applies it to
the cropped rows, float32 taps times float32 samples summed in float64 and rounded once.  ``sample`` then returns
``sinc_resampled_length(n_signal, sr, resample_to)`` samples per row, everything behind Resample (normalize, derivative,
RandomMute, ``freq_mask`` and its length rule) works on those, and the all-pass keeps the dataset's rate, as in the reference.
Resample takes no random draws.

A batch with one of these options in play (a ratio, a muted item, a flag, another rate) is ONE call of the widest entry point,
rh_feed_batch_resample_i16_f32, on the table of ``_row_table``: equal rates switch Resample off, and with neither flag nothing
follows the chain kernel.  Any other batch is rh_feed_batch_i16_f32 on two columns of the same table.

Not built: ``Compress`` / ``RandomCompress`` (sox ``compand`` through torchaudio, rave/transforms.py:114-145): sox can neither
be run here nor modelled against anything.
"""
from __future__ import annotations

import bisect
import math
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib as L
from .ops import _twiddle


def pole_to_z_filter(omega: float, amplitude: float = .9):
    """rave/dataset.py:290-294."""
    z0 = amplitude * np.exp(1j * omega)
    a = [1, -2 * np.real(z0), abs(z0) ** 2]
    b = [abs(z0) ** 2, -2 * np.real(z0), 1]
    return b, a


def random_angle(rng: np.random.Generator, min_f=20, max_f=8000, sr=24000) -> float:
    """rave/dataset.py:283-288."""
    lo, hi = math.log(min_f), math.log(max_f)
    return 2 * math.pi * math.exp(rng.random() * (hi - lo) + lo) / sr


def pitch_factors(max_factor: int, pitch_range: Sequence[float]):
    """RandomPitch._get_factors (rave/transforms.py:63-75): every x / y with 1 <= x, y < max_factor, x != y, inside the range,
    sorted; unreduced duplicates (2/3 and 4/6) are kept, since they shift what ``bisect_left`` picks."""
    factor_list, ratio_list = [], []
    for x in range(1, max_factor):
        for y in range(1, max_factor):
            if x == y:
                continue
            factor = x / y
            if pitch_range[0] <= factor <= pitch_range[1]:
                i = bisect.bisect_left(factor_list, factor)
                factor_list.insert(i, factor)
                ratio_list.insert(i, (x, y))
    return factor_list, ratio_list


def resample_taps(up: int, down: int) -> np.ndarray:
    """The filter of scipy.signal.resample_poly(x, up, down) for a reduced ratio, in float64: up * firwin(2H + 1, 1 / m,
    window=('kaiser', 5.0)) with m = max(up, down), H = 10 m -- a windowed sinc scaled to unit gain at DC."""
    m = max(up, down)
    half = 10 * m
    t = np.arange(-half, half + 1, dtype=np.float64)
    h = np.sinc(t / m) / m * np.kaiser(2 * half + 1, 5.0)
    return up * (h / h.sum())


def resampled_length(length: int, up: int, down: int) -> int:
    return -(-length * up // down)


def sinc_resample_kernel(orig: int, new: int):
    """The filters of torchaudio.functional.resample(x.float(), orig, new) with its defaults (torchaudio 0.12 - 2.x,
    _get_sinc_resample_kernel: sinc_interp_hann, lowpass_filter_width 6, rolloff .99), built as it builds them, with torch CPU ops
    in float32 (the dtype of the waveform): (table, width), ``table`` float32 (n, K), n = new / gcd, K = 2 width + orig / gcd."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * 0.99
    width = math.ceil(6 * o / base)
    idx = torch.arange(-width, width + o, dtype=torch.float32)[None, None] / o
    t = torch.arange(0, -n, -1, dtype=torch.float32)[:, None, None] / n + idx
    t *= base
    t.clamp_(-6, 6)
    window = torch.cos(t * math.pi / 6 / 2) ** 2
    t *= math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t) * (window * (base / o))
    return kernels.reshape(n, 2 * width + o), width


def sinc_resampled_length(length: int, orig: int, new: int) -> int:
    """Samples torchaudio.functional.resample keeps of ``length``: ceil(new * length / orig)."""
    return -(-new * length // orig)


# mirror of kResSpan / kResOut (csrc/feed.hip): what one pass of the resampling kernel stages in LDS
RES_SPAN, RES_OUT = 8192, 6144


class PitchTable:
    """Host side of RandomPitch: the sorted factor / ratio lists and ONE float64 tap table for the distinct reduced ratios
    (``offset[(up, down)]`` is where a ratio's 2H + 1 taps start)."""

    def __init__(self, pitch_range: Sequence[float], p_pitch: float = .5, max_factor: int = 20):
        self.lo, self.hi = float(pitch_range[0]), float(pitch_range[1])
        self.p_pitch = p_pitch
        self.factor_list, self.ratio_list = pitch_factors(max_factor, (self.lo, self.hi))
        if not self.ratio_list:
            raise RuntimeError(f"rand_pitch: no ratio x / y with x, y < {max_factor} inside [{self.lo}, {self.hi}]")
        self.offset, taps, n = {}, [], 0
        for up, down in sorted({self.reduce(r) for r in self.ratio_list}):
            h = resample_taps(up, down)
            self.offset[(up, down)] = n
            taps.append(h)
            n += len(h)
        self.taps = np.concatenate(taps)

    @staticmethod
    def reduce(ratio):
        g = math.gcd(*ratio)
        return ratio[0] // g, ratio[1] // g

    def pick(self, u: float, length: int, n_signal: int):
        """RandomPitch.__call__ (rave/transforms.py:81-87) for the uniform draw ``u``."""
        hi = min(self.hi, length / n_signal)
        i = min(bisect.bisect_left(self.factor_list, u * (hi - self.lo) + self.lo), len(self.factor_list) - 1)
        return self.ratio_list[i]

    def shortest(self, length: int) -> int:
        """The shortest item RandomPitch can return for stored items of ``length`` samples."""
        return min(resampled_length(length, *self.reduce(r)) for r in self.ratio_list)


def draw_batch(rng: np.random.Generator, n_items: int, length: int, batch: int, n_signal: int, sr: int = 44100,
               p_mangle: float = .8, pitch: Optional[PitchTable] = None):
    """The random draws of one minibatch: (items, in_points, angles) and, with ``pitch``, per item None or (up, down).  The
    ratios are drawn after the other three, so without ``pitch`` the generator is consumed exactly as before; a pitched item's
    crop point is drawn again, from [0, n_out - n_signal] (RandomCrop runs on the pitched item)."""
    if n_signal > length:
        raise RuntimeError("GpuBatchFeed: n_signal longer than the stored items")
    items = rng.integers(0, n_items, batch)
    in_points = rng.integers(0, length - n_signal + 1, batch)                           # randint(0, L - n) inclusive
    angles = [random_angle(rng, 20, 2000, sr) if rng.random() < p_mangle else None for _ in range(batch)]
    if pitch is None:
        return items, in_points, angles
    ratios = [None] * batch
    for b in range(batch):
        if rng.random() < pitch.p_pitch:
            ratios[b] = pitch.pick(rng.random(), length, n_signal)
            n_out = resampled_length(length, *pitch.reduce(ratios[b]))
            in_points[b] = rng.integers(0, n_out - n_signal + 1)
    return items, in_points, angles, ratios


MASK_BINS = 2048          # FrequencyMasking: bins a band can hold (the 2049 of nperseg = 4096 without Nyquist) = the hop


def draw_bands(rng: np.random.Generator, batch: int, prob: float, max_size: int):
    """FrequencyMasking's draws (rave/transforms.py:187-191) for one minibatch: per item None (random() >= prob) or
    (freq_idx, mask_size), mask_size = randrange(1, max_size), freq_idx = randrange(0, 2049 - mask_size)."""
    bands = [None] * batch
    for b in range(batch):
        if rng.random() < prob:
            mask_size = int(rng.integers(1, max_size))
            bands[b] = (int(rng.integers(0, MASK_BINS + 1 - mask_size)), mask_size)
    return bands


def check_bands(bands, batch: int):
    """The injected or drawn bands of ``sample``: one (freq_idx, mask_size) or None per item; None when no item is masked."""
    if bands is None:
        return None
    if len(bands) != batch:
        raise RuntimeError(f"GpuBatchFeed: {len(bands)} bands for a batch of {batch}")
    for b, band in enumerate(bands):
        if band is not None and not (len(band) == 2 and band[1] >= 1 and band[0] >= 0 and band[0] + band[1] <= MASK_BINS):
            raise RuntimeError(f"GpuBatchFeed: item {b}: band {tuple(band)} is not (freq_idx >= 0, mask_size >= 1) inside the "
                               f"{MASK_BINS} bins below Nyquist")
    return bands if any(band is not None for band in bands) else None


def check_resample(orig, new):
    """(table, width) of ``sinc_resample_kernel`` for Resample(orig, new), or an error: rates that are not positive integers, or
    a ratio whose filters one pass of the kernel cannot stage (K taps per filter <= kResSpan, n filters <= kResOut)."""
    for rate in (orig, new):
        if isinstance(rate, bool) or not isinstance(rate, (int, np.integer)) or not 1 <= rate < 2 ** 31:
            raise RuntimeError(f"GpuBatchFeed: Resample needs sr and resample_to as positive integer rates, not {orig!r} -> {new!r}")
    orig, new = int(orig), int(new)
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    k = 2 * math.ceil(6 * o / (min(o, n) * 0.99)) + o
    if k > RES_SPAN:
        raise RuntimeError(f"GpuBatchFeed: Resample {orig} -> {new} ({o}/{n}) needs {k} taps per filter, more than kResSpan = {RES_SPAN}")
    if n > RES_OUT:
        raise RuntimeError(f"GpuBatchFeed: Resample {orig} -> {new} ({o}/{n}) needs {n} filters, more than kResOut = {RES_OUT}")
    return sinc_resample_kernel(orig, new)


def check_max_gain_db(max_gain_db) -> float:
    """The gain cap of normalize_signal (rave/dataset.py:196) as a finite float; anything else is an error."""
    if isinstance(max_gain_db, bool) or not isinstance(max_gain_db, (int, float, np.integer, np.floating)) \
            or not math.isfinite(max_gain_db):
        raise RuntimeError(f"GpuBatchFeed: max_gain_db must be a finite number of dB, not {max_gain_db!r}")
    return float(max_gain_db)


# mirror of ``rh_feed_pitch_row`` (include/rave_hip.h)
ROW_DTYPE = np.dtype([("base", np.int64), ("in_point", np.int64), ("mean", np.float64), ("coef", np.float64, 5),
                      ("length", np.int32), ("up", np.int32), ("down", np.int32), ("tap_offset", np.int32),
                      ("mute", np.int32), ("reserved", np.int32)], align=True)


class GpuBatchFeed:
    """``pcm``: int16 tensor (n_items, n_channels, length) on the GPU.  ``sample`` returns a (B, n_channels, n_signal)
    float32 minibatch ready for ``RAVE.training_step``.  ``rand_pitch=(lo, hi)``: RandomPitch(n_signal, [lo, hi], max_factor,
    prob=p_pitch) in front of the crop; ``p_mute``: RandomMute(p_mute) at the end of the chain; ``normalize`` / ``derivative``:
    normalize_signal(x, max_gain_db) and the derivator between Dequantize and RandomMute; ``freq_mask``: FrequencyMasking(freq_mask,
    freq_mask_max_size) on the finished chain, None = off; ``resample_to``: Resample(sr, resample_to) behind Dequantize, None or
    ``sr`` itself = off, otherwise ``sample`` returns (B, n_channels, ceil(resample_to n_signal / sr)) (module docstring)."""

    def __init__(self, pcm: torch.Tensor, sr: int = 44100, seed: int = 0, p_mangle: float = .8, bit_depth: int = 16,
                 rand_pitch: Optional[Sequence[float]] = None, p_pitch: float = .5, max_factor: int = 20, p_mute: float = 0.,
                 normalize: bool = False, derivative: bool = False, max_gain_db: float = 30.,
                 freq_mask: Optional[float] = None, freq_mask_max_size: int = 80, resample_to: Optional[int] = None):
        self.normalize, self.derivative, self.max_gain_db = bool(normalize), bool(derivative), check_max_gain_db(max_gain_db)
        self.workspace = None
        if freq_mask is not None and not 0. <= freq_mask <= 1.:
            raise RuntimeError("GpuBatchFeed: freq_mask must be None or a probability between 0 and 1")
        if not 2 <= freq_mask_max_size <= MASK_BINS + 1:
            raise RuntimeError(f"GpuBatchFeed: freq_mask_max_size must be 2..{MASK_BINS + 1} (mask_size = randrange(1, max_size) bins "
                               f"of the {MASK_BINS} below Nyquist)")
        self.freq_mask, self.freq_mask_max_size = freq_mask, int(freq_mask_max_size)
        self.mask_input = None                      # the chain's output when a batch is masked: float32, cached like ``workspace``
        if pcm.dtype != torch.int16 or pcm.dim() != 3 or not pcm.is_cuda:
            raise RuntimeError("GpuBatchFeed: pcm must be an int16 (items, channels, length) tensor on the GPU")
        if not 0. <= p_mute <= 1.:
            raise RuntimeError("GpuBatchFeed: p_mute must be between 0 and 1")
        self.pcm = pcm.contiguous()
        self.sr, self.p_mangle, self.bit_depth, self.p_mute = sr, p_mangle, bit_depth, p_mute
        self.rng = np.random.default_rng(seed)
        self.gen = torch.Generator(device=pcm.device).manual_seed(seed)
        self.pitch = self.taps = self.means = None
        if rand_pitch is not None:
            if len(rand_pitch) != 2:
                raise RuntimeError("GpuBatchFeed: rand_pitch must be given two floats")     # rave/dataset.py:235
            if not 2 <= max_factor <= 20:
                raise RuntimeError("GpuBatchFeed: max_factor must be 2..20 (the kernel's filters cover up, down <= 19)")
            self.pitch = PitchTable(rand_pitch, p_pitch, max_factor)
            self.taps = torch.from_numpy(self.pitch.taps).to(pcm.device)
            self._means()
        self.resample_to = self.res_taps = self.res_width = None       # None: no Resample (also when the rates are equal)
        if resample_to is not None and resample_to != sr:
            table, self.res_width = check_resample(sr, resample_to)
            self.resample_to, self.res_taps = int(resample_to), table.contiguous().to(pcm.device)

    def _means(self) -> np.ndarray:
        """Mean of every (item, channel) row of int16 / 32767 (resample_poly's padtype='mean'), float64, computed on the device
        once (at construction when ``rand_pitch`` is set: the PCM is static), a few items at a time, and kept on the host for
        the row table."""
        if self.means is None:
            n_items, n_ch, length = self.pcm.shape
            step = max(1, (1 << 24) // (n_ch * length))
            parts = [(self.pcm[i:i + step].to(torch.float32) / 32767.0).to(torch.float64).mean(-1) for i in range(0, n_items, step)]
            self.means = torch.cat(parts).reshape(n_items * n_ch).cpu().numpy()
        return self.means

    def draw(self, batch: int, n_signal: int):
        n_items, _, length = self.pcm.shape
        if self.pitch is not None and self.pitch.shortest(length) < n_signal:
            raise RuntimeError(f"GpuBatchFeed: rand_pitch down to {self.pitch.lo} can shorten the {length}-sample items to "
                               f"{self.pitch.shortest(length)} samples, fewer than n_signal = {n_signal}")
        return draw_batch(self.rng, n_items, length, batch, n_signal, self.sr, self.p_mangle, self.pitch)

    def sample(self, batch: int, n_signal: int, draws=None, noise: Optional[torch.Tensor] = None, mute=None,
               bands=None) -> torch.Tensor:
        """``draws``: (items, in_points, angles) or (items, in_points, angles, ratios), ``ratios[b]`` = None or (up, down) and
        ``in_points[b]`` then counted in resampled samples; ``mute``: optional mask, True = the item is silenced; ``bands``
        (with ``freq_mask``): per item None or (freq_idx, mask_size).  Like ``mute``, the bands are drawn only when the
        ``draws`` are; they are drawn last, and only with ``freq_mask`` set: a feed without it consumes its generator exactly as
        before."""
        if self.freq_mask is None and bands is not None:
            raise RuntimeError("GpuBatchFeed: bands given to a feed built without freq_mask")
        n_out = n_signal if self.resample_to is None else sinc_resampled_length(n_signal, self.sr, self.resample_to)
        if self.freq_mask is not None and (n_out < 2 * MASK_BINS or n_out % MASK_BINS):
            what = "n_signal" if self.resample_to is None else f"the {n_out} samples Resample makes of n_signal = {n_signal}"
            raise RuntimeError(f"GpuBatchFeed: freq_mask needs {what} to be a multiple of {MASK_BINS} of at least {2 * MASK_BINS}, "
                               f"not {n_out} (scipy.signal.stft would pad the item or shorten its window)")
        drawn = draws is None
        if drawn:
            draws = self.draw(batch, n_signal)
            if mute is None and self.p_mute > 0:
                mute = self.rng.random(batch) < self.p_mute
        if self.freq_mask is not None and bands is None and drawn:
            bands = draw_bands(self.rng, batch, self.freq_mask, self.freq_mask_max_size)
        bands = check_bands(bands, batch)
        items, in_points, angles = draws[:3]
        ratios = draws[3] if len(draws) > 3 else None
        n_ch, dev = self.pcm.shape[1], self.pcm.device
        rows = batch * n_ch
        if noise is None:
            noise = torch.rand(rows, n_signal, device=dev, generator=self.gen)
        noise = noise.to(dev, torch.float32).contiguous()
        out = torch.empty(batch, n_ch, n_out, device=dev, dtype=torch.float32)
        dst = out                                   # where the chain writes: the batch itself unless a mask launch follows
        if bands is not None:
            if self.mask_input is None or self.mask_input.numel() < out.numel():     # regrown only when rows x n_signal grows
                self.mask_input = torch.empty(out.numel(), device=dev, dtype=torch.float32)
            dst = self.mask_input
        table = self._row_table(items, in_points, angles, ratios, mute)
        pitched = ratios is not None and any(r is not None for r in ratios)
        muted = mute is not None and any(mute)
        resample, post = self.resample_to is not None, self.normalize or self.derivative
        if not (pitched or muted or post or resample):
            off_d = torch.from_numpy(table["base"] + table["in_point"]).to(dev)
            coef_d = torch.from_numpy(np.ascontiguousarray(table["coef"])).to(dev)
            L.check(L.lib.rh_feed_batch_i16_f32(L.ptr(self.pcm), L.ptr(off_d), L.ptr(coef_d), L.ptr(noise), rows, n_signal,
                                                self.bit_depth, L.ptr(dst), L.stream()), "feed_batch")
            return self._mask(dst, out, bands)
        # every other batch is one call of the widest entry point: equal rates switch its Resample stage off, and with neither
        # flag set nothing follows the chain kernel; ``what`` names the entry point such a call reduces to, as its messages do
        new = self.resample_to if resample else self.sr
        what = "feed_batch_resample" if resample else "feed_batch_post" if post else "feed_batch_pitch"
        ws, ws_bytes = None, 0
        if resample or post:
            need = L.lib.rh_feed_resample_workspace_bytes(rows, n_signal, self.sr, new)
            if need < 0:
                raise RuntimeError(f"GpuBatchFeed: Resample {self.sr} -> {self.resample_to} of {n_signal} samples leaves int32")
            if self.workspace is None or self.workspace.numel() * 8 < need:            # regrown only when it must grow
                self.workspace = torch.empty(need // 8, device=dev, dtype=torch.float64)
            ws, ws_bytes = self.workspace, self.workspace.numel() * 8
        table_d = torch.from_numpy(table.view(np.uint8)).to(dev)
        L.check(L.lib.rh_feed_batch_resample_i16_f32(L.ptr(self.pcm), self.pcm.numel(), table.ctypes.data, L.ptr(table_d),
                                                     L.ptr(self.taps), 0 if self.taps is None else self.taps.numel(), L.ptr(noise),
                                                     rows, n_signal, self.bit_depth, n_ch, int(self.normalize), self.max_gain_db,
                                                     int(self.derivative), self.sr, new, L.ptr(self.res_taps),
                                                     self.res_taps.numel() if resample else 0, self.res_width if resample else 0,
                                                     L.ptr(ws), ws_bytes, L.ptr(dst), L.stream()), what)
        return self._mask(dst, out, bands)

    def _row_table(self, items, in_points, angles, ratios, mute) -> np.ndarray:
        """The ``ROW_DTYPE`` table of a batch, a row per (item, channel): filled per item, repeated over the channels; only
        ``base`` and ``mean`` differ between the rows of an item.  An item without an angle keeps NaN coefficients (the all-pass
        missed it), one without a ratio 1/1 and the mean 0, which the kernel then never reads."""
        _, n_ch, length = self.pcm.shape
        batch = len(angles)
        coef = np.full((batch, 5), np.nan)
        for b, angle in enumerate(angles):
            if angle is not None:
                bb, aa = pole_to_z_filter(angle, .99)
                coef[b] = (bb[0], bb[1], bb[2], aa[1], aa[2])
        it = np.zeros(batch, dtype=ROW_DTYPE)
        it["in_point"] = np.asarray(in_points, dtype=np.int64)[:batch]
        it["coef"] = coef
        it["length"] = length
        it["up"] = it["down"] = 1
        if mute is not None:
            it["mute"] = np.asarray(mute, dtype=bool)[:batch]
        pitched = [b for b in range(batch) if ratios[b] is not None] if ratios is not None else []
        if pitched:
            it["up"][pitched] = [int(ratios[b][0]) for b in pitched]
            it["down"][pitched] = [int(ratios[b][1]) for b in pitched]
            it["tap_offset"][pitched] = [self._tap_offset(ratios[b]) for b in pitched]
        table = np.repeat(it, n_ch)
        row = np.repeat(np.asarray(items, dtype=np.int64)[:batch] * n_ch, n_ch) + np.arange(batch * n_ch) % n_ch
        table["base"] = row * length
        if pitched:
            rows = (np.array(pitched)[:, None] * n_ch + np.arange(n_ch)).ravel()        # the table rows of the pitched items
            table["mean"][rows] = self._means()[row[rows]]
        return table

    def _mask(self, chain_out: torch.Tensor, out: torch.Tensor, bands) -> torch.Tensor:
        """FrequencyMasking of the finished chain: ``chain_out`` (the cached buffer) -> ``out``, every channel of an item with the
        item's band; nothing to do (``chain_out`` is ``out``) when no item of the batch is masked."""
        if bands is None:
            return out
        batch, n_ch, n_signal = out.shape
        table = np.zeros((batch, n_ch, 2), dtype=np.int32)                             # rows x {first_bin, n_bins}; 0 bins = copy
        for b, band in enumerate(bands):
            if band is not None:
                table[b] = (int(band[0]), int(band[1]))
        table_d = torch.from_numpy(table).to(out.device)
        L.check(L.lib.rh_feed_freq_mask_f32(L.ptr(chain_out), L.ptr(out), L.ptr(table_d), batch * n_ch, n_signal,
                                            L.ptr(_twiddle(2 * MASK_BINS, out.device)), L.stream()), "feed_freq_mask")
        return out

    def _tap_offset(self, ratio) -> int:
        """Where the taps of ``ratio`` start in the table; 0 (never read) for a ratio that reduces to 1/1.  A ratio outside 1..19
        or outside the table of this feed is left to the entry point's own checks, which refuse it."""
        if self.pitch is None or min(ratio) < 1:
            return -1
        return self.pitch.offset.get(PitchTable.reduce(ratio), 0 if ratio[0] == ratio[1] else -1)


def load_lmdb_dataset(db_path: str, n_channels: Optional[int] = None, audio_key: str = "waveform", device=None,
                      max_items: Optional[int] = None):
    """The dataset ``scripts/preprocess.py`` wrote (``db_path/data.mdb`` + ``db_path/metadata.yaml``) as ONE int16 tensor
    (items, channels, length) -- what ``rave.dataset.AudioDataset`` (rave/dataset.py:33-84) serves item by item:
    every key of the environment in cursor order, ``np.frombuffer(ae.buffers['waveform'].data, int16).reshape(channels, -1)``.
    Returns (pcm, info): ``pcm`` on ``device`` (None: host memory, pinned when a GPU is present) for ``GpuBatchFeed``;
    ``info`` = dict(sr, channels, lazy, n_items, length, dropped).  Chunks are of equal length by construction
    (scripts/preprocess.py:83-98 drops an incomplete tail); should a store hold other lengths, the items that differ from the
    most common length are dropped and counted.  ``lazy`` stores (file paths decoded by ffmpeg on the fly, rave/dataset.py:
    87-170) hold no PCM and are refused."""
    import os
    import yaml
    from .lmdb_reader import LmdbReader, parse_audio_example
    info = {}
    meta_path = os.path.join(db_path, "metadata.yaml")
    if os.path.exists(meta_path):
        with open(meta_path) as f:
            info = yaml.safe_load(f) or {}
    if info.get("lazy"):
        raise RuntimeError("rave_amd.data.load_lmdb_dataset: lazy dataset (audio decoded on the fly by ffmpeg): no PCM in the store")
    ch = int(n_channels or info.get("channels", 1))
    # two passes, one copy (a list of per-item copies + np.stack + pin_memory held the dataset three times): the first
    # pass only counts the items and their lengths, the second writes each item straight into its row of ONE preallocated
    # (pinned, when a GPU is present and the data stays on the host) int16 tensor
    def items(db):
        n = 0
        for k, v in db.items():
            buffers, _ = parse_audio_example(v)
            if audio_key not in buffers:
                continue
            raw = buffers[audio_key]["data"]
            if len(raw) % (2 * ch):
                raise RuntimeError(f"load_lmdb_dataset: item {k!r} holds {len(raw)} bytes, not a whole number of {ch}-channel int16 frames")
            yield raw
            n += 1
            if max_items is not None and n >= max_items:
                return

    with LmdbReader(db_path) as db:
        lengths = [len(raw) // (2 * ch) for raw in items(db)]
        if not lengths:
            raise RuntimeError(f"load_lmdb_dataset: no '{audio_key}' buffers found under {db_path}")
        common = max(set(lengths), key=lengths.count)
        n_keep = lengths.count(common)
        pcm = torch.empty(n_keep, ch, common, dtype=torch.int16, pin_memory=(device is None and torch.cuda.is_available()))
        view = pcm.numpy()
        row = 0
        for raw in items(db):
            if len(raw) // (2 * ch) == common:
                view[row] = np.frombuffer(raw, dtype=np.int16).reshape(ch, -1)
                row += 1
    if device is not None:
        pcm = pcm.to(device)
    keep, chunks = range(n_keep), lengths
    out = dict(sr=int(info.get("sr", 44100)), channels=ch, lazy=False, n_items=len(keep), length=common,
               dropped=len(chunks) - len(keep))
    return pcm, out
