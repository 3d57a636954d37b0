"""rave_amd -- MI355X (gfx950) native hot path of RAVE: PQMF filterbank + Conv1d residual stacks.

``rave_amd.cc`` mirrors the ``cached_conv`` operator API the reference's blocks are written
against, ``rave_amd.pqmf`` / ``rave_amd.blocks`` / ``rave_amd.discriminator``
mirror the reference's leaf modules with identical constructor signatures and state_dict
layouts; all arithmetic runs in hand-written HIP kernels behind the C ABI of
``include/rave_hip.h`` (``rave_amd/librave_hip.so``).
"""
__version__ = "0.1.0"


def __getattr__(name):
    # rave_amd.MelSpectrogram (torchaudio.transforms.MelSpectrogram's stand-in, rave_amd/mel.py), resolved on first use: importing
    # the package itself stays free of torch (rave_amd.build runs before anything else exists)
    if name == "MelSpectrogram":
        from .mel import MelSpectrogram
        return MelSpectrogram
    if name == "DifferentiableMelSpectrogram":      # the same with a gradient, for losses.SpectralDistance(mel=n)
        from .mel import DifferentiableMelSpectrogram
        return DifferentiableMelSpectrogram
    if name == "Spectrogram":           # torchaudio.transforms.Spectrogram's stand-in (rave_amd/spectrogram.py)
        from .spectrogram import Spectrogram
        return Spectrogram
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
