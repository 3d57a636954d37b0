#!/usr/bin/env python
"""Writes tests/golden/mel_tiny.pt from the UNMODIFIED reference on the CPU: ``rave.RAVE._mel_encode`` (rave/model.py:238-242)
applied with the test-side ``MelSpectrogram`` of tests/mel_reference.py in float32 (torchaudio itself is not installed where
the fixtures are made), and the reference's mel-sized encoder (configs/hybrid.gin:17-20).

    python tools/make_golden_mel.py            # needs the reference tree (oracle/ref_import.py: RAVE_REFERENCE_ROOT)

Recorded data only: a seeded input (2, 1, 4096) that differs along every axis, the mel tensor, the encoder's state_dict, its
output, a cotangent, every parameter gradient and the sign of every LeakyReLU input (tests/gate_flips.py); and the sorted
state_dict keys and shapes of the spectrogram module.

It also runs the reference's own ``training_step`` once in mel mode and prints what happens:
``encode(return_mb=True)`` hands the MEL tensor to the PQMF (rave/model.py:255-256), so the multiband distance is asked for
a 2048-point reflect-padded STFT of a handful of samples.
"""
import os
import sys
from functools import partial

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 30
CAPACITY, LATENT = 16, 16
MEL = dict(sample_rate=44100, n_fft=2048, win_length=2048, hop_length=256, normalized=True, n_mels=128)


def reference_mel_rave(rave, spectrogram, n_samples_check=None):
    """The reference's RAVE with hybrid.gin's bindings at a small capacity (configs/v2.gin + hybrid.gin transcribed)."""
    from rave import blocks, core, discriminator, pqmf
    dil = [[1, 3, 9], [1, 3, 9], [1, 3, 9], [1, 3]]
    enc = partial(blocks.VariationalEncoder,
                  encoder=partial(blocks.EncoderV2, data_size=128, capacity=CAPACITY, ratios=[2, 2, 2], latent_size=LATENT, n_out=2,
                                  kernel_size=3, dilations=[1]))
    dec = partial(blocks.GeneratorV2, data_size=16, capacity=CAPACITY, ratios=[4, 4, 4, 2], latent_size=LATENT, kernel_size=3,
                  dilations=dil, amplitude_modulation=True, recurrent_layer=partial(blocks.GRU, num_layers=2))
    common = dict(out_size=1, capacity=CAPACITY, n_layers=4, stride=4)
    mpd = partial(discriminator.MultiPeriodDiscriminator, periods=[2, 3, 5, 7, 11],
                  convnet=partial(discriminator.ConvNet, conv=nn.Conv2d, kernel_size=(5, 1), **common))
    msd = partial(discriminator.MultiScaleDiscriminator, n_discriminators=3,
                  convnet=partial(discriminator.ConvNet, conv=nn.Conv1d, kernel_size=15, **common))
    stft = partial(core.MultiScaleSTFT, scales=[2048, 1024, 512, 256, 128], sample_rate=44100, magnitude=True)
    dist = partial(core.AudioDistanceV1, multiscale_stft=stft, log_epsilon=1e-7)
    return rave.RAVE(latent_size=LATENT, sampling_rate=44100, pqmf=partial(pqmf.CachedPQMF, attenuation=100, n_band=16),
                     encoder=enc, decoder=dec, discriminator=partial(discriminator.CombineDiscriminators, discriminators=[mpd, msd]),
                     phase_1_duration=1000000, gan_loss=core.hinge_gan, valid_signal_crop=True,
                     feature_matching_fun=partial(core.mean_difference, norm="L1", relative=True), num_skipped_features=1,
                     audio_distance=dist, multiband_audio_distance=dist, weights={"feature_matching": 20},
                     update_discriminator_every=4, n_channels=1, n_bands=16, spectrogram=spectrogram, input_mode="mel")


def main() -> None:
    from ref_import import import_reference
    from ref_models import attach_optimizers
    import mel_reference as R
    rave = import_reference()
    torch.manual_seed(SEED)
    spec = R.MelSpectrogram(**MEL)
    model = reference_mel_rave(rave, spec)
    x = R.white_noise((2, 1, 4096), 1.0, SEED + 1)
    x[1] *= 0.25                                   # the rows differ in level as well
    with torch.no_grad():
        mel = model._mel_encode(x)                 # rave/model.py:238-242, unmodified
    enc = model.encoder
    from gate_flips import OracleGates
    with OracleGates() as gates:                   # the sign of every LeakyReLU input, in call order (tests/gate_flips.py)
        z = enc(mel)
    dz = torch.randn(z.shape, generator=torch.Generator().manual_seed(SEED + 2))
    z.backward(dz)
    out = dict(seed=SEED, mel_kwargs=MEL, capacity=CAPACITY, latent_size=LATENT, x=x, mel=mel.clone(),
               state_dict={k: v.detach().clone() for k, v in enc.state_dict().items()}, z=z.detach().clone(), dz=dz,
               grads={k: p.grad.clone() for k, p in enc.named_parameters()}, gates=[m.clone() for m in gates.masks],
               spectrogram_keys=sorted((k, tuple(v.shape)) for k, v in spec.state_dict().items()))
    path = os.path.join(ROOT, "tests", "golden", "mel_tiny.pt")
    torch.save(out, path)
    print(path, os.path.getsize(path), "bytes; mel", tuple(mel.shape), "z", tuple(z.shape))

    # ---- the reference's own training_step in mel mode, on a clip of the length the configs train with
    attach_optimizers(model)
    xs = R.white_noise((2, 1, 65536), 0.1, SEED + 3)
    with torch.no_grad():
        _, x_mb = model.encode(xs, return_mb=True)
    print("reference encode(return_mb=True) in mel mode returns x_multiband of shape", tuple(x_mb.shape),
          "(the PQMF of the raw audio would be (2, 16, 4096))")
    try:
        model.training_step(xs.clone(), 1)
        print("reference training_step in mel mode: ran")
    except Exception as e:                          # noqa: BLE001 -- the finding itself
        print(f"reference training_step in mel mode: {type(e).__name__}: {e}")


if __name__ == "__main__":
    main()
