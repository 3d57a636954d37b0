"""Stand-in for ``rave.model.RAVE`` (rave/model.py:133-424) used where the reference package
cannot travel (the GPU box): same sub-module names (``pqmf``, ``encoder``, ``decoder``,
``discriminator`` -> identical state_dict keys for the hot path) and a ``training_step`` that
restates rave/model.py:288-413 statement by statement, driving the HIP drop-in modules.

With the reference installed nothing here is needed: ``rave.model.RAVE`` itself runs on the
drop-ins.  This file is host-side plumbing, not the product.
"""
from __future__ import annotations

from functools import partial
from typing import Callable, Dict, Optional

import torch
import torch.nn as nn

from . import blocks, cc, descript_discriminator, discriminator, losses, pqmf, quantization

_default_loss_weights = {
    "audio_distance": 1.,
    "multiband_audio_distance": 1.,
    "adversarial": 1.,
    "feature_matching": 20,
}


def _loss_combine_fused() -> bool:
    """RH_LOSS_COMBINE=0: the generator loss as the reference's chain of scalar ATen operations (same bits)."""
    import os
    return os.environ.get("RH_LOSS_COMBINE", "1") != "0"


def _pqmf_encode(pq, x: torch.Tensor):
    """rave/model.py:116-122."""
    batch_size = x.shape[:-2]
    x_multiband = x.reshape(-1, 1, x.shape[-1])
    x_multiband = pq(x_multiband)
    return x_multiband.reshape(*batch_size, -1, x_multiband.shape[-1])


def valid_signal_crop(x: torch.Tensor, left_rf, right_rf):
    """rave/core.py:220-225: drop the samples the receptive field does not fully cover (in band samples: the
    receptive field is measured in audio samples, ``dim`` = the multiband channel count)."""
    dim = x.shape[1]
    x = x[..., int(left_rf) // dim:]
    if int(right_rf):
        x = x[..., :-int(right_rf) // dim]
    return x


def _pqmf_decode(pq, x: torch.Tensor, batch_size, n_channels: int):
    """rave/model.py:125-130."""
    x = x.reshape(x.shape[0] * n_channels, -1, x.shape[-1])
    x = pq.inverse(x)
    return x.reshape(*batch_size, n_channels, -1)


class RAVE(nn.Module):
    def __init__(self, latent_size, sampling_rate, encoder, decoder, discriminator, phase_1_duration,
                 gan_loss, valid_signal_crop, feature_matching_fun, num_skipped_features,
                 audio_distance: Callable[[], nn.Module], multiband_audio_distance: Callable[[], nn.Module],
                 n_bands: int = 16, weights: Optional[Dict[str, float]] = None,
                 pqmf: Optional[Callable[[], nn.Module]] = None, update_discriminator_every: int = 2,
                 n_channels: int = 1, spectrogram: Optional[nn.Module] = None, input_mode: str = "pqmf",
                 output_mode: str = "pqmf", latent_analysis: bool = False):
        super().__init__()
        # rave/model.py:168-175.  "mel" (configs/hybrid.gin, v2_with_augs.gin) feeds the encoder log1p of `spectrogram`; the
        # raw-waveform modes are not built
        if input_mode not in ("pqmf", "mel", "raw") or output_mode not in ("pqmf", "raw"):
            raise ValueError(f"RAVE: input_mode {input_mode!r} / output_mode {output_mode!r}")
        for which, mode in (("input_mode", input_mode), ("output_mode", output_mode)):
            if mode == "raw":
                raise NotImplementedError(f'rave_amd RAVE: {which} = "raw" is not built (the raw-waveform configs)')
        if input_mode == "mel" and spectrogram is None:
            raise ValueError('RAVE: input_mode = "mel" needs `spectrogram`')
        self.pqmf = pqmf(n_channels=n_channels)
        self.spectrogram = spectrogram   # (None is a plain attribute: the default model keeps its state_dict keys)
        self.input_mode = input_mode
        self.output_mode = output_mode
        self.encoder = encoder(n_channels=n_channels)
        self.decoder = decoder(n_channels=n_channels)
        self.discriminator = discriminator(n_channels=n_channels)
        self.audio_distance = audio_distance()
        self.multiband_audio_distance = multiband_audio_distance()
        self.gan_loss = gan_loss
        self.latent_size = latent_size
        self.warmup = phase_1_duration
        self.weights = dict(_default_loss_weights)
        self.weights.update(weights or {})
        self.warmed_up = False
        self.sr = sampling_rate
        self.valid_signal_crop = valid_signal_crop
        self.n_channels = n_channels
        self.feature_matching_fun = feature_matching_fun
        self.num_skipped_features = num_skipped_features
        self.update_discriminator_every = update_discriminator_every
        self.beta_factor = 1.
        self._beta_dev = None          # 0-d device copy of beta_factor read by the recorded (hipGraph) step
        self.register_buffer("receptive_field", torch.tensor([0, 0]).long())
        # rave/model.py:196-198: the export-time analysis buffers validation_epoch_end fills.  Opt-in: without the keyword the
        # module tree and state_dict are what they were before the analysis existed
        self.latent_analysis = bool(latent_analysis)
        if self.latent_analysis:
            self.register_buffer("latent_pca", torch.eye(latent_size))
            self.register_buffer("latent_mean", torch.zeros(latent_size))
            self.register_buffer("fidelity", torch.zeros(latent_size))
        self.logged: Dict[str, torch.Tensor] = {}
        self._opts = None
        self._gen_sched = None
        self._prep = None
        # OPT-IN (default off = the reference's exact work per step): skip gradient work
        # whose result the reference computes and then discards -- on generator steps the discriminator's weight
        # gradients (dis_opt.zero_grad() runs before they could be used), on discriminator steps everything behind
        # y_raw / x_raw (gen_opt.zero_grad() discards it).  Parameter trajectories are identical.
        self.skip_dead_grads = False

    def beta_device(self, device) -> torch.Tensor:
        """0-d device tensor holding ``beta_factor`` (created once, updated in place: see training_step)."""
        if self._beta_dev is None or self._beta_dev.device != device:
            self._beta_dev = torch.full((), float(self.beta_factor), device=device, dtype=torch.float32)
        elif not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            self._beta_dev.fill_(float(self.beta_factor))
        return self._beta_dev

    def prepare_weights(self, with_discriminator: bool = False, reuse: bool = False):
        """Refresh weight norm + packed weights of every conv in two launches (see rave_amd/prep.py);
        pair with release_weights().  training_step does this itself.  ``reuse=True``: inference forwards -- keep the
        packed operands while no parameter changed (rave_amd.prep.WeightPrep.run)."""
        from .prep import WeightPrep
        if self._prep is None:
            self._prep = (WeightPrep(nn.ModuleList([self.encoder, self.decoder])), WeightPrep(self.discriminator))
        self._prep[0].run(reuse)
        if with_discriminator:
            self._prep[1].run(reuse)

    def set_phase_flags_eagerly(self) -> None:
        """Read every buffer-derived host flag once outside a capture (so that a following capture finds them cached
        with the CURRENT buffer values) and push the warm-up state to the blocks."""
        from .blocks import host_flag
        self.encoder.set_warmed_up(self.warmed_up)
        self.decoder.set_warmed_up(self.warmed_up)
        for mod in self.modules():
            for name in ("enabled", "inited"):
                if torch.is_tensor(getattr(mod, name, None)):
                    host_flag(mod, name)

    def release_weights(self):
        if self._prep is not None:
            self._prep[0].release()
            self._prep[1].release()

    # ---- rave/model.py:226-236
    def configure_optimizers(self, capturable: bool = False):
        """``capturable``: step counters and learning rates live on the device, so that the optimizer step can be
        recorded into a hipGraph (GraphedTrainingStep); same update."""
        gen_p = list(self.encoder.parameters()) + list(self.decoder.parameters())
        dis_p = list(self.discriminator.parameters())
        # same optimiser and hyper-parameters as the reference; on the GPU PyTorch's single-kernel ("fused")
        # implementation of the same update replaces the default multi-pass foreach one
        fused = all(p.is_cuda for p in gen_p + dis_p)
        lr_g, lr_d = 1e-3, 1e-4
        kw = {}
        if capturable:
            dev = gen_p[0].device
            lr_g, lr_d = torch.tensor(lr_g, device=dev), torch.tensor(lr_d, device=dev)
            kw["capturable"] = True
        import os
        if fused and os.environ.get("RH_ADAM", "1") != "0":
            # the same update on one HIP kernel pass at HBM speed (rave_amd/optim.py; RH_ADAM=0: torch's fused kernel)
            from .optim import FusedAdam
            gen_opt = FusedAdam(gen_p, lr_g, (.5, .9))
            dis_opt = FusedAdam(dis_p, lr_d, (.5, .9))
        else:
            gen_opt = torch.optim.Adam(gen_p, lr_g, (.5, .9), fused=fused, **kw)
            dis_opt = torch.optim.Adam(dis_p, lr_d, (.5, .9), fused=fused, **kw)
        self._opts = (gen_opt, dis_opt)
        # rave/model.py:234-236: the generator learning rate decays linearly to 0.1x over phase 1
        self._gen_sched = LinearLR(gen_opt, start_factor=1.0, end_factor=0.1, total_iters=self.warmup)
        return gen_opt, dis_opt

    def lr_schedulers(self):
        self.optimizers()
        return self._gen_sched

    def on_train_batch_end(self, outputs=None, batch=None, batch_idx=None) -> None:
        """rave/model.py:272-274 (Lightning hook; a driver loop calls it after every training_step)."""
        self.lr_schedulers().step()

    def optimizers(self):
        if self._opts is None:
            self.configure_optimizers()
        return self._opts

    # ---- rave/model.py:244-270
    def _mel_encode(self, x: torch.Tensor):
        """rave/model.py:238-242: ``log1p(spectrogram(x)[..., :-1])`` as (*batch, n_channels * n_mels, frames).  The drop-in
        module does all of it in one HIP launch (rave_amd.mel.MelSpectrogram.log_mel); any other callable runs the reference's
        statements.  Never requires grad: nothing trainable is upstream of the audio."""
        batch_size = x.shape[:-2]
        with torch.no_grad():
            if hasattr(self.spectrogram, "log_mel"):
                m = self.spectrogram.log_mel(x)
            else:
                m = torch.log1p(self.spectrogram(x)[..., :-1])
        return m.reshape(*batch_size, -1, m.shape[-1])

    def encode(self, x, return_mb: bool = False):
        """In mel mode ``return_mb`` gives the PQMF of the RAW audio: the reference (rave/model.py:255-256) hands the mel tensor
        to the PQMF there, which its own training_step cannot run with; the raw-mode branch of the
        same function shows the intent."""
        x_mb = _pqmf_encode(self.pqmf, x) if (self.input_mode == "pqmf" or return_mb) else None
        z = self.encoder(x_mb if self.input_mode == "pqmf" else self._mel_encode(x))
        if return_mb:
            return z, x_mb
        return z

    def decode(self, z):
        batch_size = z.shape[:-2]
        y = self.decoder(z)
        return _pqmf_decode(self.pqmf, y, batch_size=batch_size, n_channels=self.n_channels)

    def forward(self, x):
        z = self.encode(x, return_mb=False)
        z = self.encoder.reparametrize(z)[0]
        return self.decode(z)

    def _fused_feature_matching(self, features):
        """The feature-matching distance of rave/model.py:359-372 in one HIP pass over the unsplit feature maps
        (rave_amd.ops.feature_matching) when the configured function is ``mean_difference(norm="L1"[, relative])`` on GPU
        tensors; None -> the generic per-map formulation runs.  ``RH_FM_FUSED=0`` disables."""
        import os
        fun = self.feature_matching_fun
        if os.environ.get("RH_FM_FUSED", "1") == "0" or not isinstance(fun, partial) or fun.func is not losses.mean_difference or fun.args:
            return None
        kw = dict(fun.keywords)
        if kw.pop("norm", "L1") != "L1":
            return None
        relative = bool(kw.pop("relative", False))
        if kw:
            return None
        maps, weights = [], []
        for scale in features:
            used = list(scale[self.num_skipped_features:])
            if not used:
                return None
            for f in used:
                if not (torch.is_tensor(f) and f.is_cuda and f.dtype == torch.float32 and f.shape[0] % 2 == 0 and f.numel() > 0):
                    return None
                maps.append(f)
                weights.append(1.0 / (len(used) * len(features)))
        if not maps:
            return None
        from . import ops
        total = None
        for i in range(0, len(maps), 80):          # one kernel-argument table holds 80 maps (descript: > 100 per step)
            part = ops.feature_matching(maps[i:i + 80], weights[i:i + 80], relative)
            total = part if total is None else total + part
        return total

    def _fused_gan_losses(self, features):
        """(loss_dis, loss_adv, pred_real, pred_fake) of rave/model.py:354-376 in one HIP call over the last (score) map of every
        discriminator head (rave_amd.ops.gan_losses: two launches forward, one backward) when ``gan_loss`` is one of
        losses.hinge_gan / ls_gan / nonsaturating_gan -- the function itself, a ``partial`` of it without arguments, or a wrapper
        that carries its ``gan_mode`` attribute -- and every score map is a float32 GPU tensor with an even, dense batch
        dimension; None -> the per-head loop runs.  ``RH_GAN_LOSS=0`` disables."""
        fn = self.gan_loss
        if isinstance(fn, partial) and not fn.args and not fn.keywords:
            fn = fn.func
        mode = getattr(fn, "gan_mode", None)
        if not isinstance(mode, int) or mode not in (0, 1, 2):
            return None
        from . import ops
        if not ops.gan_loss_on():
            return None
        heads = []
        for scale in features:
            s = scale[-1] if len(scale) else None
            if not (torch.is_tensor(s) and s.is_cuda and s.dtype == torch.float32 and ops._dense_batch_major(s)):
                return None
            heads.append(s)
        if not heads:
            return None
        total = None
        for i in range(0, len(heads), 80):         # one kernel-argument table holds 80 heads
            part = ops.gan_losses(heads[i:i + 80], mode)
            total = part if total is None else tuple(a + b for a, b in zip(total, part))
        return total

    @staticmethod
    def _join_side() -> None:
        """The weight-gradient side stream (rave_amd.ops._OnSide) is joined by a callback at the end of every backward pass;
        joining again before the optimizer reads the gradients is a no-op then, and the safety net when a pass ended
        without running its callbacks."""
        from . import ops
        ops.join_side_streams()

    def split_features(self, features):
        """rave/model.py:276-286."""
        feature_real, feature_fake = [], []
        for scale in features:
            true, fake = zip(*map(lambda x: torch.split(x, x.shape[0] // 2, 0), scale))
            feature_real.append(true)
            feature_fake.append(fake)
        return feature_real, feature_fake

    # ---- rave/model.py:288-424
    def training_step(self, batch, batch_idx, eps: Optional[torch.Tensor] = None, grad_sync=None,
                      capture_safe: bool = False, grad_begin=None):
        """``eps`` injects the reparametrisation noise (parity runs); ``grad_begin(optimizer_index)`` is called right
        after that optimizer's ``zero_grad()`` and ``grad_sync(optimizer_index)`` between backward and optimizer.step
        (data-parallel gradient averaging: rave_amd.ddp.GradReducer.begin / finish).
        ``capture_safe``: no host synchronisation inside the step (the reference's ``reg.item()`` test,
        rave/model.py:393, becomes "always add the regulariser" -- identical whenever it is non-zero, i.e. always
        for the variational encoder), so that the step can be recorded into a hipGraph."""
        gen_opt, dis_opt = self.optimizers()
        # all weight-normalised convs: weight norm + MFMA repack refreshed in two launches (plumbing;
        # the reference's weight_norm pre-hooks do the same work layer by layer)
        if batch.is_cuda:
            # a fresh zeroed pool of range slots for this step's activations (ops.range_reset: one fill launch; recorded into
            # a hipGraph it re-zeroes them at every replay)
            from . import ops as _ops
            _ops.range_reset(batch.device)
            # the discriminator only runs (and only then normalises its weights) in phase 2
            self.prepare_weights(with_discriminator=bool(self.warmed_up))
        x_raw = batch
        x_raw.requires_grad = True
        batch_size = x_raw.shape[:-2]
        self.encoder.set_warmed_up(self.warmed_up)
        self.decoder.set_warmed_up(self.warmed_up)

        x_multiband = _pqmf_encode(self.pqmf, x_raw)                   # (= self.encode(x_raw, return_mb=True), unrolled)
        rf = (0, 0)
        if self.valid_signal_crop:                                     # rave/model.py:321-329
            # the buffer is read on the host (as the reference does); while a hipGraph is being recorded the value
            # seen by the preceding eager iterations is used (it only changes in validation)
            if not (batch.is_cuda and torch.cuda.is_current_stream_capturing()):
                self._rf_host = tuple(int(v) for v in self.receptive_field.tolist())
            rf = getattr(self, "_rf_host", (0, 0))
        x_mb_loss = valid_signal_crop(x_multiband, rf[0], rf[1]) if rf[0] + rf[1] else x_multiband
        # mel mode: only the encoder sees the mel tensor, the multiband distance keeps the PQMF of the raw audio (see encode)
        z = self.encoder(x_multiband if self.input_mode == "pqmf" else self._mel_encode(x_raw))
        z, reg = self.encoder.reparametrize(z, eps)[:2]

        y = self.decoder(z)
        y_multiband = y[..., :x_multiband.shape[-1]]
        if rf[0] + rf[1]:
            y_multiband = valid_signal_crop(y_multiband, rf[0], rf[1])
        x_multiband = x_mb_loss

        # the generator loss terms as (value, first factor): on the GPU the products and the weighted sum of
        # rave/model.py:336-344, 392-412 are ONE launch each way (ops.loss_combine, same bits as the ATen chain below)
        terms = {}
        # Round 5: the multiband distance runs BESIDE the PQMF synthesis and the fullband distance, on the stream the
        # weight-gradient branch uses later in the pass (idle until then; still two streams in the recorded graph).  autograd
        # runs a node's backward on the stream its forward ran on, so the two distances overlap in both directions: 9.74-9.75 ms
        # per step against 9.95-10.01 in three alternated pairs (profiles/round5_ab_knobs_and_negative_results.txt); same bits
        # (no atomics anywhere).  RH_LOSS_SIDE_STREAM=0 / RH_BWD_SIDE_STREAM=0: one stream.
        import os
        loss_side = None
        if batch.is_cuda and os.environ.get("RH_LOSS_SIDE_STREAM", "1") != "0":
            from . import ops
            loss_side = ops._side_stream(batch.device) if ops._side_enabled() else None
        if loss_side is not None:
            loss_side.wait_stream(torch.cuda.current_stream(batch.device))
            with torch.cuda.stream(loss_side):
                multiband_distance = self.multiband_audio_distance(x_multiband, y_multiband)
            for t_ in (x_multiband, y_multiband):
                t_.record_stream(loss_side)
            # the distances were allocated from the side stream's pool and are consumed on the compute stream (loss_combine)
            for v_ in multiband_distance.values():
                if torch.is_tensor(v_):
                    v_.record_stream(torch.cuda.current_stream(batch.device))
        else:
            multiband_distance = self.multiband_audio_distance(x_multiband, y_multiband)
        for k, v in multiband_distance.items():
            terms[f"multiband_{k}"] = (v, self.weights["multiband_audio_distance"])
        y_raw = _pqmf_decode(self.pqmf, y, batch_size=batch_size, n_channels=self.n_channels)
        y_raw = y_raw[..., :x_raw.shape[-1]]
        fullband_distance = self.audio_distance(x_raw, y_raw)
        if loss_side is not None:
            torch.cuda.current_stream(batch.device).wait_stream(loss_side)
        for k, v in fullband_distance.items():
            terms[f"fullband_{k}"] = (v, self.weights["audio_distance"])

        feature_matching_distance = 0.
        dis_step = bool(self.warmed_up) and not (batch_idx % self.update_discriminator_every)
        frozen = []
        if self.warmed_up:
            if self.skip_dead_grads and dis_step:
                xy = torch.cat([x_raw.detach(), y_raw.detach()], 0)
            else:
                xy = torch.cat([x_raw, y_raw], 0)
            if self.skip_dead_grads and not dis_step:
                frozen = [q for q in self.discriminator.parameters() if q.requires_grad]
            try:
                for q in frozen:
                    q.requires_grad_(False)
                features = self.discriminator(xy)
            finally:
                for q in frozen:
                    q.requires_grad_(True)
            feature_real, feature_fake = self.split_features(features)
            loss_dis = 0
            loss_adv = 0
            pred_real = 0
            pred_fake = 0
            fused_fm = self._fused_feature_matching(features)
            fused_gan = self._fused_gan_losses(features)
            for scale_real, scale_fake in zip(feature_real, feature_fake):
                if fused_fm is None:
                    current = sum(map(self.feature_matching_fun,
                                      scale_real[self.num_skipped_features:],
                                      scale_fake[self.num_skipped_features:])) / len(scale_real[self.num_skipped_features:])
                    feature_matching_distance = feature_matching_distance + current
                if fused_gan is None:
                    _dis, _adv = self.gan_loss(scale_real[-1], scale_fake[-1])
                    pred_real = pred_real + scale_real[-1].detach().mean()       # rave/model.py:372-373 (logged only)
                    pred_fake = pred_fake + scale_fake[-1].detach().mean()
                    loss_dis = loss_dis + _dis
                    loss_adv = loss_adv + _adv
            if fused_gan is not None:
                loss_dis, loss_adv, pred_real, pred_fake = fused_gan
            feature_matching_distance = fused_fm if fused_fm is not None else feature_matching_distance / len(feature_real)
        else:
            loss_dis = torch.zeros((), device=x_raw.device, dtype=x_raw.dtype)     # (no host-to-device copy)
            loss_adv = torch.zeros((), device=x_raw.device, dtype=x_raw.dtype)

        if capture_safe:
            # per-step host scalars must not be baked into a recorded graph: beta_factor is changed every step by the
            # reference's BetaWarmupCallback (rave/model.py:83-107), so the captured step reads it from a 0-d device
            # tensor that GraphedTrainingStep refreshes (fill_) before every replay -- same f32 product as `reg * float`
            terms["regularization"] = (reg, self.beta_device(reg.device))
        elif reg.item():
            terms["regularization"] = (reg, self.beta_factor)
        if self.warmed_up:
            terms["feature_matching"] = (feature_matching_distance, self.weights["feature_matching"])
            terms["adversarial"] = (loss_adv, self.weights["adversarial"])
        fused_sum = _loss_combine_fused() and all(torch.is_tensor(v) and v.is_cuda and v.dtype == torch.float32
                                                  and v.numel() == 1 for v, _ in terms.values()) and 0 < len(terms) <= 16
        loss_gen = {}
        loss_gen_value = None
        if fused_sum:
            from . import ops
            names = list(terms)
            w1 = [0. if torch.is_tensor(terms[k][1]) else terms[k][1] for k in names]
            w1_dev = [terms[k][1] if torch.is_tensor(terms[k][1]) else None for k in names]
            loss_gen_value, scaled = ops.loss_combine([terms[k][0] for k in names], w1, [self.weights.get(k, 1.) for k in names],
                                                      w1_dev)
            for i, k in enumerate(names):
                loss_gen[k] = scaled[i]
        else:
            for k, (v, w) in terms.items():
                loss_gen[k] = (v * w) if torch.is_tensor(w) else (w * v)

        if dis_step:
            dis_opt.zero_grad()
            if grad_begin is not None:
                grad_begin(1)
            loss_dis.backward()
            if grad_sync is not None:
                grad_sync(1)
            self._join_side()
            dis_opt.step()
        else:
            gen_opt.zero_grad()
            if grad_begin is not None:
                grad_begin(0)
            if loss_gen_value is None:
                loss_gen_value = 0.
                for k, v in loss_gen.items():
                    loss_gen_value += v * self.weights.get(k, 1.)
            loss_gen_value.backward()
            if grad_sync is not None:
                grad_sync(0)
            self._join_side()
            gen_opt.step()

        self.release_weights()
        if self._prep is not None:       # (fused optimizers do not bump parameter version counters)
            for pr in self._prep:
                pr.invalidate()
        self.logged = dict(loss_gen)
        self.logged["loss_dis"] = loss_dis
        if self.warmed_up:                      # rave/model.py:418-421
            self.logged["pred_real"] = pred_real
            self.logged["pred_fake"] = pred_fake
        return self.logged


    # ---- rave/model.py:426-443
    def validation_step(self, x, batch_idx, eps: Optional[torch.Tensor] = None):
        """Returns (cat([x, y], -1), latent mean or None), as the reference; the validation distance is kept in
        ``self.logged["validation"]`` (the reference logs it through the trainer).  ``eps`` injects the reparametrisation
        draw (parity runs).  Lightning calls this under ``model.eval()``: AdaptiveInstanceNormalization sites then run
        their statistics / transfer branch (blocks.AdaptiveInstanceNormalization)."""
        if x.is_cuda:
            self.prepare_weights(reuse=True)
        z = self.encode(x)
        if isinstance(self.encoder, blocks.VariationalEncoder):
            mean = torch.split(z, z.shape[1] // 2, 1)[0]
        else:
            mean = None
        z = self.encoder.reparametrize(z, eps)[0]
        y = self.decode(z)
        distance = self.audio_distance(x, y)
        # a NEW dict (the current one may be the object a GraphedTrainingStep hands back at every replay: writing into it would
        # leak a stale entry into all later training logs -- ADVICE r5), the value detached
        self.logged = dict(self.logged, validation=sum(distance.values()).detach())
        self.release_weights()
        return torch.cat([x, y], -1), mean

    # ---- rave/core.py:180-217
    def measure_receptive_field(self):
        """``rave.core.get_rave_receptive_field``: the input gradient of one output sample of the eval-mode model, the signal
        length doubled from 2**15 until both ends of the gradient are zero; returns the number of non-zero entries in the left
        and in the right half.  On the GPU the probe runs on the exact-f32 kernels: the x6 kernels enter every operand as two
        f16 pieces under a per-tensor scale, so a gradient entry far enough below its tensor's maximum becomes an exact zero
        there -- and the tail of a receptive field is made of such entries ("Latent-space analysis").  Everything
        the probe touches is put back: train / eval flags, the kernel mode, parameter gradients, the packed weights."""
        import contextlib
        from . import ops
        modes = [(mod, mod.training) for mod in self.modules()]
        gated = [mod for mod in self.modules() if hasattr(mod, "gru_state") or hasattr(mod, "temporal")]
        device = next(iter(self.parameters())).device
        exact = ops._ExactF32() if device.type == "cuda" else contextlib.nullcontext()
        n = 2 ** 15
        try:
            self.eval()
            for mod in gated:
                mod.disable()
            with torch.enable_grad(), exact:
                while True:
                    x = torch.randn(1, self.n_channels, n, requires_grad=True, device=device)
                    if x.is_cuda:
                        self.prepare_weights(reuse=True)
                    z = self.encode(x)
                    z = self.encoder.reparametrize(z)[0]
                    y = self.decode(z)
                    y[0, 0, n // 2].backward()
                    assert x.grad is not None, "input has no grad"
                    left_grad, right_grad = x.grad.detach().reshape(-1).chunk(2, 0)
                    if bool(left_grad[0] == 0) and bool(right_grad[-1] == 0):
                        break
                    n *= 2
            left = int((left_grad != 0).sum())
            right = int((right_grad != 0).sum())
        finally:
            self._join_side()
            self.zero_grad()
            self.release_weights()
            for mod in gated:
                mod.enable()
            for mod, training in modes:
                mod.training = training
        return left, right

    # ---- rave/model.py:445-488
    def validation_epoch_end(self, out):
        """``out``: the list of validation_step results of the epoch.  Fills ``receptive_field`` the first time (any model), then
        -- ``latent_analysis=True``, before the GAN phase, variational encoder -- ``latent_mean`` / ``latent_pca`` /
        ``fidelity`` from the posterior means in ``out`` (rave_amd.latent.LatentAnalysis: one HIP call per batch, no
        concatenation, one small device-to-host copy) and the reference's ``fidelity_p`` log values into ``self.logged``.
        The reference's audio logging is not restated."""
        if not int(self.receptive_field.sum()):
            lrf, rrf = self.measure_receptive_field()
            self.receptive_field[0] = lrf
            self.receptive_field[1] = rrf
            self.__dict__.pop("_rf_host", None)       # training_step's host copy: the next step reads the buffer again
        if not len(out):
            return
        if self.warmed_up or not isinstance(self.encoder, blocks.VariationalEncoder) or not self.latent_analysis:
            return
        from .latent import LatentAnalysis
        analysis = LatentAnalysis()
        for _, mean in out:
            analysis.update(mean)
        result = analysis.finish()
        if result is None:
            return
        latent_mean, components, fidelity = result
        self.latent_mean.copy_(latent_mean)
        self.latent_pca.copy_(components)
        self.fidelity.copy_(fidelity)
        logged = dict(self.logged)
        for p in (.8, .9, .95, .99):
            # rave/model.py:483-488: np.argmax(var > p), the first index whose cumulative share exceeds p (var is f32 there too)
            logged[f"fidelity_{p}"] = float(torch.argmax((fidelity > p).to(torch.uint8)))
        self.logged = logged


class LinearLR:
    """torch.optim.lr_scheduler.LinearLR(start_factor, end_factor, total_iters) in closed form:
    lr_t = base * (start + (end - start) * min(t, total) / total).  A learning rate that lives on the device
    (capturable optimizers) is updated IN PLACE, so that a recorded hipGraph keeps reading the current value
    (torch's scheduler rebinds ``param_group["lr"]`` to a new object)."""

    def __init__(self, optimizer, start_factor: float, end_factor: float, total_iters: int):
        self.opt, self.start, self.end, self.total = optimizer, start_factor, end_factor, max(int(total_iters), 1)
        self.base = [float(g["lr"]) for g in optimizer.param_groups]
        self.t = 0

    def get_last_lr(self):
        f = self.start + (self.end - self.start) * min(self.t, self.total) / self.total
        return [b * f for b in self.base]

    def step(self):
        self.t += 1
        for g, lr in zip(self.opt.param_groups, self.get_last_lr()):
            if torch.is_tensor(g["lr"]):
                g["lr"].fill_(lr)
            else:
                g["lr"] = lr


class GraphedTrainingStep:
    """The static training step as ONE hipGraph launch: prepare_weights -> forward -> losses
    -> backward -> Adam of ``RAVE.training_step`` recorded once per (phase, step kind) for a fixed batch shape through
    ``torch.cuda.CUDAGraph`` (hipGraph on ROCm) and replayed.  ~650 kernel launches per step leave the host: the eager
    step is within a few % of being launch-bound on the host (9.3 ms of pure CPU time per step measured).

    Eager ``training_step`` stays the parity path; tests assert bit-identical parameters after 8 steps of both.
    The model must have been set up with ``configure_optimizers(capturable=True)``.

    What a recorded step reads at REPLAY time (device memory, updated in place): parameters, optimizer state, the
    learning rates (LinearLR), ``beta_factor`` (RAVE.beta_device, refreshed here before every replay) and the input
    batch / noise.  What is BAKED IN at capture time: the loss ``weights``, the phase (``warmed_up``) and step kind
    (one graph per (phase, kind) key), ``valid_signal_crop``'s receptive field, every buffer-derived host flag.
    Data-dependent one-time initialisation cannot be recorded: a model whose RVQ codebooks are not initialised yet
    (``EuclideanCodebook.inited == 0`` with the quantizer enabled) is refused -- run eager steps until the k-means
    init has happened, then construct / call this class."""

    def __init__(self, model: "RAVE", example_batch: torch.Tensor, inject_eps: bool = False, warmup_iters: int = 3,
                 grad_begin=None, grad_sync=None, before_step=None):
        """``grad_begin`` / ``grad_sync``: the data-parallel reducer's begin / finish (rave_amd.ddp.GradReducer), recorded
        INTO the graph -- the bucket all-reduces are stream-ordered RCCL launches, capturable like any kernel, so a
        data-parallel rank replays one graph per step exactly like a single-GPU run.  ``before_step``: called at the
        start of the recorded region (rave_amd.ddp.BufferSync.sync: the per-step buffer broadcast)."""
        self.model = model
        self.sync_kw = dict(grad_begin=grad_begin, grad_sync=grad_sync)
        self.before_step = before_step
        self.x = example_batch.detach().clone()
        self.eps = None
        if inject_eps:
            self.eps = torch.zeros(self.x.shape[0], model.latent_size, self.x.shape[-1] // self._hop(), device=self.x.device)
        self.warmup_iters = warmup_iters
        self.graphs = {}
        self.range_pools = {}            # key -> the range-slot pools the recording took (ops.range_capture_end): alive with the graph
        self.logged = {}

    def _hop(self) -> int:
        # one dry encode to learn the latent rate; train-mode side effects (v1 BatchNorm running statistics, lazily
        # initialised buffers) are undone so that the snapshot taken before the capture is the caller's state
        saved = {k: v.clone() for k, v in self.model.named_buffers()}
        with torch.no_grad():
            z = self.model.encode(self.x[:1])
            for k, v in self.model.named_buffers():
                v.copy_(saved[k])
        _reset_host_shadows(self.model)
        return self.x.shape[-1] // z.shape[-1]

    def _check_capturable(self) -> None:
        m = self.model
        enc = getattr(m, "encoder", None)
        enabled = getattr(enc, "enabled", None)
        if enabled is not None and bool(enabled):
            for name, mod in m.named_modules():
                inited = getattr(mod, "inited", None)
                if torch.is_tensor(inited) and not bool(inited):
                    raise RuntimeError(
                        f"GraphedTrainingStep: {name}.inited == 0 -- the RVQ k-means initialisation is host-driven, "
                        "data-dependent work that a recorded graph cannot contain; run eager training_step()s until the "
                        "codebooks are initialised, then capture")

    def _key(self, batch_idx: int):
        m = self.model
        return bool(m.warmed_up) and not (batch_idx % m.update_discriminator_every)

    def capture(self, batch: torch.Tensor, batch_idx: int, eps: Optional[torch.Tensor] = None) -> None:
        """Records the graph of this (phase, step kind) WITHOUT replaying it: the warm-up iterations run (and are rolled back),
        the capture executes nothing.  Data-parallel callers use it to agree across ranks that every rank recorded its step
        before any rank replays one -- a rank that replays while another fell back to the eager step would wait in a
        collective nobody else enters."""
        self(batch, batch_idx, eps, _replay=False)

    def __call__(self, batch: torch.Tensor, batch_idx: int, eps: Optional[torch.Tensor] = None, _replay: bool = True):
        m = self.model
        key = (bool(m.warmed_up), self._key(batch_idx))
        with torch.no_grad():            # (training_step marks its input as requiring grad, rave/model.py:292)
            self.x.copy_(batch)
            if self.eps is not None:
                self.eps.copy_(eps)
        if key not in self.graphs:
            self._check_capturable()
            # a few eager iterations on a side stream first (allocator warm-up, lazy one-time initialisations),
            # restoring parameters / optimizer state afterwards so that the capture does not change the trajectory
            state = ({k: v.clone() for k, v in m.state_dict().items()},
                     [_clone_opt(o) for o in m.optimizers()])
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(self.warmup_iters):
                    if self.before_step is not None:
                        self.before_step()
                    m.training_step(self.x, batch_idx, eps=self.eps, capture_safe=True, **self.sync_kw)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            m.load_state_dict(state[0])
            for o, st in zip(m.optimizers(), state[1]):
                _restore_opt(o, st)
            for o in m.optimizers():
                o.zero_grad(set_to_none=True)
            # host shadows of flag buffers were filled by the warm-up run; the restore may have changed the buffers
            _reset_host_shadows(m)
            self._check_capturable()
            for mod in m.modules():          # host-side caches keyed on parameter versions (the restore bumped them)
                if hasattr(mod, "refresh_host_caches"):
                    mod.refresh_host_caches()
            m.set_phase_flags_eagerly()
            g = torch.cuda.CUDAGraph()
            import os
            kw = {}
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                # The process group's watchdog thread wakes every 100 ms and queries the end events of the collectives it
                # still lists -- those of the eager warm-up steps, long complete.  This HIP runtime refuses hipEventQuery on an
                # event whose STREAM has meanwhile joined a capture (hipErrorCapturedEvent, although the event was recorded
                # before), which the watchdog turns into an abort of the process: about one data-parallel capture in eight
                # (profiles/round6_rccl_watchdog_abort.txt).  Let it retire the finished collectives before the recording starts.
                import time
                torch.cuda.synchronize()
                time.sleep(0.5)
            if os.environ.get("RH_GRAPH_PRIORITY", "0") == "1":
                # experiment: record the step on a HIGH-priority stream, so that the data-gradient chain (the critical path)
                # wins the arbitration against the weight-gradient branch, which forks onto a default-priority stream
                kw["stream"] = torch.cuda.Stream(priority=-1)
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                # RCCL's watchdog thread polls the events of earlier collectives (hipEventQuery) whenever it likes; under the
                # default capture_error_mode = "global" such a call from ANOTHER thread while this one records is an error, which
                # the watchdog turns into an abort of the process (ProcessGroupNCCL.cpp: Watchdog::run) -- intermittently, about
                # one data-parallel capture in four on these boxes (round 5).  "thread_local" restricts the check to this thread.
                kw["capture_error_mode"] = "thread_local"
            # A step that cannot be recorded (e.g. a collective of a backend without capture support) must leave the process fit for
            # the caller's eager fallback: (1) the streams the refused step forked are joined back INSIDE the recording -- ending a
            # capture with unjoined work fails and, on this runtime, leaves every stream of it in capture mode for good
            # (tools/debug/gloo_capture_recover.py); (2) the refused call's error code is read away from the runtime's per-thread
            # "last error", where the next checked call of this thread would trip over it.
            err = None
            try:
                with torch.cuda.graph(g, **kw):
                    try:
                        if self.before_step is not None:
                            self.before_step()
                        logged = m.training_step(self.x, batch_idx, eps=self.eps, capture_safe=True, **self.sync_kw)
                    except Exception as e:        # noqa: BLE001 -- handed on below, after the recording has been closed
                        err = e
                        from . import ops as _ops
                        _ops.abandon_side_streams(rejoin=True)
            except Exception as e:                # noqa: BLE001 -- the recording could not be closed either
                err = err or e
            from . import ops as _ops
            # the slot pools taken inside the recording belong to the graph (each replay re-zeroes them): eager work from here on
            # takes its slots from a fresh pool
            pools = _ops.range_capture_end()
            if err is not None:
                _ops.abandon_side_streams()
                for _ in range(3):
                    try:
                        torch.cuda.synchronize()
                        torch.zeros(1, device=self.x.device)
                        break
                    except Exception:             # noqa: BLE001 -- the stale error itself
                        continue
                raise err
            # the capture itself does not execute anything: parameters are still the restored ones
            self.graphs[key] = (g, logged)
            self.range_pools[key] = pools
        g, logged = self.graphs[key]
        if not _replay:
            return logged
        m.beta_device(self.x.device)     # per-step scalar the recorded step reads from device memory
        g.replay()
        if m._prep is not None:          # the replayed optimizer changed parameters behind the version counters
            for pr in m._prep:
                pr.invalidate()
        self.logged = logged
        return logged


def _reset_host_shadows(model: nn.Module) -> None:
    """Forget every host-side shadow of a flag buffer (blocks.host_flag / blocks._set_warmed_up): the next read goes to
    the device again.  Needed after anything that rewrites buffers behind the modules' back (load_state_dict)."""
    for mod in model.modules():
        mod.__dict__.pop("_host_flags", None)
        if "_warmed_up_host" in mod.__dict__:
            mod._warmed_up_host = None


def _clone_opt(opt):
    return {id(p): {k: (v.clone() if torch.is_tensor(v) else v) for k, v in st.items()} for p, st in opt.state.items()}


def _restore_opt(opt, saved):
    # two passes: state tensors may be SHARED between parameters (an optimizer may alias one step counter into several
    # state[p]["step"]) -- first reset whatever the warm-up iterations created, then restore the saved values, so that a
    # restored counter is never zeroed afterwards through an alias (dict order must not decide)
    for p in list(opt.state.keys()):
        if id(p) not in saved:
            # state created by the warm-up iterations: keep the tensors (a state created INSIDE the capture would be
            # re-initialised by every replay) but reset them to the freshly-initialised values (all zero)
            for k, v in opt.state[p].items():
                if torch.is_tensor(v):
                    v.zero_()
    for p in list(opt.state.keys()):
        if id(p) in saved:
            for k, v in saved[id(p)].items():
                if torch.is_tensor(v):
                    opt.state[p][k].copy_(v)
                else:
                    opt.state[p][k] = v


V2_DILATIONS = [[1, 3, 9], [1, 3, 9], [1, 3, 9], [1, 3]]


def build_v1(n_channels: int = 1, capacity: int = 64, ratios=(4, 4, 4, 2), latent_size: int = 128,
             n_band: int = 16, sampling_rate: int = 44100, use_noise: bool = True, latent_analysis: bool = False) -> "RAVE":
    """configs/v1.gin: v1 Encoder (BatchNorm) / Generator (ResidualStack, loudness + noise branches),
    multi-scale discriminator only, feature matching L1 x10, discriminator every 2nd step."""
    cc.set_default_padding_mode("centered")
    blocks.set_normalization_mode("weight_norm")
    ratios = list(ratios)
    enc = partial(blocks.VariationalEncoder,
                  encoder=partial(blocks.Encoder, data_size=n_band, capacity=capacity, latent_size=latent_size,
                                  ratios=ratios, n_out=2, sample_norm=False, repeat_layers=1))
    dec = partial(blocks.Generator, latent_size=latent_size, capacity=capacity, data_size=n_band, ratios=ratios,
                  loud_stride=1, use_noise=use_noise)
    msd = partial(discriminator.MultiScaleDiscriminator, n_discriminators=3,
                  convnet=partial(discriminator.ConvNet, out_size=1, capacity=capacity, n_layers=4, stride=4,
                                  conv=nn.Conv1d, kernel_size=15))
    stft = partial(losses.MultiScaleSTFT, scales=[2048, 1024, 512, 256, 128], sample_rate=sampling_rate, magnitude=True)
    dist = partial(losses.AudioDistanceV1, multiscale_stft=stft, log_epsilon=1e-7)
    return RAVE(latent_size=latent_size, sampling_rate=sampling_rate,
                pqmf=partial(pqmf.CachedPQMF, attenuation=100, n_band=n_band), encoder=enc, decoder=dec,
                discriminator=msd, phase_1_duration=1000000, gan_loss=losses.hinge_gan, valid_signal_crop=False,
                feature_matching_fun=partial(losses.mean_difference, norm="L1"), num_skipped_features=0,
                audio_distance=dist, multiband_audio_distance=dist, weights={"feature_matching": 10},
                update_discriminator_every=2, n_channels=n_channels, n_bands=n_band, latent_analysis=latent_analysis)


def build_v2_small(**kw) -> "RAVE":
    """configs/v2_small.gin: CAPACITY 48, RATIOS [4,2,2,2], NoiseGeneratorV2, discriminator every 2nd step."""
    d = dict(capacity=48, ratios=(4, 2, 2, 2), noise=True, update_discriminator_every=2)
    d.update(kw)
    return build_v2(**d)


def build_v2(n_channels: int = 1, capacity: int = 96, ratios=(4, 4, 4, 2), latent_size: int = 128,
             n_band: int = 16, dilations=None, sampling_rate: int = 44100, causal: bool = False,
             disc_capacity: Optional[int] = None, snake: bool = False, adain: bool = False,
             noise: bool = False, update_discriminator_every: int = 4, discriminator_kind: str = "v2",
             encoder_kind: str = "variational", noise_augmentation: int = 0, num_quantizers: int = 16,
             codebook_size: int = 1024, log_epsilon: float = 1e-7, num_skipped_features: int = 1,
             spectral_capacity: int = 32, gru_layers: int = 0, mel_input: bool = False, n_fft: int = 2048,
             hop_length: int = 256, n_mels: int = 128, encoder_ratios=(2, 2, 2), encoder_dilations=(1,),
             latent_analysis: bool = False, hip_frontend: bool = False, phase_distance: bool = False,
             gan_loss: str = "hinge", encodec_distance: bool = False) -> RAVE:
    """configs/v1.gin + configs/v2.gin transcribed (cf. oracle/ref_models.py for the citations).
    ``snake`` / ``adain`` add the generator-side overlays of configs/v3.gin (snake.gin: every activation
    -> blocks.Snake; adain.gin: AdaptiveInstanceNormalization before every unit); ``causal`` =
    configs/causal.gin.  ``discriminator_kind``: "v2" (MPD + MSD, v2.gin:53-75), "descript"
    (descript_discriminator.gin), "spectral" (spectral_discriminator.gin: MSD + Encodec STFT nets).
    ``encoder_kind``: "variational" or "discrete" (discrete.gin: EncoderV2(n_out=1) + RVQ + noise channels).
    ``gru_layers`` > 0 puts blocks.GRU in front of the decoder (the generator half of configs/hybrid.gin:33-38).
    ``mel_input`` is the encoder half (hybrid.gin:11-31, 40-42): RAVE.input_mode = "mel" with rave_amd.MelSpectrogram
    (``n_fft``, ``hop_length``, ``n_mels``, normalized) and EncoderV2(data_size = n_mels * n_channels as the reference's
    encoder computes it, ``encoder_ratios``, ``encoder_dilations``); the decoder keeps ``ratios`` / ``dilations``.
    ``latent_analysis`` registers the reference's ``latent_pca`` / ``latent_mean`` / ``fidelity`` buffers (rave/model.py:196-198),
    which ``validation_epoch_end`` then fills; off by default, the state_dict keys are then unchanged.
    ``hip_frontend`` hands the complex spectrograms of the "spectral" and "descript" discriminators to
    rave_amd/csrc/spectrogram.hip (the gin route: rave_amd/configs/mi355x_spectrogram*.gin); off by default.
    ``phase_distance`` binds the fullband distance to losses.WeightedInstantaneousSpectralDistance (weighted, over the
    normalised complex multi-scale STFT) as rave_amd/configs/mi355x_phase.gin does: the step then logs and trains on
    ``fullband_phase_distance`` as well; off by default.
    ``gan_loss``: "hinge" (every stock config), "ls" or "nonsaturating" -- losses.hinge_gan / ls_gan / nonsaturating_gan
    (rave/core.py:151-170; the gin route: rave_amd/configs/mi355x_gan_loss.gin).
    ``encodec_distance`` binds the fullband distance to losses.EncodecAudioDistance over the plain losses.SpectralDistance
    (scales 2048 ... 128, L1 + L2, power 1, normalised) as rave_amd/configs/mi355x_encodec.gin does: the step then logs and trains
    on ``fullband_waveform_distance`` as well; off by default."""
    if phase_distance and encodec_distance:
        raise ValueError("build_v2: phase_distance and encodec_distance both bind the fullband distance; choose one")
    if gan_loss not in losses.GAN_LOSSES:
        raise ValueError(f"build_v2: gan_loss {gan_loss!r}, expected one of {sorted(losses.GAN_LOSSES)}")
    ratios = list(ratios)
    spectrogram = None
    if mel_input:
        enc_rate, dec_rate = int(hop_length), int(n_band)
        for r in encoder_ratios:
            enc_rate *= int(r)
        for r in ratios:
            dec_rate *= int(r)
        if enc_rate != dec_rate:
            raise ValueError(f"build_v2(mel_input=True): the encoder makes one latent frame per hop_length x prod(encoder_ratios) = "
                             f"{enc_rate} samples, the decoder turns one into n_band x prod(ratios) = {dec_rate}: they must agree")
        from .mel import MelSpectrogram
        spectrogram = MelSpectrogram(sample_rate=sampling_rate, n_fft=n_fft, win_length=n_fft, hop_length=hop_length,
                                     normalized=True, n_mels=n_mels)
    cc.set_default_padding_mode("causal" if causal else "centered")
    blocks.set_normalization_mode("weight_norm")
    dil = dilations or V2_DILATIONS
    extra = {}
    blocks.set_dilated_unit_activation(blocks.Snake if snake else None)
    if snake:
        extra["activation"] = blocks.Snake
    if adain:
        extra["adain"] = blocks.AdaptiveInstanceNormalization
    # the encoder's own geometry: the PQMF bands at the decoder's ratios, or (hybrid.gin:17-20) the mel channels at its own
    enc_geom = dict(data_size=n_band, ratios=ratios, dilations=dil)
    if mel_input:
        enc_geom = dict(data_size=int(n_mels), ratios=[int(r) for r in encoder_ratios], dilations=[int(d) for d in encoder_dilations])
    if encoder_kind == "variational":
        enc = partial(blocks.VariationalEncoder,
                      encoder=partial(blocks.EncoderV2, capacity=capacity, latent_size=latent_size, n_out=2, kernel_size=3,
                                      **enc_geom, **extra))
    elif encoder_kind == "discrete":   # configs/discrete.gin:24-40
        enc = partial(blocks.DiscreteEncoder,
                      encoder_cls=partial(blocks.EncoderV2, capacity=capacity, latent_size=latent_size, n_out=1, kernel_size=3,
                                          **enc_geom, **extra),
                      vq_cls=partial(quantization.ResidualVectorQuantization, num_quantizers=num_quantizers,
                                     dim=latent_size, codebook_size=codebook_size),
                      num_quantizers=num_quantizers, noise_augmentation=noise_augmentation)
    else:
        raise ValueError(encoder_kind)
    dec_latent = latent_size + noise_augmentation      # core.get_augmented_latent_size (v2.gin:24-26,47)
    if noise:   # configs/v2_small.gin:42-57
        extra_dec = dict(noise_module=partial(blocks.NoiseGeneratorV2, hidden_size=64, data_size=n_band,
                                              ratios=[2, 2, 2], noise_bands=32))
    else:
        extra_dec = {}
    if gru_layers > 0:
        extra_dec["recurrent_layer"] = partial(blocks.GRU, num_layers=gru_layers)
    dec = partial(blocks.GeneratorV2, data_size=n_band, capacity=capacity, ratios=ratios,
                  latent_size=dec_latent, kernel_size=3, dilations=dil, amplitude_modulation=True, **extra,
                  **extra_dec)
    common = dict(out_size=1, capacity=disc_capacity or capacity, n_layers=4, stride=4)
    mpd = partial(discriminator.MultiPeriodDiscriminator, periods=[2, 3, 5, 7, 11],
                  convnet=partial(discriminator.ConvNet, conv=nn.Conv2d, kernel_size=(5, 1), **common))
    msd = partial(discriminator.MultiScaleDiscriminator, n_discriminators=3,
                  convnet=partial(discriminator.ConvNet, conv=nn.Conv1d, kernel_size=15, **common))
    if discriminator_kind == "v2":
        disc = partial(discriminator.CombineDiscriminators, discriminators=[mpd, msd])
    elif discriminator_kind == "descript":
        disc = partial(descript_discriminator.DescriptDiscriminator, hip_frontend=hip_frontend)
    elif discriminator_kind == "spectral":   # configs/spectral_discriminator.gin
        mssd = partial(discriminator.MultiScaleSpectralDiscriminator, scales=[4096, 2048, 1024, 512, 256], hip_frontend=hip_frontend,
                       convnet=partial(discriminator.EncodecConvNet, capacity=spectral_capacity))
        disc = partial(discriminator.CombineDiscriminators, discriminators=[msd, mssd])
    else:
        raise ValueError(discriminator_kind)
    stft = partial(losses.MultiScaleSTFT, scales=[2048, 1024, 512, 256, 128], sample_rate=sampling_rate,
                   magnitude=True)
    dist = partial(losses.AudioDistanceV1, multiscale_stft=stft, log_epsilon=log_epsilon)
    full_dist = dist
    if phase_distance:      # rave_amd/configs/mi355x_phase.gin: the fullband distance only, the multiband one stays
        full_dist = partial(losses.WeightedInstantaneousSpectralDistance, weighted=True,
                            multiscale_stft=partial(losses.MultiScaleSTFT, scales=[2048, 1024, 512, 256, 128],
                                                    sample_rate=sampling_rate, magnitude=False, normalized=True))
    if encodec_distance:    # rave_amd/configs/mi355x_encodec.gin: the fullband distance only, the multiband one stays
        full_dist = partial(losses.EncodecAudioDistance, scales=[2048, 1024, 512, 256, 128],
                            spectral_distance=partial(losses.SpectralDistance, sampling_rate=sampling_rate, norm=["L1", "L2"],
                                                      power=1, normalized=True))
    model = RAVE(latent_size=latent_size, sampling_rate=sampling_rate,
                 pqmf=partial(pqmf.CachedPQMF, attenuation=100, n_band=n_band),
                 encoder=enc, decoder=dec, discriminator=disc, phase_1_duration=1000000,
                 gan_loss=losses.GAN_LOSSES[gan_loss], valid_signal_crop=True,
                 feature_matching_fun=partial(losses.mean_difference, norm="L1", relative=True),
                 num_skipped_features=num_skipped_features, audio_distance=full_dist, multiband_audio_distance=dist,
                 weights={"feature_matching": 20}, update_discriminator_every=update_discriminator_every,
                 n_channels=n_channels, n_bands=n_band, spectrogram=spectrogram,
                 input_mode="mel" if mel_input else "pqmf", latent_analysis=latent_analysis)
    cc.set_default_padding_mode("centered")
    blocks.set_dilated_unit_activation(None)
    return model


def build_v3(n_channels: int = 2, causal: bool = True, **kw) -> RAVE:
    """configs/v3.gin (+ causal.gin; BASELINE config 5 is stereo): v2 + adain.gin + snake.gin +
    descript_discriminator.gin."""
    d = dict(n_channels=n_channels, causal=causal, snake=True, adain=True, discriminator_kind="descript")
    d.update(kw)
    return build_v2(**d)


def build_discrete(spectral: bool = True, **kw) -> RAVE:
    """configs/discrete.gin (+ spectral_discriminator.gin; BASELINE config 4): RATIOS [4,4,2,2], EncoderV2(n_out=1)
    + 16-stage RVQ (1024 codes) + 128 noise channels, log_epsilon 1, num_skipped_features 0."""
    d = dict(ratios=(4, 4, 2, 2), encoder_kind="discrete", noise_augmentation=128, log_epsilon=1.0,
             num_skipped_features=0, discriminator_kind="spectral" if spectral else "v2")
    d.update(kw)
    return build_v2(**d)
