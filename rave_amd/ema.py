"""Exponential average of the weights (`rave train --ema f`) on the HIP kernels of rave_amd/csrc/ema.hip: the ``EMA`` callback of
the reference's scripts/train.py:81-120 with the same interface (``weights`` / ``factor``, the Lightning hooks,
``swap_weights``, ``state_dict`` = the dict of averages), so that it can be handed to a Lightning ``Trainer`` in place of that
class or driven by a plain loop::

    ema = EMA(.999)
    for i, x in enumerate(batches):
        step(x, i)                                       # RAVE.training_step or a GraphedTrainingStep
        model.on_train_batch_end(None, x, i)
        ema.on_train_batch_end(None, model, None, x, i)
    ema.on_validation_epoch_start(None, model)           # the model now holds the averages ...
    model.validation_step(xv, 0)
    ema.on_validation_epoch_end(None, model)             # ... and its own weights again

What differs from the reference class is how the work is done, not what is computed:

* the update ``w = w * factor + p * (1 - factor)`` of EVERY ``named_parameters()`` entry (whichever optimizer owns it, or
  none) is one ``rh_ema_update_f32`` call -- one launch per 64 tensors, 12 bytes of traffic per parameter -- instead of three
  ATen kernels and two temporaries per tensor; the results are bit-identical to that expression;
* ``swap_weights`` EXCHANGES contents in place (``rh_swap_f32``) and never rebinds a tensor: a recorded
  ``GraphedTrainingStep``, the ``FusedAdam`` tables and ``WeightPrep`` all hold parameter addresses.  It then invalidates the
  module's packed-weight caches (``WeightPrep.invalidate``) and bumps the parameters' version counters: the swap goes through
  raw pointers, and ``validation_step`` / ``encode`` / ``decode`` reuse the packed operands while no counter moved -- without
  this they would silently run the weights from before the swap.  Never copy averages into a model by hand;
* the update is NOT recorded into the step's hipGraph: it is stream-ordered after the replay, called where drivers already
  call ``RAVE.on_train_batch_end``.  ``GraphedTrainingStep`` rolls its warm-up iterations back; an average kept outside the
  recording needs no rolling back.

Parameters must be contiguous f32 tensors on the GPU (there is no CPU fallback)."""
from __future__ import annotations

from typing import Any, Dict

import torch

from . import _lib as L

try:                                                     # a real Lightning callback where Lightning is installed
    from pytorch_lightning import Callback as _Callback
except ImportError:
    _Callback = object


class EMA(_Callback):
    def __init__(self, factor=.999) -> None:
        super().__init__()
        self.weights: Dict[str, torch.Tensor] = {}
        self.factor = factor
        self._table = None             # (key, rh_pair_item array): rebuilt only when an address changes

    def _average_of(self, name: str, p: torch.Tensor) -> torch.Tensor:
        """The average of ``name``, moved next to its parameter first if it came from a checkpoint (CPU / other dtype)."""
        w = self.weights[name]
        if w.shape != p.shape:
            raise RuntimeError(f"rave_amd EMA: the average of {name} has shape {tuple(w.shape)}, the parameter {tuple(p.shape)}")
        if w.device != p.device or w.dtype != torch.float32 or not w.is_contiguous():
            w = self.weights[name] = w.detach().to(device=p.device, dtype=torch.float32).contiguous()
        return w

    def _pair_table(self, pairs):
        key = tuple((w.data_ptr(), p.data_ptr(), p.numel()) for w, p in pairs)
        if self._table is None or self._table[0] != key:
            arr = (L.PairItem * len(pairs))()
            for i, (a, b, n) in enumerate(key):
                arr[i].a, arr[i].b, arr[i].n = a, b, n
            self._table = (key, arr)
        return self._table[1]

    @staticmethod
    def _parameters(module):
        named = list(module.named_parameters())
        for n, p in named:
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"rave_amd EMA: parameters must be contiguous fp32 tensors on the GPU ({n} is not)")
        return named

    # ---- scripts/train.py:88-96
    @torch.no_grad()
    def on_train_batch_end(self, trainer, pl_module, outputs, batch, batch_idx) -> None:
        pairs = []
        for n, p in self._parameters(pl_module):
            if n not in self.weights:
                self.weights[n] = p.detach().clone()     # first sight: taken as it is, not averaged in this call
                continue
            pairs.append((self._average_of(n, p), p))
        if pairs:
            L.check(L.lib.rh_ema_update_f32(self._pair_table(pairs), len(pairs), float(self.factor), L.stream()), "ema_update")

    # ---- scripts/train.py:98-102
    @torch.no_grad()
    def swap_weights(self, module) -> None:
        pairs = [(self._average_of(n, p), p) for n, p in self._parameters(module)]
        if not pairs:
            return
        L.check(L.lib.rh_swap_f32(self._pair_table(pairs), len(pairs), L.stream()), "swap")
        # the kernel wrote through raw pointers: tell every cache keyed on the parameters' versions
        for _, p in pairs:
            torch.autograd.graph.increment_version(p)
        for prep in getattr(module, "_prep", None) or ():
            prep.invalidate()

    def on_validation_epoch_start(self, trainer, pl_module) -> None:
        if self.weights:
            self.swap_weights(pl_module)
        else:
            print("no ema weights available")

    def on_validation_epoch_end(self, trainer, pl_module) -> None:
        if self.weights:
            self.swap_weights(pl_module)
        else:
            print("no ema weights available")

    def state_dict(self) -> Dict[str, Any]:
        return self.weights.copy()

    @torch.no_grad()
    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        """Copies INTO the averages this object already holds (their addresses are in the pair table); a name it does not
        know yet takes the given tensor, which moves to its parameter's device at the next update or swap."""
        for n, t in state_dict.items():
            w = self.weights.get(n)
            if w is not None and w.shape == t.shape:
                w.copy_(t)
            else:
                self.weights[n] = t
