"""The ``Model`` plug-in protocol this backend implements (mirrors the reference's base class, realpdebench/model/model.py:4-26,
in meaning, not in text): ``forward``, ``train_loss`` and ``load_checkpoint(checkpoint_path, device) -> meta dict``."""
import torch
import torch.nn as nn

from ._common import META_KEYS, LayoutCache


class Model(nn.Module):
    """Every MI355X model subclasses this; subclasses provide the HIP-backed ``forward``."""

    def __init__(self):
        super().__init__()
        self._layouts = LayoutCache()      # kernel-side layouts derived from the parameters

    def _apply(self, fn, *args, **kwargs):
        self._layouts.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._layouts.invalidate()
        return super().load_state_dict(*args, **kwargs)

    def _new_state(self):
        """What ``_forward_hip`` records into for ``_backward_hip`` (``_common.HipFunction``)."""
        return {}

    def _require_hip(self, x):
        if not x.is_cuda:
            raise RuntimeError(f"realpdebench_amd.{type(self).__name__} runs on MI355X only: there is no CPU fallback")

    def forward(self, x):
        raise NotImplementedError(f"{type(self).__name__}.forward")

    def train_loss(self, input, target):
        """Elementwise ``mse_loss(pred, target)`` like the reference's models (callers take ``.mean()``)."""
        pred = self.forward(input)
        return (pred - target) ** 2

    def load_checkpoint(self, checkpoint_path, device):
        """Restores ``model_state_dict`` (reference key names / dtypes; weights only, as in the reference) and returns
        the bookkeeping entries of the checkpoint under the reference's meta-data names."""
        ckpt = torch.load(checkpoint_path, map_location=device)
        self.load_state_dict(ckpt["model_state_dict"])
        return {meta: ckpt[key] for key, meta in META_KEYS.items()}
