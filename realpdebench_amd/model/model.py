"""The ``Model`` plug-in protocol this backend implements (mirrors the reference's base class, realpdebench/model/model.py:4-26,
in meaning, not in text): ``forward``, ``train_loss`` and ``load_checkpoint(checkpoint_path, device) -> meta dict``."""
import torch
import torch.nn as nn

from .. import ops
from ._common import META_KEYS, LayoutCache


class Model(nn.Module):
    """Every MI355X model subclasses this; subclasses provide the HIP-backed ``forward``.

    The opt-in evaluation arithmetic is one protocol on every model: ``set_arith(name)`` takes a name of the
    class's ``ARITHS`` (the default first) and stores it as ``arith``; each class says in its own docstring what the switch moves.
    Where single products can be routed, ``ALL_F16X2_SITES`` names the ones that are wired and tested, ``F16X2_SITES`` the ones
    ``"f16x2"`` moves, and ``f16x2_ran`` the ones the last f16x2 evaluation forward did move, in the order of ``ALL_F16X2_SITES``."""
    ARITHS = ("f32", "f16x2")
    arith = "f32"
    ALL_F16X2_SITES = F16X2_SITES = ()
    f16x2_ran = ()
    # A class with routed token GEMMs names its kernel pair here, as names in ``ops``: (shape predicate, launch).  rpb_gemm3h holds K
    # up to 512 resident and rpb_gemm3hk streams K above 512; they stay two pairs, so that no site changes its kernel with its shape.
    F16X2_GEMM = None

    def __init__(self):
        super().__init__()
        self._layouts = LayoutCache()      # kernel-side layouts derived from the parameters

    def _apply(self, fn, *args, **kwargs):
        self._layouts.invalidate()
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        self._layouts.invalidate()
        return super().load_state_dict(*args, **kwargs)

    def set_arith(self, arith):
        """Each class says in its own docstring what the switch moves."""
        if arith not in self.ARITHS:
            names = [repr(a) for a in self.ARITHS]
            raise ValueError(f"arith must be {', '.join(names[:-1])} or {names[-1]}, got {arith!r}")
        self.arith = arith
        return self

    def _routed_planes(self, ran, site, key, sources, weight, M, N, K, **default_only):
        """The fp16 planes of ``site``'s weight if its product is routed to the class's f16x2 GEMM, else None.  Routed: the f16x2
        evaluation forward is running (``ran`` is its list of moved sites, None in every other forward), the site is in
        ``F16X2_SITES``, the kernel takes the shape, and no argument that only the default kernel has is set.  The planes come from
        the derived-weight cache: rebuilt when a source tensor changes in place or is rebound, and after ``load_state_dict``;
        ``weight`` (a tensor, or a callable where forming it costs a launch) is evaluated only then."""
        if ran is None or site not in self.F16X2_SITES or any(v is not None for v in default_only.values()):
            return None
        if not getattr(ops, self.F16X2_GEMM[0])(M, N, K):
            return None
        return self._layouts.get("f16x2_" + key, sources, lambda: ops.gemm3h_wprep(weight() if callable(weight) else weight))

    def _dense(self, ran, site, key, sources, weight, A, out, M, N, K, *, bias=None, act=0, residual=None, **default_only):
        """out[M,N] = epilogue(A[M,K] @ weight[N,K]^T), the only statement of a routed dense product: on the class's f16x2 GEMM, recorded
        in ``ran``, where ``_routed_planes`` routes it, else ``ops.gemm_nt`` with ``default_only`` (``pre_out``, ``mask``, ``drop`` ...)
        as well.  Returns the fp32 weight the default kernel read, for a caller that saves it for the backward, or None."""
        wz = self._routed_planes(ran, site, key, sources, weight, M, N, K, **default_only)
        if wz is not None:
            getattr(ops, self.F16X2_GEMM[1])(A, wz, out, M, N, K, bias=bias, act=act, residual=residual)
            ran.append(site)
            return None
        W = weight() if callable(weight) else weight
        ops.gemm_nt(A, W, out, M, N, K, bias=bias, act=act, residual=residual, **default_only)
        return W

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
