"""DPOT (AFNO patch transformer) on MI355X -- drop-in for ``realpdebench.model.dpot.DPOT`` with ``model_type='dpot'``
(reference realpdebench/model/dpot.py:21-289 wrapping dpot_libs/models/dpot.py:22-404), built by ``load_model`` like
``realpdebench/model/load_model.py:108-131`` for the configuration family of the reference's ``configs/*/dpot_{s,l}.yaml``:
2-D ``DPOTNet``, ``normalize=False``, GELU, ``time_agg`` 'exp_mlp' or 'mlp'; data at another resolution than ``img_size`` (the
reference's own samples are 64 x 128 / 64 x 64) goes through the wrapper's FFT ``resize`` (dpot_libs/utils/utilities.py:277) as
dense operators: one token GEMM over (w, channel) rows and two rpb_axis_gemm stages along h, in front of and behind the network.

Pipeline (token rows channels-last; every product runs in a HIP kernel of ``csrc/``):
  PatchEmbed (dpot.py:183-211): the wrapper's channel padding with ones, the (x, y, t) grid channels and the patch gather in ONE
  kernel (rpb_dpot_patch_tokens, token order (b, px, py, t)) -> token GEMM + GELU -> token GEMM (+ bias), + pos_embed
  (rpb_rowtable_add) -> TimeAggregator (dpot.py:227-241) as ONE token GEMM with K = T*E on weights pre-scaled by cos(t gamma)
  (rpb_dpot_tagg_prep; the (b, px, py, t) order makes the (t, channel) contraction contiguous) ->
  depth x Block (dpot.py:139-180): GroupNorm(8) (rpb_gn_tokens) -> AFNO2D (dpot.py:22-108): rfft2 / irfft2 as two small real DFT
  GEMM stages each (rpb_axis_gemm; all kept modes), the block-diagonal complex MLP on the fp32 MFMA (rpb_afno_mlp), + skip ->
  GroupNorm(8) -> 1x1-conv MLP as two token GEMMs (GELU / residual fused) ->
  out_layer (dpot.py:306-312): ConvTranspose2d(stride = kernel) as a token GEMM to pixel-major rows, two per-pixel GEMMs ->
  rpb_dpot_unpatch to ``[B, T_out, H, W, C_data]``.
The training backward mirrors it with the same kernels (data gradients = token GEMMs on transposed weights, weight gradients =
TN GEMMs, rpb_afno_mlp mode 1 / rpb_afno_wgrad, rpb_gn_tokens_bwd); there is no PyTorch fallback.  ``cls_head`` (dpot.py:296-302)
exists for state_dict compatibility; its output is discarded by the wrapper (model/dpot.py:224) and never computed here.
"""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ._common import HipFunction, colsum, sum_rows, wgrad
from .model import Model as _ModelBase


def _rup(v, m):
    return (v + m - 1) // m * m


def _out_cols(n):
    """Padded width of the last per-pixel layer: 32 / 64 / 128 (the streaming weight-gradient kernel's widths) when it fits."""
    return next((c for c in (32, 64, 128) if n <= c), _rup(n, 32))


class _AFNO2D(nn.Module):
    """Parameter container of dpot.py:22-48 (same shapes and initial distribution)."""

    def __init__(self, width, num_blocks):
        super().__init__()
        bs = width // num_blocks
        scale = 1.0 / (bs * bs)
        self.w1 = nn.Parameter(scale * torch.rand(2, num_blocks, bs, bs))
        self.b1 = nn.Parameter(scale * torch.rand(2, num_blocks, bs))
        self.w2 = nn.Parameter(scale * torch.rand(2, num_blocks, bs, bs))
        self.b2 = nn.Parameter(scale * torch.rand(2, num_blocks, bs))


class _Block(nn.Module):
    def __init__(self, width, n_blocks, mlp_ratio):
        super().__init__()
        hid = int(width * mlp_ratio)
        self.norm1 = nn.GroupNorm(8, width)
        self.filter = _AFNO2D(width, n_blocks)
        self.norm2 = nn.GroupNorm(8, width)
        self.mlp = nn.Sequential(nn.Conv2d(width, hid, 1), nn.GELU(), nn.Conv2d(hid, width, 1))


class _PatchEmbed(nn.Module):
    def __init__(self, patch, in_chans, embed_dim, out_dim):
        super().__init__()
        self.proj = nn.Sequential(nn.Conv2d(in_chans, embed_dim, patch, patch), nn.GELU(), nn.Conv2d(embed_dim, out_dim, 1))


class _TimeAgg(nn.Module):
    def __init__(self, n_t, C, kind):
        super().__init__()
        self.w = nn.Parameter(1 / (n_t * C ** 0.5) * torch.randn(n_t, C, C))
        if kind == "exp_mlp":
            self.gamma = nn.Parameter(2 ** torch.linspace(-10, 10, C).unsqueeze(0))


class _DPOTNet(nn.Module):
    """Parameter tree of dpot_libs/models/dpot.py:245-325 (names = the reference's state_dict keys)."""

    def __init__(self, img_size, patch_size, in_channels, out_channels, in_timesteps, out_timesteps, n_blocks, embed_dim,
                 out_layer_dim, depth, mlp_ratio, n_cls, time_agg):
        super().__init__()
        self.patch_embed = _PatchEmbed(patch_size, in_channels + 3, out_channels * patch_size + 3, embed_dim)
        n = img_size // patch_size
        self.pos_embed = nn.Parameter(torch.zeros(1, embed_dim, n, n))
        self.blocks = nn.ModuleList([_Block(embed_dim, n_blocks, mlp_ratio) for _ in range(depth)])
        self.cls_head = nn.Sequential(nn.Linear(embed_dim, embed_dim), nn.GELU(), nn.Linear(embed_dim, embed_dim), nn.GELU(),
                                      nn.Linear(embed_dim, n_cls))
        self.time_agg_layer = _TimeAgg(in_timesteps, embed_dim, time_agg)
        self.out_layer = nn.Sequential(nn.ConvTranspose2d(embed_dim, out_layer_dim, patch_size, patch_size), nn.GELU(),
                                       nn.Conv2d(out_layer_dim, out_layer_dim, 1), nn.GELU(),
                                       nn.Conv2d(out_layer_dim, out_channels * out_timesteps, 1))
        nn.init.trunc_normal_(self.pos_embed, std=.02)


class DPOT(_ModelBase):
    """``set_arith`` selects the arithmetic of the evaluation / rollout forward's dense products: ``"f32"`` (default, the parity path:
    token GEMMs from three bf16 planes with six products per fp32 product, the AFNO block MLP on the fp32 MFMA) or ``"f16x2"`` (opt-in:
    operands as two fp16 planes, three products, dropped term <= 2^-22; one power-of-two scale per weight tensor, one per token row for
    the GEMMs and one per (token, block) for the AFNO MLP, all formed on the device; csrc/rpb_gemm3hk.hip, csrc/rpb_dpot_h.hip, DESIGN.md
    section 14.1).  ``F16X2_SITES`` names the products that move; one whose shape ``rpb_gemm3hk_supported`` /
    ``rpb_afno_mlp_f16x2_supported`` refuses (``out2`` at K = 32, the narrow last layer) stays on the default kernel, and so does
    every other kernel of the model (DFT stages, GroupNorm, PatchEmbed's first GEMM, the spectral resize).  Only ``_forward_hip``
    without saved activations changes -- eval and rollout, every window of the sliding-window path included; the training step is
    the same under either setting.  The fp16 planes live in the derived-weight cache and cost 4 bytes per weight element of the
    moved sites: about the size of the fp32 weights themselves (about 2.5 GB with every site on at dpot_l: 1.8 GB FeedForward, 0.6 GB
    out0, 0.1 GB AFNO composites)."""
    batch_independent = True      # no batch statistics (GroupNorm / LayerNorm): a step may run in micro-batches (trainer.ArenaTrainer)
    # The products set_arith("f16x2") can move: FeedForward "mlp0" (bias + GELU, K = E) and "mlp2" (bias + residual, K = hidden), the
    # out layer's "out0" (bias + GELU, N = ps^2 OD) and "out2" (bias + GELU, K = OD), the TimeAggregator's "tagg" (H1 . WcT, K = T E1p)
    # on rpb_gemm3hk, and the AFNO block MLP "afno" on rpb_afno_mlp_f16x2.  ALL_F16X2_SITES is what is wired and tested; F16X2_SITES
    # is the default routing, by the rule of DESIGN.md section 13.3: a site is in it only if profiles/dpot_arith_probe.txt shows it
    # faster than the default kernel in the same run by more than the spread.  All six are, at dpot_s and dpot_l, B = 16 and 64:
    # mlp0 1.14x-2.03x, mlp2 1.11x-1.82x, out0 1.28x-2.60x, out2 1.63x-1.68x, tagg 1.20x-1.74x, afno 1.70x-1.84x; the eval forward
    # 7.91 -> 6.51 ms (dpot_s, B = 64) and 197.3 -> 106.3 ms (dpot_l, B = 64).
    ALL_F16X2_SITES = ("mlp0", "mlp2", "out0", "out2", "tagg", "afno")
    F16X2_SITES = ALL_F16X2_SITES
    F16X2_GEMM = ("gemm3hk_supported", "gemm_nt_f16x2k")

    def __init__(self, shape_in, shape_out, img_size=128, in_channels=4, out_channels=4, in_timesteps=1, out_timesteps=1,
                 patch_size=8, embed_dim=512, depth=12, n_blocks=8, modes=32, mlp_ratio=4, out_layer_dim=32, normalize=False,
                 act="gelu", time_agg="exp_mlp", n_cls=1, model_type="dpot", checkpoint_path=None, **kwargs):
        super().__init__()
        self.shape_in, self.shape_out = tuple(int(v) for v in shape_in), tuple(int(v) for v in shape_out)
        unsupported = []
        if model_type != "dpot":
            unsupported.append(f"model_type={model_type!r} (DPOTNet3D)")
        if normalize:
            unsupported.append("normalize=True")
        if act != "gelu":
            unsupported.append(f"act={act!r}")
        if time_agg not in ("exp_mlp", "mlp"):
            unsupported.append(f"time_agg={time_agg!r}")
        if kwargs.get("mixing_type", "afno") != "afno":
            unsupported.append("mixing_type != 'afno'")
        if embed_dim % n_blocks or (embed_dim // n_blocks) % 16 or embed_dim % 32 or embed_dim % 8:
            unsupported.append(f"embed_dim={embed_dim} / n_blocks={n_blocks} (block size must be a multiple of 16)")
        if ((in_channels + 3) * patch_size * patch_size) % 32 or out_layer_dim % 32 or int(embed_dim * mlp_ratio) % 32:
            unsupported.append("patch / out_layer / mlp widths must give GEMM depths that are multiples of 32")
        if img_size % patch_size:
            unsupported.append("img_size % patch_size != 0")
        self.needs_resize = tuple(self.shape_in[1:3]) != (img_size, img_size)
        if self.needs_resize and ((self.shape_in[2] * self.shape_in[-1]) % 32 or (img_size * self.shape_in[-1]) % 32
                                  or (self.shape_out[2] * self.shape_out[-1]) % 32 or (img_size * self.shape_out[-1]) % 32):
            unsupported.append(f"data resolution {self.shape_in[1:3]} != img_size {img_size} with width x channels not a multiple "
                               "of 32 (the spectral resize runs as token GEMMs over (w, channel) rows)")
        if unsupported:
            raise NotImplementedError("MI355X DPOT covers the configuration family of the reference's configs/*/dpot_*.yaml "
                                      "at the model's native resolution; unsupported: " + "; ".join(unsupported))
        self.data_in_channels, self.data_out_channels = self.shape_in[-1], self.shape_out[-1]
        self.data_in_timesteps, self.data_out_timesteps = self.shape_in[0], self.shape_out[0]
        assert self.data_in_timesteps == in_timesteps, \
            f"Data input timesteps ({self.data_in_timesteps}) must be equal to in_timesteps ({in_timesteps})"       # model/dpot.py:82
        assert self.data_out_timesteps >= out_timesteps
        if self.data_in_channels > in_channels or (self.data_in_channels < in_channels and in_channels != 4):
            raise ValueError("data channels are padded with ones up to the model's 4 input channels (model/dpot.py:213-221)")
        if self.data_out_channels > out_channels:
            raise ValueError("out_channels must cover the data's output channels (model/dpot.py:110-112)")
        self.img_size, self.patch_size = int(img_size), int(patch_size)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.in_timesteps, self.out_timesteps = int(in_timesteps), int(out_timesteps)
        self.embed_dim, self.depth, self.n_blocks, self.modes = int(embed_dim), int(depth), int(n_blocks), int(modes)
        self.hidden = int(embed_dim * mlp_ratio)
        self.out_layer_dim, self.time_agg, self.model_type = int(out_layer_dim), time_agg, model_type
        self.checkpoint_path = checkpoint_path
        self.dpot_model = _DPOTNet(img_size, patch_size, in_channels, out_channels, in_timesteps, out_timesteps, n_blocks, embed_dim,
                                   out_layer_dim, depth, mlp_ratio, n_cls, time_agg)
        self._plan = None
        if checkpoint_path is not None:
            self.load_checkpoint(checkpoint_path)

    # ------------------------------------------------------------------ checkpoints (model/dpot.py:291-400)
    def load_checkpoint(self, checkpoint_path, device="cpu"):
        try:                                               # model/dpot.py:320-324: safe load first; the released DPOT files carry an
            ck = torch.load(checkpoint_path, map_location="cpu", weights_only=True)       # argparse.Namespace and need the fallback
        except Exception:
            import logging
            logging.warning("DPOT.load_checkpoint: %s needs weights_only=False (pickled non-tensor objects); only load files you trust",
                            checkpoint_path)
            ck = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        sd = ck.get("model", ck.get("model_state_dict", ck)) if isinstance(ck, dict) else ck
        own = self.dpot_model.state_dict()
        ok = {}
        for k, v in sd.items():
            for pre in ("dpot_model.", "module."):
                if k.startswith(pre):
                    k = k[len(pre):]
            if k in own and tuple(v.shape) == tuple(own[k].shape):
                ok[k] = v
        self.dpot_model.load_state_dict(ok, strict=False)
        self.dpot_model.to(device)
        keys = ("train_losses", "val_losses", "iteration", "best_iteration", "best_val_loss")
        if isinstance(ck, dict) and all(k in ck for k in keys):            # model/dpot.py:390-399: this trainer's own checkpoints
            return {"all_train_losses": ck["train_losses"], "all_val_losses": ck["val_losses"], "iteration": ck["iteration"],
                    "best_iteration": ck["best_iteration"], "best_val_loss": ck["best_val_loss"]}
        return None

    # ------------------------------------------------------------------ constants
    def _consts(self, device):
        if self._plan is not None and self._plan["device"] == device:
            return self._plan
        n = self.img_size // self.patch_size
        mk = min(self.modes, n)                    # dpot.py:69-72: x[:, :kept, :kept] (slices clip at the spectrum's extent)
        mky = min(self.modes, n // 2 + 1)
        x = np.arange(n)
        sq = 1.0 / math.sqrt(n)
        th = 2 * np.pi * np.outer(x, np.arange(mk)) / n                          # [x][kx]
        F1 = np.zeros((n, 2 * mk))
        F1[:, 0::2], F1[:, 1::2] = np.cos(th) * sq, -np.sin(th) * sq
        thy = 2 * np.pi * np.outer(x, np.arange(mky)) / n                        # [y][ky]
        F2 = np.zeros((2 * n, 2 * mky))                                          # k = (ri, y) -> o = (ky, ri')
        F2[:n, 0::2], F2[n:, 0::2] = np.cos(thy) * sq, np.sin(thy) * sq
        F2[:n, 1::2], F2[n:, 1::2] = -np.sin(thy) * sq, np.cos(thy) * sq
        cw = np.full(mky, 2.0)
        cw[0] = 1.0
        if n % 2 == 0 and mky == n // 2 + 1:
            cw[-1] = 1.0
        I1 = np.zeros((2 * mky, 2 * n))                                          # k = (ky, ri) -> o = (ri', y)
        c, s = (np.cos(thy) * sq * cw).T, (np.sin(thy) * sq * cw).T              # [ky][y]
        I1[0::2, :n], I1[1::2, :n] = c, -s
        I1[0::2, n:], I1[1::2, n:] = s, c
        I2 = np.zeros((2 * mk, n))                                               # k = (kx, ri) -> o = x
        I2[0::2, :], I2[1::2, :] = (np.cos(th) * sq).T, (-np.sin(th) * sq).T
        f = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)
        T = self.in_timesteps
        lin = lambda m: torch.tensor(np.linspace(0, 1, m), dtype=torch.float32)                 # dpot.py:352-363
        self._plan = dict(device=device, n=n, mk=mk, mky=mky, F1=f(F1), F2=f(F2), I1=f(I1), I2=f(I2), F1t=f(F1.T), F2t=f(F2.T),
                          I1t=f(I1.T), I2t=f(I2.T), gx=lin(self.img_size).to(device), gy=lin(self.img_size).to(device),
                          gt=lin(T).to(device), tt=torch.linspace(0, 1, T).to(device))           # dpot.py:238
        return self._plan

    # ------------------------------------------------------------------ spectral resize (dpot_libs/utils/utilities.py:277-305)
    @staticmethod
    def _resize_ops(n_in, n_out, C, device):
        """``resize`` = irfft2 . (copy the low-frequency corners) . rfft2, scaled by the size ratio -- a linear map of each (h, w) plane.
        With Cx = IFFT_x S_x FFT_x = A + iB (complex, [Ho x Hi]) and the real matrices Ry = c2r_y S_y rfft_y, Qy = c2r_y S_y (i rfft_y)
        ([Wo x Wi]) it is  T(X) = A X Ry^T + B X Qy^T  (B != 0 when an even size keeps only one of the two +-Nyquist rows).
        Returned: KY [(2, w', c)][(w, c)] = [Ry; Qy] (x) I_C for the (w, channel)-row token GEMM, AXt / BXt [h][h'] as rpb_axis_gemm
        stage matrices, and their transposes for the adjoint.  Built in fp64 from numpy's FFT applied to the identity."""
        (hi, wi), (ho, wo) = n_in, n_out
        top1, bot1 = min((hi + 1) // 2, (ho + 1) // 2), min(hi // 2, ho // 2)
        top2 = min(wi // 2 + 1, wo // 2 + 1)
        Fx = np.fft.fft(np.eye(hi), axis=0)                                   # [kx][h]
        Sel = np.zeros((ho, hi), dtype=complex)                                # f_z rows <- f rows
        Sel[:top1] = Fx[:top1]
        if bot1 > 0:
            Sel[ho - bot1:] = Fx[hi - bot1:]
        Cx = np.fft.ifft(Sel, axis=0) * (ho / hi)                              # [h'][h]; ifft carries 1/Ho
        Fy = np.fft.rfft(np.eye(wi), axis=0)                                   # [ky][w]
        Zy = np.zeros((wo // 2 + 1, wi), dtype=complex)
        Zy[:top2] = Fy[:top2]
        Ry = np.fft.irfft(Zy, n=wo, axis=0) * (wo / wi)                        # [w'][w]
        Qy = np.fft.irfft(1j * Zy, n=wo, axis=0) * (wo / wi)
        eye = np.eye(C)
        KY = np.concatenate([np.kron(Ry, eye), np.kron(Qy, eye)], 0)           # [(term, w', c)][(w, c)]
        f = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float32, device=device)
        A, Bm = Cx.real, Cx.imag
        return dict(KY=f(KY), KYt=f(KY.T), AXt=f(A.T), BXt=f(Bm.T), AX=f(A), BX=f(Bm), n_in=n_in, n_out=n_out, C=C)

    def _resize_plan(self, device):
        if getattr(self, "_rs", None) is not None and self._rs["device"] == device:
            return self._rs
        S = self.img_size
        (Hi, Wi, Ci), (Ho, Wo, Co) = self.shape_in[1:], self.shape_out[1:]
        self._rs = dict(device=device, inp=self._resize_ops((Hi, Wi), (S, S), Ci, device),
                        out=self._resize_ops((S, S), (Ho, Wo), Co, device))
        return self._rs

    @staticmethod
    def _resize_apply(x, op, adjoint=False):
        """x [G, h, w, C] (G = B*T) -> [G, h', w', C]; ``adjoint``: the transposed map (gradient w.r.t. the resize input)."""
        (hi, wi), (ho, wo), C = op["n_in"], op["n_out"], op["C"]
        G = x.shape[0]
        f = dict(device=x.device, dtype=torch.float32)
        if not adjoint:
            tmp = torch.empty(G * hi, 2 * wo * C, **f)
            ops.gemm_nt(x, op["KY"], tmp, G * hi, 2 * wo * C, wi * C)
            out = torch.empty(G, ho, wo, C, **f)
            N = wo * C
            ops.axis_gemm(tmp, out, op["AXt"], G, hi, ho, N, hi * 2 * N, 2 * N, ho * N, N, tag="resizeA")
            ops.axis_gemm(ops.Sub(tmp, N), out, op["BXt"], G, hi, ho, N, hi * 2 * N, 2 * N, ho * N, N, accumulate=True, tag="resizeB")
            return out
        N = wo * C
        tmp = torch.empty(G * hi, 2 * N, **f)
        ops.axis_gemm(x, tmp, op["AX"], G, ho, hi, N, ho * N, N, hi * 2 * N, 2 * N, tag="resizeAt")
        ops.axis_gemm(x, ops.Sub(tmp, N), op["BX"], G, ho, hi, N, ho * N, N, hi * 2 * N, 2 * N, tag="resizeBt")
        out = torch.empty(G, hi, wi, C, **f)
        ops.gemm_nt(tmp, op["KYt"], out, G * hi, wi * C, 2 * N)
        return out

    # ------------------------------------------------------------------ spectral stages
    def _rfft2(self, Y, A1, S, B, pl, E, fwd=True):
        """fwd: tokens Y [B][n][n][E] -> S [(b,kx,ky)][2][E];  not fwd: the adjoint (S -> Y)."""
        n, mk, mky = pl["n"], pl["mk"], pl["mky"]
        if fwd:
            ops.axis_gemm(Y, A1, pl["F1"], B, n, 2 * mk, n * E, n * n * E, n * E, 2 * mk * n * E, n * E, tag="dpotF1")
            ops.axis_gemm(A1, S, pl["F2"], B * mk, 2 * n, 2 * mky, E, 2 * n * E, E, 2 * mky * E, E, tag="dpotF2")
        else:
            ops.axis_gemm(S, A1, pl["F2t"], B * mk, 2 * mky, 2 * n, E, 2 * mky * E, E, 2 * n * E, E, tag="dpotF2t")
            ops.axis_gemm(A1, Y, pl["F1t"], B, 2 * mk, n, n * E, 2 * mk * n * E, n * E, n * n * E, n * E, tag="dpotF1t")

    def _irfft2(self, Z, A1, Y, B, pl, E, fwd=True):
        n, mk, mky = pl["n"], pl["mk"], pl["mky"]
        if fwd:
            ops.axis_gemm(Z, A1, pl["I1"], B * mk, 2 * mky, 2 * n, E, 2 * mky * E, E, 2 * n * E, E, tag="dpotI1")
            ops.axis_gemm(A1, Y, pl["I2"], B, 2 * mk, n, n * E, 2 * mk * n * E, n * E, n * n * E, n * E, tag="dpotI2")
        else:
            ops.axis_gemm(Y, A1, pl["I2t"], B, n, 2 * mk, n * E, n * n * E, n * E, 2 * mk * n * E, n * E, tag="dpotI2t")
            ops.axis_gemm(A1, Z, pl["I1t"], B * mk, 2 * n, 2 * mky, E, 2 * n * E, E, 2 * mky * E, E, tag="dpotI1t")

    # ------------------------------------------------------------------ forward (one window)
    @torch.no_grad()
    def _forward_hip(self, x, save=None):
        net = self.dpot_model
        if self.needs_resize:                                  # model/dpot.py:204-208: data resolution -> the model's
            rs = self._resize_plan(x.device)
            Bx, Tx = x.shape[:2]
            x = self._resize_apply(x.reshape(Bx * Tx, *x.shape[2:]), rs["inp"]).view(Bx, Tx, self.img_size, self.img_size, x.shape[-1])
        B, T, H, W, Cd = x.shape
        E, ps, Cm, Co, To = self.embed_dim, self.patch_size, self.in_channels, self.out_channels, self.out_timesteps
        pl = self._consts(x.device)
        n, mk, mky = pl["n"], pl["mk"], pl["mky"]
        f = dict(device=x.device, dtype=torch.float32)
        new = lambda *shape: torch.empty(*shape, **f)
        nb, bs = self.n_blocks, E // self.n_blocks
        Mt, M1 = B * n * n, B * n * n * T
        training = save is not None
        ran = [] if self.arith == "f16x2" and not training else None      # the f16x2 eval forward: the sites it moved
        # ---- PatchEmbed
        Kp = (Cm + 3) * ps * ps
        E1 = Co * ps + 3
        E1p = _rup(E1, 32)
        P = new(M1, Kp)
        ops.dpot_patch_tokens(x, pl["gx"], pl["gy"], pl["gt"], P, B, T, H, W, Cd, Cm, ps)
        pe0, pe2 = net.patch_embed.proj[0], net.patch_embed.proj[2]
        H1 = torch.zeros(M1, E1p, **f)
        H1pre = torch.zeros(M1, E1p, **f) if training else None
        ops.gemm_nt(P, pe0.weight.data.view(E1, Kp), H1, M1, E1, Kp, bias=pe0.bias.data, act=1, ldo=E1p, pre_out=H1pre)
        W2p = torch.zeros(E, E1p, **f)
        W2p[:, :E1] = pe2.weight.data.view(E, E1)
        pos = net.pos_embed.data[0].permute(1, 2, 0).reshape(n * n, E).contiguous()
        ta = net.time_agg_layer
        gamma = ta.gamma.data.view(E) if self.time_agg == "exp_mlp" else torch.zeros(E, **f)
        Wf, Wb, ecos = new(E, T * E), new(T * E, E), new(T, E)
        ops.dpot_tagg_prep(ta.w.data, gamma, pl["tt"], Wf, Wb, ecos, T, E)
        X = new(Mt, E)
        # PatchEmbed's second conv, + pos_embed and the TimeAggregator are one linear map of the 35-wide hidden layer: contract the
        # weights first -- WcT[j][(t, k)] = sum_i (cos(t gamma_i) w[t][i][j]) W2[i][k] (20 small GEMMs), the constant part
        # (b2 + pos[xy]) sum_t Wb_t -- and the aggregation is ONE token GEMM with K = T * 64 instead of T * E (29x fewer FLOPs on the
        # largest product of the model; the [B n^2 T][E] token tensor is never materialised).  The layer-0 algebra of the FNO path again.
        W2pT = W2p.t().contiguous()
        WcT = new(E, T * E1p)                                              # rows (j, t) of Wf x W2^T: one GEMM, M = E * T
        ops.gemm_nt(Wf, W2pT, WcT, E * T, E1p, E)
        tsrc = [pe2.weight, ta.w] + ([ta.gamma] if self.time_agg == "exp_mlp" else [])      # what WcT is made of
        self._dense(ran, "tagg", "tagg", tsrc, WcT, H1, X, Mt, E, T * E1p)
        WsumT = new(E, E)                                                  # [j][i] = sum_t Wb[(t, i)][j]
        ops.reduce_partials_batched(Wf, E, T, E, WsumT)
        posb = pos + pe2.bias.data                                         # [n^2][E]: parameter-sized
        PosT = new(n * n, E)
        ops.gemm_nt(posb, WsumT, PosT, n * n, E, E)
        ops.rowtable_add(X, PosT, Mt, E, 1, n * n)
        if not training:
            del Wf
        # ---- blocks
        ntok = B * mk * mky
        tapes = []
        A1 = new(B * 2 * mk * n * E)
        afno_h = ran is not None and "afno" in self.F16X2_SITES and ops.afno_f16x2_supported(nb, bs)
        for bi, blk in enumerate(net.blocks):
            fl = blk.filter
            Y1, st1 = new(Mt, E), new(B * 8, 2)
            ops.gn_tokens_fwd(X, None, blk.norm1.weight.data, blk.norm1.bias.data, Y1, st1, B, n * n, E, 8, blk.norm1.eps)
            S = new(ntok, 2 * E)
            self._rfft2(Y1, A1, S, B, pl, E)
            Hs = new(ntok, 2 * E) if training else None
            O2 = new(ntok, 2 * E)
            if afno_h:
                w1z = self._layouts.get(f"f16x2_afno1_{bi}", [fl.w1], lambda: ops.afno_wprep_f16x2(fl.w1.data, nb, bs))
                w2z = self._layouts.get(f"f16x2_afno2_{bi}", [fl.w2], lambda: ops.afno_wprep_f16x2(fl.w2.data, nb, bs))
                ops.afno_mlp_f16x2(S, w1z, fl.b1.data, w2z, fl.b2.data, O2, ntok, nb, bs)
                ran.append("afno")
            else:
                W1c, W2c = new(nb, 2 * bs, 2 * bs), new(nb, 2 * bs, 2 * bs)
                ops.afno_wprep(fl.w1.data, W1c, nb, bs, False)
                ops.afno_wprep(fl.w2.data, W2c, nb, bs, False)
                ops.afno_mlp(S, W1c, fl.b1.data, W2c, fl.b2.data, None, Hs, O2, ntok, nb, bs, 0)
            Fo = new(Mt, E)
            self._irfft2(O2, A1, Fo, B, pl, E)
            Y2, st2 = new(Mt, E), new(B * 8, 2)
            ops.gn_tokens_fwd(Fo, Y1, blk.norm2.weight.data, blk.norm2.bias.data, Y2, st2, B, n * n, E, 8, blk.norm2.eps)
            m0, m2 = blk.mlp[0], blk.mlp[2]
            hid = self.hidden
            Hh = new(Mt, hid)
            Hpre = new(Mt, hid) if training else None
            self._dense(ran, "mlp0", f"mlp0_{bi}", [m0.weight], m0.weight.data.view(hid, E), Y2, Hh, Mt, hid, E, bias=m0.bias.data,
                        act=1, pre_out=Hpre)
            Xn = new(Mt, E)
            self._dense(ran, "mlp2", f"mlp2_{bi}", [m2.weight], m2.weight.data.view(E, hid), Hh, Xn, Mt, E, hid, bias=m2.bias.data,
                        residual=X)
            if training:
                tapes.append(dict(X=X, Y1=Y1, st1=st1, S=S, Hs=Hs, Fo=Fo, st2=st2, Y2=Y2, Hh=Hh, Hpre=Hpre))
            X = Xn
        # ---- out_layer
        ol0, ol2, ol4 = net.out_layer[0], net.out_layer[2], net.out_layer[4]
        OD = self.out_layer_dim
        NU = ps * ps * OD
        wt = lambda: ol0.weight.data.permute(2, 3, 1, 0).reshape(NU, E).contiguous()    # [(i, j, oc)][c]
        bt = ol0.bias.data.repeat(ps * ps)
        U = new(Mt, NU)
        Upre = new(Mt, NU) if training else None
        Wt = self._dense(ran, "out0", "out0", [ol0.weight], wt, X, U, Mt, NU, E, bias=bt, act=1, pre_out=Upre)      # (planes of the permuted Wt)
        Mp = Mt * ps * ps
        V = new(Mp, OD)
        Vpre = new(Mp, OD) if training else None
        self._dense(ran, "out2", "out2", [ol2.weight], ol2.weight.data.view(OD, OD), U, V, Mp, OD, OD, bias=ol2.bias.data, act=1,
                    pre_out=Vpre)
        NO = To * Co
        NOp = _out_cols(NO)
        W3p, b3p = torch.zeros(NOp, OD, **f), torch.zeros(NOp, **f)
        W3p[:NO] = ol4.weight.data.view(NO, OD)
        b3p[:NO] = ol4.bias.data
        O = new(Mp, NOp)
        ops.gemm_nt(V, W3p, O, Mp, NOp, OD, bias=b3p)
        Cdo = self.data_out_channels
        pred = new(B, To, H, W, Cdo)
        ops.dpot_unpatch(O, pred, B, To, H, W, Cdo, Co, ps, NOp)
        if self.needs_resize:                                  # model/dpot.py:229-231: back to the data resolution
            Ho, Wo = self.shape_out[1:3]
            pred = self._resize_apply(pred.view(B * To, H, W, Cdo), rs["out"]).view(B, To, Ho, Wo, Cdo)
        if ran is not None:
            self.f16x2_ran = tuple(s for s in self.ALL_F16X2_SITES if s in ran)
        if training:
            save.update(B=B, Cd=Cd, P=P, H1=H1, H1pre=H1pre, W2p=W2p, Wb=Wb, ecos=ecos, gamma=gamma, tapes=tapes, Xlast=X, Wt=Wt,
                        WcT=WcT, WsumT=WsumT, posb=posb, Wf=Wf,
                        U=U, Upre=Upre, V=V, Vpre=Vpre, W3p=W3p)
        return pred

    # ------------------------------------------------------------------ backward
    @torch.no_grad()
    def _backward_hip(self, sv, g_pred, need_gx=False):
        """{parameter: gradient}; with ``need_gx`` also ``grads['__x__']``, the gradient w.r.t. the window's input frames (sliding-window
        training feeds predictions back in as inputs, model/dpot.py:256-309)."""
        net = self.dpot_model
        B = sv["B"]
        E, ps, Cm, Co, To, T = self.embed_dim, self.patch_size, self.in_channels, self.out_channels, self.out_timesteps, self.in_timesteps
        H = W = self.img_size
        pl = self._consts(g_pred.device)
        n, mk, mky = pl["n"], pl["mk"], pl["mky"]
        f = dict(device=g_pred.device, dtype=torch.float32)
        new = lambda *shape: torch.empty(*shape, **f)
        Tr = lambda w: w.t().contiguous()
        nb, bs, hid, OD = self.n_blocks, E // self.n_blocks, self.hidden, self.out_layer_dim
        Mt, M1, Mp = B * n * n, B * n * n * T, B * n * n * ps * ps
        NO, NOp, NU = To * Co, _out_cols(To * Co), ps * ps * OD
        Cdo = self.data_out_channels
        grads = {}
        ol0, ol2, ol4 = net.out_layer[0], net.out_layer[2], net.out_layer[4]
        if self.needs_resize:
            rs = self._resize_plan(g_pred.device)
            g_pred = self._resize_apply(g_pred.reshape(B * To, *g_pred.shape[2:]), rs["out"], adjoint=True).view(B, To, H, W, Cdo)
        # ---- out_layer
        gO = new(Mp, NOp)
        ops.dpot_unpatch_bwd(g_pred, gO, B, To, H, W, Cdo, Co, ps, NOp)
        dW3, db3 = self._wgrad_rows(gO, sv["V"], Mp, NOp, OD)
        grads[ol4.weight], grads[ol4.bias] = dW3[:NO].reshape(ol4.weight.shape).contiguous(), db3[:NO].contiguous()
        gV = new(Mp, OD)
        ops.gemm_nt(gO, Tr(sv["W3p"]), gV, Mp, OD, NOp, act=2, aux=sv["Vpre"])
        del gO
        dW2, db2 = self._wgrad_rows(gV, sv["U"], Mp, OD)
        grads[ol2.weight], grads[ol2.bias] = dW2.reshape(ol2.weight.shape), db2
        gU = new(Mt, NU)
        ops.gemm_nt(gV, Tr(ol2.weight.data.view(OD, OD)), gU, Mp, OD, OD, act=2, aux=sv["Upre"])
        del gV
        dWt, dbt = wgrad(gU, sv["Xlast"], Mt, NU, E, one_reduction=True)
        grads[ol0.weight] = dWt.view(ps, ps, OD, E).permute(3, 2, 0, 1).contiguous()
        grads[ol0.bias] = dbt.view(ps * ps, OD).sum(0)
        g = new(Mt, E)
        ops.gemm_nt(gU, Tr(sv["Wt"]), g, Mt, E, NU)
        del gU
        # ---- blocks, last to first
        ntok = B * mk * mky
        A1 = new(B * 2 * mk * n * E)
        splits = ops.afno_wgrad_splits(ntok)
        wpart = new(splits * nb * 4 * bs * bs)
        # every block ends ~10 partial reductions (weight / bias / norm gradients) that nobody reads before the pass is over: they are
        # queued and run as ONE grouped launch after the loop (68 launches of ~15 us were 1.0 of the 9.8 ms step)
        defer = ops.deferred_reductions()
        with defer:
            for blk, tp in zip(reversed(list(net.blocks)), reversed(sv["tapes"])):
                fl, m0, m2 = blk.filter, blk.mlp[0], blk.mlp[2]
                dWm2, dbm2 = wgrad(g, tp["Hh"], Mt, E, hid, one_reduction=True)
                grads[m2.weight], grads[m2.bias] = dWm2.reshape(m2.weight.shape), dbm2
                gH = new(Mt, hid)
                ops.gemm_nt(g, Tr(m2.weight.data.view(E, hid)), gH, Mt, hid, E, act=2, aux=tp["Hpre"])
                dWm0, dbm0 = wgrad(gH, tp["Y2"], Mt, hid, E, one_reduction=True)
                grads[m0.weight], grads[m0.bias] = dWm0.reshape(m0.weight.shape), dbm0
                gY2 = new(Mt, E)
                ops.gemm_nt(gH, Tr(m0.weight.data.view(hid, E)), gY2, Mt, E, hid)
                del gH
                pg, pb = new(B, E), new(B, E)
                gz = new(Mt, E)
                ops.gn_tokens_bwd(tp["Fo"], tp["Y1"], blk.norm2.weight.data, tp["st2"], gY2, None, gz, pg, pb, B, n * n, E, 8)
                grads[blk.norm2.weight] = sum_rows(pg, B, E, deferrable=True)
                grads[blk.norm2.bias] = sum_rows(pb, B, E, deferrable=True)
                # AFNO: z = irfft2(mlp_c(rfft2(y1))) + y1
                gO2 = new(ntok, 2 * E)
                self._irfft2(gO2, A1, gz, B, pl, E, fwd=False)
                W2t, W1t = new(nb, 2 * bs, 2 * bs), new(nb, 2 * bs, 2 * bs)
                ops.afno_wprep(fl.w2.data, W2t, nb, bs, True)
                ops.afno_wprep(fl.w1.data, W1t, nb, bs, True)
                gHs, gS = new(ntok, 2 * E), new(ntok, 2 * E)
                ops.afno_mlp(gO2, W2t, None, W1t, None, tp["Hs"], gHs, gS, ntok, nb, bs, 1)
                dw2, dw1 = torch.empty_like(fl.w2), torch.empty_like(fl.w1)
                ops.afno_wgrad(tp["Hs"], gO2, wpart, dw2, ntok, nb, bs, True)
                ops.afno_wgrad(tp["S"], gHs, wpart, dw1, ntok, nb, bs, False)
                grads[fl.w2], grads[fl.w1] = dw2, dw1
                grads[fl.b2] = colsum(gO2, ntok, 2 * E, deferrable=True).view(fl.b2.shape)
                grads[fl.b1] = colsum(gHs, ntok, 2 * E, deferrable=True).view(fl.b1.shape)
                gY1 = new(Mt, E)
                self._rfft2(gY1, A1, gS, B, pl, E, fwd=False)
                gY1 = ops.add(gY1, gz)
                gX = new(Mt, E)
                pg, pb = new(B, E), new(B, E)                  # (fresh partial rows: norm2's are still waiting for the grouped reduction)
                ops.gn_tokens_bwd(tp["X"], None, blk.norm1.weight.data, tp["st1"], gY1, g, gX, pg, pb, B, n * n, E, 8)
                grads[blk.norm1.weight] = sum_rows(pg, B, E, deferrable=True)
                grads[blk.norm1.bias] = sum_rows(pb, B, E, deferrable=True)
                g = gX
        # ---- TimeAggregator
        ta = net.time_agg_layer
        pe0, pe2 = net.patch_embed.proj[0], net.patch_embed.proj[2]
        E1 = Co * ps + 3
        E1p = _rup(E1, 32)
        Kp = (Cm + 3) * ps * ps
        dw, dgamma = torch.empty_like(ta.w), new(E)
        # adjoint of the contracted map X0 = Hb WcT^T + (b2 + pos) Wsum  (Hb = the hidden layer as [B n^2][T * 64] rows)
        Hb, W2p, WcT = sv["H1"], sv["W2p"], sv["WcT"]
        KT = T * E1p
        GP = new(n * n, E)
        ops.rowtable_grad(g, GP, B, E, 1, n * n)                            # sum over the samples
        Wsum = Tr(sv["WsumT"])                                              # [i][j]
        dposb = new(n * n, E)
        ops.gemm_nt(GP, Wsum, dposb, n * n, E, E)
        grads[net.pos_embed] = dposb.view(n, n, E).permute(2, 0, 1).unsqueeze(0).contiguous()
        grads[pe2.bias] = colsum(dposb, n * n, E, deferrable=True)
        dWsum, _ = wgrad(sv["posb"], GP, n * n, E, E, one_reduction=True)          # [i][j]
        dWcT, _ = wgrad(g, Hb, Mt, E, KT, ldg=E, lda=KT, one_reduction=True)       # [j][(t, k)]
        gH1 = new(M1, E1p)
        ops.gemm_nt(g, Tr(WcT), gH1, Mt, KT, E, act=2, aux=sv["H1pre"])      # d hidden pre-activation, rows [B n^2][T * 64]
        dWf = new(E, T * E)                                                 # [j][(t, i)] = sum_k dWcT[j][(t, k)] W2[i][k]: rows (j, t)
        ops.gemm_nt(dWcT, W2p, dWf, E * T, E, E1p)
        dW2p, _ = wgrad(sv["Wf"], dWcT, E * T, E, E1p, ldg=E, lda=E1p, one_reduction=True)     # [i][k] = sum_(j,t) Wf[(j,t)][i] dWcT[(j,t)][k]
        dWb = dWf.view(E, T, E).permute(1, 2, 0).contiguous()               # parameter-sized re-layout to [(t, i)][j]
        ops.dpot_tagg_finish(dWb, ta.w.data, sv["gamma"], pl["tt"], dw, dgamma, T, E, dWsum=dWsum)
        del dWb, dWf
        grads[pe2.weight] = dW2p[:, :E1].reshape(pe2.weight.shape).contiguous()
        grads[ta.w] = dw
        if self.time_agg == "exp_mlp":
            grads[ta.gamma] = dgamma.view(1, E)
        dW1, db1 = wgrad(gH1, sv["P"], M1, E1, Kp, ldg=E1p, lda=Kp, one_reduction=True)
        grads[pe0.weight], grads[pe0.bias] = dW1.reshape(pe0.weight.shape), db1
        if need_gx:
            # gradient of the token rows, then the inverse of the patch gather (patches do not overlap) and of the input resize
            W1p = torch.zeros(E1p, Kp, **f)
            W1p[:E1] = pe0.weight.data.view(E1, Kp)
            gP = new(M1, Kp)
            ops.gemm_nt(gH1, Tr(W1p), gP, M1, Kp, E1p)
            Cd = sv["Cd"]
            gx = new(B, T, H, W, Cd)
            ops.dpot_patch_tokens_bwd(gP, gx, B, T, H, W, Cd, Cm, ps)
            if self.needs_resize:
                rs = self._resize_plan(g_pred.device)
                Hi, Wi = rs["inp"]["n_in"]
                gx = self._resize_apply(gx.view(B * T, H, W, Cd), rs["inp"], adjoint=True).view(B, T, Hi, Wi, Cd)
            grads["__x__"] = gx
        return grads

    @staticmethod
    def _wgrad_rows(G, A, M, CO, CI=None):
        """(dW [CO][CI], db [CO]) = (G^T A, colsum G) for the per-pixel layers over M >> C rows: the streaming weight-gradient kernel of
        the FNO path (both operands read once in MFMA layout) instead of the split-token TN GEMM, which is launch-bound at these widths."""
        CI = CO if CI is None else CI
        if (CO, CI) not in ((32, 32), (64, 64), (128, 128), (128, 32), (128, 64), (64, 32)):      # instances of csrc/rpb_cell.hip
            return wgrad(G, A, M, CO, CI, one_reduction=True)
        slots = ops.cell_wgrad_slots(M, CO, CI)
        part = torch.empty(slots, CO * CI + CO, device=G.device, dtype=torch.float32)
        ops.cell_wgrad(G, A, part, M, CO, CI)
        tot = torch.empty(CO * CI + CO, device=G.device, dtype=torch.float32)
        ops.reduce_partials(part, slots, CO * CI + CO, out_f32=tot, deferrable=True)
        return tot[:CO * CI].view(CO, CI), tot[CO * CI:]

    # ------------------------------------------------------------------ Model protocol
    def _window(self, x):
        """model/dpot.py:180-237 at native resolution: one DPOTNet call on ``in_timesteps`` frames."""
        self._require_hip(x)
        x = x.contiguous().float()
        params = [p for p in self.parameters()]
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in params):
            return HipFunction.apply(x, self, *params)
        return self._forward_hip(x, save=None)

    def forward(self, x):
        B, T_in, H, W, C = x.shape
        T_out = self.data_out_timesteps
        if tuple(x.shape[2:]) != tuple(self.shape_in[1:]) or T_in < self.in_timesteps:
            raise ValueError(f"expected input [B,>={self.in_timesteps},{','.join(map(str, self.shape_in[1:]))}], got {tuple(x.shape)}")
        if self.out_timesteps == T_out:
            return self._window(self._exact_window(x))
        cur, outs = x, []                                                     # model/dpot.py:151-178: sliding windows
        for t in range(0, T_out, self.out_timesteps):
            win = cur[:, -self.in_timesteps:]
            if t + self.out_timesteps > T_out:
                rem = T_out - t
                if rem < self.out_timesteps // 2:
                    break
                outs.append(self._window(win)[:, :rem])
            else:
                pred = self._window(win)
                cur = torch.cat([cur, pred], dim=1)
                outs.append(pred)
        return torch.cat(outs, dim=1)

    def train_loss(self, input, target):
        """model/dpot.py:239-309.  out_timesteps == T_out (every reference YAML): the scalar mean squared error of one window.
        out_timesteps < T_out: sliding windows -- each window's prediction is appended to the input of the next one, so the loss
        back-propagates through the fed-back predictions (``HipFunction`` returns the window's input gradient); a last partial window
        with at least out_timesteps // 2 frames counts with weight remaining / out_timesteps.  The reference returns the ELEMENT-WISE
        sum there (its callers take ``.mean()``), and a partial window's ``[B, remaining, ...]`` loss is added to the full windows'
        ``[B, out_timesteps, ...]`` tensor by broadcasting, which only type-checks for remaining == 1 (or no partial window);
        reproduced as is, including the error for other remainders."""
        T_in, T_out, To = input.shape[1], target.shape[1], self.out_timesteps
        if T_in < self.in_timesteps or To > T_out:
            raise ValueError(f"DPOT.train_loss: input frames {T_in} < in_timesteps {self.in_timesteps} or out_timesteps {To} > target frames {T_out}")
        if To == T_out:
            pred = self._window(self._exact_window(input))
            return ((pred - target) ** 2).mean()
        total, nwin, cur = 0, 0, input
        for t in range(0, T_out, To):
            win = cur[:, -self.in_timesteps:]
            if t + To > T_out:
                rem = T_out - t
                if rem < To // 2:
                    break
                pred = self._window(win)[:, :rem]
                total = total + ((pred - target[:, t:t + rem]) ** 2) * (rem / To)        # broadcasts against [B, To, ...] like the reference
                nwin += rem / To
            else:
                pred = self._window(win)
                total = total + (pred - target[:, t:t + To]) ** 2
                nwin += 1
                cur = torch.cat([cur, pred], dim=1)
        if nwin == 0:
            raise ValueError(f"No valid training windows found. out_timesteps ({To}) may be too large for target length ({T_out})")
        return total / nwin

    def _exact_window(self, x):
        """The single-window branches of the reference hand the WHOLE input to DPOTNet, whose TimeAggregator is sized for
        in_timesteps frames (model/dpot.py:147-148, 253-256): more frames than that fail there with a shape error."""
        if x.shape[1] != self.in_timesteps:
            raise ValueError(f"DPOT: the single-window path takes exactly in_timesteps = {self.in_timesteps} input frames, got {x.shape[1]} "
                             "(the reference's TimeAggregator fails on any other count)")
        return x
