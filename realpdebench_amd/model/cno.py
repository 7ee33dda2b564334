"""CNO3d on MI355X -- drop-in for ``realpdebench.model.cno.CNO3d`` (reference realpdebench/model/cno.py, built by ``load_model`` like
model/load_model.py:60-75) for the reference's ``configs/*/cno.yaml``.

``load_model`` passes only ``in_dim``, ``out_dim``, ``out_dim_mult``, ``in_size`` and ``N_layers``, so every shipped config runs with
``activation='LeakyReLU'`` (cno.py:256), a six-block neck and no up- or down-sampling: the model is 35 ``Conv3d(3, padding=1)`` layers
at full resolution, each followed by an eval BatchNorm3d, LeakyReLU(0.2), a residual add or a channel concat.

Evaluation forward, ``train_loss`` as a value, the autoregressive rollout and checkpoint I/O.  By default the training step is refused:
every attempt to backpropagate raises ``NotImplementedError`` (``_common.EvalByDefault``), ``trainer.make_trainer`` refuses the model at
construction and BatchNorm3d uses its running statistics in every mode.  ``enable_training()`` (``hip_training: true`` through
``load_model``; ``sync_bn=True`` / ``sync_bn: true`` for data-parallel training with SyncBN) opts an instance in:
in ``train()`` mode ``forward`` / ``train_loss`` then run through ``_common.HipFunction`` with batch-statistics BatchNorm
(csrc/rpb_rowbn.hip), the data gradient is rpb_cno_conv3x on flipped, transposed taps (the exact-fp32
implicit GEMM for the seven ``EXACT_DGRAD`` layers) and the weight gradient is ``_common.wgrad``; ``eval()`` mode stays the code below,
untouched.

The data flow is stated once, as data: ``Schedule`` lists the 35 layer steps over buffer handles, and derives from that list where a
buffer has its last producer, where it is read for the last time and whether anyone reads its fp32 rows.  Three executors walk it and
supply only what differs: ``_eval_bf16x3``, ``_eval_f16x2`` and ``_train_rows`` (whose tape the backward pass walks).

Pipeline (activations channels-last rows ``[B * T * H * W][C]``, mesh (T, H, W)):
  rpb_cno_pack      x [M][in_dim] -> bf16 planes P[3][M][64], columns in_dim..63 zero
  rpb_cno_conv3x    x 35: implicit GEMM on the planes + ``v = acc * sc + sh``, LeakyReLU, residual; the result leaves as bf16 planes for the
                    next convolution (and as fp32 rows only where a residual add reads it later, and at the end)
Layers narrower than 64 channels run padded to 64 with zero weight rows / columns and ``sc = sh = 0``; the pad columns of every plane
buffer a convolution reads are zeroed here (zero weights do not cancel NaN).  A concat is two producers writing disjoint column ranges
of one plane buffer.

``set_arith("f16x2")`` (opt-in, evaluation forward only) runs the same 35 layers on two fp16 planes per operand:
  rpb_cno_pack_f16x2     x -> exponent e and fp16 planes P[2][M][64] of x * 2^e
  rpb_cno_conv3x_f16x2   x 35: fp32 rows of the result, and the maximum of |v| into the destination buffer's word (atomicMax)
  rpb_amax_exp_finish, rpb_split2h   once per buffer, after its last producer: word -> exponent, rows -> planes
No host synchronisation; a concat is two producers of one row buffer and one word.

Parameters carry the reference's names, shapes and dtypes (the same ``nn`` module tree, ``decoder_inv.3`` -- constructed, never used in
``forward`` -- included), so ``state_dict`` / ``load_state_dict`` are the reference's; kernel layouts are derived tensors rebuilt when a
parameter changed.
"""
from collections import namedtuple

import torch
import torch.nn as nn

from .. import _lib
from .. import ops
from ..ops import Sub, _p, _ptr, _stream, amax_exp_finish, conv3_f16x2_weights, conv3x_wprep, gemm_nt, split2h, split3
from ..ops import add as ops_add
from ._common import EvalByDefault, batch_norm_rows, batch_norm_rows_bwd, flipped_weight, padded_weight, weight_grad_view, wgrad
from .model import Model

I16 = torch.int16
N_LAYERS = 3
MAX_CH = 64                    # widest first-layer input / last-layer output: one 64-channel tile
# Layers whose data gradient runs on the exact-fp32 implicit GEMM (rpb_gemm_nt) instead of the bf16x3 kernel: the ones that add into the
# gradient of the neck's residual chain.  A BatchNorm shift gradient is a column sum of that gradient, which sees a per-channel bias of
# the error sqrt(M) times stronger than its unbiased part; the bf16x3 kernel's error as a data gradient has such a bias (column mean 3-4
# times the unbiased expectation, tests/test_gpu_cno_train_kernels.py prints it) and along the chain's identity path it adds up block by
# block, where every other path goes through a BatchNorm backward that removes it.
EXACT_DGRAD = frozenset(["ED_expansion.3"] + [f"res_nets.{i}.1" for i in range(3, 9)])
# reference defaults of every keyword load_model never passes (cno.py:240-256)
DEFAULTS = dict(N_res=1, N_res_neck=6, channel_multiplier=32, conv_kernel=3, cutoff_den=2.0001, filter_size=6, lrelu_upsampling=2,
                half_width_mult=0.8, radial=False, batch_norm=True, out_size=1, expand_input=False, latent_lift_proj_dim=64, add_inv=True)


# ----------------------------------------------------------------------------------------------------------- the data flow, once
Layer = namedtuple("Layer", "name src dst col act res")      # src / dst / res: indices into ``bufs``; dst None: the model output


class Buf(namedtuple("Buf", "ld written")):
    """An activation buffer, rows [M][ld]: its producers write columns 0..written-1."""

    @property
    def zero(self):
        """The producers leave columns unwritten that a convolution reads: they must read as zero (zero weights do not cancel NaN)."""
        return self.written < self.ld


class Schedule:
    """The 35 layers ``forward`` runs (cno.py:466-521), as plain data: no storage, no device.  ``bufs[0]`` is the packed input;
    ``layers`` in launch order, each reading ``src`` whole and writing its ``Co`` channels at column ``col`` of ``dst`` after the affine,
    LeakyReLU (``act``) and the residual add of ``res``; ``keep``: name -> buffer of the five tensors ``forward(x, keep=)`` hands out.
    A concat is two producers writing column ranges of one buffer.  Derived from the list, for the executors:
      last_write[b]   index of the last layer that writes b (``finish`` of the f16x2 path runs there, once per buffer)
      last_read[b]    index of the last layer that reads b as ``src`` or ``res`` (the evaluation executors drop its storage there)
      residuals       the buffers some later layer adds as ``res``
      kept            ``keep`` the other way round: buffer -> name"""

    def __init__(self, in_dim, ef=(16, 32, 64, 128)):
        self.bufs, self.layers, self.keep = [], [], {}

        def buf(width):
            self.bufs.append(Buf(max(width, 64), width))
            return len(self.bufs) - 1

        def layer(name, src, dst=None, col=0, act=True, res=None):
            self.layers.append(Layer(name, src, dst, col, act, res))
            return dst

        def res_block(i, x, width):
            """res_nets[i]: x + BN(conv(L(BN(conv x))))"""
            h, y = buf(width), buf(width)
            layer(f"res_nets.{i}.1", x, h)
            return layer(f"res_nets.{i}.2", h, y, act=False, res=x)

        x = layer("lift.0", buf(in_dim), buf(64))
        x = self.keep["lift"] = layer("lift.1", x, buf(ef[0]), act=False)
        skip = []
        for i in range(N_LAYERS):
            skip.append(res_block(i, x, ef[i]))
            self.keep[f"skip{i}"] = skip[i]
            x = layer(f"encoder.{i}", x, buf(ef[i + 1]))
        for j in range(6):                                            # the neck, in REVERSE index order (cno.py:490-491)
            x = res_block(N_LAYERS + 5 - j, x, ef[3])
        self.keep["neck"] = x
        x, width = layer("ED_expansion.3", x, buf(ef[3])), ef[3]
        for i in range(N_LAYERS):                                     # decoder: cat(x, ED_expansion(skip)) is two producers of one buffer
            x = layer(f"decoder_inv.{i}", x, buf(width))              # 128, 128, 64 channels
            w = ef[2 - i]                                             # 64, 32, 16: each producer's channels
            cat, width = buf(2 * w), 2 * w                            # (2 * 16 = 32 of 64 columns: 32..63 stay zero)
            layer(f"decoder.{i}", x, cat, col=0)
            x = layer(f"ED_expansion.{2 - i}", skip[2 - i], cat, col=w)
        x = layer("project.0", x, buf(64))
        layer("project.1", x, act=False)

        self.last_write = {L.dst: i for i, L in enumerate(self.layers) if L.dst is not None}
        self.last_read = {b: i for i, L in enumerate(self.layers) for b in (L.src, L.res) if b is not None}
        self.residuals = {L.res for L in self.layers} - {None}
        self.kept = {b: name for name, b in self.keep.items()}


# ----------------------------------------------------------------------------------------------------------- parameter tree
class CNOBlock3d(nn.Module):
    """conv -> BatchNorm3d (optional) -> LeakyReLU(0.2) (cno.py:28-100)."""

    def __init__(self, in_channels, out_channels, batch_norm=True):
        super().__init__()
        self.convolution = nn.Conv3d(in_channels, out_channels, kernel_size=3, padding=1)
        self.batch_norm = nn.BatchNorm3d(out_channels) if batch_norm else False
        self.activation = nn.LeakyReLU(negative_slope=0.2)


class LiftProjectBlock3d(nn.Module):
    """CNOBlock (no BatchNorm) -> conv (cno.py:106-152; lift and project are built with batch_norm=False)."""

    def __init__(self, in_channels, out_channels, latent_dim=64):
        super().__init__()
        self.inter_CNOBlock = CNOBlock3d(in_channels, latent_dim, batch_norm=False)
        self.convolution = nn.Conv3d(latent_dim, out_channels, kernel_size=3, stride=1, padding=1)
        self.batch_norm = False


class ResidualBlock3d(nn.Module):
    """x + BN(conv(L(BN(conv x)))) (cno.py:159-231): the residual is added after the second BatchNorm, no activation follows."""

    def __init__(self, channels):
        super().__init__()
        self.convolution1 = nn.Conv3d(channels, channels, kernel_size=3, stride=1, padding=1)
        self.convolution2 = nn.Conv3d(channels, channels, kernel_size=3, stride=1, padding=1)
        self.batch_norm1 = nn.BatchNorm3d(channels)
        self.batch_norm2 = nn.BatchNorm3d(channels)
        self.activation = nn.LeakyReLU(negative_slope=0.2)


def fold_affine(conv, bn, N):
    """(sc, sh) [N] of ``v = acc * sc + sh``: sc = gamma / sqrt(var + eps), sh = beta + (bias - mean) * sc, formed in float64 and rounded
    once; without BatchNorm sc = 1, sh = bias.  Pad channels get sc = sh = 0."""
    bias = conv.bias.detach().double()
    Co = bias.numel()
    if isinstance(bn, nn.BatchNorm3d):
        sc64 = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
        sh64 = bn.bias.detach().double() + (bias - bn.running_mean.detach().double()) * sc64
    else:
        sc64, sh64 = torch.ones_like(bias), bias
    sc, sh = torch.zeros(N, dtype=torch.float32, device=bias.device), torch.zeros(N, dtype=torch.float32, device=bias.device)
    sc[:Co], sh[:Co] = sc64.float(), sh64.float()
    return sc, sh


class _Planes:
    """bf16 plane buffer P[3][M][ld] (int16 bit patterns).  ``zero``: the producers leave columns unwritten that a convolution reads."""

    def __init__(self, M, ld, device, zero):
        self.t = (torch.zeros if zero else torch.empty)(3 * M * ld, dtype=I16, device=device)
        self.ld = ld

    def ptr(self, col=0):
        return _p(self.t, I16) + 2 * col


class _Act:
    """One activation buffer of the training forward: fp32 rows [M][ld] (what a weight gradient reads) next to the bf16 planes (what the
    next convolution reads).  ``zero``: as ``_Planes``."""

    def __init__(self, M, ld, device, zero):
        self.rows = (torch.zeros if zero else torch.empty)(M, ld, dtype=torch.float32, device=device)
        self.planes = _Planes(M, ld, device, zero)
        self.ld = ld

    def at(self, col=0):
        return Sub(self.rows, col)


class _ActH:
    """One activation buffer of the f16x2 evaluation forward: fp32 rows [M][ld] (what the producers write and a residual reads), the
    fp16 planes [2][M][ld] of the rows scaled by 2^e (what the next convolution reads) and one int32 word of the forward's ``words``
    tensor: the producers max their |v| bit patterns into it, ``finish`` turns it into e and splits the rows.  ``zero``: the producers
    leave columns unwritten that a convolution reads.  ``rows=False``: the first layer's input, whose planes rpb_cno_pack_f16x2 writes."""

    def __init__(self, M, ld, device, zero, words, index, rows=True):
        self.rows = (torch.zeros if zero else torch.empty)(M, ld, dtype=torch.float32, device=device) if rows else None
        self.planes = torch.empty(2 * M * ld, dtype=I16, device=device)
        self.word = Sub(words, index)
        self.M, self.ld, self.ready = M, ld, False

    def at(self, col=0):
        return Sub(self.rows, col)

    def finish(self):
        """After the last producer: word -> exponent, rows -> planes over the whole row width (zero columns give zero planes)."""
        amax_exp_finish(self.word)
        split2h(self.rows, self.planes, self.M, self.ld, self.word)
        self.ready = True
        return self


def _iptr(t):
    """address of an int32 word: a tensor, an ``ops.Sub`` (a word of an int32 tensor, or of an fp32 allocation whatever it holds), or
    the address itself"""
    if t is None or isinstance(t, int):
        return t
    return _p(t, t.t.dtype) if isinstance(t, Sub) else _p(t, torch.int32)


class CNO3d(EvalByDefault, Model):
    """``set_arith`` selects the arithmetic of the evaluation / rollout forward's 35 convolutions: ``"f32"`` (default, the parity path:
    operands as three bf16 planes, six products per fp32 product) or ``"f16x2"`` (opt-in: operands as two fp16 planes of the tensor
    scaled by a power of two, three products, dropped term <= 2^-22; csrc/rpb_cno3h.hip).  Only the evaluation
    forward changes: the opt-in training step (``enable_training()``) stays on its kernels under either setting."""
    batch_independent = True                       # BatchNorm runs on its running statistics only
    training_unavailable = EvalByDefault.TRAIN_MSG.format("CNO", "CNO3d")
    # An enabled instance computes batch statistics: they couple the samples of a step, so it stops declaring ``batch_independent`` (no
    # micro-batching) and refuses more than one rank (per-rank statistics would break "N ranks == 1 rank") unless it was enabled with
    # ``sync_bn=True``: then the statistics of every BatchNorm layer, forward and backward, are summed over the ranks (the ``dp.StatsSync``
    # the trainer attaches as ``bn_sync``; ``_common.batch_norm_rows``), and every ``train()``-mode forward is collective.
    BATCH_STATISTICS = True
    DP_MSG = ("CNO3d training computes BatchNorm statistics per rank: data-parallel training (SyncBN) is not built, run it on one rank "
              "-- or opt in with enable_training(sync_bn=True) (sync_bn: true next to hip_training: true in a config)")

    def __init__(self, in_dim, in_size, N_layers, N_res=1, N_res_neck=6, channel_multiplier=32, conv_kernel=3, cutoff_den=2.0001,
                 filter_size=6, lrelu_upsampling=2, half_width_mult=0.8, radial=False, batch_norm=True, out_dim=1, out_dim_mult=1,
                 out_size=1, expand_input=False, latent_lift_proj_dim=64, add_inv=True, activation="LeakyReLU"):
        super().__init__()
        given = dict(N_res=N_res, N_res_neck=N_res_neck, channel_multiplier=channel_multiplier, conv_kernel=conv_kernel,
                     cutoff_den=cutoff_den, filter_size=filter_size, lrelu_upsampling=lrelu_upsampling, half_width_mult=half_width_mult,
                     radial=radial, batch_norm=batch_norm, out_size=out_size, expand_input=expand_input,
                     latent_lift_proj_dim=latent_lift_proj_dim, add_inv=add_inv)
        unsupported = []
        if int(N_layers) != N_LAYERS:
            unsupported.append(f"N_layers={N_layers} (every cno.yaml has 3)")
        if activation != "LeakyReLU":
            unsupported.append(f"activation={activation!r} (only 'LeakyReLU': the filtered activations are not built)")
        for k, v in given.items():
            if v != DEFAULTS[k]:
                unsupported.append(f"{k}={v!r} (only the reference default {DEFAULTS[k]!r}: load_model never passes it)")
        if int(out_dim) * int(out_dim_mult) > MAX_CH or int(out_dim) * int(out_dim_mult) < 1:
            unsupported.append(f"out_dim * out_dim_mult = {int(out_dim) * int(out_dim_mult)} (1..{MAX_CH})")
        if not 1 <= int(in_dim) <= MAX_CH:
            unsupported.append(f"in_dim={in_dim} (1..{MAX_CH})")
        if unsupported:
            raise NotImplementedError("MI355X CNO3d covers the configuration family of the reference's configs/*/cno.yaml; unsupported: "
                                      + "; ".join(unsupported))
        self.in_dim, self.in_size, self.N_layers = int(in_dim), in_size, N_LAYERS
        self.out_dim_mult, self.out_dim = int(out_dim_mult), int(out_dim) * int(out_dim_mult)     # out_dim: the total, as in cno.py:270
        self.N_res, self.N_res_neck, self.add_inv = 1, 6, True
        self.lift_dim = channel_multiplier // 2
        self.encoder_features = ef = [self.lift_dim] + [2 ** i * channel_multiplier for i in range(N_LAYERS)]        # 16, 32, 64, 128
        dec_in = [ef[3], 2 * ef[2], 2 * ef[1]]                                                                       # 128, 128, 64
        dec_out = [ef[2], ef[1], ef[0]]                                                                              # 64, 32, 16
        inv = dec_in + [ef[0] + dec_out[-1]]                                                                         # 128, 128, 64, 32
        self.lift = LiftProjectBlock3d(self.in_dim, ef[0], latent_lift_proj_dim)
        self.project = LiftProjectBlock3d(ef[0] + dec_out[-1], self.out_dim, latent_lift_proj_dim)
        self.encoder = nn.ModuleList([CNOBlock3d(ef[i], ef[i + 1]) for i in range(N_LAYERS)])
        self.ED_expansion = nn.ModuleList([CNOBlock3d(ef[i], ef[i]) for i in range(N_LAYERS + 1)])
        self.decoder = nn.ModuleList([CNOBlock3d(dec_in[i], dec_out[i]) for i in range(N_LAYERS)])
        self.decoder_inv = nn.ModuleList([CNOBlock3d(inv[i], inv[i]) for i in range(N_LAYERS + 1)])                  # [3] is never used
        self.res_nets = nn.Sequential(*([ResidualBlock3d(ef[l]) for l in range(N_LAYERS)] + [ResidualBlock3d(ef[N_LAYERS]) for _ in range(6)]))
        self.schedule = Schedule(self.in_dim, ef)

    # ------------------------------------------------------------------ kernel-side layouts
    def _convs(self):
        """name -> (conv, BatchNorm3d or False) of the 35 convolutions ``forward`` runs."""
        out = {"lift.0": (self.lift.inter_CNOBlock.convolution, False), "lift.1": (self.lift.convolution, False),
               "project.0": (self.project.inter_CNOBlock.convolution, False), "project.1": (self.project.convolution, False)}
        for i in range(N_LAYERS):
            out[f"encoder.{i}"] = (self.encoder[i].convolution, self.encoder[i].batch_norm)
            out[f"decoder.{i}"] = (self.decoder[i].convolution, self.decoder[i].batch_norm)
            out[f"decoder_inv.{i}"] = (self.decoder_inv[i].convolution, self.decoder_inv[i].batch_norm)
        for i in range(N_LAYERS + 1):
            out[f"ED_expansion.{i}"] = (self.ED_expansion[i].convolution, self.ED_expansion[i].batch_norm)
        for i, r in enumerate(self.res_nets):
            out[f"res_nets.{i}.1"] = (r.convolution1, r.batch_norm1)
            out[f"res_nets.{i}.2"] = (r.convolution2, r.batch_norm2)
        return out

    def _prep(self, device):
        """The evaluation forward's layouts under the selected arithmetic (one cache entry per arithmetic, same invalidation rule)."""
        tensors, arith = list(self.parameters()) + list(self.buffers()), self.arith
        return self._layouts.get("prep_" + arith, tensors, lambda: self._build_prep(device, arith))

    def _build_prep(self, device, arith):
        """Per layer the folded affine and the weights: three bf16 planes (``"f32"``; ``ew`` None) or two scaled fp16 planes with their
        exponent ``ew`` (``"f16x2"``; int32 [1] on the device)."""
        prep = {}
        for name, (conv, bn) in self._convs().items():
            Co, Ci = conv.weight.shape[:2]
            N, K = max(Co, 64), max(Ci, 64)
            wm = padded_weight(conv, N, K).to(device)
            wz, ew = conv3_f16x2_weights(wm, N, K) if arith == "f16x2" else (self.k_wprep(wm, N, K), None)
            sc, sh = fold_affine(conv, bn, N)
            prep[name] = dict(wz=wz, ew=ew, sc=sc.to(device), sh=sh.to(device), N=N, K=K, Co=Co)
        return prep

    def _prep_train(self, device):
        """The training step's layouts: they depend on the convolutions alone (BatchNorm enters through the statistics kernels)."""
        tensors = [t for conv, _ in self._convs().values() for t in (conv.weight, conv.bias)]
        return self._layouts.get("prep_train", tensors, lambda: self._build_prep_train(device))

    def _build_prep_train(self, device):
        """Per layer: ``wz`` / ``sc`` = 1 / ``sh`` = bias of the forward convolution and ``wd``, the flipped, transposed taps of its data
        gradient (``lift.0`` has none; fp32 rows [K][27 N] for the ``EXACT_DGRAD`` layers, rpb_conv3x_wprep planes otherwise); ``unit[n]``: the
        (1, 0) affine of the bf16x3 data-gradient launches."""
        prep = {"unit": {n: (torch.ones(n, device=device), torch.zeros(n, device=device)) for n in (64, 128)}}
        for name, (conv, _) in self._convs().items():
            Co, Ci = conv.weight.shape[:2]
            N, K = max(Co, 64), max(Ci, 64)
            sc, sh = fold_affine(conv, False, N)
            wd = None if name == "lift.0" else flipped_weight(conv, N, K).to(device)
            prep[name] = dict(wz=self.k_wprep(padded_weight(conv, N, K).to(device), N, K), sc=sc.to(device), sh=sh.to(device),
                              wd=wd if wd is None or name in EXACT_DGRAD else self.k_wprep(wd, K, N), N=N, K=K, Co=Co, Ci=Ci)
        return prep

    # ------------------------------------------------------------------ the kernels, one method per family (tests call these)
    @staticmethod
    def k_wprep(wm, N, K):
        wz = torch.empty(3 * N * 27 * K, device=wm.device, dtype=I16)
        conv3x_wprep(wm, wz, N, K)
        return wz

    @staticmethod
    def k_pack(x, planes, M, Cin):
        """x [M][Cin] fp32 -> planes P[3][M][64], columns Cin..63 zero."""
        _lib.call("rpb_cno_pack", _ptr(x), _ptr(planes, I16), M, Cin, _stream(), label="cno_pack", nbytes=4 * M * Cin + 6 * M * 64)

    @staticmethod
    def k_conv(planes, wz, sc, sh, M, N, Ci, mesh, nvalid, act, res=None, ldr=0, out=None, ldo=0, out_planes=None, ldp=0):
        """One CNO layer (rpb_cno_conv3x).  ``planes`` / ``out_planes``: int16 tensors or raw addresses (already at the first column);
        ``res`` / ``out``: fp32 tensors, ``ops.Sub`` or raw addresses."""
        _lib.call("rpb_cno_conv3x", _ptr(planes, I16), _ptr(wz, I16), _ptr(sc), _ptr(sh), _ptr(res), _ptr(out), _ptr(out_planes, I16), M, N, Ci,
                  nvalid, int(act), ldr, ldo, ldp, *mesh, _stream(), label=f"cno_conv3x[N{N},Ci{Ci}]",
                  nbytes=6 * M * Ci + (4 * M * nvalid if out is not None else 0) + (6 * M * nvalid if out_planes is not None else 0)
                  + (4 * M * nvalid if res is not None else 0), flops=2 * M * N * 27 * Ci)

    @staticmethod
    def k_pack_f16x2(x, planes, M, Cin, e):
        """x [M][Cin] fp32 -> e[0] with max|x| * 2^e in [2^14, 2^15) and fp16 planes P[2][M][64] of x * 2^e, columns Cin..63 zero."""
        _lib.call("rpb_cno_pack_f16x2", _ptr(x), _ptr(planes, I16), M, Cin, _iptr(e), _stream(), label="cno_pack_f16x2",
                  nbytes=8 * M * Cin + 4 * M * 64)

    @staticmethod
    def k_conv_f16x2(planes, wz, sc, sh, M, N, Ci, mesh, nvalid, act, ea, ew, res=None, ldr=0, out=None, ldo=0, amax=None):
        """One CNO layer on two fp16 planes (rpb_cno_conv3x_f16x2).  ``planes``: int16 tensor or raw address; ``res`` / ``out``: fp32 tensors,
        ``ops.Sub`` or raw addresses (already at the first column); ``amax`` / ``ea`` / ``ew``: int32 tensors, ``ops.Sub`` or raw addresses."""
        _lib.call("rpb_cno_conv3x_f16x2", _ptr(planes, I16), _ptr(wz, I16), _ptr(sc), _ptr(sh), _ptr(res), _ptr(out), _iptr(amax), M, N, Ci,
                  nvalid, int(act), ldr, ldo, *mesh, _iptr(ea), _iptr(ew), _stream(), label=f"cno_conv3x_f16x2[N{N},Ci{Ci}]",
                  nbytes=4 * M * Ci + 4 * M * nvalid + (4 * M * nvalid if res is not None else 0), flops=2 * M * N * 27 * Ci)

    # ------------------------------------------------------------------ the training step
    def _train_rows(self, x, mesh, state):
        """x [M][in_dim] fp32 -> [M][out_dim] fp32 with batch-statistics BatchNorm (the running statistics are updated): the schedule on
        ``_Act`` buffers, all of which stay (the tape holds them).  A BatchNorm layer is the raw convolution (fp32 rows ``y``), the
        statistics and one row pass that writes fp32 rows and planes of ``v``.  ``state`` (a dict, or None) receives the tape the
        backward pass walks: per layer the buffers it read and wrote, ``y`` and (a, b, mean, rstd)."""
        dev, M, S = x.device, x.shape[0], self.schedule
        prep, convs = self._prep_train(dev), self._convs()
        tape, counters = [], []
        acts = {0: _Act(M, S.bufs[0].ld, dev, S.bufs[0].zero)}        # the input: rows zeroed and filled, the pack kernel writes the planes
        acts[0].rows[:, :self.in_dim] = x
        self.k_pack(x, acts[0].planes.t, M, self.in_dim)
        out = None
        for L in S.layers:
            name, col, act = L.name, L.col, L.act
            if L.dst is not None and L.dst not in acts:
                acts[L.dst] = _Act(M, S.bufs[L.dst].ld, dev, S.bufs[L.dst].zero)
            src, dst, res = acts[L.src], acts.get(L.dst), acts.get(L.res)
            s, (conv, bn) = prep[name], convs[name]
            N, K, Co = s["N"], s["K"], s["Co"]
            assert src.ld == K, name
            rec = dict(name=name, src=src, dst=dst, col=col, act=act, res=res, y=None, ab=None, out=None)
            tape.append(rec)
            if bn is False:                                           # lift / project: the evaluation forward's fused launch
                if dst is None:
                    out = rec["out"] = torch.empty(M, Co, device=dev, dtype=torch.float32)
                self.k_conv(src.planes.ptr(), s["wz"], s["sc"], s["sh"], M, N, K, mesh, Co, act, out=out if dst is None else dst.at(col),
                            ldo=Co if dst is None else dst.ld, out_planes=None if dst is None else dst.planes.ptr(col),
                            ldp=0 if dst is None else dst.ld)
                continue
            y = torch.empty(M, N, device=dev, dtype=torch.float32)
            self.k_conv(src.planes.ptr(), s["wz"], s["sc"], s["sh"], M, N, K, mesh, N, 0, out=y, ldo=N)
            ab = batch_norm_rows(y, N, M, Co, bn, sync=self.bn_sync)  # a, b, mean, rstd
            ops.rowbn_act_fwd(y, N, ab[0], ab[1], M, Co, act, res=None if res is None else res.rows, ldr=0 if res is None else res.ld,
                              out=dst.at(col), ldo=dst.ld, out_planes=dst.planes.ptr(col), ldp=dst.ld)
            rec["y"], rec["ab"] = y, ab
            counters.append(bn.num_batches_tracked)
        torch._foreach_add_(counters, 1)
        if state is not None:
            for rec in tape:                                          # the backward pass reads fp32 rows only
                rec["src"].planes = None
            state.update(tape=tape, M=M, mesh=mesh)
        return out

    @torch.no_grad()
    def _forward_hip(self, x, state):
        x = x.contiguous().float()
        B, T, H, W, C = x.shape
        return self._shaped(self._train_rows(x.view(B * T * H * W, C), (T, H, W), state), x.shape)

    @torch.no_grad()
    def _backward_hip(self, state, g_out, need_gx=False):
        """{parameter: gradient} from dLoss/d(out): the tape in reverse.  Per layer: the BatchNorm + LeakyReLU backward row passes give
        ``dy`` (fp32 rows for ``wgrad``, planes for the data gradient), ``wgrad`` gives (dW, db), rpb_cno_conv3x on the flipped taps adds
        the data gradient into the gradient buffer of the layer's input (the first consumer writes it, later ones pass it as ``res``);
        the ``EXACT_DGRAD`` layers take the exact-fp32 implicit GEMM on the fp32 rows instead.
        A residual hands its gradient to the block input unchanged; a concat is two layers reading column ranges of one buffer.
        ``state`` is only read: a second call gives bit-equal gradients."""
        if need_gx:
            raise NotImplementedError("CNO3d training computes no input gradient (no trainer asks for one)")
        tape, M, mesh = state["tape"], state["M"], state["mesh"]
        dev = g_out.device
        prep, convs, rows = self._prep_train(dev), self._convs(), ops.rowbn_rows()
        g, grads = {}, {}                                             # id(_Act) -> fp32 [M][ld] gradient of that buffer
        gpad = torch.zeros(M, 64, device=dev, dtype=torch.float32)
        gpad[:, :self.out_dim] = g_out.reshape(M, self.out_dim)
        for rec in reversed(tape):
            name, src, dst, col, act = rec["name"], rec["src"], rec["dst"], rec["col"], rec["act"]
            s, (conv, bn) = prep[name], convs[name]
            N, K, Co, Ci = s["N"], s["K"], s["Co"], s["Ci"]
            gt, ldg = (gpad, 64) if dst is None else (g[id(dst)], dst.ld)
            gv = Sub(gt, col)
            if rec["res"] is not None:                                # the residual passes gv on to the block input
                k = id(rec["res"])
                g[k] = ops_add(g[k], gt) if k in g else gt
            need_dx, exact = s["wd"] is not None, name in EXACT_DGRAD
            dyp = torch.empty(3 * M * N, device=dev, dtype=I16) if need_dx and not exact else None
            if bn is not False:
                y, ab = rec["y"], rec["ab"]
                part = torch.empty(rows, 2 * Co, device=dev, dtype=torch.float64)
                dy = torch.empty(M, N, device=dev, dtype=torch.float32)
                ops.rowbn_act_bwd_stats(gv, ldg, y, N, *ab, M, Co, act, part)
                grads[bn.weight], grads[bn.bias] = batch_norm_rows_bwd(part, gv, ldg, y, N, ab, M, Co, N, act, dy, N, dy_planes=dyp, ldp=N,
                                                                           sync=self.bn_sync)
            elif act:                                                 # lift.0 / project.0: the gate from the sign of the saved v
                dy = torch.empty(M, N, device=dev, dtype=torch.float32)
                ops.rowbn_act_bwd_apply(gv, ldg, M, Co, N, 1, y=dst.rows, ldy=dst.ld, dy=dy, ldd=N, dy_planes=dyp, ldp=N)
            else:                                                     # lift.1 / project.1: dy = gv, a 64-wide buffer with zero pad columns
                assert col == 0 and ldg == N, name
                dy = gt
                split3(dy, dyp, M, N)
            dW, db = wgrad(dy, src.rows, M, N, 27 * K, ldg=N, lda=K, conv=mesh)
            grads[conv.weight], grads[conv.bias] = weight_grad_view(dW, Co, Ci, N, K), db[:Co]
            k = id(src)
            if need_dx and exact:                                     # exact-fp32 implicit GEMM on the fp32 rows; a new buffer (no aliasing)
                gs = torch.empty(M, K, device=dev, dtype=torch.float32)
                gemm_nt(dy, s["wd"], gs, M, K, 27 * N, conv=mesh, residual=g.get(k))
                g[k] = gs
            elif need_dx:
                one, zero = prep["unit"][K]
                first = k not in g
                gs = torch.empty(M, K, device=dev, dtype=torch.float32) if first else g[k]
                self.k_conv(dyp, s["wd"], one, zero, M, K, N, mesh, K, 0, res=None if first else gs, ldr=K, out=gs, ldo=K)
                g[k] = gs
        return grads

    # ------------------------------------------------------------------ forward
    def _eval_bf16x3(self, x, mesh, keep=None):
        """x [M][in_dim] fp32 -> [M][out_dim] fp32: the schedule on ``_Planes`` buffers.  A layer also writes its fp32 rows [M][Co] where
        someone reads them: a later residual, ``keep`` (a dict: the fp32 rows of the lift output, ``skip[0..2]`` and the neck output, for
        tests; the extra fp32 stores do not change any value) or the caller.  A buffer's storage goes after its last reader."""
        dev, M, S, prep = x.device, x.shape[0], self.schedule, self._prep(x.device)
        wanted = S.residuals | (set(S.kept) if keep is not None else set())
        planes, rows = {0: _Planes(M, 64, dev, zero=False)}, {}      # (the pack kernel writes the input's zero pad itself)
        self.k_pack(x, planes[0].t, M, self.in_dim)
        for i, L in enumerate(S.layers):
            s, src, res = prep[L.name], planes[L.src], None if L.res is None else rows[L.res]     # (the residual's rows [M][width])
            assert src.ld == s["K"], L.name
            if L.dst is not None and L.dst not in planes:
                planes[L.dst] = _Planes(M, S.bufs[L.dst].ld, dev, S.bufs[L.dst].zero)
            dst = planes.get(L.dst)
            out = torch.empty(M, s["Co"], device=dev, dtype=torch.float32) if dst is None or L.dst in wanted else None
            self.k_conv(src.ptr(), s["wz"], s["sc"], s["sh"], M, s["N"], s["K"], mesh, s["Co"], L.act, res=res,
                        ldr=0 if res is None else res.shape[1], out=out, ldo=s["Co"], out_planes=None if dst is None else dst.ptr(L.col),
                        ldp=0 if dst is None else dst.ld)
            if dst is not None and out is not None:                   # (such a buffer has this one producer, at column 0)
                rows[L.dst] = out
                if keep is not None and L.dst in S.kept:
                    keep[S.kept[L.dst]] = out
            for b in (L.src, L.res):
                if S.last_read.get(b) == i:
                    planes.pop(b, None)
                    rows.pop(b, None)
        return out

    def _eval_f16x2(self, x, mesh, keep=None):
        """``_eval_bf16x3`` under ``set_arith("f16x2")``: the schedule on ``_ActH`` buffers.  Every layer writes fp32 rows and maxes into
        the word of its destination; when all producers of a buffer are done (two for a concat) ``finish`` turns the word into the
        exponent and splits the rows into planes -- one extra read and write of the activation per buffer, no host synchronisation
        (DESIGN.md section 17.2).  Residuals and ``keep`` read the fp32 rows, which always exist here."""
        dev, M, S, prep = x.device, x.shape[0], self.schedule, self._prep(x.device)
        words = torch.zeros(len(S.bufs), dtype=torch.int32, device=dev)      # one word per buffer, zeroed once
        acts = {0: _ActH(M, 64, dev, False, words, 0, rows=False)}    # (the pack kernel writes the input's zero pad and the exponent itself)
        self.k_pack_f16x2(x, acts[0].planes, M, self.in_dim, acts[0].word)
        acts[0].ready = True
        out = None
        for i, L in enumerate(S.layers):
            s, src, res = prep[L.name], acts[L.src], acts.get(L.res)
            assert src.ld == s["K"] and src.ready, L.name
            if L.dst is None:                                         # the model output: no amax
                out = torch.empty(M, s["Co"], device=dev, dtype=torch.float32)
            elif L.dst not in acts:
                acts[L.dst] = _ActH(M, S.bufs[L.dst].ld, dev, S.bufs[L.dst].zero, words, L.dst)
            dst = acts.get(L.dst)
            self.k_conv_f16x2(src.planes, s["wz"], s["sc"], s["sh"], M, s["N"], s["K"], mesh, s["Co"], L.act, src.word, s["ew"],
                              res=None if res is None else res.rows, ldr=0 if res is None else res.ld,
                              out=out if dst is None else dst.at(L.col), ldo=s["Co"] if dst is None else dst.ld,
                              amax=None if dst is None else dst.word)
            if dst is not None and S.last_write[L.dst] == i:
                dst.finish()
                if keep is not None and L.dst in S.kept:
                    keep[S.kept[L.dst]] = dst.rows[:, :S.bufs[L.dst].written].contiguous()
            for b in (L.src, L.res):
                if S.last_read.get(b) == i:
                    acts.pop(b, None)
        return out

    def check_input(self, shape):
        """The shapes ``forward`` takes: [B, T, H, W, in_dim] with in_dim < T."""
        if len(shape) != 5 or shape[-1] != self.in_dim:
            raise ValueError(f"CNO3d was built for inputs [B, T, H, W, {self.in_dim}], got {tuple(shape)}")
        if not shape[-1] < shape[1]:
            raise ValueError(f"CNO3d: input {tuple(shape)} has C >= T.  The reference permutes to channels-first only when C < T "
                             "(cno.py:467) and otherwise convolves with T as the channel axis; this port requires C < T")

    def _shaped(self, out, shape):
        """rows [M][out_dim] -> [B, T * out_dim_mult, H, W, out_dim / out_dim_mult]"""
        B, T, H, W, _ = shape
        out = out.view(B, T, H, W, self.out_dim)
        if self.out_dim_mult > 1:                                     # cno.py:519-520 on channels-last memory: a view, not a time-major split
            out = out.reshape(B, -1, H, W, self.out_dim // self.out_dim_mult)
        return out

    def forward(self, x, keep=None):
        if keep is None:
            return super().forward(x)
        if self.hip_training and self.training:
            raise ValueError("keep= belongs to the evaluation forward")
        return super().forward(x, keep=keep)

    def _forward_eval(self, x, keep=None):
        B, T, H, W, C = x.shape
        run = self._eval_f16x2 if self.arith == "f16x2" else self._eval_bf16x3
        out = run(x.view(B * T * H * W, C), (T, H, W), keep=keep)
        if keep is not None:
            for k in keep:
                keep[k] = keep[k].view(B, T, H, W, -1)
        return self._shaped(out, x.shape)
