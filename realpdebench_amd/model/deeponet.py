"""DeepONet on MI355X -- drop-in for ``realpdebench.model.deeponet.DeepONet`` (reference realpdebench/model/deeponet.py, built by
``load_model`` like model/load_model.py:132-143) for the reference's ``configs/*/deeponet.yaml`` (p = 64 / 128 / 256).

Evaluation forward, ``train_loss`` as a value, the autoregressive rollout and checkpoint I/O.  By default the training step is refused:
every attempt to backpropagate raises ``NotImplementedError`` (``_common.EvalByDefault``) instead of returning tensors without a graph,
``trainer.make_trainer`` refuses the model at construction, dropout is the identity and BatchNorm3d uses its running statistics in
every mode.  ``enable_training()`` (``hip_training: true`` through ``load_model``; ``sync_bn=True`` / ``sync_bn: true`` for data-parallel
training with SyncBN) opts an instance in: in ``train()`` mode ``forward`` /
``train_loss`` then run through ``_common.HipFunction`` with batch-statistics BatchNorm and active dropout (``_forward_hip`` /
``_backward_hip`` below, csrc/rpb_rowbn.hip and csrc/rpb_deeponet_train.hip); ``eval()`` mode stays the pipeline
below, untouched.

Pipeline (activations channels-last fp32 rows ``[B * T * H * W][C]``):
  branch  stage 1  rpb_im2col (27 C_in columns, zero-padded to a multiple of 64) + rpb_gemm3x (N = 32 zero-padded to 64)
                   -> rpb_don_bn_relu_pool (C = 32 of ld = 64: the upper 32 channels leave as zeros)
          stage 2  rpb_split3 + rpb_conv3x (Ci = 64 with zero weights on the upper 32, N = 64) -> rpb_don_bn_relu_pool
          stage 3  rpb_split3 + rpb_conv3x (64 -> 128) -> rpb_don_bn_relu_pool
          stage 4  rpb_split3 + rpb_conv3x (128 -> 256) -> rpb_don_bn_relu_pool mode 1 (AdaptiveAvgPool3d((1, 4, 4))) -> [B][4][4][256]
          fc       rpb_gemm3x (4096 -> 512, ReLU; weight columns permuted from the reference's (c, h, w) flatten to (h, w, c))
                   -> rpb_gemm3x (512 -> p) = b [B][p]
  trunk   rpb_don_trunk over the grid of ``get_grid`` (np.linspace per axis) -> t [N][p], cached for the last (T_out, H, W) until a
          trunk weight changes
  output  rpb_don_point_mlp: out[b][n] = output_net(b[b] * t[n]) in one launch

``set_arith("f16x2")`` (opt-in, evaluation forward only) moves the output net to rpb_don_point_mlp_f16x2
(csrc/rpb_deeponet_h.hip: two fp16 planes per operand, one power-of-two scale per point formed in registers) and stages 2-4 to
rpb_amax_exp + rpb_split2h + rpb_conv3x_f16x2; stage 1, the branch Linear layers and the trunk stay on the kernels above.

Parameters carry the reference's names, shapes and dtypes (``nn`` modules of the same tree, ``nn.Sequential`` indices included), so
``state_dict`` / ``load_state_dict`` are the reference's; kernel layouts are derived tensors rebuilt when a parameter changed.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib, ops
from ..ops import Sub, _p, _stream, amax_exp, conv3_f16x2_weights, conv3x, conv3x_f16x2, conv3x_wprep, reduce_partials, split2h, split3
from ..ops import add as ops_add
from ._common import (EvalByDefault, batch_norm_rows, batch_norm_rows_bwd, flipped_weight, padded_weight, reduces_stats, weight_grad_view,
                      wgrad)
from .model import Model

I16 = torch.int16
P_SUPPORTED = (64, 128, 256)
_COL_FLOATS = 1 << 28          # stage-1 im2col buffer bound (1 GiB): larger batches run the first stage in chunks of samples
_POINT_ROWS = 1 << 16          # training step: (sample, point) rows per chunk of the output net (its 512-wide rows: 128 MiB per buffer)


# ----------------------------------------------------------------------------------------------------------- layouts (plain torch)
def bf16_planes(x):
    """fp32 -> (hi, mid, lo) bf16 bit patterns (int16), hi + mid + lo == x exactly: truncation at every level (csrc/rpb_mma.h)."""
    x = x.contiguous().float()
    mask = torch.tensor(-65536, dtype=torch.int32, device=x.device)
    top = lambda v: (v.view(torch.int32) & mask).view(torch.float32)
    h = top(x)
    r = x - h
    m = top(r)
    l = r - m
    return tuple((v.view(torch.int32) >> 16).to(torch.int16) for v in (h, m, l))


def _lane_planes(w, plane_dim):
    """[..., 64 lanes, 8] fp32 in operand order -> int16 with the three planes inserted at ``plane_dim``."""
    return torch.stack(bf16_planes(w), dim=plane_dim).contiguous()


def point_weights(W1, b1, W2, b2, W3, b3):
    """The operands of ``rpb_don_point_mlp`` from output_net's Linear(p, 512), Linear(512, 128), Linear(128, C_out).

    v_mfma_f32_32x32x16_bf16: lane (m = lane % 32, kg = lane // 32) of the A operand holds row m, k = 8 kg + e; register r of the
    accumulator is row 8 (r // 4) + 4 kg + r % 4.  Layer 1 contracts over the trunk index in natural order; layers 2 and 3 contract
    over the previous layer's accumulator registers, i.e. k-step s, lane group kg, element e <-> unit 8 (2 s + e // 4) + 4 kg + e % 4
    of a 32-unit tile.  Returns (w1z [16][p/16][3][64][8], b1z [16][2][16], w2z [16][2][4][3][64][8], b2z [4][2][16],
    w3z [4][2][3][64][8], b3)."""
    p, Cout = W1.shape[1], W3.shape[0]
    assert W1.shape == (512, p) and W2.shape == (128, 512) and W3.shape == (Cout, 128) and Cout <= 16 and p % 16 == 0
    KS = p // 16
    w1 = W1.reshape(16, 32, KS, 2, 8).permute(0, 2, 3, 1, 4).reshape(16, KS, 64, 8)                     # (blk, ks, kg * 32 + m, e)
    w2 = W2.reshape(4, 32, 16, 2, 2, 2, 4).permute(2, 3, 0, 5, 1, 4, 6).reshape(16, 2, 4, 64, 8)        # (blk, s, mt, kg * 32 + m, eh * 4 + i)
    W3p = torch.zeros(32, 128, dtype=W3.dtype, device=W3.device)
    W3p[:Cout] = W3
    w3 = W3p.reshape(32, 4, 2, 2, 2, 4).permute(1, 2, 4, 0, 3, 5).reshape(4, 2, 64, 8)                  # (mt, s, kg * 32 + m, eh * 4 + i)
    regs = lambda b, tiles: b.reshape(tiles, 4, 2, 4).permute(0, 2, 1, 3).reshape(tiles, 2, 16).contiguous().float()
    return (_lane_planes(w1, 2), regs(b1, 16), _lane_planes(w2, 3), regs(b2, 4), _lane_planes(w3, 2), b3.contiguous().float())


def pow2_scale(m):
    """(2^e, 2^-e) as fp32 tensors of m's shape, e the exponent with m 2^e in [2^14, 2^15) (the rule of ``rpb_amax_exp``), capped at 62;
    e = 0 for m == 0.  ``m``: finite fp32, >= 0.  Integer arithmetic on the bit patterns, on m's device: no host synchronisation."""
    e = 141 - (m.float().contiguous().view(torch.int32) >> 23)
    e = torch.where(m == 0, torch.zeros_like(e), e.clamp(max=62))
    return ((e + 127) << 23).view(torch.float32), ((127 - e) << 23).view(torch.float32)


def f16_planes(x):
    """fp32 (already scaled into fp16's range) -> (hi, lo) fp16 bit patterns (int16), both rounded to nearest even: hi + lo == x to
    2^-22 |x| (``split8h`` of csrc/rpb_mma.h)."""
    x = x.contiguous().float()
    h = x.half()
    l = (x - h.float()).half()
    return h.view(torch.int16), l.view(torch.int16)


def point_weights_f16x2(W1, b1, W2, b2, W3, b3):
    """The operands of ``rpb_don_point_mlp_f16x2``: ``point_weights`` with every weight scaled by its own 2^ew (max|W| 2^ew in
    [2^14, 2^15)) and split into two fp16 planes in the same lane order.  Returns (w1h [16][p/16][2][64][8], b1z, w2h [16][2][4][2][64][8],
    b2z, w3h [4][2][2][64][8], b3, sc); sc [5] fp32 on the weights' device: 2^-ew1, 2^-ew2, 2^-ew3 and the two constants of the kernel's
    bound |h1_u| <= max_u ||W1_u||_1 max_k |x_k| + max|b1|, both rounded up.  Plain torch, no host synchronisation."""
    p, Cout = W1.shape[1], W3.shape[0]
    assert W1.shape == (512, p) and W2.shape == (128, 512) and W3.shape == (Cout, 128) and Cout <= 16 and p % 16 == 0
    KS = p // 16
    s1, i1 = pow2_scale(W1.abs().max())
    s2, i2 = pow2_scale(W2.abs().max())
    s3, i3 = pow2_scale(W3.abs().max())
    w1 = (W1.float() * s1).reshape(16, 32, KS, 2, 8).permute(0, 2, 3, 1, 4).reshape(16, KS, 64, 8)
    w2 = (W2.float() * s2).reshape(4, 32, 16, 2, 2, 2, 4).permute(2, 3, 0, 5, 1, 4, 6).reshape(16, 2, 4, 64, 8)
    W3p = torch.zeros(32, 128, dtype=torch.float32, device=W3.device)
    W3p[:Cout] = W3.float() * s3
    w3 = W3p.reshape(32, 4, 2, 2, 2, 4).permute(1, 2, 4, 0, 3, 5).reshape(4, 2, 64, 8)
    regs = lambda b, tiles: b.reshape(tiles, 4, 2, 4).permute(0, 2, 1, 3).reshape(tiles, 2, 16).contiguous().float()
    planes = lambda w, dim: torch.stack(f16_planes(w), dim=dim).contiguous()
    l1 = W1.double().abs().sum(1).max()
    l1f = l1.float()
    l1f = torch.where(l1f.double() < l1, torch.nextafter(l1f, torch.full_like(l1f, float("inf"))), l1f)       # rounded up
    sc = torch.stack([i1, i2, i3, l1f, b1.float().abs().max()]).contiguous()
    return (planes(w1, 2), regs(b1, 16), planes(w2, 3), regs(b2, 4), planes(w3, 2), b3.contiguous().float(), sc)


def adaptive_bins(n_in, n_out):
    """AdaptiveAvgPool bins: [floor(i In / Out), ceil((i + 1) In / Out)) -- they overlap when In % Out != 0, replicate when In < Out."""
    return [(i * n_in // n_out, -((-(i + 1) * n_in) // n_out)) for i in range(n_out)]


def pooled_extents(T, H, W):
    """(T, H, W) entering each of the four branch stages (MaxPool3d(2) floors)."""
    out = [(T, H, W)]
    for _ in range(3):
        T, H, W = T // 2, H // 2, W // 2
        out.append((T, H, W))
    return out


# ----------------------------------------------------------------------------------------------------------- parameter tree
class _Branch(nn.Module):
    def __init__(self, input_channels, p, dropout_rate):
        super().__init__()
        chans = (input_channels, 32, 64, 128, 256)
        for i in range(4):
            pool = nn.MaxPool3d(2) if i < 3 else nn.AdaptiveAvgPool3d((1, 4, 4))
            setattr(self, f"conv{i + 1}", nn.Sequential(nn.Conv3d(chans[i], chans[i + 1], kernel_size=3, padding=1),
                                                        nn.BatchNorm3d(chans[i + 1]), nn.ReLU(), pool))
        self.fc = nn.Sequential(nn.Linear(256 * 4 * 4, 512), nn.ReLU(), nn.Dropout(dropout_rate), nn.Linear(512, p))


class _Trunk(nn.Module):
    def __init__(self, p):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(3, 64), nn.ReLU(), nn.Linear(64, 128), nn.ReLU(), nn.Linear(128, p))


RANK_SEED_SHIFT = 56           # the rank enters the dropout seed base above every step a run reaches (``rank_seed_base``)


def rank_seed_base(base, rank):
    """The base of rank ``rank``'s dropout seeds: ``(base + rank * 2^56) mod 2^62``.  ``train.py`` seeds every rank alike, so without
    the rank all ranks would draw one mask.  Rank 0 keeps ``base`` (the single-rank seeds); the seeds of ``drop_seed`` over distinct
    (rank, step, layer, chunk) are distinct for rank < 64 and step < 2^32."""
    assert 0 <= rank < 1 << (62 - RANK_SEED_SHIFT)
    return (int(base) + (int(rank) << RANK_SEED_SHIFT)) % (1 << 62)


def drop_seed(base, step, layer, chunk):
    """The Philox seed of one dropout launch of the training step: ``(base + step * 2^24 + layer * 2^22 + chunk) mod 2^62``.  ``base``:
    the instance's ``dropout_seed``; ``step``: the number of training forwards the instance has run (one per optimiser step: batch
    statistics allow no micro-batches); ``layer``: 0 = branch.fc.2, 1 = output_net.2, 2 = output_net.5; ``chunk``: the output net's chunk of
    points (< 2^22; 0 for the branch).  The GEMM epilogue keys Philox on (seed, element index WITHIN the launch), so a seed without the
    chunk would repeat one mask in every chunk.  Distinct (step, layer, chunk) give distinct seeds for step < 2^38."""
    assert 0 <= layer < 3 and 0 <= chunk < 1 << 22 and step >= 0
    return (int(base) + (int(step) << 24) + (layer << 22) + chunk) % (1 << 62)


class DeepONet(EvalByDefault, Model):
    """``set_arith`` selects the arithmetic of the evaluation / rollout forward's output net and of the convolutions of branch stages
    2-4: ``"f32"`` (default, the parity path: operands as three bf16 planes, six products per fp32 product) or ``"f16x2"`` (opt-in:
    operands as two fp16 planes of the tensor scaled by a power of two -- one per point inside the output net --, three products,
    dropped term <= 2^-22; csrc/rpb_deeponet_h.hip).  Only the evaluation forward changes: the opt-in training
    step (``enable_training()``) stays on its kernels under either setting."""
    batch_independent = True                        # BatchNorm runs on its running statistics only
    training_unavailable = EvalByDefault.TRAIN_MSG.format("DeepONet", "DeepONet")
    BATCH_STATISTICS = True                         # an enabled instance: see enable_training
    DP_MSG = ("DeepONet training computes BatchNorm statistics per rank: data-parallel training (SyncBN) is not built, run it on one rank "
              "-- or opt in with enable_training(sync_bn=True) (sync_bn: true next to hip_training: true in a config)")
    _point_rows = _POINT_ROWS                       # (tests force several chunks by lowering it on an instance)
    # what set_arith("f16x2") moves: the output net ("point") and branch stages 2-4 ("convs"; tools/deeponet_probe.py measures both)
    ALL_F16X2_SITES = F16X2_SITES = ("point", "convs")

    def __init__(self, shape_in, shape_out, input_channels, output_channels, p, dropout_rate=0.1, device="cuda"):
        super().__init__()
        self.shape_in, self.shape_out = tuple(int(v) for v in shape_in), tuple(int(v) for v in shape_out)
        self.input_channels, self.output_channels, self.p, self.device = int(input_channels), int(output_channels), int(p), device
        unsupported = []
        if self.p not in P_SUPPORTED:
            unsupported.append(f"p={p} (the point kernel is built for 64, 128 and 256)")
        if not 1 <= self.output_channels <= 16:
            unsupported.append(f"output_channels={output_channels} (1..16)")
        if self.shape_in[-1] != self.input_channels or self.shape_out[-1] != self.output_channels:
            unsupported.append("input_channels / output_channels differ from the last entries of shape_in / shape_out")
        T, H, W = pooled_extents(*self.shape_in[:3])[3]
        if min(T, H, W) < 1:
            unsupported.append(f"shape_in={self.shape_in}: three MaxPool3d(2) leave an empty extent")
        if unsupported:
            raise NotImplementedError("MI355X DeepONet covers the configuration family of the reference's configs/*/deeponet.yaml; "
                                      "unsupported: " + "; ".join(unsupported))
        self.branch = _Branch(self.input_channels, self.p, dropout_rate)
        self.trunk = _Trunk(self.p)
        self.output_net = nn.Sequential(nn.Linear(self.p, 512), nn.ReLU(), nn.Dropout(dropout_rate), nn.Linear(512, 128), nn.ReLU(),
                                        nn.Dropout(dropout_rate), nn.Linear(128, self.output_channels))
        self.dropout_rate = float(dropout_rate)
        self.dropout_seed, self._drop_step, self._mask_override = 0, 0, None      # the opt-in training step, see enable_training / drop_seed

    # ------------------------------------------------------------------ the opt-in training step
    def enable_training(self, seed=None, sync_bn=False):
        """Opt this instance into the HIP training step (batch-statistics BatchNorm, active dropout; ``hip_training: true`` in a config).
        Batch statistics couple the samples of a step, so the instance stops declaring ``batch_independent`` (no micro-batching) and
        refuses more than one rank (per-rank statistics would break "N ranks == 1 rank") unless ``sync_bn`` is set (``sync_bn: true``):
        then the four BatchNorm layers take their statistics and backward sums over the global batch through the ``dp.StatsSync`` the
        trainer attaches as ``bn_sync`` (``_common.EvalByDefault.enable_training``; equal per-rank batches), every ``train()``-mode
        forward -- a ``torch.no_grad()`` one included -- is collective, ``eval()`` is untouched, and the rank enters the base of the
        dropout seeds (``rank_seed_base``: rank 0 draws the single-rank masks, the others their own).  An explicit ``_mask_override``
        holds the rank's own rows.  ``seed``: the base of the dropout seeds (``drop_seed``); default: torch's initial seed, as the
        trainer's run was seeded.

        The step number of the seeds, ``_drop_step``, counts the training forwards this INSTANCE has completed since this call: a
        ``no_grad`` forward in ``train()`` mode uses one up like a step with a graph, a forward that raises uses none.  It is not part of
        ``state_dict`` (the checkpoint stays the reference's), so a run resumed from a checkpoint under the same seed starts again at
        step 0 and redraws the masks of the first steps; a caller that minds sets ``model._drop_step`` to the resumed iteration."""
        self.dropout_seed = int(torch.initial_seed() if seed is None else seed) % (1 << 62)
        self._drop_step = 0
        return super().enable_training(sync_bn=sync_bn)

    # ------------------------------------------------------------------ kernel-side layouts
    def _prep(self, device):
        tensors = list(self.branch.parameters()) + list(self.branch.buffers()) + list(self.output_net.parameters())
        return self._layouts.get("prep", tensors, lambda: self._build_prep(device))

    def _build_prep(self, device):
        f = dict(device=device, dtype=torch.float32)
        prep = {}
        for i in range(4):
            conv, bn = getattr(self.branch, f"conv{i + 1}")[:2]
            Co, Ci = conv.weight.shape[:2]
            N = max(Co, 64)
            bias = torch.zeros(N, **f)
            bias[:Co] = conv.bias.detach()
            if i == 0:                                                            # im2col + GEMM, K padded to a multiple of 64
                K = -(-27 * Ci // 64) * 64
                wm = torch.zeros(N, K, **f)
                wm[:Co, :27 * Ci] = conv.weight.detach().permute(0, 2, 3, 4, 1).reshape(Co, 27 * Ci)      # tap-major, channel-minor rows
                wz = self.k_gemm_wprep(wm)
            else:                                                                 # conv3x: Ci padded to a multiple of 64 (stage 2: 32 -> 64)
                K = max(Ci, 64)
                wz = torch.empty(3 * N * 27 * K, device=device, dtype=torch.int16)
                conv3x_wprep(padded_weight(conv, N, K).to(device), wz, N, K)
            sc64 = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
            sh64 = bn.bias.detach().double() - bn.running_mean.detach().double() * sc64
            prep[f"s{i + 1}"] = dict(wz=wz, bias=bias, N=N, K=K, C=Co, sc=sc64.float().contiguous(), sh=sh64.float().contiguous())
        fc0, fc3 = self.branch.fc[0], self.branch.fc[3]
        w0 = fc0.weight.detach().reshape(512, 256, 4, 4).permute(0, 2, 3, 1).reshape(512, 4096).contiguous()     # (c, h, w) -> (h, w, c) columns
        prep["fc0"] = (self.k_gemm_wprep(w0), fc0.bias.detach().contiguous())
        prep["fc3"] = (self.k_gemm_wprep(fc3.weight.detach().contiguous()), fc3.bias.detach().contiguous())
        o = self.output_net
        prep["point"] = point_weights(*(t.detach() for t in (o[0].weight, o[0].bias, o[3].weight, o[3].bias, o[6].weight, o[6].bias)))
        return prep

    def _prep_f16x2(self, device):
        """What ``set_arith("f16x2")`` adds to ``_prep``: the output net's weights as scaled fp16 planes with their device-side
        constants (``point_weights_f16x2``) and, per convolution of stages 2-4, ``ops.conv3_f16x2_weights`` planes + exponent."""
        tensors = [getattr(self.branch, f"conv{i}")[0].weight for i in (2, 3, 4)] + list(self.output_net.parameters())
        return self._layouts.get("prep_f16x2", tensors, lambda: self._build_prep_f16x2(device))

    def _build_prep_f16x2(self, device):
        prep = {}
        for i in (2, 3, 4):
            conv = getattr(self.branch, f"conv{i}")[0]
            Co, Ci = conv.weight.shape[:2]
            N, K = max(Co, 64), max(Ci, 64)
            prep[f"s{i}"] = conv3_f16x2_weights(padded_weight(conv, N, K).to(device), N, K)
        o = self.output_net
        prep["point"] = point_weights_f16x2(*(t.detach() for t in (o[0].weight, o[0].bias, o[3].weight, o[3].bias, o[6].weight, o[6].bias)))
        return prep

    def _trunk(self, T, H, W, device):
        """t [N][p] of the (T, H, W) grid.  ONE grid is kept (84 MB at the cylinder shape): it is recomputed when the grid, the device or a
        trunk weight changed."""
        def build():
            fc = self.trunk.fc
            wt = [fc[i].weight.detach().t().contiguous() for i in (0, 2, 4)]
            bs = [fc[i].bias.detach().contiguous() for i in (0, 2, 4)]
            return self.k_trunk(T, H, W, wt, bs, device)

        return self._layouts.get("trunk", self.trunk.parameters(), build, extra=(T, H, W))

    # ------------------------------------------------------------------ the kernels, one method per family (tests call these)
    @staticmethod
    def k_gemm_wprep(w):
        N, K = w.shape
        wz = torch.empty(3 * N * K, device=w.device, dtype=torch.int16)
        _lib.call("rpb_gemm3x_wprep", _p(w), _p(wz, I16), N, K, _stream(), label="gemm3x_wprep", nbytes=10 * N * K)
        return wz

    @staticmethod
    def k_gemm(a, wz, bias, N, relu):
        M, K = a.shape
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
        _lib.call("rpb_gemm3x", _p(a), _p(wz, I16), _p(bias), None, None, _p(out), M, N, K, K, N, 3 if relu else 0, None, None, None, 0, 0.0,
                  _stream(), label=f"don_gemm3x[N{N},K{K}]", nbytes=4 * (M * K + M * N) + 6 * N * K, flops=2 * M * N * K)
        return out

    @staticmethod
    def k_conv1(x, s):
        """Stage-1 convolution: x [B][T][H][W][Cin] -> [B * T * H * W][64] (channels 32..63 are zero weights + zero bias)."""
        B, T, H, W, Cin = x.shape
        M = B * T * H * W
        col = torch.empty(M, s["K"], device=x.device, dtype=torch.float32)
        _lib.call("rpb_im2col", _p(x), _p(col), B, T, H, W, Cin, 3, s["K"], _stream(), label="don_im2col", nbytes=4 * M * (Cin + s["K"]))
        return DeepONet.k_gemm(col, s["wz"], s["bias"], s["N"], relu=False)

    @staticmethod
    def k_conv(x, s, mesh):
        """Stages 2-4: x [M][Ci] (Ci % 64 == 0) -> [M][N] through the three bf16 planes of x."""
        M, Ci = x.shape
        N = s["N"]
        planes = torch.empty(3 * M * Ci, device=x.device, dtype=torch.int16)
        _lib.call("rpb_split3", _p(x), _p(planes, I16), M, Ci, Ci, _stream(), label="don_split3", nbytes=10 * M * Ci)
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
        _lib.call("rpb_conv3x", _p(planes, I16), _p(s["wz"], I16), _p(s["bias"]), _p(out), M, N, Ci, N, *mesh, _stream(),
                  label=f"don_conv3x[N{N},Ci{Ci}]", nbytes=6 * M * Ci + 4 * M * N, flops=2 * M * N * 27 * Ci)
        return out

    @staticmethod
    def k_conv_f16x2(x, s, wh, mesh):
        """``k_conv`` on two fp16 planes of x 2^ea (rpb_amax_exp + rpb_split2h + rpb_conv3x_f16x2); ``wh`` = (planes, exponent) of the
        weights (``ops.conv3_f16x2_weights``)."""
        M, Ci = x.shape
        N = s["N"]
        ea = torch.empty(1, device=x.device, dtype=torch.int32)
        planes = torch.empty(2 * M * Ci, device=x.device, dtype=torch.int16)
        amax_exp(x, ea, M, Ci)
        split2h(x, planes, M, Ci, ea)
        out = torch.empty(M, N, device=x.device, dtype=torch.float32)
        conv3x_f16x2(planes, wh[0], out, M, N, Ci, mesh, ea, wh[1], bias=s["bias"])
        return out

    @staticmethod
    def k_bn_relu_pool(x, sc, sh, B, T, H, W, C, ldo, mode):
        """x [B * T * H * W][ldx] -> MaxPool3d(2) (mode 0) or AdaptiveAvgPool3d((1, 4, 4)) (mode 1) of relu(x * sc + sh), [cells][ldo]."""
        ldx = x.shape[-1]
        To, Ho, Wo = (1, 4, 4) if mode else (T // 2, H // 2, W // 2)
        out = torch.empty(B * To * Ho * Wo, ldo, device=x.device, dtype=torch.float32)
        _lib.call("rpb_don_bn_relu_pool", _p(x), _p(sc), _p(sh), _p(out), B, T, H, W, C, ldx, ldo, mode, _stream(), label="don_bn_relu_pool",
                  nbytes=4 * (x.shape[0] * C + out.numel()), flops=3 * x.shape[0] * C)
        return out

    @staticmethod
    def k_trunk(T, H, W, wt, bs, device):
        p = wt[2].shape[1]
        axes = [torch.tensor(np.linspace(0, 1, n), dtype=torch.float).to(device) for n in (T, H, W)]      # get_grid: float64 linspace, cast
        t = torch.empty(T * H * W, p, device=device, dtype=torch.float32)
        _lib.call("rpb_don_trunk", _p(axes[0]), _p(axes[1]), _p(axes[2]), _p(wt[0]), _p(bs[0]), _p(wt[1]), _p(bs[1]), _p(wt[2]), _p(bs[2]),
                  _p(t), T, H, W, p, _stream(), label="don_trunk", nbytes=4 * t.numel(), flops=2 * T * H * W * (3 * 64 + 64 * 128 + 128 * p))
        return t

    @staticmethod
    def k_point_mlp(t, b, pw):
        w1z, b1z, w2z, b2z, w3z, b3 = pw
        N, p = t.shape
        B, Cout = b.shape[0], b3.shape[0]
        out = torch.empty(B, N, Cout, device=t.device, dtype=torch.float32)
        _lib.call("rpb_don_point_mlp", _p(t), _p(b), _p(w1z, I16), _p(b1z), _p(w2z, I16), _p(b2z), _p(w3z, I16), _p(b3), _p(out), B, N, p, Cout, _stream(),
                  label="don_point_mlp", nbytes=4 * (B * N * Cout + N * p + B * p) + 6 * (512 * p + 128 * 512 + 32 * 128),
                  flops=2 * B * N * (p * 512 + 512 * 128 + 128 * Cout))
        return out

    @staticmethod
    def k_point_mlp_f16x2(t, b, pw, out=None):
        """``k_point_mlp`` on two fp16 planes; ``pw`` = ``point_weights_f16x2(...)``; ``out``: B N C_out floats to write (a tensor or an
        ``ops.Sub`` of one), default a new tensor."""
        w1h, b1z, w2h, b2z, w3h, b3, sc = pw
        N, p = t.shape
        B, Cout = b.shape[0], b3.shape[0]
        if out is None:
            out = torch.empty(B, N, Cout, device=t.device, dtype=torch.float32)
        _lib.call("rpb_don_point_mlp_f16x2", _p(t), _p(b), _p(w1h, I16), _p(b1z), _p(w2h, I16), _p(b2z), _p(w3h, I16), _p(b3), _p(sc), _p(out),
                  B, N, p, Cout, _stream(), label="don_point_mlp_f16x2",
                  nbytes=4 * (B * N * Cout + N * p + B * p) + 4 * (512 * p + 128 * 512 + 32 * 128),
                  flops=2 * B * N * (p * 512 + 512 * 128 + 128 * Cout))
        return out

    # ------------------------------------------------------------------ forward
    def branch_forward(self, x, prep, keep=None, prep_h=None):
        """b [B][p]; ``keep`` (a list) receives the four pooled stage outputs, channels-last [B][T'][H'][W'][C] (tests); ``prep_h``
        (``_prep_f16x2``): stages 2-4 on the f16x2 convolution."""
        B = x.shape[0]
        ext = pooled_extents(*x.shape[1:4])
        s1 = prep["s1"]
        (T, H, W), (T1, H1, W1) = ext[0], ext[1]
        nb = max(1, _COL_FLOATS // (T * H * W * s1["K"]))
        h = torch.empty(B * T1 * H1 * W1, 64, device=x.device, dtype=torch.float32)
        for b0 in range(0, B, nb):                                  # stage 1 in chunks of samples: the im2col buffer stays bounded
            nbc = min(nb, B - b0)
            c = self.k_conv1(x[b0:b0 + nbc], s1)
            h[b0 * T1 * H1 * W1:(b0 + nbc) * T1 * H1 * W1] = self.k_bn_relu_pool(c, s1["sc"], s1["sh"], nbc, T, H, W, 32, 64, 0)
        if keep is not None:
            keep.append(h.view(B, T1, H1, W1, 64)[..., :32])
        for i in (2, 3, 4):
            s, (T, H, W) = prep[f"s{i}"], ext[i - 1]
            c = self.k_conv(h, s, (T, H, W)) if prep_h is None else self.k_conv_f16x2(h, s, prep_h[f"s{i}"], (T, H, W))
            h = self.k_bn_relu_pool(c, s["sc"], s["sh"], B, T, H, W, s["C"], s["C"], 0 if i < 4 else 1)
            if keep is not None:
                keep.append(h.view(B, *((T // 2, H // 2, W // 2) if i < 4 else (1, 4, 4)), s["C"]))
        z = self.k_gemm(h.view(B, 4096), *prep["fc0"], 512, relu=True)
        return self.k_gemm(z, *prep["fc3"], self.p, relu=False)

    def check_input(self, shape):
        if len(shape) != 5 or shape[1] != self.shape_in[0] or shape[-1] != self.input_channels:
            raise ValueError(f"DeepONet was built for inputs [B, {self.shape_in[0]}, H, W, {self.input_channels}], got {tuple(shape)}")
        if min(pooled_extents(*shape[1:4])[3]) < 1:
            raise ValueError(f"DeepONet: input {tuple(shape)} leaves an empty extent after three MaxPool3d(2)")

    def _forward_eval(self, x):
        B, _, H, W, _ = x.shape                                       # T_out from shape_out, H and W from the input (deeponet.py:122-126)
        T_out = self.shape_out[0]
        prep = self._prep(x.device)
        prep_h = self._prep_f16x2(x.device) if self.arith == "f16x2" else None
        sites = () if prep_h is None else self.F16X2_SITES
        b = self.branch_forward(x, prep, prep_h=prep_h if "convs" in sites else None)
        t = self._trunk(T_out, H, W, x.device)
        if prep_h is not None:
            self.f16x2_ran = tuple(s for s in self.ALL_F16X2_SITES if s in sites)
        if "point" in sites:
            return self.k_point_mlp_f16x2(t, b, prep_h["point"]).view(B, T_out, H, W, self.output_channels)
        return self.k_point_mlp(t, b, prep["point"]).view(B, T_out, H, W, self.output_channels)

    # ------------------------------------------------------------------ the training step
    def _prep_train(self, device):
        """The training step's layouts: they depend on the parameters alone (BatchNorm enters through the statistics kernels)."""
        return self._layouts.get("prep_train", list(self.parameters()), lambda: self._build_prep_train(device))

    def _build_prep_train(self, device):
        """Forward operands as ``_build_prep`` (without the folded running statistics) and, per GEMM, the transposed weight of its data
        gradient (``*_t``; the flipped, transposed taps ``wd`` for the convolutions of stages 2-4)."""
        f = dict(device=device, dtype=torch.float32)
        wp, prep = self.k_gemm_wprep, {}
        for i in range(4):
            conv = getattr(self.branch, f"conv{i + 1}")[0]
            Co, Ci = conv.weight.shape[:2]
            N = max(Co, 64)
            bias = torch.zeros(N, **f)
            bias[:Co] = conv.bias.detach()
            if i == 0:
                K = -(-27 * Ci // 64) * 64
                wm = torch.zeros(N, K, **f)
                wm[:Co, :27 * Ci] = conv.weight.detach().permute(0, 2, 3, 4, 1).reshape(Co, 27 * Ci)
                prep["s1"] = dict(wz=wp(wm), bias=bias, N=N, K=K, C=Co, Ci=Ci)
            else:
                K = max(Ci, 64)
                wz = torch.empty(3 * N * 27 * K, device=device, dtype=I16)
                conv3x_wprep(padded_weight(conv, N, K).to(device), wz, N, K)
                wd = torch.empty(3 * N * 27 * K, device=device, dtype=I16)
                conv3x_wprep(flipped_weight(conv, N, K).to(device), wd, K, N)
                prep[f"s{i + 1}"] = dict(wz=wz, wd=wd, bias=bias, N=N, K=K, C=Co, Ci=Ci)

        def linear(name, lin, w=None, n_pad=None):
            w = lin.weight.detach() if w is None else w
            b = lin.bias.detach()
            if n_pad is not None and n_pad > w.shape[0]:                # zero rows up to the narrowest GEMM tile
                w = torch.cat([w, torch.zeros(n_pad - w.shape[0], w.shape[1], **f)])
                b = torch.cat([b, torch.zeros(n_pad - b.shape[0], **f)])
            w = w.contiguous()
            prep[name] = dict(wz=wp(w), wz_t=wp(w.t().contiguous()), bias=b.contiguous(), N=w.shape[0], K=w.shape[1])

        fc0, fc3, tr, o = self.branch.fc[0], self.branch.fc[3], self.trunk.fc, self.output_net
        linear("fc0", fc0, fc0.weight.detach().reshape(512, 256, 4, 4).permute(0, 2, 3, 1).reshape(512, 4096))
        linear("fc3", fc3)
        w1 = torch.zeros(64, 64, **f)
        w1[:, :3] = tr[0].weight.detach()
        linear("t0", tr[0], w1)
        linear("t2", tr[2])
        linear("t4", tr[4])
        linear("o0", o[0])
        linear("o3", o[3])
        linear("o6", o[6], n_pad=64)
        return prep

    def _coords(self, T, H, W, device):
        """[N][64] fp32: the (t, h, w) coordinates of ``get_grid`` (float64 linspace per axis, cast) in columns 0..2, zeros beyond."""
        def build():
            axes = [torch.tensor(np.linspace(0, 1, n), dtype=torch.float) for n in (T, H, W)]
            c = torch.zeros(T * H * W, 64)
            c[:, :3] = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
            return c.to(device)

        return self._layouts.get("coords", (), build, extra=(T, H, W, str(device)))

    @staticmethod
    def _gemm(a, s, out, M, act=0, aux=None, drop=None, t=False):
        """out [M][N] = epilogue(a [M][K] W^T) on rpb_gemm3x; ``t``: the transposed weight (data gradient, no bias); ``drop``: None, a
        mask tensor (or ``ops.Sub`` at its first row) or (seed, keep)."""
        N, K = (s["K"], s["N"]) if t else (s["N"], s["K"])
        mask = None if drop is None or isinstance(drop, tuple) else drop
        seed, keep = drop if isinstance(drop, tuple) else (0, 0.0)
        _lib.call("rpb_gemm3x", _p(a), _p(s["wz_t" if t else "wz"], I16), None if t else _p(s["bias"]), None, None, _p(out), M, N, K, K, N, act,
                  _p(aux), None, _p(mask), int(seed), float(keep), _stream(), label=f"don_gemm3x[N{N},K{K}]",
                  nbytes=4 * (M * K + M * N) + 6 * N * K, flops=2 * M * N * K)
        return out

    # the row passes of the training step that are DeepONet's own (csrc/rpb_deeponet_train.hip); row operands: fp32 tensors or ``ops.Sub`` at
    # the first column
    @staticmethod
    def k_pool_bwd(y, ldy, g, ldg, ab, gz, ldz, B, T, H, W, C, mode, part):
        _lib.call("rpb_don_pool_bwd", _p(y), ldy, _p(g), ldg, _p(ab[0]), _p(ab[1]), _p(ab[2]), _p(ab[3]), _p(gz), ldz, B, T, H, W, C, mode,
                  _p(part, torch.float64), _stream(), label="don_pool_bwd", nbytes=8 * B * T * H * W * C)

    @staticmethod
    def k_point_mul(t, b, x, q0, R, B, N, p):
        _lib.call("rpb_don_point_mul", _p(t), _p(b), _p(x), q0, R, B, N, p, _stream(), label="don_point_mul", nbytes=8 * R * p)

    @staticmethod
    def k_point_mul_bwd(gx, t, b, gt, part, n0, R, N, p):
        _lib.call("rpb_don_point_mul_bwd", _p(gx), _p(t), _p(b), _p(gt), _p(part), n0, R, N, p, _stream(), label="don_point_mul_bwd",
                  nbytes=16 * R * p)

    def _bn_batch(self, y, ld, M, C, bn, parts=None):
        """``batch_norm_rows`` and the stage's batch counter"""
        ab = batch_norm_rows(y, ld, M, C, bn, parts, sync=self.bn_sync)
        bn.num_batches_tracked += 1
        return ab

    def _drop(self, layer, chunk, step, row0=0):
        """The dropout argument of one GEMM launch: None (rate 0), the explicit mask's rows from ``row0`` (tests), or (seed, keep)."""
        if self.dropout_rate <= 0:
            return None
        if self._mask_override is not None:
            m = self._mask_override[layer]
            return Sub(m, row0 * m.shape[1])
        rank = self.bn_sync.rank if self.bn_sync is not None else 0
        return (drop_seed(rank_seed_base(self.dropout_seed, rank), step, layer, chunk), 1.0 - self.dropout_rate)

    def _point_chunk(self, prep, t, b, q0, R, B, N, step, ci):
        """x, h1, h2 of the points q0 .. q0 + R - 1 (forward, and the backward's recomputation with the same seeds / masks)."""
        dev, p = t.device, self.p
        x = torch.empty(R, p, device=dev, dtype=torch.float32)
        self.k_point_mul(t, b, x, q0, R, B, N, p)
        h1 = self._gemm(x, prep["o0"], torch.empty(R, 512, device=dev, dtype=torch.float32), R, act=3, drop=self._drop(1, ci, step, q0))
        h2 = self._gemm(h1, prep["o3"], torch.empty(R, 128, device=dev, dtype=torch.float32), R, act=3, drop=self._drop(2, ci, step, q0))
        return x, h1, h2

    @torch.no_grad()
    def _forward_hip(self, x, state):
        """Training forward: batch-statistics BatchNorm (running statistics updated), active dropout, the trunk and the output net as
        GEMM chains.  ``state`` (a dict, or None) receives what the backward pass reads: per stage the input rows, the convolution
        output and (a, b, mean, rstd); the branch's hidden row, ``b``; the trunk's hidden rows, ``t``; the step number of the dropout
        seeds.  Nothing of size B N 512 is kept: the backward pass recomputes the output net chunk by chunk."""
        x = x.contiguous().float()
        dev, f = x.device, dict(device=x.device, dtype=torch.float32)
        B, T, H, W, Cin = x.shape
        T_out, p, Cout = self.shape_out[0], self.p, self.output_channels
        prep, ext, rows = self._prep_train(dev), pooled_extents(T, H, W), ops.rowbn_rows()
        world = self.bn_sync.world_size if reduces_stats(self.bn_sync) else 1       # SyncBN: the statistics see the rows of every rank
        for Ti, Hi, Wi in ext:                                        # before anything is launched: no statistic moves, no step is used up
            if world * B * Ti * Hi * Wi < 2:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size [{B}, C, {Ti}, {Hi}, {Wi}]")
        step = self._drop_step
        stages = []
        # stage 1 in chunks of samples (the im2col buffer stays bounded); the 64-wide rows are kept (the backward pass needs them anyway),
        # the statistics are accumulated over the chunks before anything is pooled
        s1, cells = prep["s1"], T * H * W
        nb = max(1, _COL_FLOATS // (cells * s1["K"]))
        nchunk = -(-B // nb)
        y = torch.empty(B * cells, 64, **f)
        parts = torch.empty(1, nchunk * rows, 64, device=dev, dtype=torch.float64)
        for k, b0 in enumerate(range(0, B, nb)):
            nbc = min(nb, B - b0)
            col = torch.empty(nbc * cells, s1["K"], **f)
            _lib.call("rpb_im2col", _p(x[b0:b0 + nbc]), _p(col), nbc, T, H, W, Cin, 3, s1["K"], _stream(), label="don_im2col",
                      nbytes=4 * nbc * cells * (Cin + s1["K"]))
            self._gemm(col, s1, Sub(y, b0 * cells * 64), nbc * cells)
            ops.rowbn_stats(Sub(y, b0 * cells * 64), 64, nbc * cells, 32, parts[0, k * rows:(k + 1) * rows])
        ab = self._bn_batch(y, 64, B * cells, 32, self.branch.conv1[1], parts)
        h = self.k_bn_relu_pool(y, ab[0], ab[1], B, T, H, W, 32, 64, 0)
        stages.append(dict(y=y, ab=ab, src=None))
        for i in (2, 3, 4):
            s, (Ti, Hi, Wi) = prep[f"s{i}"], ext[i - 1]
            M = B * Ti * Hi * Wi
            y = self.k_conv(h, s, (Ti, Hi, Wi))
            ab = self._bn_batch(y, s["N"], M, s["C"], getattr(self.branch, f"conv{i}")[1])
            stages.append(dict(y=y, ab=ab, src=h))
            h = self.k_bn_relu_pool(y, ab[0], ab[1], B, Ti, Hi, Wi, s["C"], s["C"], 0 if i < 4 else 1)
        h4 = h.view(B, 4096)
        z = self._gemm(h4, prep["fc0"], torch.empty(B, 512, **f), B, act=3, drop=self._drop(0, 0, step))
        b = self._gemm(z, prep["fc3"], torch.empty(B, p, **f), B)
        # trunk: three GEMMs over the coordinate matrix, the two hidden activations kept
        N = T_out * H * W
        coords = self._coords(T_out, H, W, dev)
        u1 = self._gemm(coords, prep["t0"], torch.empty(N, 64, **f), N, act=3)
        u2 = self._gemm(u1, prep["t2"], torch.empty(N, 128, **f), N, act=3)
        t = self._gemm(u2, prep["t4"], torch.empty(N, p, **f), N)
        # output net in chunks of points
        Q, RC = B * N, self._point_rows
        out = torch.empty(Q, Cout, **f)
        o = torch.empty(min(RC, Q), 64, **f)
        for ci, q0 in enumerate(range(0, Q, RC)):
            R = min(RC, Q - q0)
            _, _, h2 = self._point_chunk(prep, t, b, q0, R, B, N, step, ci)
            self._gemm(h2, prep["o6"], o, R)
            out[q0:q0 + R] = o[:R, :Cout]
        self._drop_step = step + 1                                    # a forward that ran to its end used this step's seeds
        if state is not None:
            state.update(x=x, stages=stages, h4=h4, z=z, b=b, coords=coords, u1=u1, u2=u2, t=t, step=step, shape=(B, T, H, W, T_out))
        return out.view(B, T_out, H, W, Cout)

    @torch.no_grad()
    def _backward_hip(self, state, g_out, need_gx=False):
        """{parameter: gradient} from dLoss/d(out).  The output net walks the forward's chunks again (x, h1, h2 recomputed with the same
        seeds), then the trunk from ``gt``, the branch's Linear layers from ``gb`` and the four stages in reverse: pooling + ReLU +
        BatchNorm backward row passes give ``dy``, ``wgrad`` gives (dW, db), rpb_conv3x on the flipped taps gives the gradient of the
        stage's input.  No atomics; ``state`` is only read: a second call gives bit-equal gradients."""
        if need_gx:
            raise NotImplementedError("DeepONet training computes no input gradient (no trainer asks for one)")
        dev, f = g_out.device, dict(device=g_out.device, dtype=torch.float32)
        B, T, H, W, T_out = state["shape"]
        p, Cout, N = self.p, self.output_channels, T_out * H * W
        prep, rows = self._prep_train(dev), ops.rowbn_rows()
        t, b, step = state["t"], state["b"], state["step"]
        grads, acc = {}, {}

        def accumulate(key, dW, db):                                    # chunk after chunk, in order
            acc[key] = (dW, db) if key not in acc else (ops_add(acc[key][0], dW), ops_add(acc[key][1], db))

        # ---- output net
        Q, RC = B * N, self._point_rows
        gq = g_out.reshape(Q, Cout)
        gt, gb = torch.zeros(N, p, **f), torch.zeros(B, p, **f)
        part = torch.empty(rows, p, **f)
        for ci, q0 in enumerate(range(0, Q, RC)):
            R = min(RC, Q - q0)
            x, h1, h2 = self._point_chunk(prep, t, b, q0, R, B, N, step, ci)
            go = torch.zeros(R, 64, **f)
            go[:, :Cout] = gq[q0:q0 + R]
            accumulate("o6", *wgrad(go, h2, R, 64, 128))
            gh2 = self._gemm(go, prep["o6"], torch.empty(R, 128, **f), R, act=4, aux=h2, drop=self._drop(2, ci, step, q0), t=True)
            accumulate("o3", *wgrad(gh2, h1, R, 128, 512))
            gh1 = self._gemm(gh2, prep["o3"], torch.empty(R, 512, **f), R, act=4, aux=h1, drop=self._drop(1, ci, step, q0), t=True)
            accumulate("o0", *wgrad(gh1, x, R, 512, p))
            gx = self._gemm(gh1, prep["o0"], torch.empty(R, p, **f), R, t=True)
            q = q0
            while q < q0 + R:                                            # one launch per sample the chunk touches: gt[n] += has one writer
                s, n0 = divmod(q, N)
                Rs = min(N - n0, q0 + R - q)
                self.k_point_mul_bwd(Sub(gx, (q - q0) * p), t, Sub(b, s * p), gt, part, n0, Rs, N, p)
                reduce_partials(part, rows, p, out_f32=Sub(gb, s * p), accumulate=True)
                q += Rs
        o = self.output_net
        grads[o[6].weight], grads[o[6].bias] = acc["o6"][0][:Cout].contiguous(), acc["o6"][1][:Cout].contiguous()
        grads[o[3].weight], grads[o[3].bias] = acc["o3"]
        grads[o[0].weight], grads[o[0].bias] = acc["o0"]
        # ---- trunk
        tr, u1, u2 = self.trunk.fc, state["u1"], state["u2"]
        grads[tr[4].weight], grads[tr[4].bias] = wgrad(gt, u2, N, p, 128)
        gu2 = self._gemm(gt, prep["t4"], torch.empty(N, 128, **f), N, act=4, aux=u2, t=True)
        grads[tr[2].weight], grads[tr[2].bias] = wgrad(gu2, u1, N, 128, 64)
        gu1 = self._gemm(gu2, prep["t2"], torch.empty(N, 64, **f), N, act=4, aux=u1, t=True)
        dW, grads[tr[0].bias] = wgrad(gu1, state["coords"], N, 64, 64)
        grads[tr[0].weight] = dW[:, :3].contiguous()
        # ---- branch: the two Linear layers
        fc, z, h4 = self.branch.fc, state["z"], state["h4"]
        grads[fc[3].weight], grads[fc[3].bias] = wgrad(gb, z, B, p, 512)
        gz0 = self._gemm(gb, prep["fc3"], torch.empty(B, 512, **f), B, act=4, aux=z, drop=self._drop(0, 0, step), t=True)
        dW, grads[fc[0].bias] = wgrad(gz0, h4, B, 512, 4096)
        grads[fc[0].weight] = dW.view(512, 4, 4, 256).permute(0, 3, 1, 2).reshape(512, 4096)       # (h, w, c) columns -> the reference's (c, h, w)
        g, ldg = self._gemm(gz0, prep["fc0"], torch.empty(B, 4096, **f), B, t=True), 256          # [B][4][4][256]
        # ---- branch: the four stages, last first
        ext = pooled_extents(T, H, W)
        for i in (4, 3, 2, 1):
            s, (Ti, Hi, Wi), st = prep[f"s{i}"], ext[i - 1], state["stages"][i - 1]
            conv, bn = getattr(self.branch, f"conv{i}")[:2]
            C, Nw, M = s["C"], s["N"], B * Ti * Hi * Wi
            y, ab = st["y"], st["ab"]
            dy = torch.empty(M, Nw, **f)
            part64 = torch.empty(rows, 2 * C, device=dev, dtype=torch.float64)
            self.k_pool_bwd(y, Nw, g, ldg, ab, dy, Nw, B, Ti, Hi, Wi, C, 1 if i == 4 else 0, part64)
            grads[bn.weight], grads[bn.bias] = batch_norm_rows_bwd(part64, dy, Nw, y, Nw, ab, M, C, Nw, 0, dy, Nw,
                                                                       sync=self.bn_sync)       # in place on dy
            if i == 1:                                                  # the im2col GEMM form, chunked like the forward
                cells = Ti * Hi * Wi
                nb = max(1, _COL_FLOATS // (cells * s["K"]))
                tot = None
                for b0 in range(0, B, nb):
                    nbc = min(nb, B - b0)
                    col = torch.empty(nbc * cells, s["K"], **f)
                    _lib.call("rpb_im2col", _p(state["x"][b0:b0 + nbc]), _p(col), nbc, Ti, Hi, Wi, s["Ci"], 3, s["K"], _stream(),
                              label="don_im2col", nbytes=4 * nbc * cells * (s["Ci"] + s["K"]))
                    dWc = wgrad(Sub(dy, b0 * cells * 64), col, nbc * cells, 64, s["K"])
                    tot = dWc if tot is None else (ops_add(tot[0], dWc[0]), ops_add(tot[1], dWc[1]))
                Ci = s["Ci"]
                grads[conv.weight] = tot[0][:C, :27 * Ci].reshape(C, 3, 3, 3, Ci).permute(0, 4, 1, 2, 3).contiguous()
                grads[conv.bias] = tot[1][:C].contiguous()
                break
            K = s["K"]
            dW, db = wgrad(dy, st["src"], M, Nw, 27 * K, ldg=Nw, lda=K, conv=(Ti, Hi, Wi))
            grads[conv.weight], grads[conv.bias] = weight_grad_view(dW, C, s["Ci"], Nw, K), db[:C].contiguous()
            planes = torch.empty(3 * M * Nw, device=dev, dtype=I16)
            split3(dy, planes, M, Nw)
            g, ldg = torch.empty(M, K, **f), K
            conv3x(planes, s["wd"], g, M, K, Nw, (Ti, Hi, Wi))
        return grads
