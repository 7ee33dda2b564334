"""DeepONet on MI355X -- drop-in for ``realpdebench.model.deeponet.DeepONet`` (reference realpdebench/model/deeponet.py, built by
``load_model`` like model/load_model.py:132-143) for the reference's ``configs/*/deeponet.yaml`` (p = 64 / 128 / 256).

Evaluation forward, ``train_loss`` as a value, the autoregressive rollout and checkpoint I/O.  The training step is not built: every
attempt to backpropagate raises ``NotImplementedError`` (``_common.EvalOnly``) instead of returning tensors without a graph, and
``trainer.make_trainer`` refuses the model at construction.  Dropout is the identity and BatchNorm3d uses its running statistics in
every mode (no batch-statistics path exists).

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

Parameters carry the reference's names, shapes and dtypes (``nn`` modules of the same tree, ``nn.Sequential`` indices included), so
``state_dict`` / ``load_state_dict`` are the reference's; kernel layouts are derived tensors rebuilt when a parameter changed.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..ops import _p, _stream, conv3x_wprep
from ._common import EvalOnly, padded_weight
from .model import Model

I16 = torch.int16
P_SUPPORTED = (64, 128, 256)
_COL_FLOATS = 1 << 28          # stage-1 im2col buffer bound (1 GiB): larger batches run the first stage in chunks of samples


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


class DeepONet(EvalOnly, Model):
    batch_independent = True                        # BatchNorm runs on its running statistics only
    training_unavailable = EvalOnly.TRAIN_MSG.format("DeepONet", "DeepONet")

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

    # ------------------------------------------------------------------ checkpoints
    def load_checkpoint(self, checkpoint_path, device="cpu"):
        """The base class's loader (``model_state_dict`` + bookkeeping, realpdebench/model/model.py); a bare weights file gives the
        bookkeeping entries of an untrained run (iteration 0, no losses), as MWT3d does."""
        ck = torch.load(checkpoint_path, map_location="cpu")
        if "model_state_dict" in ck:
            meta = super().load_checkpoint(checkpoint_path, "cpu")
        else:
            self.load_state_dict(ck)
            meta = self._bookkeeping({})
        self.to(device)
        return meta

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

    # ------------------------------------------------------------------ forward
    def branch_forward(self, x, prep, keep=None):
        """b [B][p]; ``keep`` (a list) receives the four pooled stage outputs, channels-last [B][T'][H'][W'][C] (tests)."""
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
            c = self.k_conv(h, s, (T, H, W))
            h = self.k_bn_relu_pool(c, s["sc"], s["sh"], B, T, H, W, s["C"], s["C"], 0 if i < 4 else 1)
            if keep is not None:
                keep.append(h.view(B, *((T // 2, H // 2, W // 2) if i < 4 else (1, 4, 4)), s["C"]))
        z = self.k_gemm(h.view(B, 4096), *prep["fc0"], 512, relu=True)
        return self.k_gemm(z, *prep["fc3"], self.p, relu=False)

    def forward(self, x):
        self._require_eval(x)
        self._require_hip(x)
        if x.dim() != 5 or x.shape[1] != self.shape_in[0] or x.shape[-1] != self.input_channels:
            raise ValueError(f"DeepONet was built for inputs [B, {self.shape_in[0]}, H, W, {self.input_channels}], got {tuple(x.shape)}")
        if min(pooled_extents(*x.shape[1:4])[3]) < 1:
            raise ValueError(f"DeepONet: input {tuple(x.shape)} leaves an empty extent after three MaxPool3d(2)")
        with torch.no_grad():
            x = x.contiguous().float()
            B, _, H, W, _ = x.shape                                   # T_out from shape_out, H and W from the input (deeponet.py:122-126)
            T_out = self.shape_out[0]
            prep = self._prep(x.device)
            b = self.branch_forward(x, prep)
            t = self._trunk(T_out, H, W, x.device)
            return self.k_point_mlp(t, b, prep["point"]).view(B, T_out, H, W, self.output_channels)
