"""Plain-torch restatement of the DeepONet evaluation forward (reference realpdebench/model/deeponet.py), stage by stage, on the
channels-last layout of realpdebench_amd.model.deeponet.  Runs on the CPU in fp32 or fp64 (the dtype of ``x``); the GPU tests compare
every kernel family against the matching function here, and tests/test_deeponet_host.py compares this file against the
reference's vectors.  ``sd`` is a reference-layout state dict."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5


def bn_relu(x, bn):
    """x [..., C] channels-last; bn = (weight, bias, running_mean, running_var)."""
    g, b, mu, var = (t.to(x.dtype) for t in bn)
    return F.relu((x - mu) / torch.sqrt(var + EPS) * g + b)


def max_pool(x):
    """MaxPool3d(2) with floor semantics on [B, T, H, W, C]: a trailing odd frame / row / column is dropped."""
    B, T, H, W, C = x.shape
    x = x[:, :T // 2 * 2, :H // 2 * 2, :W // 2 * 2].reshape(B, T // 2, 2, H // 2, 2, W // 2, 2, C)
    return x.amax(dim=(2, 4, 6))


def bins(n_in, n_out):
    return [(i * n_in // n_out, math.ceil((i + 1) * n_in / n_out)) for i in range(n_out)]


def adaptive_pool(x, out=(1, 4, 4)):
    """AdaptiveAvgPool3d(out) on [B, T, H, W, C] by the bin rule [floor(i In / Out), ceil((i + 1) In / Out))."""
    B, T, H, W, C = x.shape
    y = torch.empty(B, *out, C, dtype=x.dtype)
    for a, (t0, t1) in enumerate(bins(T, out[0])):
        for b, (h0, h1) in enumerate(bins(H, out[1])):
            for c, (w0, w1) in enumerate(bins(W, out[2])):
                y[:, a, b, c] = x[:, t0:t1, h0:h1, w0:w1].mean(dim=(1, 2, 3))
    return y


def conv(x, w, b):
    """Conv3d(3, padding 1) on channels-last [B, T, H, W, Ci] -> [B, T, H, W, Co]."""
    return F.conv3d(x.permute(0, 4, 1, 2, 3), w.to(x.dtype), b.to(x.dtype), padding=1).permute(0, 2, 3, 4, 1)


def _bn(sd, i):
    return tuple(sd[f"branch.conv{i}.1.{n}"] for n in ("weight", "bias", "running_mean", "running_var"))


def conv_bn_relu_pool(sd, i, x):
    y = bn_relu(conv(x, sd[f"branch.conv{i}.0.weight"], sd[f"branch.conv{i}.0.bias"]), _bn(sd, i))
    return max_pool(y) if i < 4 else adaptive_pool(y)


def branch_fc(sd, pooled):
    """pooled [B, 1, 4, 4, 256] channels-last; the reference flattens (c, h, w)."""
    z = pooled.permute(0, 4, 1, 2, 3).reshape(pooled.shape[0], -1)
    z = F.relu(F.linear(z, sd["branch.fc.0.weight"].to(z.dtype), sd["branch.fc.0.bias"].to(z.dtype)))
    return F.linear(z, sd["branch.fc.3.weight"].to(z.dtype), sd["branch.fc.3.bias"].to(z.dtype))


def branch(sd, x, keep=None):
    for i in (1, 2, 3, 4):
        x = conv_bn_relu_pool(sd, i, x)
        if keep is not None:
            keep.append(x)
    return branch_fc(sd, x)


def grid(T, H, W, dtype):
    """get_grid: np.linspace(0, 1, n) in float64, cast to float32 (then to ``dtype``), [T * H * W, 3]."""
    ax = [torch.tensor(np.linspace(0, 1, n), dtype=torch.float).to(dtype) for n in (T, H, W)]
    return torch.stack(torch.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def _mlp(z, layers):
    for j, (w, b) in enumerate(layers):
        z = F.linear(z, w.to(z.dtype), b.to(z.dtype))
        if j + 1 < len(layers):
            z = F.relu(z)
    return z


def trunk(sd, T, H, W, dtype=torch.float64):
    return _mlp(grid(T, H, W, dtype), [(sd[f"trunk.fc.{i}.weight"], sd[f"trunk.fc.{i}.bias"]) for i in (0, 2, 4)])


def point_mlp(sd, t, b):
    """t [N, p], b [B, p] -> [B, N, C_out]"""
    return _mlp(b[:, None, :] * t[None], [(sd[f"output_net.{i}.weight"], sd[f"output_net.{i}.bias"]) for i in (0, 3, 6)])


def forward(sd, x, shape_out, keep=None):
    B, _, H, W, _ = x.shape
    b = branch(sd, x, keep)
    if keep is not None:
        keep.append(b)
    out = point_mlp(sd, trunk(sd, shape_out[0], H, W, x.dtype), b)
    return out.reshape(B, shape_out[0], H, W, -1)
