"""Shared by tests/golden/make_golden_mwt.py (reference side) and tests/test_mwt_host.py / tests/test_gpu_mwt.py: the cases, the
seeded weights and inputs of the MWT3d fixture and the fixed sub-sampling of what it stores for the native shape."""
from collections import OrderedDict

import torch

K, ALPHA, C = 3, 5, 4            # the hyper-parameters of every reference configs/*/mwt.yaml
W36 = C * K * K

# name -> (shape_in, shape_out, nCZ, batch)
CASES = OrderedDict([
    ("a", ((8, 16, 32, 3), (8, 16, 32, 3), 2, 2)),          # W = 2H; every level from 8 x 16 down overlaps its corner blocks
    ("b", ((10, 16, 16, 5), (10, 16, 16, 3), 2, 2)),        # W = H, T = 10 (6 rfft bins), C_in != C_out (controlled_cylinder)
    ("c", ((20, 64, 128, 3), (20, 64, 128, 3), 4, 1)),      # native cylinder shape, stored through strided()
])
ROLLOUT_STEPS = 3


def state_shapes(shape_in, shape_out, nCZ):
    """Reference ``state_dict`` layout of MWT3d(k=3, alpha=5, c=4, L=0): name -> (shape, dtype), in the reference's order."""
    mult = shape_in[2] // shape_in[1]
    dout = shape_out[-1] * shape_out[0] // shape_in[0]
    f, cf = torch.float32, torch.complex64
    s = OrderedDict()
    s["Lk.weight"], s["Lk.bias"] = ((W36, shape_in[-1]), f), ((W36,), f)
    for i in range(nCZ):
        p = f"MWT_CZ.{i}."
        for b in ("ec_s", "ec_d"):
            s[p + b] = ((4 * K * K, K * K), f)
        for b in ("rc_ee", "rc_eo", "rc_oe", "rc_oo"):
            s[p + b] = ((2 * K * K, K * K), f)
        for j in range(1, 5):
            s[p + f"A.weights{j}"] = ((W36, W36, ALPHA, ALPHA, ALPHA), cf)
        s[p + "A.Lo.weight"], s[p + "A.Lo.bias"] = ((W36, W36), f), ((W36,), f)
        for m in ("B", "C"):
            s[p + m + ".conv.0.weight"], s[p + m + ".conv.0.bias"] = ((W36, W36, 3, 3, 3), f), ((W36,), f)
            s[p + m + ".Lo.weight"], s[p + m + ".Lo.bias"] = ((W36, W36), f), ((W36,), f)
        s[p + "T0.weight"], s[p + "T0.bias"] = ((W36, W36 * mult), f), ((W36,), f)
    for i in range(nCZ):
        p = f"BN.{i}."
        for b in ("weight", "bias", "running_mean", "running_var"):
            s[p + b] = ((W36,), f)
        s[p + "num_batches_tracked"] = ((), torch.int64)
    s["Lc0.weight"], s["Lc0.bias"] = ((128, W36), f), ((128,), f)
    s["Lc1.weight"], s["Lc1.bias"] = ((dout, 128), f), ((dout,), f)
    return s


_BUFFERS = ("ec_s", "ec_d", "rc_ee", "rc_eo", "rc_oe", "rc_oo")


def _u(shape, g, scale):
    return (torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1) * scale


def seeded_weights(shape_in, shape_out, nCZ, seed=5):
    """Every learnable entry (and the unused BN.*) from torch.rand with fixed seeds -- no transcendental functions, so the values are
    the same on every host.  The filter buffers are NOT here: each side builds its own.  Scales: uniform +-sqrt(3 / fan_in) keeps
    the activations of order one through the blocks, biases of +-0.2 mix the ReLU gates."""
    out = OrderedDict()
    for n, (name, (shape, dtype)) in enumerate(state_shapes(shape_in, shape_out, nCZ).items()):
        if name.rsplit(".", 1)[-1] in _BUFFERS:
            continue
        g = torch.Generator().manual_seed(seed * 1000 + n)
        if dtype == torch.int64:
            out[name] = torch.tensor(7, dtype=torch.int64)
        elif dtype == torch.complex64:
            sc = (1.0 / shape[0]) ** 0.5
            out[name] = torch.complex(_u(shape, g, sc), _u(shape, g, sc))
        elif name.startswith("BN."):
            out[name] = torch.rand(*shape, generator=g, dtype=torch.float32) + 0.5
        elif name.endswith(".bias"):
            out[name] = _u(shape, g, 0.2)
        else:
            fan_in = 1
            for v in shape[1:]:
                fan_in *= v
            out[name] = _u(shape, g, (3.0 / fan_in) ** 0.5)
    return out


def case_inputs(name, seed=23):
    shape_in, shape_out, _, B = CASES[name]
    g = torch.Generator().manual_seed(seed + ord(name))
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32) * 2 - 1
    return u(B, *shape_in), u(B, *shape_out)


def normalizer_stats(name):
    """(mean_inputs, mean_targets, std_inputs, std_targets) of the Gaussian normaliser of the rollout, seeded."""
    shape_in, shape_out, _, _ = CASES[name]
    g = torch.Generator().manual_seed(99 + ord(name))
    mi = torch.rand(shape_in[-1], generator=g, dtype=torch.float32) - 0.5
    si = torch.rand(shape_in[-1], generator=g, dtype=torch.float32) + 0.5
    co = shape_out[-1]
    return mi, mi[:co].clone(), si, si[:co].clone()


def strided(t):
    """[B, T', H, W, C] -> every 5th frame, every 8th row / column (the native-shape case only; fixed here, not at test time)."""
    return t[:, ::5, ::8, ::8, :].contiguous()


def stored(name, t):
    return strided(t) if name == "c" else t.contiguous()


def roll_stored(name, t):
    """The rollout [B, 3 T, H, W, C_in]: every 2nd frame / row / column for the small cases (the fixture stays under 1 MiB)."""
    return strided(t) if name == "c" else t[:, ::2, ::2, ::2, :].contiguous()


def inter_stored(t):
    """Per-level tensors [B, Nx, Ny, T, 36] of CZ block 0: sample 0, rows / columns thinned to 4 rows where the level has more."""
    sx = max(1, t.shape[1] // 4)
    return t[:1, ::sx, ::sx].contiguous()
