"""Shared by tests/golden/make_golden_deeponet.py (reference side) and tests/test_deeponet_host.py / tests/test_gpu_deeponet.py: the
cases, the seeded weights and inputs of the DeepONet fixture and the fixed sub-sampling of what it stores."""
from collections import OrderedDict

import torch

# name -> (shape_in, shape_out, p, batch)
CASES = OrderedDict([
    ("a", ((8, 32, 64, 3), (8, 32, 64, 3), 64, 2)),        # pooled grid 1 x 4 x 8: identity / pair bins in the adaptive pool; fsi's p
    ("b", ((10, 64, 32, 5), (10, 64, 32, 3), 128, 3)),     # control channels, T 10 -> 5 -> 2 -> 1 through the flooring pools, odd batch
    ("c", ((20, 20, 44, 3), (5, 20, 44, 2), 256, 1)),      # T_out != T_in, C_out != C_in, N = 4400 (tail tile), odd extents in every pool,
])                                                         # overlapping (5 -> 4) and replicated (2 -> 4) adaptive bins, mean over T 2 -> 1
ROLLOUT_STEPS = 3
ROLLOUT_CASES = ("a", "b")                                 # T_out == T_in
CHANS = (32, 64, 128, 256)


def state_shapes(shape_in, shape_out, p):
    """Reference ``state_dict`` layout of DeepONet: name -> (shape, dtype), in the reference's order."""
    f = torch.float32
    s = OrderedDict()
    ci = shape_in[-1]
    for i, co in enumerate(CHANS):
        q = f"branch.conv{i + 1}."
        s[q + "0.weight"], s[q + "0.bias"] = ((co, ci, 3, 3, 3), f), ((co,), f)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[q + "1." + n] = ((co,), f)
        s[q + "1.num_batches_tracked"] = ((), torch.int64)
        ci = co
    for name, (o, i) in (("branch.fc.0", (512, 4096)), ("branch.fc.3", (p, 512)), ("trunk.fc.0", (64, 3)), ("trunk.fc.2", (128, 64)),
                         ("trunk.fc.4", (p, 128)), ("output_net.0", (512, p)), ("output_net.3", (128, 512)),
                         ("output_net.6", (shape_out[-1], 128))):
        s[name + ".weight"], s[name + ".bias"] = ((o, i), f), ((o,), f)
    return s


def _u(shape, g, scale):
    return (torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1) * scale


def seeded_weights(shape_in, shape_out, p, seed=11):
    """Every entry from torch.rand with fixed seeds -- no transcendental functions, so the values are the same on every host.
    Weights are uniform +-1.6 sqrt(3 / fan_in): activations of order one through the ReLU layers; make_golden_deeponet.py asserts
    the ReLU gate fractions, the stage standard deviations and the BatchNorm statistics this gives."""
    out = OrderedDict()
    for n, (name, (shape, dtype)) in enumerate(state_shapes(shape_in, shape_out, p).items()):
        g = torch.Generator().manual_seed(seed * 1000 + n)
        leaf = name.rsplit(".", 1)[-1]
        if dtype == torch.int64:
            out[name] = torch.tensor(7, dtype=torch.int64)
        elif leaf == "running_mean":
            out[name] = _u(shape, g, 0.45)                                   # in [-0.5, 0.5], not the init value 0
        elif leaf == "running_var":
            out[name] = torch.rand(*shape, generator=g, dtype=torch.float32) * 1.4 + 0.55      # in [0.5, 2], not the init value 1
        elif ".1." in name and name.startswith("branch.conv"):               # BatchNorm weight / bias
            out[name] = torch.rand(*shape, generator=g, dtype=torch.float32) * 0.5 + 0.75 if leaf == "weight" else _u(shape, g, 0.3)
        elif leaf == "bias":
            out[name] = _u(shape, g, 0.2)
        else:
            fan_in = 1
            for v in shape[1:]:
                fan_in *= v
            out[name] = _u(shape, g, 1.6 * (3.0 / fan_in) ** 0.5)
    return out


def case_inputs(name, seed=31):
    shape_in, shape_out, _, B = CASES[name]
    g = torch.Generator().manual_seed(seed + ord(name))
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32) * 2 - 1
    return u(B, *shape_in), u(B, *shape_out)


def normalizer_stats(name):
    """(mean_inputs, mean_targets, std_inputs, std_targets) of the Gaussian normaliser of the rollout, seeded."""
    shape_in, shape_out, _, _ = CASES[name]
    g = torch.Generator().manual_seed(77 + ord(name))
    mi = torch.rand(shape_in[-1], generator=g, dtype=torch.float32) - 0.5
    si = torch.rand(shape_in[-1], generator=g, dtype=torch.float32) + 0.5
    co = shape_out[-1]
    return mi, mi[:co].clone(), si, si[:co].clone()


def stored(name, t):
    """[B, T, H, W, C]: every 2nd row / column for the two larger cases (the fixture stays well under 1 MiB); case c whole."""
    return t.contiguous() if name == "c" else t[:, :, ::2, ::2, :].contiguous()


def roll_stored(name, t):
    """The rollout [B, 3 T, H, W, C_in]: every 2nd frame, every 4th row / column."""
    return t[:, ::2, ::4, ::4, :].contiguous()


def pool_stored(t):
    """Pooled stage outputs [B, T', H', W', C] of case a: sample 0, rows / columns thinned to 4 rows where the stage has more."""
    sx = max(1, t.shape[2] // 4)
    return t[:1, :, ::sx, ::sx].contiguous()
