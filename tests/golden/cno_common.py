"""Shared by tests/golden/make_golden_cno.py (reference side) and tests/test_cno_host.py / tests/test_gpu_cno.py: the cases, the seeded
weights and inputs of the CNO3d fixture and the fixed sub-sampling of what it stores."""
from collections import OrderedDict

import torch

# name -> (shape_in, shape_out, batch); all with C < T (cno.py:467) and N_layers = 3
CASES = OrderedDict([
    ("a", ((6, 10, 12, 3), (6, 10, 12, 3), 2)),        # M = 1440 = 11 x 128 + 32: a tail tile, and the sample boundary (720) inside a tile
    ("b", ((8, 6, 10, 5), (8, 6, 10, 3), 3)),          # control channels, odd batch
    ("c", ((4, 9, 7, 3), (8, 9, 7, 2), 1)),            # out_dim_mult = 2, odd H and W, M = 252
])
N_LAYERS = 3
ROLLOUT_STEPS = 3
ROLLOUT_CASES = ("a", "b")                             # T_out == T_in
INTERMEDIATES = ("lift", "skip0", "skip1", "skip2", "neck")      # of case a
WIDTHS = (16, 32, 64, 128)


def out_dim_mult(shape_in, shape_out):
    return shape_out[0] // shape_in[0]


def state_shapes(shape_in, shape_out):
    """Reference ``state_dict`` layout of CNO3d(N_layers=3): name -> (shape, dtype), in the reference's order (232 entries,
    ``decoder_inv.3`` -- never used in forward -- and every ``num_batches_tracked`` included)."""
    f = torch.float32
    s = OrderedDict()

    def conv(q, ci, co):
        s[q + ".weight"], s[q + ".bias"] = ((co, ci, 3, 3, 3), f), ((co,), f)

    def bn(q, c):
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[q + "." + n] = ((c,), f)
        s[q + ".num_batches_tracked"] = ((), torch.int64)

    def block(q, ci, co):
        conv(q + ".convolution", ci, co)
        bn(q + ".batch_norm", co)

    w = WIDTHS
    cout = shape_out[-1] * out_dim_mult(shape_in, shape_out)
    conv("lift.inter_CNOBlock.convolution", shape_in[-1], 64)
    conv("lift.convolution", 64, w[0])
    conv("project.inter_CNOBlock.convolution", 2 * w[0], 64)
    conv("project.convolution", 64, cout)
    for i in range(3):
        block(f"encoder.{i}", w[i], w[i + 1])
    for i in range(4):
        block(f"ED_expansion.{i}", w[i], w[i])
    for i, (ci, co) in enumerate(((128, 64), (128, 32), (64, 16))):
        block(f"decoder.{i}", ci, co)
    for i, c in enumerate((128, 128, 64, 32)):
        block(f"decoder_inv.{i}", c, c)
    for i, c in enumerate((16, 32, 64) + (128,) * 6):
        q = f"res_nets.{i}"
        conv(q + ".convolution1", c, c)
        conv(q + ".convolution2", c, c)
        bn(q + ".batch_norm1", c)
        bn(q + ".batch_norm2", c)
    return s


def _u(shape, g, scale):
    return (torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1) * scale


def seeded_weights(shape_in, shape_out, seed=17):
    """Every entry from torch.rand with fixed seeds -- no transcendental functions, so the values are the same on every host.
    Default init gives block outputs of standard deviation 0.02-0.06; here convolution weights are uniform +-gain sqrt(3 / fan_in)
    with gain 1.4 (LeakyReLU(0.2) keeps 0.52 of the variance) and 0.6 on the second convolution of a residual block (the sum of nine
    residual adds stays of order one).  make_golden_cno.py asserts the LeakyReLU gate fractions, the block standard deviations and the
    BatchNorm statistics this gives."""
    out = OrderedDict()
    for n, (name, (shape, dtype)) in enumerate(state_shapes(shape_in, shape_out).items()):
        g = torch.Generator().manual_seed(seed * 1000 + n)
        leaf = name.rsplit(".", 1)[-1]
        is_bn = "batch_norm" in name
        if dtype == torch.int64:
            out[name] = torch.tensor(7, dtype=torch.int64)
        elif leaf == "running_mean":
            out[name] = _u(shape, g, 0.45)                                   # in [-0.5, 0.5], not the init value 0
        elif leaf == "running_var":
            out[name] = torch.rand(*shape, generator=g, dtype=torch.float32) * 1.4 + 0.55      # in [0.5, 2], not the init value 1
        elif is_bn:
            out[name] = torch.rand(*shape, generator=g, dtype=torch.float32) * 0.5 + 0.75 if leaf == "weight" else _u(shape, g, 0.3)
        elif leaf == "bias":
            out[name] = _u(shape, g, 0.2)
        else:
            fan_in = 1
            for v in shape[1:]:
                fan_in *= v
            gain = 0.6 if name.endswith("convolution2.weight") else 1.4
            out[name] = _u(shape, g, gain * (3.0 / fan_in) ** 0.5)
    return out


def case_inputs(name, seed=41):
    shape_in, shape_out, B = CASES[name]
    g = torch.Generator().manual_seed(seed + ord(name))
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32) * 2 - 1
    return u(B, *shape_in), u(B, *shape_out)


def normalizer_stats(name):
    """(mean_inputs, mean_targets, std_inputs, std_targets) of the Gaussian normaliser of the rollout, seeded."""
    shape_in, shape_out, _ = CASES[name]
    g = torch.Generator().manual_seed(87 + ord(name))
    mi = torch.rand(shape_in[-1], generator=g, dtype=torch.float32) - 0.5
    si = torch.rand(shape_in[-1], generator=g, dtype=torch.float32) + 0.5
    co = shape_out[-1]
    return mi, mi[:co].clone(), si, si[:co].clone()


def inter_stored(t):
    """Intermediates [B, T, H, W, C] of case a: sample 1 (rows beyond the sample boundary), every 2nd row / column."""
    return t[1:2, :, ::2, ::2, :].contiguous()
