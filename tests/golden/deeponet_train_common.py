"""Shared by tests/golden/make_golden_deeponet_train.py (reference side) and tests/test_deeponet_train_host.py /
tests/test_gpu_deeponet_train.py: the cases of the DeepONet training fixture, their seeded inputs and dropout masks and the fixed
sub-sampling of what it stores.  Weights are ``deeponet_common.seeded_weights``; the model runs in ``train()`` mode (batch statistics,
active dropout)."""
from collections import OrderedDict

import torch

import deeponet_common as DC

# name -> (shape_in, shape_out, p, batch, dropout_rate)
CASES = OrderedDict([
    # pooled grids (8,8,16) (4,4,8) (2,2,4) (1,1,2): adaptive bins replicated in H (1 -> 4) and W (2 -> 4); N = 1024; the Adam case
    ("a", ((8, 8, 16, 3), (8, 8, 16, 3), 64, 2, 0.0)),
    # control channels, odd batch, T_out != T_in, T 10 -> 5 -> 2 -> 1 (a dropped frame at the second pool), H 12 -> 6 -> 3 -> 1 (a dropped
    # row at the third), W 40 -> 20 -> 10 -> 5: adaptive bins replicated in H (1 -> 4), overlapping in W (5 -> 4); N = 480
    ("b", ((10, 12, 40, 5), (1, 12, 40, 3), 128, 3, 0.0)),
    # B = 1, C_out != C_in, every extent of the first pool odd (21, 11, 45), then (10, 5, 22) and (5, 2, 11): a dropped frame, row and
    # column; stage 4 sees (2, 1, 5): mean over T, replicated H (1 -> 4), overlapping W (5 -> 4); N = 2475 (no multiple of 32)
    ("c", ((21, 11, 45, 3), (5, 11, 45, 2), 256, 1, 0.0)),
    # dropout 0.1 with the seeded explicit masks of ``dropout_masks``; N = 128.  Small on purpose: among n ReLU inputs the smallest lies
    # about 1 / (0.8 n) standard deviations from zero.  The output net's first layer has B N 512 of them and its margin is about 4e-6,
    # so from n of about 0.3 M on a seed that passes sits right AT the margin, where another summation order can still turn a gate; the
    # 0.13 M inputs here leave a typical seed several margins of room
    ("d", ((8, 8, 16, 3), (1, 8, 16, 3), 64, 2, 0.1)),
])
# Input seeds.  The backward pass is discontinuous at every ReLU gate and at every max-pool arg-max: where fp32 and fp64 decide
# differently at one element, a gradient moves by per cent, not by rounding.  make_golden_deeponet_train.py keeps a seed only if, in the
# reference's fp64 run, every ReLU input and every gap between the two largest values of a max-pool window with a positive maximum
# lies at least three times the reference's own fp32-vs-fp64 deviation of that tensor away from zero (both in standard deviations of
# the tensor; the generator derives and prints that margin per tensor), and if the reference's fp32 run then agrees with its fp64 run
# to 1e-5 on every real gradient.  It asserts both and prints how many seeds it tried; SEEDS holds what it found, searching upwards
# from SEED_START.  The chance of a seed falls with the number of ReLU inputs (B N 512 in the output net alone), which is why the
# shapes are no larger than this.
SEED_START = {"a": 100, "b": 200, "c": 300, "d": 400}
SEEDS = {"a": 202, "b": 260, "c": 366, "d": 404}            # tried: 103, 61, 67, 5
N_SAMPLES = 128
N_OUT_SAMPLES = 2048
ADAM_CASE, ADAM_STEPS, ADAM_LR, ADAM_T_MAX = "a", 2, 1e-3, 10
TRACKED_BEFORE = 7                               # seeded_weights stores num_batches_tracked = 7
ZERO_BIAS = tuple(f"branch.conv{i}.0.bias" for i in (1, 2, 3, 4))     # in front of a BatchNorm: the gradient is zero analytically


def case_inputs(name, step=0, seed=None):
    """(x, y) of optimiser step ``step`` (a fresh batch per step), uniform in [-1, 1)."""
    shape_in, shape_out, _, B, _ = CASES[name]
    g = torch.Generator().manual_seed((SEEDS[name] if seed is None else seed) + 1000 * step)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32) * 2 - 1
    return u(B, *shape_in), u(B, *shape_out)


def weights(name):
    shape_in, shape_out, p, _, _ = CASES[name]
    return DC.seeded_weights(shape_in, shape_out, p)


def dropout_masks(name):
    """The pre-scaled inverted-dropout masks of the three dropout sites (branch.fc.2 [B][512], output_net.2 [B N][512], output_net.5
    [B N][128]; rows (sample, point)) from CPU generators; None at rate 0.  Not stored in the fixture."""
    shape_in, shape_out, _, B, rate = CASES[name]
    if rate <= 0:
        return None
    N = shape_out[0] * shape_in[1] * shape_in[2]
    keep = 1.0 - rate
    out = []
    for j, shape in enumerate(((B, 512), (B * N, 512), (B * N, 128))):
        g = torch.Generator().manual_seed(90001 + 17 * j + ord(name))
        out.append((torch.rand(*shape, generator=g, dtype=torch.float32) < keep).float() / keep)
    return out


def param_names(name):
    """(names with a real gradient, the four convolution biases in front of a BatchNorm), in ``state_dict`` order."""
    shape_in, shape_out, p, _, _ = CASES[name]
    keys = [k for k in DC.state_shapes(shape_in, shape_out, p) if k.rsplit(".", 1)[-1] in ("weight", "bias")]
    return [k for k in keys if k not in ZERO_BIAS], list(ZERO_BIAS)


def stat_names(name):
    shape_in, shape_out, p, _, _ = CASES[name]
    return [k for k in DC.state_shapes(shape_in, shape_out, p) if k.rsplit(".", 1)[-1] in ("running_mean", "running_var")]


def sample_index(n, numel, count=N_SAMPLES):
    """The flat indices stored of tensor number ``n`` (with repeats where the tensor is smaller)."""
    g = torch.Generator().manual_seed(7919 + n)
    return torch.randint(0, numel, (count,), generator=g)


def out_samples(out):
    return out.reshape(-1)[sample_index(100003, out.numel(), N_OUT_SAMPLES)]
