"""Shared by tests/golden/make_golden_cno_train.py (reference side) and tests/test_cno_train_host.py / tests/test_gpu_cno_train.py: the
cases of the CNO3d training fixture, their seeded inputs and the fixed sub-sampling of the gradients it stores.  Weights are
``cno_common.seeded_weights``; the model runs in ``train()`` mode (batch statistics)."""
from collections import OrderedDict

import torch

import cno_common as CC

# name -> (shape_in, shape_out, batch); M = batch * T * H * W
CASES = OrderedDict([
    ("d", ((5, 6, 8, 3), (5, 6, 8, 3), 3)),      # M = 720: a tail tile, two sample boundaries inside tiles; wgrad on the exact-fp32 kernel
    ("g", ((4, 3, 16, 3), (4, 3, 16, 3), 2)),    # M = 384, W = 16: wgrad takes the split-bf16 kernel at the 64 / 128-channel layers
    ("h", ((8, 4, 6, 5), (8, 4, 6, 3), 3)),      # M = 576: control channels
    ("c", ((4, 9, 7, 3), (8, 9, 7, 2), 1)),      # M = 252: out_dim_mult = 2, odd mesh, B = 1
])
# Input seeds.  The backward pass is discontinuous in the LeakyReLU inputs: where fp32 and fp64 take different gates at one element,
# the gradient of that layer's channel moves by per cent, not by rounding.  fp32 arithmetic reaches a LeakyReLU input with an error
# of about 1.3e-6 standard deviations (the reference's own fp32-vs-fp64 output deviation), so a seed is kept only if, in the
# reference's fp64 run, every LeakyReLU input of every layer lies at least GATE_MARGIN = 4e-6 (three times that) standard deviations
# from zero, and if the reference's fp32 run then agrees with its fp64 run to 1e-5 on every gradient.  make_golden_cno_train.py
# asserts both; the seeds are the first ones from 102 / 216 / 331 / 447 upwards that meet the margin (about one seed in fifty does).
GATE_MARGIN = 4e-6
SEEDS = {"d": 173, "g": 216, "h": 467, "c": 448}
N_SAMPLES = 128
ADAM_CASE, ADAM_STEPS, ADAM_LR, ADAM_T_MAX = "g", 2, 1e-3, 10
TRACKED_BEFORE = 7                               # seeded_weights stores num_batches_tracked = 7


def case_inputs(name, step=0):
    """(x, y) of optimiser step ``step`` (a fresh batch per step), uniform in [-1, 1)."""
    shape_in, shape_out, B = CASES[name]
    g = torch.Generator().manual_seed(SEEDS[name] + 1000 * step)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float32) * 2 - 1
    return u(B, *shape_in), u(B, *shape_out)


def weights(name):
    shape_in, shape_out, _ = CASES[name]
    return CC.seeded_weights(shape_in, shape_out)


def param_names(name):
    """(names with a real gradient, the 31 convolution biases in front of a BatchNorm, names without any gradient), in
    ``state_dict`` order."""
    shape_in, shape_out, _ = CASES[name]
    keys = list(CC.state_shapes(shape_in, shape_out))
    has_bn = {k[:-len(".batch_norm.weight")] for k in keys if k.endswith(".batch_norm.weight")}
    real, zero_bias, none = [], [], []
    for k in keys:
        leaf = k.rsplit(".", 1)[-1]
        if leaf not in ("weight", "bias"):
            continue                                                  # running statistics, num_batches_tracked
        if k.startswith("decoder_inv.3."):
            none.append(k)
        elif leaf == "bias" and (k.endswith("convolution1.bias") or k.endswith("convolution2.bias")
                                 or (k.endswith(".convolution.bias") and k[:-len(".convolution.bias")] in has_bn)):
            zero_bias.append(k)
        else:
            real.append(k)
    assert len(zero_bias) == 31 and len(none) == 4, (len(zero_bias), len(none))
    return real, zero_bias, none


def stat_names(name):
    """The running statistics the forward updates, in ``state_dict`` order (``decoder_inv.3`` never runs)."""
    shape_in, shape_out, _ = CASES[name]
    return [k for k in CC.state_shapes(shape_in, shape_out)
            if k.rsplit(".", 1)[-1] in ("running_mean", "running_var") and not k.startswith("decoder_inv.3.")]


def sample_index(n, numel):
    """The 128 flat indices stored of gradient number ``n`` (with repeats where the tensor is smaller)."""
    g = torch.Generator().manual_seed(7919 + n)
    return torch.randint(0, numel, (N_SAMPLES,), generator=g)
