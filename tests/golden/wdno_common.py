"""Shared by tests/golden/make_golden_wdno.py (reference side) and tests/test_wdno_host.py / tests/test_gpu_wdno.py: the cases of the
WDNO fixture, its seeded weights, inputs and noise draws, and the fixed sub-sampling of what it stores.

Weights are not stored: ``fill`` makes every ``model.*`` entry of the state dict from a generator seeded by the entry's name (torch.rand
only -- no transcendental function, so the values are the same on every host).  The schedule buffers and the rotary ``freqs`` keep the
values their constructors give them.

Noise draws are not stored either (seven state-sized tensors per case would not fit a fixture file): ``noise(case, run, k, shape)`` is
draw ``k`` of a run -- the sum of twelve seeded uniforms minus six (mean 0, variance 1), added one by one so that every host forms the
same bits -- and the fixture records each draw's sum and sum of squares, which the tests check before they use it."""
import zlib
from collections import OrderedDict

import torch

DIM, DIM_MULTS, B = 64, (1, 2), 2
CASES = OrderedDict([
    # bior1.1: coefficient mesh (2, 8, 12) padded to (4, 8, 12) -- the pad condition is live in T only; 24 state channels
    ("a", dict(wave="bior1.1", shape_in=(4, 16, 24, 2), shape_out=(4, 16, 24, 1), coef=(2, 8, 12), padded=(4, 8, 12),
               runs=OrderedDict([("ddim", dict(timesteps=1000, sampling_timesteps=3, eta=1.0)),
                                 ("anc", dict(timesteps=4, sampling_timesteps=None, eta=0.0))]))),
    # bior1.3, T_out = 2 T_in: coefficient mesh (5, 7, 7) padded to (8, 8, 8), pad_x = 1, odd extents, the crop live in the reconstruction
    ("b", dict(wave="bior1.3", shape_in=(6, 10, 10, 1), shape_out=(12, 10, 10, 1), coef=(5, 7, 7), padded=(8, 8, 8),
               runs=OrderedDict([("ddim", dict(timesteps=1000, sampling_timesteps=3, eta=1.0))]))),
])
LOSS_T = (700, 150)                     # the fixed diffusion steps of the train_loss vectors (one per sample), timesteps = 1000
N_DATASET = 4


def channels(case):
    c = CASES[case]
    return 8 * (c["shape_in"][-1] + c["shape_out"][-1] * c["shape_out"][0] // c["shape_in"][0])


def state_shape(case):
    return (B, *CASES[case]["padded"], channels(case))


def n_draws(case, run):
    """sample_noise calls of one forward: DDIM draws twice at the start (wdno.py:382-383) and once per step but the last; the ancestral
    loop once at the start and once per step with t > 0"""
    r = CASES[case]["runs"][run]
    return 2 + r["sampling_timesteps"] - 1 if r["sampling_timesteps"] is not None else 1 + r["timesteps"] - 1


def _gen(*words):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(w) for w in words).encode()))


def _u(g, shape, scale=1.0):
    return (torch.rand(*shape, generator=g, dtype=torch.float32) * 2 - 1) * scale


def fill(name, shape):
    """the seeded value of state-dict entry ``name`` (a ``model.*`` key), or None for an entry that keeps its constructed value"""
    if not name.startswith("model.") or name.endswith("rotary_emb.freqs"):
        return None
    g = _gen("wdno-weight", name)
    shape = tuple(shape)
    if name.endswith("norm.weight") or name.endswith("norm.gamma"):
        return torch.rand(*shape, generator=g, dtype=torch.float32) * 0.5 + 0.75
    if name.endswith("norm.bias"):
        return _u(g, shape, 0.2)
    if name.endswith("relative_attention_bias.weight"):
        return _u(g, shape, 1.0)
    if name.endswith(".bias"):
        return _u(g, shape, 0.1)
    fan_in = 1
    for v in shape[1:]:
        fan_in *= v
    return _u(g, shape, (3.0 / fan_in) ** 0.5)


def seeded_state(state_dict):
    """``state_dict`` with every ``model.*`` entry replaced by its seeded value"""
    out = OrderedDict()
    for k, v in state_dict.items():
        f = fill(k, v.shape)
        out[k] = v if f is None else f.to(v.dtype)
    return out


def noise(case, run, k, shape=None):
    g = _gen("wdno-noise", case, run, k)
    shape = tuple(shape or state_shape(case))
    acc = torch.rand(*shape, generator=g, dtype=torch.float32)
    for _ in range(11):
        acc = acc + torch.rand(*shape, generator=g, dtype=torch.float32)
    return acc - 6.0


def noise_checksum(t):
    return torch.stack((t.double().sum(), (t.double() ** 2).sum()))


def case_inputs(case):
    c = CASES[case]
    g = _gen("wdno-input", case)
    return _u(g, (B, *c["shape_in"])), _u(g, (B, *c["shape_out"]))


class Dataset(torch.utils.data.Dataset):
    """the four-sample numerical dataset the rescaler is computed from; sample 0 also gives the model its shapes"""
    dataset_type = "numerical"

    def __init__(self, case):
        c = CASES[case]
        g = _gen("wdno-dataset", case)
        # channel- and sample-dependent amplitudes, so that the per-column maxima differ
        amp_i = torch.rand(N_DATASET, 1, 1, 1, c["shape_in"][-1], generator=g) * 2 + 0.5
        amp_o = torch.rand(N_DATASET, 1, 1, 1, c["shape_out"][-1], generator=g) * 2 + 0.5
        self.inputs = _u(g, (N_DATASET, *c["shape_in"])) * amp_i
        self.targets = _u(g, (N_DATASET, *c["shape_out"])) * amp_o

    def __len__(self):
        return N_DATASET

    def __getitem__(self, i):
        return self.inputs[i], self.targets[i]


def thin(t):
    """state-sized tensors [B, Tp, Hp, Wp, C] as stored: sample 1, every second row and column"""
    return t[1:2, :, ::2, ::2, :].contiguous()
