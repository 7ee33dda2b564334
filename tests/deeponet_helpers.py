"""Shared by tests/test_deeponet_host.py and tests/test_gpu_deeponet.py (a plain module, not a test file): the DeepONet fixture, the
tolerance rule and small helpers.

Tolerance of every comparison with a reference vector: Rel-L2 < max(1e-5, 4 x the reference's own fp32-vs-fp64 Rel-L2 stored next to
it, taken over the whole tensor before the fixture's fixed sub-sampling); the factor 4 allows for another summation order."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import deeponet_common as DC                      # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "deeponet_small.npz"))
CFG = json.load(open(os.path.join(ROOT, "tests", "golden", "deeponet_configs.json")))
SCENARIOS = ["cylinder", "controlled_cylinder", "fsi", "foil", "combustion"]


def tol(key):
    return max(1e-5, 4 * float(GOLD[key + "_selferr"]))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def sd_of(case):
    shape_in, shape_out, p, _ = DC.CASES[case]
    return DC.seeded_weights(shape_in, shape_out, p)


class One(torch.utils.data.Dataset):
    """A one-sample dataset of the given shapes: what ``load_model`` reads its shapes from."""

    def __init__(self, shape_in, shape_out):
        self.s = (torch.zeros(*shape_in), torch.zeros(*shape_out))

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.s
