"""Shared by tests/test_cno_host.py and tests/test_gpu_cno.py (a plain module, not a test file): the CNO3d fixture, the tolerance rules
and small helpers.

Host restatement (fp64) against a reference vector: Rel-L2 < 4 x the reference's own fp32-vs-fp64 Rel-L2 stored next to it (taken over
the whole tensor before the fixture's fixed sub-sampling) -- the fp64 restatement stands where the reference's fp64 run stood.
GPU model against a reference vector: Rel-L2 < max(1e-5, 4 x that error), the rule of tests/deeponet_helpers.py; the factor 4 allows
for another summation order."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import cno_common as CC                           # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cno_small.npz"))
CFG = json.load(open(os.path.join(ROOT, "tests", "golden", "cno_configs.json")))
SCENARIOS = ["cylinder", "controlled_cylinder", "fsi", "foil", "combustion"]
TRAIN_MSG = "CNO training step is not built yet"


def host_tol(key):
    return 4 * float(GOLD[key + "_selferr"])


def tol(key):
    return max(1e-5, 4 * float(GOLD[key + "_selferr"]))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def sd_of(case):
    shape_in, shape_out, _ = CC.CASES[case]
    return CC.seeded_weights(shape_in, shape_out)


def new_model(case):
    from realpdebench_amd.model.cno import CNO3d
    shape_in, shape_out, _ = CC.CASES[case]
    return CNO3d(in_dim=shape_in[-1], out_dim=shape_out[-1], out_dim_mult=CC.out_dim_mult(shape_in, shape_out), in_size=shape_in[2],
                 N_layers=CC.N_LAYERS)


class One(torch.utils.data.Dataset):
    """A one-sample dataset of the given shapes: what ``load_model`` reads its shapes from."""

    def __init__(self, shape_in, shape_out):
        self.s = (torch.zeros(*shape_in), torch.zeros(*shape_out))

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.s
