"""Shared by tests/test_cno_train_host.py and tests/test_gpu_cno_train.py (a plain module, not a test file): the CNO3d training fixture
(tests/golden/cno_train_small.npz, written by tests/golden/make_golden_cno_train.py), its tolerance rule and small helpers.

GPU model against a reference value: Rel-L2 < max(1e-5, 4 x the reference's own fp32-vs-fp64 deviation stored next to it) -- the rule
of tests/cno_helpers.py; the factor 4 allows for another summation order and the bf16x3 split."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import cno_common as CC                           # noqa: E402
import cno_train_common as TC                     # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "cno_train_small.npz"))
TRAIN_MSG = "CNO training step is not built yet"


def tol(selferr):
    return max(1e-5, 4 * float(selferr))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def new_model(case):
    from realpdebench_amd.model.cno import CNO3d
    shape_in, shape_out, _ = TC.CASES[case]
    m = CNO3d(in_dim=shape_in[-1], out_dim=shape_out[-1], out_dim_mult=CC.out_dim_mult(shape_in, shape_out), in_size=shape_in[2],
              N_layers=CC.N_LAYERS)
    m.load_state_dict(TC.weights(case))
    return m


def stat_slices(case):
    """name -> slice of the fixture's concatenated running statistics"""
    sd, out, pos = TC.weights(case), {}, 0
    for k in TC.stat_names(case):
        out[k] = slice(pos, pos + sd[k].numel())
        pos += sd[k].numel()
    return out


def compare_gradients(case, grads, rule, report=None):
    """``grads``: {parameter name: gradient or None}.  Holds the Rel-L2 of the 128 samples and the relative error of the norm of every
    parameter with a real gradient to ``rule(selferr)``; returns (worst samples / bound, worst norm / bound, the list of misses) -- the
    caller prints ``report`` (one line per parameter) and then asserts that nothing missed."""
    real, _, _ = TC.param_names(case)
    worst, misses = [0.0, 0.0], []
    for i, n in enumerate(real):
        gt = grads[n].detach().double().cpu().reshape(-1)
        bound = rule(GOLD[f"{case}_g_selferr"][i])
        es = rel(gt[TC.sample_index(i, gt.numel())], GOLD[f"{case}_gsamp"][i])
        en = abs(float(gt.norm()) - float(GOLD[f"{case}_gnorm"][i])) / float(GOLD[f"{case}_gnorm"][i])
        if report is not None:
            report.append(f"  {n}: samples {es:.2e} norm {en:.2e} (bound {bound:.1e})")
        worst = [max(worst[0], es / bound), max(worst[1], en / bound)]
        if not es < bound:
            misses.append((n, "samples", es, bound))
        if not en < bound:
            misses.append((n, "norm", en, bound))
    return worst[0], worst[1], misses
