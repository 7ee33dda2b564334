"""TEST INFRASTRUCTURE ONLY -- shared by tests/test_mwt_train_host.py and tests/test_gpu_mwt_train.py: the fixture of the MWT3d training
step (tests/golden/mwt_train_small.npz) and the comparison of a set of gradients with it."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import mwt_common as MC                      # noqa: E402
import mwt_train_common as TC                # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "mwt_train_small.npz"))
TRAIN_MSG = "MWT training step is not built yet"


def tol(selferr):
    """the project's MWT rule (tests/test_mwt_host.py): max(1e-5, 4 x the reference's own fp32-versus-fp64 deviation)"""
    return max(1e-5, 4 * float(selferr))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def new_model(case, device="cpu"):
    from realpdebench_amd.model.mwt import MWT3d
    shape_in, shape_out = TC.CASES[case]
    m = MWT3d(k=MC.K, alpha=MC.ALPHA, c=MC.C, nCZ=TC.NCZ, L=0, base="legendre", shape_in=shape_in, shape_out=shape_out)
    m.load_state_dict(TC.weights(case), strict=False)
    return m.to(device)


def compare_gradients(case, grads):
    """``grads``: name -> gradient, for exactly the fixture's parameters with one.  Per parameter the norm and the 128 stored samples
    against the fp64 reference, each within ``tol(selferr)``; a parameter whose reference gradient is exactly zero must be exactly zero.
    Prints the worst figures, returns the list of misses."""
    real = [str(n) for n in GOLD[f"{case}_real"]]
    assert sorted(grads) == sorted(real), sorted(set(grads) ^ set(real))
    misses, worst = [], (0.0, "")
    for i, name in enumerate(real):
        g = TC.flat_real(grads[name].detach().cpu()).double()
        gnorm, gsamp, bound = float(GOLD[f"{case}_gnorm"][i]), GOLD[f"{case}_gsamp"][i], tol(GOLD[f"{case}_g_selferr"][i])
        if gnorm == 0:
            if bool(g.any()):
                misses.append((name, "reference gradient is exactly zero", float(g.abs().max())))
            continue
        e_norm = abs(float(g.norm()) - gnorm) / gnorm
        e_samp = rel(g[TC.sample_index(i, g.numel())], gsamp)
        e = max(e_norm, e_samp)
        if e / bound > worst[0]:
            worst = (e / bound, f"{name}: norm {e_norm:.2e} samples {e_samp:.2e} bound {bound:.1e}")
        if not e < bound:
            misses.append((name, e_norm, e_samp, bound))
    print(f"case {case}: worst gradient {worst[1]}")
    return misses
