"""Shared by tests/golden/make_golden_dmd.py (reference side) and tests/test_dmd_host.py / tests/test_gpu_dmd.py: the cases and the
inputs of the DMD fixture.  The inputs are stored in dmd_small.npz as well (``case_inputs`` goes through sin / cos); the generator
asserts that what it stores is what this module builds."""
from collections import OrderedDict

import numpy as np

# name -> (B, T, H, W, C, f, n_modes, n_predict)
CASES = OrderedDict([
    ("a", (3, 20, 8, 16, 3, 2, 10, 20)),        # the config family in miniature
    ("b", (2, 10, 6, 10, 5, 2, 10, 10)),        # the controlled-cylinder family; n_modes >= rank, so no selection
    ("c", (1, 5, 3, 7, 2, 2, 3, 7)),            # f = C, odd everything, S != T
    ("d", (2, 20, 4, 4, 16, 2, None, 20)),      # n = 32, barely above T - 1, wide cells
])
NOISE = {"a": 0.3, "b": 0.05, "c": 1.0, "d": 0.5}      # Gaussian noise relative to the waves' rms
ROLLOUT_CASE, ROLLOUT_STEPS = "b", 2                   # T_out == T_in, control channels, C_out = 3
ROLLOUT_C_OUT = 3
NWAVES = 4

# what the generator asserts of the reference alone on every sample, so that no test can hide behind the fixture
COND_MAX = 1e3                 # cond(X1): far from the 2^-20 rank floor
LSTSQ_MARGIN = 4.0             # every singular value of Phi over the lstsq cutoff eps32 max(n, r), at least
SELF_ERR_MAX = 2.5e-6          # Rel-L2 between the reference on float32 and on float64 input


def case_inputs(name):
    """``x`` float32 [B,T,H,W,C]: NWAVES travelling waves per channel (random wave vectors, speeds and phases) + Gaussian noise."""
    B, T, H, W, C, f, _, _ = CASES[name]
    rng = np.random.default_rng(4100 + ord(name))
    t = np.arange(T)[:, None, None]
    h = np.arange(H)[None, :, None] / H
    w = np.arange(W)[None, None, :] / W
    x = np.zeros((B, T, H, W, C))
    for b in range(B):
        for c in range(C):
            for _ in range(NWAVES):
                kh, kw = rng.integers(0, 3), rng.integers(1, 4)
                om, ph, amp = rng.uniform(0.2, 1.2), rng.uniform(0, 2 * np.pi), rng.uniform(0.5, 1.5)
                x[b, :, :, :, c] += amp * np.sin(2 * np.pi * (kh * h + kw * w) - om * t + ph)
    x += NOISE[name] * np.sqrt(np.mean(x ** 2)) * rng.standard_normal(x.shape)
    return x.astype(np.float32)


def normalizer_stats(C_in, C_out):
    """A non-trivial Gaussian normaliser: (mean_inputs, mean_targets, std_inputs, std_targets), float32."""
    ci, co = np.arange(C_in, dtype=np.float32), np.arange(C_out, dtype=np.float32)
    return 0.2 - 0.1 * ci, -0.1 + 0.15 * co, 1.5 + 0.25 * ci, 0.8 + 0.2 * co
