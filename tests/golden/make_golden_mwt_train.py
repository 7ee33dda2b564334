"""MWT3d training vectors from the reference (build container only; needs /root/reference, sympy and scipy):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mwt_train.py [--search N]
Writes tests/golden/mwt_train_small.npz -- data only.  Per case of mwt_train_common.CASES, from the reference in ``train()`` mode with
the seeded weights, run in fp64 (complex128 parameters and spectrum buffers: make_golden_mwt.as_double): the mean loss, per parameter
with a gradient its norm and 128 seeded-index samples (complex gradients as (re, im) pairs), next to each the reference's own
fp32-versus-fp64 deviation (``*_selferr``, Rel-L2 over the whole tensor), and the names of the parameters without a gradient.  Case p
also stores the losses of two Adam steps (lr 1e-3, cosine, T_max 10, a fresh batch per step).

The fp32 side runs with oneDNN off (as make_golden_cno_train.py: with it on the fp32 convolution backward can deviate by 1e-2).  The
ReLU gates make the backward discontinuous, so the generator records every ReLU input of both runs and asserts what
mwt_train_common.GATE_MARGIN states; ``--search N`` tries N seeds per case from the stored one upwards and prints which pass."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
import mwt_common as MC                                                   # noqa: E402
import mwt_train_common as TC                                             # noqa: E402
from make_golden_mwt import as_double                                     # noqa: E402
from realpdebench.model.MWT_libs.models import MWT3d                      # noqa: E402


def rel(a, b):
    a, b = TC.flat_real(a).double(), TC.flat_real(b).double()
    return float((a - b).norm() / b.norm())


def build(name, double):
    shape_in, shape_out = TC.CASES[name]
    m = MWT3d(k=MC.K, alpha=MC.ALPHA, c=MC.C, nCZ=TC.NCZ, L=0, base="legendre", shape_in=shape_in, shape_out=shape_out)
    missing = m.load_state_dict(TC.weights(name), strict=False)
    assert all(k.rsplit(".", 1)[-1] in MC._BUFFERS for k in missing.missing_keys) and not missing.unexpected_keys
    if double:
        m = m.double()
        for p in m.parameters():
            if p.is_complex():
                p.data = p.data.to(torch.complex128)
    return m.train()


class record_relu:
    """Every ReLU input of the reference, in call order (nn.ReLU goes through F.relu as well)."""

    def __init__(self, sink):
        self.sink = sink

    def __enter__(self):
        self.relu = torch.nn.functional.relu
        torch.nn.functional.relu = lambda t, inplace=False: (self.sink.append(t.detach().clone()), self.relu(t, inplace=inplace))[1]

    def __exit__(self, *exc):
        torch.nn.functional.relu = self.relu


def run(name, double, steps=1, seed=None):
    """One backward (steps = 1), or ``steps`` Adam steps; returns what the first step saw and every step's loss."""
    dt = torch.float64 if double else torch.float32
    m = build(name, double)
    opt = torch.optim.Adam(m.parameters(), lr=TC.ADAM_LR)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=TC.ADAM_T_MAX)
    first, losses = None, []
    for k in range(steps):
        x, y = (t.to(dt) for t in TC.case_inputs(name, k, seed))
        opt.zero_grad()
        gates = []
        with record_relu(gates):
            loss = m.train_loss(x, y).mean()
        loss.backward()
        losses.append(float(loss.detach().double()))
        if k == 0:
            first = dict(gates=gates, grads={n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()})
        if steps > 1:
            opt.step()
            sched.step()
    return first, losses


def both(name, steps=1, seed=None):
    with torch.backends.mkldnn.flags(enabled=False):
        f32, l32 = run(name, False, steps, seed)
    with as_double():
        f64, l64 = run(name, True, steps, seed)
    return f32, l32, f64, l64


def gate_figures(f32, f64):
    """(largest fp32-vs-fp64 RMS deviation of a ReLU input, smallest |ReLU input| of the fp64 run), both in standard deviations of
    the tensor they belong to."""
    assert len(f32["gates"]) == len(f64["gates"]) > 0
    err = max(float((a.double() - b).pow(2).mean().sqrt() / b.std()) for a, b in zip(f32["gates"], f64["gates"]))
    margin = min(float(b.abs().min() / b.std()) for b in f64["gates"])
    return err, margin, sum(b.numel() for b in f64["gates"])


def search(n):
    for name in TC.CASES:
        real, _ = TC.param_names(name)
        for seed in range(TC.SEEDS[name], TC.SEEDS[name] + n):
            f32, _, f64, _ = both(name, seed=seed)
            err, margin, count = gate_figures(f32, f64)
            worst = max(rel(f32["grads"][k], f64["grads"][k]) for k in real)
            ok = err <= TC.GATE_ERR and margin >= TC.GATE_MARGIN and worst <= 1e-5
            print(f"case {name} seed {seed}: {count} gate inputs, fp32 error {err:.2e}, margin {margin:.2e}, worst grad selferr {worst:.2e}"
                  f"{'  <-- passes' if ok else ''}", flush=True)
            if ok:
                break


def main():
    z = {}
    for name in TC.CASES:
        real, none = TC.param_names(name)
        f32, l32, f64, l64 = both(name)
        assert all(f64["grads"][n] is None for n in none) and all(f64["grads"][n] is not None for n in real)
        assert set(f64["grads"]) == set(real) | set(none)
        z[f"{name}_loss"], z[f"{name}_loss_selferr"] = l64[0], abs(l32[0] - l64[0]) / abs(l64[0])
        gs = [TC.flat_real(f64["grads"][n]) for n in real]
        z[f"{name}_real"], z[f"{name}_none"] = np.array(real), np.array(none)
        z[f"{name}_gnorm"] = np.array([float(g.norm()) for g in gs])
        z[f"{name}_gsamp"] = torch.stack([g[TC.sample_index(i, g.numel())] for i, g in enumerate(gs)]).numpy()
        z[f"{name}_g_selferr"] = np.array([rel(f32["grads"][n], f64["grads"][n]) for n in real])
        # a spectral weight whose every reached entry loses the corner overlap (Nx <= 2 at every level: case r, weights1 and weights3)
        # has an exactly zero gradient in both runs: norm 0, selferr 0 by definition
        dead = z[f"{name}_gnorm"] == 0
        assert all(float(f32["grads"][n].abs().max()) == 0 for n, dd in zip(real, dead) if dd)
        z[f"{name}_g_selferr"] = np.where(dead, 0.0, z[f"{name}_g_selferr"])
        assert all(float(np.abs(row).max()) > 0 for row, dd in zip(z[f"{name}_gsamp"], dead) if not dd)
        err, margin, count = gate_figures(f32, f64)
        worst = float(z[f"{name}_g_selferr"].max())
        print(f"case {name}: loss {l64[0]:.6f} selferr {z[name + '_loss_selferr']:.2e}; worst grad selferr {worst:.2e} "
              f"({real[int(z[name + '_g_selferr'].argmax())]}); smallest grad norm {z[name + '_gnorm'].min():.2e}")
        print(f"  {count} ReLU inputs: fp32 error {err:.2e} (GATE_ERR {TC.GATE_ERR:.0e}), smallest |input| of the fp64 run {margin:.2e} "
              f"standard deviations (required {TC.GATE_MARGIN:.1e})")
        assert err <= TC.GATE_ERR, "the fp32 error at a ReLU input exceeds mwt_train_common.GATE_ERR"
        assert margin >= TC.GATE_MARGIN, "a ReLU input within fp32 reach of zero: take another input seed (mwt_train_common.SEEDS)"
        assert worst <= 1e-5, "the fp32 reference deviates from fp64 by more than 1e-5: a polluted fixture (is oneDNN off?)"
        if name == TC.ADAM_CASE:
            _, a32, _, a64 = both(name, TC.ADAM_STEPS)
            z[f"{name}_adam_loss"] = np.array(a64)
            z[f"{name}_adam_loss_selferr"] = np.array([abs(a - b) / abs(b) for a, b in zip(a32, a64)])
            assert abs(a64[0] - l64[0]) <= 1e-12 * abs(l64[0])
            print(f"  adam losses {a64} selferr {z[name + '_adam_loss_selferr']}")
    path = os.path.join(HERE, "mwt_train_small.npz")
    np.savez_compressed(path, **z)
    print("wrote mwt_train_small.npz (%.1f kB)" % (os.path.getsize(path) / 1e3))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    if "--search" in sys.argv:
        search(int(sys.argv[sys.argv.index("--search") + 1]))
    else:
        main()
