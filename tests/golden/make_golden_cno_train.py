"""CNO3d training vectors from the reference (build container only; needs /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cno_train.py
Writes tests/golden/cno_train_small.npz -- data only.  Per case of cno_train_common.CASES, from the reference in ``train()`` mode with
the seeded weights, run in fp64: the output, the mean loss, every running statistic after the forward, and per parameter with a
gradient its norm and 128 seeded-index samples; next to each the reference's own fp32-versus-fp64 deviation (``*_selferr``, Rel-L2 over
the whole tensor).  ``bias_noise`` is the largest |g| the fp32 reference returns on the 31 convolution biases in front of a BatchNorm
(their gradient is zero: rounding noise).  Case g also stores the losses of two Adam steps (lr 1e-3, cosine, T_max 10, a fresh batch
per step).

The fp32 side runs with oneDNN off: with it on, the fp32 convolution backward deviates from fp64 by up to 1e-2 on some seeds, and every
tolerance derived from that would be toothless.  The worst gradient selferr is asserted <= 1e-5, so a polluted fixture is not written,
and so is the distance of every LeakyReLU input from zero (cno_train_common.GATE_MARGIN: why, and how the input seeds were taken)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
import cno_common as CC                                                   # noqa: E402
import cno_train_common as TC                                             # noqa: E402
from realpdebench.model import cno as ref_cno                             # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def build(name, dt):
    shape_in, shape_out, _ = TC.CASES[name]
    m = ref_cno.CNO3d(in_dim=shape_in[-1], out_dim=shape_out[-1], out_dim_mult=CC.out_dim_mult(shape_in, shape_out), in_size=shape_in[2],
                      N_layers=CC.N_LAYERS)
    m.load_state_dict(TC.weights(name))
    return m.to(dt).train()


def run(name, dt, steps=1):
    """One backward (steps = 1), or ``steps`` Adam steps; returns what the first step saw and every step's loss."""
    m = build(name, dt)
    opt = torch.optim.Adam(m.parameters(), lr=TC.ADAM_LR)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=TC.ADAM_T_MAX)
    first, losses, seen, margin = None, [], {}, [float("inf")]

    def gate_hook(_m, inp, _o):                   # the smallest |LeakyReLU input| of the first step, in standard deviations of its layer
        if not losses:
            margin[0] = min(margin[0], float(inp[0].detach().abs().min() / inp[0].detach().std()))

    for tag, mod in m.named_modules():
        if isinstance(mod, torch.nn.LeakyReLU) and not tag.startswith("decoder_inv.3"):
            mod.register_forward_hook(gate_hook)
    forward = m.forward
    m.forward = lambda x_: seen.__setitem__("out", forward(x_)) or seen["out"]      # train_loss calls self.forward: one forward per step
    for k in range(steps):
        x, y = (t.to(dt) for t in TC.case_inputs(name, k))
        opt.zero_grad()
        loss = m.train_loss(x, y).mean()
        loss.backward()
        losses.append(float(loss.detach().double()))
        if k == 0:
            first = dict(out=seen["out"].detach(), sd={k_: v.detach().clone() for k_, v in m.state_dict().items()},
                         grads={n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()},
                         margin=margin[0])
        if steps > 1:
            opt.step()
            sched.step()
    return first, losses


def main():
    z = {}
    for name in TC.CASES:
        real, zero_bias, none = TC.param_names(name)
        with torch.backends.mkldnn.flags(enabled=False):
            f32, l32 = run(name, torch.float32)
        f64, l64 = run(name, torch.float64)
        assert tuple(f64["out"].shape[1:]) == TC.CASES[name][1]
        assert all(f64["grads"][n] is None for n in none) and all(f64["grads"][n] is not None for n in real + zero_bias)
        z[f"{name}_out"], z[f"{name}_out_selferr"] = f64["out"].numpy(), rel(f32["out"], f64["out"])
        z[f"{name}_loss"], z[f"{name}_loss_selferr"] = l64[0], abs(l32[0] - l64[0]) / abs(l64[0])
        stats = TC.stat_names(name)
        z[f"{name}_stats"] = torch.cat([f64["sd"][k] for k in stats]).numpy()
        z[f"{name}_stats_selferr"] = np.array([rel(f32["sd"][k], f64["sd"][k]) for k in stats])
        for k in stats:                                                   # the statistics moved away from the seeded values
            assert float((f64["sd"][k] - TC.weights(name)[k].double()).abs().max()) > 1e-3, k
        assert all(int(v) == TC.TRACKED_BEFORE + 1 for k, v in f64["sd"].items()
                   if k.endswith("num_batches_tracked") and not k.startswith("decoder_inv.3."))
        gs = [f64["grads"][n] for n in real]
        z[f"{name}_gnorm"] = np.array([float(g.norm()) for g in gs])
        z[f"{name}_gsamp"] = torch.stack([g.reshape(-1)[TC.sample_index(i, g.numel())] for i, g in enumerate(gs)]).numpy()
        z[f"{name}_g_selferr"] = np.array([rel(f32["grads"][n], f64["grads"][n]) for n in real])
        z[f"{name}_bias_noise"] = max(float(f32["grads"][n].abs().max()) for n in zero_bias)
        noise64 = max(float(f64["grads"][n].abs().max()) for n in zero_bias)
        worst = float(z[f"{name}_g_selferr"].max())
        print(f"case {name}: out selferr {z[name + '_out_selferr']:.2e} loss {z[name + '_loss_selferr']:.2e} stats "
              f"{z[name + '_stats_selferr'].max():.2e} worst grad {worst:.2e} ({real[int(z[name + '_g_selferr'].argmax())]}) smallest grad norm "
              f"{z[name + '_gnorm'].min():.2e} bias noise fp32 {z[name + '_bias_noise']:.1e} fp64 {noise64:.1e}")
        print(f"  smallest LeakyReLU input of the fp64 run: {f64['margin']:.2e} standard deviations (required {TC.GATE_MARGIN:.0e})")
        assert f64["margin"] >= TC.GATE_MARGIN, "a LeakyReLU input within fp32 reach of zero: take another input seed (cno_train_common.SEEDS)"
        assert worst <= 1e-5, "the fp32 reference deviates from fp64 by more than 1e-5: a polluted fixture (is oneDNN off?)"
        assert noise64 < 1e-12
        if name == TC.ADAM_CASE:
            with torch.backends.mkldnn.flags(enabled=False):
                _, a32 = run(name, torch.float32, TC.ADAM_STEPS)
            _, a64 = run(name, torch.float64, TC.ADAM_STEPS)
            z[f"{name}_adam_loss"] = np.array(a64)
            z[f"{name}_adam_loss_selferr"] = np.array([abs(a - b) / abs(b) for a, b in zip(a32, a64)])
            assert abs(a64[0] - l64[0]) <= 1e-12 * abs(l64[0])
            print(f"  adam losses {a64} selferr {z[name + '_adam_loss_selferr']}")
    path = os.path.join(HERE, "cno_train_small.npz")
    np.savez_compressed(path, **z)
    print("wrote cno_train_small.npz (%.1f kB)" % (os.path.getsize(path) / 1e3))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
