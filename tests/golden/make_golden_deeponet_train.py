"""DeepONet training vectors from the reference (build container only; needs /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_deeponet_train.py [--search]
Writes tests/golden/deeponet_train_small.npz -- data only.  Per case of deeponet_train_common.CASES, from the reference in ``train()``
mode with the seeded weights, run in fp64 (``get_grid`` wrapped to hand back doubles, as make_golden_deeponet.py does): 2048 seeded
samples of the output, the mean loss, every running statistic after the forward, and per parameter its gradient's norm and 128
seeded-index samples; next to each the reference's own fp32-versus-fp64 deviation (``*_selferr``, Rel-L2 over the whole tensor).
``bias_noise`` is the largest |g| the fp32 reference returns on the four convolution biases in front of a BatchNorm (their gradient is
zero: rounding noise).  Case d runs with dropout 0.1: the reference instance's ``nn.Dropout`` modules are swapped for a multiply by
the seeded masks of deeponet_train_common.dropout_masks.  The Adam case also stores the losses of two Adam steps (lr 1e-3, cosine,
T_max 10, a fresh batch per step).

The fp32 side runs with oneDNN off (with it on the fp32 convolution backward deviates from fp64 by far more than rounding).  A seed
is accepted only if (1) in the fp64 run every ReLU input and every gap between the two largest values of a max-pool window whose
maximum is positive lies at least GATE_MARGIN away from zero, where GATE_MARGIN of a tensor is three times the RMS of the
reference's fp32-minus-fp64 difference of that ReLU input, both measured in standard deviations of the tensor, and (2) the fp32 run
agrees with the fp64 run to 1e-5 on every real gradient.  Both are asserted for the seeds of deeponet_train_common.SEEDS;
``--search`` walks upwards from SEED_START instead, prints the first seed that passes and how many were tried, and the result is
entered into SEEDS by hand."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
import deeponet_train_common as TC                                        # noqa: E402
from realpdebench.model.deeponet import DeepONet                          # noqa: E402

MAX_TRIES = 2000
torch.set_num_threads(4)          # the fp32 run's rounding (and with it GATE_MARGIN) depends on how the sums are split over threads


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


class MaskMul(torch.nn.Module):
    """What replaces an ``nn.Dropout``: a multiply by a stored, pre-scaled mask ([rows][width], broadcast to the input's shape)."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.to(x.dtype).reshape(x.shape)


def build(name, dt):
    shape_in, shape_out, p, _, rate = TC.CASES[name]
    m = DeepONet(shape_in, shape_out, shape_in[-1], shape_out[-1], p, dropout_rate=rate, device="cpu")
    m.load_state_dict(TC.weights(name))
    masks = TC.dropout_masks(name)
    if masks is not None:
        m.branch.fc[2], m.output_net[2], m.output_net[5] = MaskMul(masks[0]), MaskMul(masks[1]), MaskMul(masks[2])
    m = m.to(dt).train()
    if dt == torch.float64:
        grid = m.get_grid
        m.get_grid = lambda shape, device: grid(shape, device).double()
    return m


def run(name, dt, seed, steps=1, backward=True):
    """One forward / backward (steps = 1), or ``steps`` Adam steps; returns what the first step saw and every step's loss."""
    m = build(name, dt)
    opt = torch.optim.Adam(m.parameters(), lr=TC.ADAM_LR)
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=TC.ADAM_T_MAX)
    first, losses, seen, relu_in, gaps = None, [], {}, [], []

    def relu_hook(_m, inp, _o):
        if not losses:
            relu_in.append(inp[0].detach())

    def pool_hook(_m, inp, _o):                    # the gap between the two largest values of every window with a positive maximum
        if not losses:
            v = inp[0].detach()
            B, C, T, H, W = v.shape
            w = v[:, :, :T // 2 * 2, :H // 2 * 2, :W // 2 * 2].reshape(B, C, T // 2, 2, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 6, 3, 5, 7)
            top = w.reshape(B, C, T // 2, H // 2, W // 2, 8).topk(2, dim=-1).values
            gap = (top[..., 0] - top[..., 1])[top[..., 0] > 0]
            gaps.append((len(relu_in) - 1, float(gap.min()) if gap.numel() else float("inf")))

    for mod in m.modules():
        if isinstance(mod, torch.nn.ReLU):
            mod.register_forward_hook(relu_hook)
        if isinstance(mod, torch.nn.MaxPool3d):
            mod.register_forward_hook(pool_hook)
    forward = m.forward
    m.forward = lambda x_: seen.__setitem__("out", forward(x_)) or seen["out"]      # train_loss calls self.forward: one forward per step
    for k in range(steps):
        x, y = (t.to(dt) for t in TC.case_inputs(name, k, seed))
        opt.zero_grad()
        loss = m.train_loss(x, y).mean()
        if backward:
            loss.backward()
        losses.append(float(loss.detach().double()))
        if k == 0:
            first = dict(out=seen["out"].detach(), sd={k_: v.detach().clone() for k_, v in m.state_dict().items()},
                         grads={n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()},
                         relu_in=relu_in, gaps=gaps)
        if steps > 1:
            opt.step()
            sched.step()
    return first, losses


def margins(f32, f64):
    """Per ReLU input: (GATE_MARGIN = 3 x RMS(fp32 - fp64) / std, smallest |input| / std, smallest max-pool gap / std), fp64 statistics."""
    out = []
    gaps = dict(f64["gaps"])
    for i, (a, b) in enumerate(zip(f32["relu_in"], f64["relu_in"])):
        std = float(b.std())
        dev = float((a.double() - b).pow(2).mean().sqrt()) / std
        out.append((3 * dev, float(b.abs().min()) / std, gaps.get(i, float("inf")) / std))
    return out


def accept(name, seed, verbose):
    """(ok, (f32, f64, l32, l64) or None) of one input seed; the forward-only margin check runs first (it rejects most seeds, and
    then no backward is run: None)."""
    with torch.backends.mkldnn.flags(enabled=False):
        p32, _ = run(name, torch.float32, seed, backward=False)
    p64, _ = run(name, torch.float64, seed, backward=False)
    mg = margins(p32, p64)
    ok = all(lo >= m and gap >= m for m, lo, gap in mg)
    if verbose or ok:
        print(f"case {name} seed {seed}: per ReLU input (GATE_MARGIN, smallest |input|, smallest pool gap) in standard deviations: "
              + ", ".join(f"({m:.1e}, {lo:.1e}, {gap:.1e})" for m, lo, gap in mg))
    if not ok:
        return False, None
    with torch.backends.mkldnn.flags(enabled=False):
        f32, l32 = run(name, torch.float32, seed)
    f64, l64 = run(name, torch.float64, seed)
    real, _ = TC.param_names(name)
    worst = max(rel(f32["grads"][n], f64["grads"][n]) for n in real)
    print(f"case {name} seed {seed}: worst gradient selferr {worst:.2e}")
    return worst <= 1e-5, (f32, f64, l32, l64)


def main():
    z = {}
    search = "--search" in sys.argv
    only = [a for a in sys.argv[1:] if a in TC.CASES] or list(TC.CASES)
    for name in only:
        real, zero_bias = TC.param_names(name)
        seed, tried = (TC.SEED_START[name] if search else TC.SEEDS[name]), 0
        while True:
            tried += 1
            ok, res = accept(name, seed, verbose=not search)
            if ok or not search:
                break
            assert tried < MAX_TRIES, f"case {name}: no seed in {MAX_TRIES} tries"
            seed += 1
        assert ok, f"case {name}: seed {seed} fails the gate margin or the 1e-5 gradient agreement (deeponet_train_common.SEEDS)"
        print(f"case {name}: seed {seed} accepted after {tried} tried (from {TC.SEED_START[name]}: {seed - TC.SEED_START[name] + 1})")
        f32, f64, l32, l64 = res
        z[f"{name}_seed"], z[f"{name}_seeds_tried"] = seed, seed - TC.SEED_START[name] + 1
        assert tuple(f64["out"].shape[1:]) == TC.CASES[name][1]
        z[f"{name}_out"], z[f"{name}_out_selferr"] = TC.out_samples(f64["out"]).numpy(), rel(f32["out"], f64["out"])
        z[f"{name}_loss"], z[f"{name}_loss_selferr"] = l64[0], abs(l32[0] - l64[0]) / abs(l64[0])
        stats = TC.stat_names(name)
        z[f"{name}_stats"] = torch.cat([f64["sd"][k] for k in stats]).numpy()
        z[f"{name}_stats_selferr"] = np.array([rel(f32["sd"][k], f64["sd"][k]) for k in stats])
        for k in stats:                                                   # the statistics moved away from the seeded values
            assert float((f64["sd"][k] - TC.weights(name)[k].double()).abs().max()) > 1e-3, k
        assert all(int(v) == TC.TRACKED_BEFORE + 1 for k, v in f64["sd"].items() if k.endswith("num_batches_tracked"))
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
        assert worst <= 1e-5 and noise64 < 1e-12
        if name == TC.ADAM_CASE:
            with torch.backends.mkldnn.flags(enabled=False):
                _, a32 = run(name, torch.float32, seed, TC.ADAM_STEPS)
            _, a64 = run(name, torch.float64, seed, TC.ADAM_STEPS)
            z[f"{name}_adam_loss"] = np.array(a64)
            z[f"{name}_adam_loss_selferr"] = np.array([abs(a - b) / abs(b) for a, b in zip(a32, a64)])
            assert abs(a64[0] - l64[0]) <= 1e-12 * abs(l64[0])
            print(f"  adam losses {a64} selferr {z[name + '_adam_loss_selferr']}")
    if only != list(TC.CASES):
        return
    path = os.path.join(HERE, "deeponet_train_small.npz")
    np.savez_compressed(path, **z)
    print("wrote deeponet_train_small.npz (%.1f kB)" % (os.path.getsize(path) / 1e3))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
