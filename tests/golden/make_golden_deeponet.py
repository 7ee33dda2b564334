"""DeepONet vectors from the reference (build container only; needs /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_deeponet.py [--write-yamls]
Writes tests/golden/deeponet_small.npz and tests/golden/deeponet_configs.json -- data only.  Per case of deeponet_common.CASES: the
eval output, the mean of the elementwise loss, the branch vector b, a 3-step rollout with a Gaussian normaliser (eval.py:311-319)
where T_out == T_in, and for each of them the reference's own fp32-versus-fp64 Rel-L2 (``*_selferr``, over the whole tensor before
the fixed sub-sampling).  Case (a) also stores the four pooled stage outputs (channels-last, thinned by deeponet_common.pool_stored).  The seeded weights are checked here,
on the CPU, so that the fixture cannot hide a failure: BatchNorm statistics away from their init values, every ReLU with 20-80 % of
its inputs positive, every stage output with a standard deviation in [0.1, 10].
``--write-yamls`` re-emits realpdebench_amd/configs/<scenario>/deeponet.yaml from the reference's values (synthetic dataset defaults on top)."""
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import deeponet_common as DC                                              # noqa: E402
from make_golden_configs import NATIVE, REF, SCENARIOS, SYNTH             # noqa: E402
from realpdebench.model.deeponet import DeepONet                          # noqa: E402

MODEL_KEYS = ("p", "dropout_rate")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def build(name, double=False):
    shape_in, shape_out, p, _ = DC.CASES[name]
    m = DeepONet(shape_in, shape_out, shape_in[-1], shape_out[-1], p, device="cpu").eval()
    m.load_state_dict(DC.seeded_weights(shape_in, shape_out, p))
    if double:                       # get_grid builds float32 coordinates by name: the fp64 run reads the same values as doubles
        m = m.double()
        grid = m.get_grid
        m.get_grid = lambda shape, device: grid(shape, device).double()
    return m


def rollout(m, x, name, dt):
    """eval.py:305-321 with the Gaussian statistics of deeponet_common (raw data = ``x``)."""
    mi, mt, si, st = (t.to(dt) for t in DC.normalizer_stats(name))
    co = DC.CASES[name][1][-1]
    para = x[..., co:] if x.shape[-1] != co else None
    preds = [(x - mi) / si]
    for _ in range(DC.ROLLOUT_STEPS):
        p = m(preds[-1]) * st + mt
        if para is not None:
            p = torch.cat([p, para], -1)
        preds.append((p - mi) / si)
    return torch.cat(preds[1:], 1)


def check_weights(name, m, x):
    """The conditions the seeded weights must meet (fp32 model, CPU)."""
    sd = m.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            assert float(v.abs().max()) <= 0.5 and float(v.abs().max()) > 0, k
        if k.endswith("running_var"):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 2 and float((v - 1).abs().max()) > 0, k
    seen = []

    def relu_hook(tag):
        def hook(_m, inp, _o):
            frac = float((inp[0] > 0).double().mean())
            seen.append((tag, frac))
            assert 0.2 <= frac <= 0.8, (name, tag, frac)
        return hook

    def std_hook(tag):
        def hook(_m, _i, out):
            s = float(out.std())
            seen.append((tag + " std", s))
            assert 0.1 <= s <= 10, (name, tag, s)
        return hook

    hooks = []
    for tag, seq in [(f"branch.conv{i}", getattr(m.branch, f"conv{i}")) for i in (1, 2, 3, 4)] + [("branch.fc", m.branch.fc), ("trunk.fc", m.trunk.fc),
                                                                                                   ("output_net", m.output_net)]:
        for j, mod in enumerate(seq):
            if isinstance(mod, torch.nn.ReLU):
                hooks.append(mod.register_forward_hook(relu_hook(f"{tag}.{j}")))
        hooks.append(seq.register_forward_hook(std_hook(tag)))
    with torch.no_grad():
        m(x)
    for h in hooks:
        h.remove()
    print(f"  case {name}: " + ", ".join(f"{t} {v:.2f}" for t, v in seen))


def run(name, double, keep=None):
    m = build(name, double)
    dt = torch.float64 if double else torch.float32
    x, y = (t.to(dt) for t in DC.case_inputs(name))
    if not double:
        check_weights(name, m, x)
    hooks = []
    if keep is not None:
        for i in (1, 2, 3, 4):
            hooks.append(getattr(m.branch, f"conv{i}").register_forward_hook(lambda _m, _i, o: keep.append(o.permute(0, 2, 3, 4, 1).contiguous())))
    with torch.no_grad():
        out = m(x)
        for h in hooks:
            h.remove()
        b = m.branch(x)
        loss = float(m.train_loss(x, y).double().mean())
        roll = rollout(m, x, name, dt) if name in DC.ROLLOUT_CASES else None
    return out, loss, roll, b, m


def main():
    z, keys = {}, {}
    for name in DC.CASES:
        keep, keep64 = ([], []) if name == "a" else (None, None)
        out, loss, roll, b, m = run(name, False, keep)
        out64, loss64, roll64, b64, _ = run(name, True, keep64)
        keys[name] = [[k_, list(v.shape), str(v.dtype)] for k_, v in m.state_dict().items()]
        z[f"{name}_out"], z[f"{name}_out_selferr"] = DC.stored(name, out).numpy(), rel(out, out64)
        z[f"{name}_loss"], z[f"{name}_loss_selferr"] = loss, abs(loss - loss64) / abs(loss64)
        z[f"{name}_b"], z[f"{name}_b_selferr"] = b.numpy(), rel(b, b64)
        msg = "out std %.3f selferr out %.2e b %.2e loss %.2e" % (float(out.std()), z[f"{name}_out_selferr"], z[f"{name}_b_selferr"], z[f"{name}_loss_selferr"])
        if roll is not None:
            z[f"{name}_roll"], z[f"{name}_roll_selferr"] = DC.roll_stored(name, roll).numpy(), rel(roll, roll64)
            msg += " roll %.2e (std %.3f)" % (z[f"{name}_roll_selferr"], float(roll.std()))
        print(name, msg)
        if keep is not None:
            for i, (t, t64) in enumerate(zip(keep, keep64)):
                z[f"a_pool{i + 1}"], z[f"a_pool{i + 1}_selferr"] = DC.pool_stored(t).numpy(), rel(t, t64)
    np.savez_compressed(os.path.join(HERE, "deeponet_small.npz"), **z)
    cfg = {}
    for scen in SCENARIOS:
        with open(os.path.join(REF, scen, "deeponet.yaml")) as fh:
            cfg[scen] = yaml.safe_load(fh)
    doc = {"state_dict": keys, "model_keys": {s: {k_: cfg[s][k_] for k_ in MODEL_KEYS + ("model_name", "N_autoregressive")} for s in SCENARIOS},
           "native_shapes": {s: {"shape_in": list(NATIVE[s][0]), "shape_out": list(NATIVE[s][1])} for s in SCENARIOS}}
    with open(os.path.join(HERE, "deeponet_configs.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote deeponet_small.npz (%.1f kB) and deeponet_configs.json" % (os.path.getsize(os.path.join(HERE, "deeponet_small.npz")) / 1e3))
    if "--write-yamls" in sys.argv:
        for scen in SCENARIOS:
            body = dict(cfg[scen])
            for k_ in SYNTH:
                if k_ in body:
                    body["ref_" + k_] = body[k_]
            body.update(dataset_name="synthetic", dataset_root="", num_workers=0, normalizer="none", checkpoint_path="",
                        shape_in=list(NATIVE[scen][0]), shape_out=list(NATIVE[scen][1]), n_train=16, n_val=4)
            path = os.path.join(ROOT, "realpdebench_amd", "configs", scen, "deeponet.yaml")
            with open(path, "w") as fh:
                fh.write(f"# Key surface and values of the reference's realpdebench/configs/{scen}/deeponet.yaml (written by "
                         "tests/golden/make_golden_deeponet.py --write-yamls).\n# DeepONet on MI355X is evaluation and rollout only: "
                         "realpdebench_amd.train refuses this model at trainer construction.\n# Deviations, on purpose: dataset_name / "
                         "dataset_root default to the synthetic generator (no dataset ships here), normalizer to \"none\"\n# and "
                         "checkpoint_path to \"\"; the reference's values are kept in the ref_* keys below.\n")
                yaml.safe_dump(body, fh, sort_keys=False, default_flow_style=None)


if __name__ == "__main__":
    main()
