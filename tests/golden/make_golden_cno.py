"""CNO3d vectors from the reference (build container only; needs /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cno.py [--write-yamls]
Writes tests/golden/cno_small.npz and tests/golden/cno_configs.json -- data only.  Per case of cno_common.CASES: the eval output, the
mean of the elementwise loss, a 3-step rollout with a Gaussian normaliser (eval.py:311-319) where T_out == T_in, and for each of them
the reference's own fp32-versus-fp64 Rel-L2 (``*_selferr``, over the whole tensor before the fixed sub-sampling).  Case (a) also stores,
thinned by cno_common.inter_stored: the lift output, skip[0..2] and the neck output (channels-last).  The seeded weights are checked
here, on the CPU, so that the fixture cannot hide a failure: BatchNorm statistics away from their init values, every LeakyReLU with
20-80 % of its inputs negative, every block output with a standard deviation in [0.1, 10].
``--write-yamls`` re-emits realpdebench_amd/configs/<scenario>/cno.yaml from the reference's values (synthetic dataset defaults on top)."""
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
import cno_common as CC                                                   # noqa: E402
from make_golden_configs import NATIVE, REF, SCENARIOS, SYNTH             # noqa: E402
from realpdebench.model import cno as ref_cno                             # noqa: E402

MODEL_KEYS = ("N_layers",)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def build(name, double=False):
    shape_in, shape_out, _ = CC.CASES[name]
    m = ref_cno.CNO3d(in_dim=shape_in[-1], out_dim=shape_out[-1], out_dim_mult=CC.out_dim_mult(shape_in, shape_out), in_size=shape_in[2],
                      N_layers=CC.N_LAYERS).eval()
    m.load_state_dict(CC.seeded_weights(shape_in, shape_out))
    return m.double() if double else m


def rollout(m, x, name, dt):
    """eval.py:305-321 with the Gaussian statistics of cno_common (raw data = ``x``)."""
    mi, mt, si, st = (t.to(dt) for t in CC.normalizer_stats(name))
    co = CC.CASES[name][1][-1]
    para = x[..., co:] if x.shape[-1] != co else None
    preds = [(x - mi) / si]
    for _ in range(CC.ROLLOUT_STEPS):
        p = m(preds[-1]) * st + mt
        if para is not None:
            p = torch.cat([p, para], -1)
        preds.append((p - mi) / si)
    return torch.cat(preds[1:], 1)


def check_weights(name, m, x):
    """The conditions the seeded weights must meet (fp32 model, CPU)."""
    for k, v in m.state_dict().items():
        if k.endswith("running_mean"):
            assert 0 < float(v.abs().max()) <= 0.5, k
        if k.endswith("running_var"):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 2 and float((v - 1).abs().max()) > 0, k
    seen, hooks = [], []

    def lrelu_hook(tag):
        def hook(_m, inp, _o):
            frac = float((inp[0] < 0).double().mean())
            seen.append((tag, frac))
            assert 0.2 <= frac <= 0.8, (name, tag, frac)
        return hook

    def std_hook(tag):
        def hook(_m, _i, out):
            s = float(out.std())
            seen.append((tag + " std", s))
            assert 0.1 <= s <= 10, (name, tag, s)
        return hook

    for tag, mod in m.named_modules():
        if tag.startswith("decoder_inv.3"):
            continue                                                      # constructed, never run
        if isinstance(mod, torch.nn.LeakyReLU):
            hooks.append(mod.register_forward_hook(lrelu_hook(tag)))
        if isinstance(mod, (ref_cno.CNOBlock3d, ref_cno.ResidualBlock3d, ref_cno.LiftProjectBlock3d)):
            hooks.append(mod.register_forward_hook(std_hook(tag)))
    with torch.no_grad():
        m(x)
    for h in hooks:
        h.remove()
    n_act = sum(1 for t, _ in seen if not t.endswith(" std"))
    assert n_act == 2 + 9 + 4 + 9, n_act                                  # lift / project, encoder + decoder + decoder_inv, ED, res_nets
    print(f"  case {name}: " + ", ".join(f"{t} {v:.2f}" for t, v in seen))


def run(name, double, keep=None):
    m = build(name, double)
    dt = torch.float64 if double else torch.float32
    x, y = (t.to(dt) for t in CC.case_inputs(name))
    if not double:
        check_weights(name, m, x)
    hooks = []
    if keep is not None:
        cl = lambda key: (lambda _m, _i, o: keep.__setitem__(key, o.permute(0, 2, 3, 4, 1).contiguous()))
        hooks.append(m.lift.register_forward_hook(cl("lift")))
        for i in range(3):
            hooks.append(m.res_nets[i].register_forward_hook(cl(f"skip{i}")))
        hooks.append(m.res_nets[-6].register_forward_hook(cl("neck")))    # the last block of the neck: it runs in reverse index order
    with torch.no_grad():
        out = m(x)
        for h in hooks:
            h.remove()
        loss = float(m.train_loss(x, y).double().mean())
        roll = rollout(m, x, name, dt) if name in CC.ROLLOUT_CASES else None
    return out, loss, roll, m


def main():
    z, keys = {}, {}
    for name in CC.CASES:
        keep, keep64 = ({}, {}) if name == "a" else (None, None)
        out, loss, roll, m = run(name, False, keep)
        out64, loss64, roll64, _ = run(name, True, keep64)
        assert tuple(out.shape[1:]) == CC.CASES[name][1], (name, out.shape)
        keys[name] = [[k_, list(v.shape), str(v.dtype)] for k_, v in m.state_dict().items()]
        assert len(keys[name]) == 232
        z[f"{name}_out"], z[f"{name}_out_selferr"] = out.numpy(), rel(out, out64)
        z[f"{name}_loss"], z[f"{name}_loss_selferr"] = loss, abs(loss - loss64) / abs(loss64)
        msg = "out std %.3f selferr out %.2e loss %.2e" % (float(out.std()), z[f"{name}_out_selferr"], z[f"{name}_loss_selferr"])
        if roll is not None:
            z[f"{name}_roll"], z[f"{name}_roll_selferr"] = roll.numpy(), rel(roll, roll64)
            msg += " roll %.2e (std %.3f)" % (z[f"{name}_roll_selferr"], float(roll.std()))
        print(name, msg)
        if keep is not None:
            for k_ in CC.INTERMEDIATES:
                z[f"a_{k_}"], z[f"a_{k_}_selferr"] = CC.inter_stored(keep[k_]).numpy(), rel(keep[k_], keep64[k_])
                print("  a_%s selferr %.2e" % (k_, z[f"a_{k_}_selferr"]))
    np.savez_compressed(os.path.join(HERE, "cno_small.npz"), **z)
    cfg = {}
    for scen in SCENARIOS:
        with open(os.path.join(REF, scen, "cno.yaml")) as fh:
            cfg[scen] = yaml.safe_load(fh)
    doc = {"state_dict": keys, "model_keys": {s: {k_: cfg[s][k_] for k_ in MODEL_KEYS + ("model_name", "N_autoregressive")} for s in SCENARIOS},
           "native_shapes": {s: {"shape_in": list(NATIVE[s][0]), "shape_out": list(NATIVE[s][1])} for s in SCENARIOS}}
    with open(os.path.join(HERE, "cno_configs.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote cno_small.npz (%.1f kB) and cno_configs.json" % (os.path.getsize(os.path.join(HERE, "cno_small.npz")) / 1e3))
    if "--write-yamls" in sys.argv:
        for scen in SCENARIOS:
            body = dict(cfg[scen])
            for k_ in SYNTH:
                if k_ in body:
                    body["ref_" + k_] = body[k_]
            body.update(dataset_name="synthetic", dataset_root="", num_workers=0, normalizer="none", checkpoint_path="",
                        shape_in=list(NATIVE[scen][0]), shape_out=list(NATIVE[scen][1]), n_train=16, n_val=4)
            path = os.path.join(ROOT, "realpdebench_amd", "configs", scen, "cno.yaml")
            with open(path, "w") as fh:
                fh.write(f"# Key surface and values of the reference's realpdebench/configs/{scen}/cno.yaml (written by "
                         "tests/golden/make_golden_cno.py --write-yamls).\n# CNO3d on MI355X is evaluation and rollout only: "
                         "realpdebench_amd.train refuses this model at trainer construction.\n# load_model reads N_layers alone; the other "
                         "model keys (values with a trailing comma parse as strings) are ignored, as in the reference.\n# Deviations, on "
                         "purpose: dataset_name / dataset_root default to the synthetic generator (no dataset ships here), normalizer to "
                         "\"none\"\n# and checkpoint_path to \"\"; the reference's values are kept in the ref_* keys below.\n")
                yaml.safe_dump(body, fh, sort_keys=False, default_flow_style=None)


if __name__ == "__main__":
    main()
