"""MWT3d vectors from the reference (build container only; needs /root/reference, sympy and scipy):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mwt.py [--write-yamls]
Writes tests/golden/mwt_small.npz and tests/golden/mwt_configs.json -- data only.  Per case of mwt_common.CASES: the eval output, the
mean of the elementwise loss, a 3-step rollout with a Gaussian normaliser (eval.py:311-319), and for each of them the reference's own
fp32-versus-fp64 Rel-L2 (``*_selferr``).  Case (a) also stores (through mwt_common.inter_stored) the per-level outputs of wavelet_transform, A, B, C and evenOdd of CZ
block 0, each with its own fp32-versus-fp64 Rel-L2.  Filter matrices and the six derived buffers are stored for k = 2, 3, 4.  The fp64 run sets the default dtype to float64 and
maps the reference's ``torch.zeros(..., dtype=cfloat)`` spectrum buffer to complex128 for its duration -- otherwise the "double" run
would round its spectrum and the evenOdd scatter to single precision.
``--write-yamls`` re-emits realpdebench_amd/configs/<scenario>/mwt.yaml from the reference's values (synthetic dataset defaults on top)."""
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
import mwt_common as MC                                                   # noqa: E402
from make_golden_configs import NATIVE, REF, SCENARIOS, SYNTH             # noqa: E402
from realpdebench.data.data_normalizer import GaussianNormalizer          # noqa: E402,F401
from realpdebench.model.MWT_libs.models import MWT3d, MWT_CZ3d            # noqa: E402
from realpdebench.model.MWT_libs.utils_MWT import get_filter              # noqa: E402

MODEL_KEYS = ("k", "alpha", "c", "nCZ", "L", "base")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def build(name, double=False):
    shape_in, shape_out, nCZ, _ = MC.CASES[name]
    m = MWT3d(k=MC.K, alpha=MC.ALPHA, c=MC.C, nCZ=nCZ, L=0, base="legendre", shape_in=shape_in, shape_out=shape_out).eval()
    missing = m.load_state_dict(MC.seeded_weights(shape_in, shape_out, nCZ), strict=False)
    assert all(k.rsplit(".", 1)[-1] in MC._BUFFERS for k in missing.missing_keys) and not missing.unexpected_keys
    if double:
        m = m.double()
        for p in m.parameters():
            if p.is_complex():
                p.data = p.data.to(torch.complex128)
    return m


class as_double:
    """float64 default dtype + complex128 spectrum buffers while the reference runs in double."""

    def __enter__(self):
        self.zeros = torch.zeros
        torch.set_default_dtype(torch.float64)
        torch.zeros = lambda *a, **k: self.zeros(*a, **{**k, "dtype": torch.complex128 if k.get("dtype") == torch.cfloat else k.get("dtype")})

    def __exit__(self, *exc):
        torch.zeros = self.zeros
        torch.set_default_dtype(torch.float32)


def rollout(m, x, name, dt):
    """eval.py:305-321 with the Gaussian statistics of mwt_common (raw data = ``x``)."""
    mi, mt, si, st = (t.to(dt) for t in MC.normalizer_stats(name))
    co = MC.CASES[name][1][-1]
    para = x[..., co:] if x.shape[-1] != co else None
    preds = [(x - mi) / si]
    for _ in range(MC.ROLLOUT_STEPS):
        p = m(preds[-1]) * st + mt
        if para is not None:
            p = torch.cat([p, para], -1)
        preds.append((p - mi) / si)
    return torch.cat(preds[1:], 1)


def run(name, double, keep=None):
    m = build(name, double)
    dt = torch.float64 if double else torch.float32
    x, y = (t.to(dt) for t in MC.case_inputs(name))
    if keep is not None:
        cz = m.MWT_CZ[0]
        sq = lambda t: t.reshape(*t.shape[:4], -1)
        for mod, tag in ((cz.A, "A"), (cz.B, "B"), (cz.C, "C")):
            mod.register_forward_hook(lambda _m, _i, o, tag=tag: keep.setdefault(tag, []).append(sq(o)))
        wt, eo = cz.wavelet_transform, cz.evenOdd
        def wt_(t):
            d, s = wt(t)
            keep.setdefault("d", []).append(sq(d)); keep.setdefault("s", []).append(sq(s))
            return d, s
        def eo_(t):
            o = eo(t)
            keep.setdefault("eo", []).append(sq(o))
            return o
        cz.wavelet_transform, cz.evenOdd = wt_, eo_
    with torch.no_grad():
        out = m(x)
        if keep is not None:
            cz.wavelet_transform, cz.evenOdd = wt, eo
            for h in (cz.A, cz.B, cz.C):
                h._forward_hooks.clear()
        loss = float(m.train_loss(x, y).double().mean())
        roll = rollout(m, x, name, dt)
    return out, loss, roll, m


def main():
    z = {}
    for k in (2, 3, 4):
        for nm, a in zip(("H0", "H1", "G0", "G1", "PHI0", "PHI1"), get_filter("legendre", k)):
            z[f"filt_k{k}_{nm}"] = a
        cz = MWT_CZ3d(k=k, alpha=2, L=0, c=1, base="legendre")
        for nm in MC._BUFFERS:
            z[f"buf_k{k}_{nm}"] = getattr(cz, nm).numpy()
    keys = {}
    for name in MC.CASES:
        keep = {} if name == "a" else None
        out, loss, roll, m = run(name, False, keep)
        keep64 = {} if name == "a" else None
        with as_double():
            out64, loss64, roll64, _ = run(name, True, keep64)
        keys[name] = [[k_, list(v.shape), str(v.dtype)] for k_, v in m.state_dict().items()]
        z[f"{name}_out"], z[f"{name}_out_selferr"] = MC.stored(name, out).numpy(), rel(out, out64)
        z[f"{name}_loss"], z[f"{name}_loss_selferr"] = loss, abs(loss - loss64) / abs(loss64)
        z[f"{name}_roll"], z[f"{name}_roll_selferr"] = MC.roll_stored(name, roll).numpy(), rel(roll, roll64)
        print(name, "out std %.3f" % float(out.std()), "selferr out %.2e roll %.2e loss %.2e" %
              (z[f"{name}_out_selferr"], z[f"{name}_roll_selferr"], z[f"{name}_loss_selferr"]), "roll std %.3f" % float(roll.std()))
        if keep is not None:
            ns = len(keep["d"])
            for i in range(ns):
                for tag, j, key in [(t_, i, f"a_cz0_{t_}{i}") for t_ in ("d", "s", "A", "B", "C")] + [("eo", i, f"a_cz0_eo{ns - 1 - i}")]:
                    z[key] = MC.inter_stored(keep[tag][j]).numpy()      # (evenOdd runs from the coarsest level upwards)
                    z[key + "_selferr"] = rel(keep[tag][j], keep64[tag][j])          # over the whole tensor, not only the stored part
    np.savez_compressed(os.path.join(HERE, "mwt_small.npz"), **z)
    cfg = {}
    for scen in SCENARIOS:
        with open(os.path.join(REF, scen, "mwt.yaml")) as fh:
            cfg[scen] = yaml.safe_load(fh)
    doc = {"state_dict": keys, "model_keys": {s: {k_: cfg[s][k_] for k_ in MODEL_KEYS + ("model_name", "N_autoregressive")} for s in SCENARIOS},
           "native_shapes": {s: {"shape_in": list(NATIVE[s][0]), "shape_out": list(NATIVE[s][1])} for s in SCENARIOS}}
    with open(os.path.join(HERE, "mwt_configs.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote mwt_small.npz (%.1f kB) and mwt_configs.json" % (os.path.getsize(os.path.join(HERE, "mwt_small.npz")) / 1e3))
    if "--write-yamls" in sys.argv:
        for scen in SCENARIOS:
            body = dict(cfg[scen])
            for k_ in SYNTH:
                if k_ in body:
                    body["ref_" + k_] = body[k_]
            body.update(dataset_name="synthetic", dataset_root="", num_workers=0, normalizer="none", checkpoint_path="",
                        shape_in=list(NATIVE[scen][0]), shape_out=list(NATIVE[scen][1]), n_train=16, n_val=4)
            path = os.path.join(ROOT, "realpdebench_amd", "configs", scen, "mwt.yaml")
            with open(path, "w") as fh:
                fh.write(f"# Key surface and values of the reference's realpdebench/configs/{scen}/mwt.yaml (written by "
                         "tests/golden/make_golden_mwt.py --write-yamls).\n# MWT3d on MI355X is evaluation and rollout only: "
                         "realpdebench_amd.train refuses this model at trainer construction.\n# Deviations, on purpose: dataset_name / "
                         "dataset_root default to the synthetic generator (no dataset ships here), normalizer to \"none\"\n# and "
                         "checkpoint_path to \"\"; the reference's values are kept in the ref_* keys below.\n")
                yaml.safe_dump(body, fh, sort_keys=False, default_flow_style=None)


if __name__ == "__main__":
    main()
