"""WDNO vectors from the reference (build container only; needs /root/reference):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_wdno.py [--write-yamls]
Writes tests/golden/wdno_small.npz and tests/golden/wdno_configs.json -- data only.

The reference's ``WDNO`` and ``wdno_libs.unet.Unet3d`` are IMPORTED, with the import-only stubs of make_golden_unet.py (``torchvision``,
``einops_exts``) and its restated ``rotary_embedding_torch.RotaryEmbedding``.  ``ptwt`` / ``pywt`` are REAL arithmetic in third-party
packages that are absent here: ``ptwt.wavedec3`` / ``ptwt.waverec3`` / ``pywt.Wavelet`` are replaced by the restatement of their
published definitions in tests/wdno_restatement.py (transform and the two filter tables).  These vectors therefore pin everything
around the transform -- conditioning, both samplers, the schedule, the loss, the rescaler, the channel orders -- and leave the transform
itself to properties (perfect reconstruction, impulse answers: tests/test_wdno_host.py).

Per case of wdno_common.CASES (Unet3d(dim=64, dim_mults=[1,2]), B = 2, seeded weights -- not stored) and per run: the conditioning
state, ``img`` after every step (thinned by wdno_common.thin), the output, the output of the same run in fp64, and the reference's own
fp32-versus-fp64 Rel-L2 of each (``*_selferr``, over the whole tensor before thinning).  Per case: ``train_loss`` for fixed ``t`` and
noise, the rescaler the reference computes from the four-sample dataset, inputs and dataset, and the checksums of every noise draw;
once, the reference's schedule buffers for timesteps = 1000 with the sigmoid schedule.
The maker asserts that the reference's state-dict key / shape list equals what wdno_configs.json stores.
``--write-yamls`` re-emits realpdebench_amd/configs/<scenario>/wdno.yaml from the reference's values (synthetic dataset defaults on top)."""
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch
import yaml
from einops import rearrange, repeat

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import wdno_common as WC                                                  # noqa: E402
import wdno_restatement as R                                              # noqa: E402
from make_golden_configs import NATIVE, REF, SCENARIOS, SYNTH             # noqa: E402

for name in ("torchvision", "torchvision.transforms", "torchvision.utils", "einops_exts", "rotary_embedding_torch", "ptwt", "pywt"):
    sys.modules.setdefault(name, types.ModuleType(name))
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
sys.modules["einops_exts"].check_shape = lambda *a, **k: None
sys.modules["einops_exts"].rearrange_many = lambda ts, pattern, **kw: [rearrange(t, pattern, **kw) for t in ts]
sys.modules["ptwt"].wavedec3 = R.wavedec3
sys.modules["ptwt"].waverec3 = R.waverec3
sys.modules["pywt"].Wavelet = R.Wavelet


class RotaryEmbedding(torch.nn.Module):
    def __init__(self, dim, theta=10000):
        super().__init__()
        self.freqs = torch.nn.Parameter(1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2].float() / dim)), requires_grad=False)

    def rotate_queries_or_keys(self, t, seq_dim=-2):
        pos = torch.arange(t.shape[seq_dim], device=t.device, dtype=self.freqs.dtype)
        f = repeat(torch.einsum("i,j->ij", pos, self.freqs), "... n -> ... (n r)", r=2)
        x1, x2 = rearrange(t, "... (d r) -> ... d r", r=2).unbind(-1)
        rot = rearrange(torch.stack((-x2, x1), dim=-1), "... d r -> ... (d r)")
        return t * f.cos() + rot * f.sin()


sys.modules["rotary_embedding_torch"].RotaryEmbedding = RotaryEmbedding
from realpdebench.model import wdno as ref_wdno                           # noqa: E402
from realpdebench.model.wdno_libs.unet import Unet3d as RefUnet           # noqa: E402

MODEL_KEYS = ("model_name", "dim", "dim_mults", "wave_type", "pad_mode", "beta_schedule", "sampling_timesteps", "ddim_sampling_eta",
              "N_autoregressive")


class Draws:
    """stands where the module-level ``torch`` of the reference's wdno.py stands while a run is recorded: ``randn`` / ``randn_like`` /
    ``randint`` hand out the prepared draws in call order, everything else is torch's own"""

    def __init__(self):
        self.queue, self.t, self.dtype = None, None, torch.float32

    def __getattr__(self, name):
        return getattr(torch, name)

    def _next(self, shape):
        if self.queue is None:
            return torch.randn(*shape)
        d = self.queue.pop(0)
        assert tuple(d.shape) == tuple(shape), (d.shape, shape)
        return d.to(self.dtype)

    def randn(self, *shape, **kw):
        return self._next(shape[0] if len(shape) == 1 and not isinstance(shape[0], int) else shape)

    def randn_like(self, t):
        return self._next(t.shape)

    def randint(self, *a, **kw):
        return self.t.clone() if self.t is not None else torch.randint(*a, **kw)


DRAWS = Draws()
ref_wdno.torch = DRAWS


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def build(case, run, root, double=False):
    c, r = WC.CASES[case], WC.CASES[case]["runs"][run]
    torch.manual_seed(0)
    unet = RefUnet(dim=WC.DIM, dim_mults=WC.DIM_MULTS, channels=WC.channels(case))
    m = ref_wdno.WDNO(unet, WC.Dataset(case), root, case, c["wave"], "zero", timesteps=r["timesteps"], beta_schedule="sigmoid",
                      sampling_timesteps=r["sampling_timesteps"], ddim_sampling_eta=r["eta"])
    assert tuple(m.coef_shape) == c["coef"] and tuple(m.padded_shape) == c["padded"], (m.coef_shape, m.padded_shape)
    m.load_state_dict(WC.seeded_state(m.state_dict()))
    return (m.double() if double else m).eval()


def run_forward(m, case, run, x, dtype):
    """one recorded forward: (cond, [img after every step], output)"""
    seen = {"cond": None, "imgs": []}
    pad_cond, in_cond = type(m).set_pad_condition, type(m).set_input_condition

    def set_input_condition(state, inp):
        if seen["cond"] is None:
            seen["cond"] = inp.clone()
        return in_cond(m, state, inp)

    def set_pad_condition(state):
        out = pad_cond(m, state)
        seen["imgs"].append(out.clone())
        return out

    m.set_input_condition, m.set_pad_condition = set_input_condition, set_pad_condition
    DRAWS.queue = [WC.noise(case, run, k) for k in range(WC.n_draws(case, run))]
    DRAWS.dtype = dtype
    with R.default_dtype(dtype):                    # the U-Net builds its time input with the default dtype (wdno_libs/unet.py:506)
        out = m(x.to(dtype))
    assert not DRAWS.queue, "the reference made fewer draws than wdno_common.n_draws says"
    DRAWS.queue = None
    del m.set_input_condition, m.set_pad_condition
    return seen["cond"], seen["imgs"][1:], out          # imgs[0] is the conditioned start state


def main():
    out, doc = {}, {"state_dict": {}, "selferr": {}}
    root = tempfile.mkdtemp()
    for case, c in WC.CASES.items():
        os.makedirs(os.path.join(root, case), exist_ok=True)
        x, y = WC.case_inputs(case)
        ds = WC.Dataset(case)
        out[f"{case}/input"], out[f"{case}/target"] = x.numpy(), y.numpy()
        out[f"{case}/ds_inputs"], out[f"{case}/ds_targets"] = ds.inputs.numpy(), ds.targets.numpy()
        for run in c["runs"]:
            m32 = build(case, run, root)
            if run == "ddim":
                sd = m32.state_dict()
                doc["state_dict"][case] = [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]
                if case == "a":                            # the schedule buffers (timesteps = 1000, sigmoid), as registered
                    for k, v in sd.items():
                        if not k.startswith("model."):
                            out["buffers/" + k] = v.numpy()
                saved = torch.load(os.path.join(root, case, f"wdno_rescaler_{c['wave']}_zero.pt"))
                out[f"{case}/rescaler"] = saved.reshape(-1).numpy()
                assert torch.equal(m32.rescaler.reshape(-1), saved.reshape(-1) * 1.4)
            m64 = build(case, run, root, double=True)
            cond, imgs, o32 = run_forward(m32, case, run, x, torch.float32)
            cond64, imgs64, o64 = run_forward(m64, case, run, x, torch.float64)
            n = len(imgs)
            assert n == (c["runs"][run]["sampling_timesteps"] or c["runs"][run]["timesteps"]), n
            pre = f"{case}/{run}/"
            out[pre + "cond"], out[pre + "out"], out[pre + "out64"] = cond.numpy(), o32.numpy(), o64.numpy()
            out[pre + "out_selferr"] = np.float64(rel(o32, o64))
            for i in range(n):
                out[pre + f"img{i}"] = WC.thin(imgs[i]).numpy()
                out[pre + f"img{i}_selferr"] = np.float64(rel(imgs[i], imgs64[i]))
            out[pre + "noise_checksums"] = torch.stack([WC.noise_checksum(WC.noise(case, run, k))
                                                         for k in range(WC.n_draws(case, run))]).numpy()
            doc["selferr"][pre + "out"] = rel(o32, o64)
            print(pre, "out", tuple(o32.shape), "selferr", rel(o32, o64), "img selferr", [rel(a, b) for a, b in zip(imgs, imgs64)],
                  "clamped fraction of the last img", float((imgs[-1].abs() == 1).double().mean()))
            if run == "ddim":                              # train_loss at fixed t and noise (timesteps = 1000)
                t = torch.tensor(WC.LOSS_T)
                nz = WC.noise(case, "loss", 0)
                DRAWS.t = t
                l32 = m32.p_losses(x, y, noise=nz.clone())
                with R.default_dtype(torch.float64):
                    l64 = m64.p_losses(x.double(), y.double(), noise=nz.double())
                DRAWS.t = None
                out[f"{case}/loss"], out[f"{case}/loss_mean"] = WC.thin(l32.detach()).numpy(), np.float64(l64.mean())
                out[f"{case}/loss_selferr"] = np.float64(rel(l32, l64))
                out[f"{case}/loss_noise_checksum"] = WC.noise_checksum(nz).numpy()
                doc["selferr"][f"{case}/loss"] = rel(l32, l64)
                print(case, "loss mean", float(l64.mean()), "selferr", rel(l32, l64))
    shutil.rmtree(root)
    # the fp64 restatement of tests/wdno_restatement.py must reproduce what it helped to make: see tests/test_wdno_host.py
    cfg = {}
    for scen in SCENARIOS:
        with open(os.path.join(REF, scen, "wdno.yaml")) as fh:
            cfg[scen] = yaml.safe_load(fh)
    doc["model_keys"] = {s: {k: cfg[s][k] for k in MODEL_KEYS} for s in sorted(cfg)}
    doc["native_shapes"] = {s: {"shape_in": list(NATIVE[s][0]), "shape_out": list(NATIVE[s][1])} for s in sorted(cfg)}
    doc["meshes"] = {}
    for s in sorted(cfg):
        p = R.Plan(NATIVE[s][0], NATIVE[s][1], cfg[s]["wave_type"], len(cfg[s]["dim_mults"]))
        doc["meshes"][s] = {"coef_shape": list(p.coef), "padded_shape": list(p.padded), "channels": p.channels}
    np.savez_compressed(os.path.join(HERE, "wdno_small.npz"), **out)
    with open(os.path.join(HERE, "wdno_configs.json"), "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    print("wrote wdno_small.npz (%.1f kB) and wdno_configs.json" % (os.path.getsize(os.path.join(HERE, "wdno_small.npz")) / 1e3))
    if "--write-yamls" in sys.argv:
        for scen in SCENARIOS:
            body = dict(cfg[scen])
            for k_ in SYNTH:
                if k_ in body:
                    body["ref_" + k_] = body[k_]
            body.update(dataset_name="synthetic", dataset_root="", num_workers=0, normalizer="none", checkpoint_path="",
                        shape_in=list(NATIVE[scen][0]), shape_out=list(NATIVE[scen][1]), n_train=16, n_val=4)
            path = os.path.join(ROOT, "realpdebench_amd", "configs", scen, "wdno.yaml")
            with open(path, "w") as fh:
                fh.write(f"# Key surface and values of the reference's realpdebench/configs/{scen}/wdno.yaml (written by "
                         "tests/golden/make_golden_wdno.py --write-yamls).\n# WDNO on MI355X is evaluation and rollout only: "
                         "realpdebench_amd.train refuses this model at trainer construction.\n# load_model reads dim, dim_mults, wave_type, "
                         "pad_mode, beta_schedule, sampling_timesteps, ddim_sampling_eta, dataset_root and dataset_name\n# (the rescaler "
                         "file wdno_rescaler_<wave_type>_<pad_mode>.pt lives under dataset_root/dataset_name, as in the reference).\n# "
                         "Deviations, on purpose: dataset_name / dataset_root default to the synthetic generator (no dataset ships here), "
                         "normalizer to \"none\"\n# and checkpoint_path to \"\"; the reference's values are kept in the ref_* keys below.\n")
                yaml.safe_dump(body, fh, sort_keys=False, default_flow_style=None)


if __name__ == "__main__":
    main()
