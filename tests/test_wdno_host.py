"""WDNO without a GPU: the restatement the fixture was made with (tests/wdno_restatement.py), the shapes, the schedule and the registry.

* The transform is pinned by PROPERTIES, because ``ptwt`` / ``pywt`` are not installed and the fixture was made with the restatement in
  their place: ``rec(dec(x)) == x`` for both wavelets at even and odd lengths, and hand-derived answers on unit impulses (from the
  published definition: per axis ``out[i] = sum_k dec[L - 1 - k] x[2 i + k - p]``, ``p = (2L - 3) // 2``).
* The fp64 restatement of the whole model, with oracle/unet_oracle.py as the denoiser, reproduces the fixture's fp64 outputs.  Bound: both
  sides are fp64 runs of the same mathematics in different operation orders; the sampler amplifies a rounding as the fixture's own
  fp32-vs-fp64 Rel-L2 says (up to 6e-5 for 2^-24), so fp64 roundings (2^-53) arrive below 2e-13 and 1e-9 leaves room for thousands of
  them.  The fp32 vectors are met within 4 x their recorded ``selferr``.
* ``coef_shape`` / ``padded_shape`` of the five config shapes, the schedule buffers against the reference's (bit for bit), the DDIM time
  pairs, the noise recipe against its recorded checksums, ``load_model`` on CPU tensors with the reference's state-dict key set."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wdno_common as WC                          # noqa: E402
import wdno_restatement as R                      # noqa: E402
from oracle import unet_oracle                    # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "wdno_small.npz"))
CFG = json.load(open(os.path.join(ROOT, "tests", "golden", "wdno_configs.json")))
S, Q = 0.7071067811865476, 0.08838834764831845
# scenario -> (coef_shape, padded_shape, state channels), from the rule Nc = (N + L - 1) // 2 and the stride 2 ** len(dim_mults)
MESHES = {
    "cylinder": ((10, 32, 64), (12, 32, 64), 48),            # bior1.1, [1, 2]
    "controlled_cylinder": ((5, 32, 64), (8, 32, 64), 64),   # bior1.1, [1, 2, 4], 5 -> 3 channels
    "fsi": ((10, 32, 32), (16, 32, 32), 48),                 # bior1.1, [1, 2, 4]
    "foil": ((12, 34, 66), (12, 36, 68), 48),                # bior1.3, [1, 2]
    "combustion": ((12, 34, 34), (12, 36, 36), 256),         # bior1.3, [1, 2], 16 -> 16 channels
}


def g(key):
    return torch.from_numpy(np.array(GOLD[key]))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def write_rescaler(root, case):
    os.makedirs(os.path.join(root, case), exist_ok=True)
    torch.save(g(f"{case}/rescaler").reshape(1, 1, 1, 1, -1), os.path.join(root, case, f"wdno_rescaler_{WC.CASES[case]['wave']}_zero.pt"))


def cpu_model(case, run, root):
    """our WDNO on CPU tensors (it cannot run there: the shapes, buffers, tables and the state dict are what is used)"""
    from realpdebench_amd.model.unet import Unet3d
    from realpdebench_amd.model.wdno import WDNO
    c, r = WC.CASES[case], WC.CASES[case]["runs"][run]
    write_rescaler(root, case)
    unet = Unet3d(dim=WC.DIM, dim_mults=WC.DIM_MULTS, channels=WC.channels(case), in_time=c["padded"][0], out_time=c["padded"][0])
    return WDNO(unet, WC.Dataset(case), str(root), case, c["wave"], "zero", timesteps=r["timesteps"], beta_schedule="sigmoid",
                sampling_timesteps=r["sampling_timesteps"], ddim_sampling_eta=r["eta"])


# ------------------------------------------------------------------------------------------------ the transform, by properties
@pytest.mark.parametrize("wave", list(R.TABLES))
@pytest.mark.parametrize("shape", [(4, 6, 8), (5, 7, 9), (6, 10, 10), (20, 64, 16)])
def test_perfect_reconstruction(wave, shape):
    x = torch.rand(3, *shape, dtype=torch.float64, generator=torch.Generator().manual_seed(sum(shape)))
    c = R.wavedec3(x, R.Wavelet(wave))
    L = len(R.TABLES[wave]["dec_lo"])
    assert tuple(c[0].shape[1:]) == tuple((n + L - 1) // 2 for n in shape) and list(c[1]) == list(R.SUBBANDS[1:])
    y = R.waverec3(c, R.Wavelet(wave))[:, :shape[0], :shape[1], :shape[2]]
    assert float((y - x).abs().max()) < 1e-13


def test_impulse_answers():
    # bior1.1 (L = 2, p = 0): an impulse at an odd index meets dec[0], at an even index dec[1]: a -> S either way, d -> -S (odd) / +S (even)
    x = torch.zeros(1, 4, 4, 4, dtype=torch.float64)
    x[0, 1, 0, 1] = 1.0
    c = R.wavedec3(x, R.Wavelet("bior1.1"))
    sign = {"aaa": 1, "aad": -1, "ada": 1, "add": -1, "daa": -1, "dad": 1, "dda": -1, "ddd": 1}
    for s in R.SUBBANDS:
        t = c[0] if s == "aaa" else c[1][s]
        want = torch.zeros(1, 2, 2, 2, dtype=torch.float64)
        want[0, 0, 0, 0] = sign[s] * S ** 3
        assert torch.allclose(t, want, atol=1e-15), s
    # bior1.3 (L = 6, p = 4), N = 8, impulse at 2: out[i] = dec[2 i - 1], i = 1, 2, 3 -> lo (Q, S, -Q), hi (0, S, 0); Nc = 6
    lo = torch.tensor([0, Q, S, -Q, 0, 0], dtype=torch.float64)
    hi = torch.tensor([0, 0, S, 0, 0, 0], dtype=torch.float64)
    x = torch.zeros(1, 8, 8, 8, dtype=torch.float64)
    x[0, 2, 2, 2] = 1.0
    c = R.wavedec3(x, R.Wavelet("bior1.3"))
    f = {"a": lo, "d": hi}
    for s in R.SUBBANDS:
        t = c[0] if s == "aaa" else c[1][s]
        assert torch.allclose(t[0], torch.einsum("i,j,k->ijk", f[s[0]], f[s[1]], f[s[2]]), atol=1e-15), s
    # and the model's own tables are the same published constants
    from realpdebench_amd.model.wdno import WAVELETS
    for wave, t in R.TABLES.items():
        assert [list(v) for v in WAVELETS[wave]] == [t["dec_lo"], t["dec_hi"], t["rec_lo"], t["rec_hi"]]


def test_state_columns_and_frame_order():
    """column 8 cv + s, cv = c r + sub = frame sub T + t of channel c (wdno.py:493-495), and its inverse (wdno.py:427-430)"""
    x = torch.rand(2, 12, 10, 10, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    cols = R.dec_state(x, 2, "bior1.3", None, (8, 8, 8))
    one = R.wavedec3(x[:, 6:, :, :, 1].reshape(2, 6, 10, 10), R.Wavelet("bior1.3"))      # channel 1, sub-frame 1 -> cv = 3
    assert torch.equal(cols[:, :5, :7, :7, 8 * 3 + 5], one[1]["dad"]) and not cols[:, 5:].any()
    assert float((R.rec_state(cols, "bior1.3", torch.ones(48, dtype=torch.float64), (6, 10, 10), 3, 2) - x).abs().max()) < 1e-13


# ------------------------------------------------------------------------------------------------ shapes, schedule, noise
@pytest.mark.parametrize("scenario", list(MESHES))
def test_config_meshes(scenario):
    from realpdebench_amd.model.wdno import WAVELETS, coef_len
    keys, shp = CFG["model_keys"][scenario], CFG["native_shapes"][scenario]
    coef, padded, ch = MESHES[scenario]
    L = len(WAVELETS[keys["wave_type"]][0])
    mine = tuple(coef_len(n, L) for n in shp["shape_in"][:3])
    f = 2 ** len(keys["dim_mults"])
    assert mine == coef and tuple((d + f - 1) // f * f for d in mine) == padded
    assert CFG["meshes"][scenario] == {"coef_shape": list(coef), "padded_shape": list(padded), "channels": ch}
    assert padded[1] - coef[1] == padded[2] - coef[2], "the reference pads W by H's pad (wdno.py:341): every config must agree"


def test_schedule_buffers_equal_the_references(tmp_path):
    from realpdebench_amd.model.wdno import SCHEDULE_BUFFERS, ddim_time_pairs
    m = cpu_model("a", "ddim", tmp_path)
    stored = sorted(k[len("buffers/"):] for k in GOLD.files if k.startswith("buffers/"))
    assert stored == sorted(SCHEDULE_BUFFERS)
    for k in SCHEDULE_BUFFERS:
        assert torch.equal(getattr(m, k), g("buffers/" + k)), k
    assert ddim_time_pairs(1000, 3) == [(999, 665), (665, 332), (332, -1)]
    assert ddim_time_pairs(1000, 10)[0] == (999, 899) and ddim_time_pairs(1000, 10)[-1][1] == -1
    filt, ddim, anc, pairs = m._constants("cpu")
    assert tuple(ddim.shape) == (3, 5) and tuple(anc.shape) == (1000, 5) and ddim.dtype == torch.float32
    # eta = 1: sigma^2 + c^2 = 1 - abar_next, and the last row only carries the two x0 scalars
    ab = m.alphas_cumprod[665].double()
    assert abs(float(ddim[0, 3].double() ** 2 + ddim[0, 4].double() ** 2 - (1 - ab))) < 1e-6 and float(ddim[0, 2]) == float(ab.float().sqrt())
    assert torch.equal(ddim[2, :2], torch.stack((m.sqrt_recip_alphas_cumprod[332], m.sqrt_recipm1_alphas_cumprod[332])))
    assert float(anc[0, 4]) == float((0.5 * m.posterior_log_variance_clipped[0]).exp())


def test_noise_recipe_matches_the_fixture():
    for case, c in WC.CASES.items():
        for run in c["runs"]:
            sums = g(f"{case}/{run}/noise_checksums")
            assert sums.shape[0] == WC.n_draws(case, run)
            for k in range(sums.shape[0]):
                d = WC.noise(case, run, k)
                assert tuple(d.shape) == WC.state_shape(case) and torch.equal(WC.noise_checksum(d), sums[k])
    d = WC.noise("a", "ddim", 1)
    assert abs(float(d.mean())) < 0.05 and abs(float(d.var()) - 1) < 0.05


# ------------------------------------------------------------------------------------------------ the fp64 restatement and the fixture
@pytest.mark.parametrize("case,run", [(c, r) for c in WC.CASES for r in WC.CASES[c]["runs"]])
def test_restatement_reproduces_the_fixture(tmp_path, case, run):
    c = WC.CASES[case]
    m = cpu_model(case, run, tmp_path)
    sd = WC.seeded_state(m.state_dict())
    usd = {k[len("model."):]: v.double() for k, v in sd.items() if k.startswith("model.")}
    plan = R.Plan(c["shape_in"], c["shape_out"], c["wave"], len(WC.DIM_MULTS))
    assert plan.coef == c["coef"] == m.coef_shape and plan.padded == c["padded"] == m.padded_shape
    # the reference's fp64 run forms the step scalars in fp64 from its fp32-rounded buffers; the model's fp32 tables are the fp32 form
    from realpdebench_amd.model.wdno import SCHEDULE_BUFFERS
    buf = {k: getattr(m, k) for k in SCHEDULE_BUFFERS}
    pairs = R.ddim_pairs(m.num_timesteps, m.sampling_timesteps)
    _, ddim32, anc32, mine = m._constants("cpu")
    assert mine == pairs and torch.equal(anc32, R.ancestral_scalars(buf))
    if run == "ddim":
        assert torch.equal(ddim32, R.ddim_scalars(buf, pairs, c["runs"][run]["eta"]))
    buf64 = {k: v.double() for k, v in buf.items()}
    ddim, anc = R.ddim_scalars(buf64, pairs, c["runs"][run]["eta"]) if run == "ddim" else None, R.ancestral_scalars(buf64)
    x = g(f"{case}/input").double()
    draws = [WC.noise(case, run, k) for k in range(WC.n_draws(case, run))]
    with R.default_dtype(torch.float64), torch.no_grad():
        unet = lambda s: unet_oracle.unet_forward(usd, s)        # noqa: E731
        if run == "ddim":
            cond, imgs, out = R.ddim_sample(unet, plan, ddim, x, m.rescaler.double(), draws[1:])      # draw 0 is discarded (wdno.py:382)
        else:
            cond, imgs, out = R.ancestral_sample(unet, plan, anc, x, m.rescaler.double(), draws)
    pre = f"{case}/{run}/"
    e64 = rel(out, g(pre + "out64"))
    print(f"[wdno-host] {case}/{run}: fp64 restatement vs the reference's fp64 run {e64:.3e}; vs its fp32 run {rel(out, g(pre + 'out')):.3e} "
          f"(selferr {float(GOLD[pre + 'out_selferr']):.3e})")
    assert e64 < 1e-9
    assert rel(cond, g(pre + "cond")) < 1e-6                      # the fp32 reference's conditioning state against fp64
    assert rel(out, g(pre + "out")) < 4 * float(GOLD[pre + "out_selferr"])
    for i, img in enumerate(imgs):
        assert rel(WC.thin(img), g(pre + f"img{i}")) < 4 * float(GOLD[pre + f"img{i}_selferr"]), i


@pytest.mark.parametrize("case", list(WC.CASES))
def test_restatement_loss_and_rescaler(tmp_path, case):
    c = WC.CASES[case]
    m = cpu_model(case, "ddim", tmp_path)
    usd = {k[len("model."):]: v.double() for k, v in WC.seeded_state(m.state_dict()).items() if k.startswith("model.")}
    plan = R.Plan(c["shape_in"], c["shape_out"], c["wave"], len(WC.DIM_MULTS))
    with R.default_dtype(torch.float64), torch.no_grad():
        loss = R.train_loss(lambda s: unet_oracle.unet_forward(usd, s), plan, m.sqrt_alphas_cumprod.double(),
                            m.sqrt_one_minus_alphas_cumprod.double(), g(f"{case}/input").double(), g(f"{case}/target").double(),
                            m.rescaler.double(), WC.noise(case, "loss", 0), torch.tensor(WC.LOSS_T))
    assert abs(float(loss.mean()) / float(GOLD[f"{case}/loss_mean"]) - 1) < 1e-9
    assert rel(WC.thin(loss), g(f"{case}/loss")) < 4 * float(GOLD[f"{case}/loss_selferr"])
    ds = WC.Dataset(case)
    assert torch.equal(ds.inputs, g(f"{case}/ds_inputs")) and torch.equal(ds.targets, g(f"{case}/ds_targets"))
    assert rel(R.rescaler_of(plan, ds.inputs.double(), ds.targets.double()).reshape(-1), g(f"{case}/rescaler")) < 1e-6


# ------------------------------------------------------------------------------------------------ registry and refusals
def test_load_model_on_cpu_tensors(tmp_path):
    from realpdebench_amd.model import load_model
    from realpdebench_amd.model.wdno import WDNO, SCHEDULE_BUFFERS
    write_rescaler(tmp_path, "a")
    kw = dict(model_name="wdno", dim=64, dim_mults=[1, 2], wave_type="bior1.1", pad_mode="zero", beta_schedule="sigmoid",
              sampling_timesteps=3, ddim_sampling_eta=1.0, dataset_root=str(tmp_path), dataset_name="a")
    m = load_model(WC.Dataset("a"), device="cpu", **kw)
    assert isinstance(m, WDNO) and m.model.init_conv_implicit and m.model.in_time == m.model.out_time == 4
    assert m.num_timesteps == 1000 and m.is_ddim_sampling and m.channels == 24
    want = {k: tuple(s) for k, s, _ in CFG["state_dict"]["a"]}
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == want and sorted(k for k in got if not k.startswith("model.")) == sorted(SCHEDULE_BUFFERS)
    assert torch.equal(m.rescaler.reshape(-1), g("a/rescaler") * 1.4)
    with pytest.raises(RuntimeError, match="no CPU fallback"), torch.no_grad():
        m(torch.zeros(1, 4, 16, 24, 2))
    with pytest.raises(NotImplementedError, match="wave_type"):
        load_model(WC.Dataset("a"), device="cpu", **{**kw, "wave_type": "haar"})
    with pytest.raises(NotImplementedError, match="pad_mode"):
        load_model(WC.Dataset("a"), device="cpu", **{**kw, "pad_mode": "reflect"})
    with pytest.raises(ValueError, match="missing wave_type, pad_mode "):
        load_model(WC.Dataset("a"), device="cpu", **{k: v for k, v in kw.items() if k not in ("wave_type", "pad_mode")})


def test_constructor_refusals(tmp_path):
    from realpdebench_amd.model.unet import Unet3d
    from realpdebench_amd.model.wdno import WDNO, rescaler_path

    class Ds(torch.utils.data.Dataset):
        dataset_type = "numerical"

        def __init__(self, si, so):
            self.s = (torch.zeros(*si), torch.zeros(*so))

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return self.s

    unet = Unet3d(dim=64, dim_mults=(1, 2), channels=24, in_time=4, out_time=4)
    os.makedirs(tmp_path / "q")
    torch.save(torch.ones(1, 1, 1, 1, 24), rescaler_path(str(tmp_path), "q", "bior1.1", "zero"))
    # (4, 16, 20): coefficient mesh (2, 8, 10) needs no pad on H and 2 on W -- the reference's quirk cannot run it
    with pytest.raises(ValueError, match="applies H's pad to both"):
        WDNO(unet, Ds((4, 16, 20, 2), (4, 16, 20, 1)), str(tmp_path), "q", "bior1.1")
    with pytest.raises(ValueError, match="channels"):
        WDNO(unet, Ds((4, 16, 24, 3), (4, 16, 24, 1)), str(tmp_path), "q", "bior1.1")
    # no rescaler file and no GPU: computing it is HIP work
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        WDNO(unet, Ds((4, 16, 24, 2), (4, 16, 24, 1)), str(tmp_path), "missing", "bior1.1")
