"""DMD on the GPU: rpb_dmd_gram and rpb_dmd_predict against fp64 products, the whole model and the 2-step feedback rollout against the
reference's vectors (tests/golden/dmd_small.npz), the evaluation loop's channel handling, the five YAMLs at native shape and the
eval entry point.

Bounds.  Gram: Rel-L2 < 1e-12 against numpy's fp64 X X^T -- every product of two fp32 values is exact in fp64, so only the order of
at most P f <= 8198 additions differs (eps64 sqrt(8198) ~ 2e-14).  Predict: Rel-L2 < 1e-6 -- fp64 accumulation, one rounding to fp32
per output (2^-24 = 6e-8 each); the project's per-kernel bound is 1e-5.  Whole model and rollout: tests/dmd_helpers.tol."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
from dmd_helpers import CFG, DC, GOLD, SCENARIOS, One, case_model, rel, tol          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (B, T, P, C, f, S): point tail + several workgroups per sample; the full tile grid; one tile + wide cells; the minimum
KERNEL_CASES = [(2, 20, 4099, 3, 2, 20), (1, 32, 257, 2, 2, 7), (3, 5, 33, 16, 2, 32), (1, 3, 7, 1, 1, 1)]


def _x(B, T, P, C):
    return torch.from_numpy(np.random.default_rng(B * 1000 + T).standard_normal((B, T, P, C), dtype=np.float32))


@pytest.mark.parametrize("B,T,P,C,f,S", KERNEL_CASES)
def test_gram_kernel(B, T, P, C, f, S):
    from realpdebench_amd import ops
    x = _x(B, T, P, C)
    X = x[..., :f].double().reshape(B, T, P * f)
    want = X @ X.transpose(1, 2)
    xd = x.to(DEV)
    G = ops.dmd_gram(xd, f)
    G2 = ops.dmd_gram(xd, f)
    assert G.dtype == torch.float64 and tuple(G.shape) == (B, T, T)
    e = rel(G.cpu(), want)
    print(f"dmd_gram B={B} T={T} P={P} C={C} f={f}: Rel-L2 {e:.2e} ({ops._lib.query('rpb_dmd_gram_groups', B, P, f)} workgroups per sample)")
    assert e < 1e-12
    assert torch.equal(G, G.transpose(1, 2)), "G must be symmetric bit for bit"
    assert torch.equal(G, G2), "two calls must be bit-equal"


@pytest.mark.parametrize("B,T,P,C,f,S", KERNEL_CASES)
def test_predict_kernel(B, T, P, C, f, S):
    from realpdebench_amd import ops
    x = _x(B, T, P, C)
    rng = np.random.default_rng(S)
    M = torch.from_numpy(rng.uniform(-1, 1, (B, T - 1, S)) * 10.0 ** rng.uniform(0, 3, (B, T - 1, S)))     # mixed sign, up to 1e3
    want = torch.einsum("bks,bkn->bsn", M, x[:, 1:, :, :f].double().reshape(B, T - 1, P * f)).reshape(B, S, P, f)
    xd, Md = x.to(DEV), M.to(DEV)
    out = ops.dmd_predict(xd, Md, f)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, S, P, f)
    e = rel(out.cpu(), want)
    print(f"dmd_predict B={B} T={T} P={P} C={C} f={f} S={S}: Rel-L2 {e:.2e}")
    assert e < 1e-6
    assert torch.equal(out, ops.dmd_predict(xd, Md, f))


@pytest.mark.parametrize("case", list(DC.CASES))
def test_model_against_reference(case):
    B, T, H, W, C, f, n_modes, S = DC.CASES[case]
    m = case_model(case, DEV).eval()
    assert m.device == torch.device(DEV)
    x = torch.from_numpy(GOLD[f"{case}/x"]).to(DEV)
    out = m(x)
    assert tuple(out.shape) == (B, S, H, W, f) and out.dtype == torch.float32
    e = rel(out.cpu(), GOLD[f"{case}/out"])
    print(f"DMD case {case}: Rel-L2 {e:.2e} vs the float32 reference (bound {tol(case + '/out'):.1e}; its own float32-vs-float64 error "
          f"{float(GOLD[case + '/out_selferr']):.2e}), {rel(out.cpu(), GOLD[case + '/out64']):.2e} vs the float64 reference")
    assert e < tol(case + "/out")
    assert torch.equal(m(x), out), "two forwards must be bit-equal"


def test_feedback_rollout_against_reference():
    from realpdebench_amd.data_normalizer import GaussianNormalizer
    from realpdebench_amd.rollout import autoregressive_rollout
    case = DC.ROLLOUT_CASE
    B, T, H, W, C, f, n_modes, S = DC.CASES[case]
    co = DC.ROLLOUT_C_OUT
    norm = GaussianNormalizer(*(torch.from_numpy(v) for v in DC.normalizer_stats(C, co)), device=DEV)
    raw = torch.from_numpy(GOLD[f"{case}/x"])
    x, _ = norm.preprocess(raw, raw[..., :co].contiguous())
    para = raw[..., co:].contiguous()
    roll = autoregressive_rollout(case_model(case, DEV), x, DC.ROLLOUT_STEPS, normalizer=norm, para_input=para)
    assert tuple(roll.shape) == (B, DC.ROLLOUT_STEPS * T, H, W, f + C - co)
    want = GOLD[f"{case}/roll"]
    for i in range(DC.ROLLOUT_STEPS):
        print(f"DMD rollout step {i}: Rel-L2 {rel(roll[:, i * T:(i + 1) * T, ..., :f].cpu(), want[:, i * T:(i + 1) * T]):.2e}")
    e = rel(roll[..., :f].cpu(), want)
    print(f"DMD rollout: Rel-L2 {e:.2e} (bound {tol(case + '/roll'):.1e})")
    assert e < tol(case + "/roll")
    # the control channels ride along, pre-processed with the statistics of the input channels that follow the predicted ones
    mi, _, si, _ = DC.normalizer_stats(C, co)
    ctrl = (para - torch.from_numpy(mi[f:f + C - co])) / torch.from_numpy(si[f:f + C - co])
    assert rel(roll[:, :T, ..., f:].cpu(), ctrl) < 1e-6


def _loader(last_channel_zero):
    from torch.utils.data import DataLoader, TensorDataset
    inp = torch.from_numpy(GOLD["a/x"])                          # [3,20,8,16,3]
    tgt = torch.from_numpy(np.random.default_rng(3).standard_normal(inp.shape, dtype=np.float32))
    if last_channel_zero:
        tgt[..., -1] = 0
    return DataLoader(TensorDataset(inp, tgt), batch_size=2, shuffle=False), inp, tgt


def test_evaluate_runs_over_the_measured_channels():
    from realpdebench_amd import eval as ev
    from realpdebench_amd.data_normalizer import IdentityNormalizer
    m = case_model("a", DEV)
    loader, inp, tgt = _loader(True)
    res, pred, target = ev.evaluate(m, loader, IdentityNormalizer(DEV), 1, 2)
    assert res["evaluated_channels"] == 2 and tuple(pred.shape) == (3, 20, 8, 16, 2) and tuple(target.shape) == (3, 20, 8, 16, 3)
    assert all(np.isfinite(v) for v in res.values())
    assert rel(pred.cpu(), GOLD["a/out"]) < tol("a/out")
    d = pred.cpu().double() - tgt[..., :2].double()
    assert abs(res["rmse"] - float((d ** 2).mean().sqrt())) < 1e-5 * res["rmse"]
    assert abs(res["normalized_mse"] - np.mean([float((d[:2] ** 2).mean()), float((d[2:] ** 2).mean())])) < 1e-5 * res["normalized_mse"]
    loader, _, _ = _loader(False)
    with pytest.raises(ValueError, match="predicts 2 channels but the targets have 3 measured"):
        ev.evaluate(m, loader, IdentityNormalizer(DEV), 1, 2)


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_native_shape_through_yaml(scenario):
    from realpdebench_amd.model import load_model
    from realpdebench_amd.rollout import autoregressive_rollout
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", scenario, "dmd.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    shape_in, shape_out = tuple(cfg["shape_in"]), tuple(cfg["shape_out"])
    assert list(shape_in) == CFG["native_shapes"][scenario]["shape_in"]
    m = load_model(One(shape_in, shape_out), device=DEV, **cfg).eval()
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((2,) + shape_in, dtype=np.float32)).to(DEV)
    out = m(x)
    assert tuple(out.shape) == (2,) + shape_out and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    para = x[..., shape_out[-1]:].contiguous()
    roll = autoregressive_rollout(m, x, 1, para_input=para)
    assert tuple(roll.shape) == (2,) + shape_in and bool(torch.isfinite(roll).all())
    assert torch.equal(roll[..., :shape_out[-1]], out) and torch.equal(roll[..., shape_out[-1]:], para)


def test_eval_entrypoint_with_the_literal_checkpoint_path(tmp_path):
    """`python -m realpdebench_amd.eval --config configs/cylinder/dmd.yaml`: the shipped YAML with its `checkpoint_path: 'no model
    needed'` (results redirected, fewer samples): no file is opened, the results land under results_path."""
    from realpdebench_amd import eval as ev
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", "cylinder", "dmd.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    assert cfg["checkpoint_path"] == "no model needed"
    cfg.update(results_path=str(tmp_path / "res"), n_train=2, n_val=4, test_batch_size=2)
    path = tmp_path / "dmd.yaml"
    path.write_text(yaml.safe_dump(cfg))
    res = ev.main(["--config", str(path)])
    assert res["evaluated_channels"] == 2 and all(np.isfinite(v) for v in res.values())
    assert os.path.exists(os.path.join(str(tmp_path / "res"), "eval.log"))
