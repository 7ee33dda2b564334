"""DeepONet on the GPU: every rpb_don_* kernel and the branch against the matching step of tests/deeponet_restatement.py (fp64,
Rel-L2 < 1e-5, the project's per-kernel bound), the whole model against the reference's vectors (tests/golden/deeponet_small.npz):
eval forward, loss mean, 3-step rollout, bit-equal repeat, checkpoint I/O, the trunk cache; the native shapes of the five YAMLs; the
backward refusal; the entry points.  Whole-model tolerance: see tests/deeponet_helpers.py (Rel-L2 < max(1e-5, 4 x the reference's own
fp32-vs-fp64 error))."""
import os
import sys

import pytest
import torch
import yaml

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeponet_common as DC                      # noqa: E402
import deeponet_restatement as R                  # noqa: E402
from deeponet_helpers import CFG, GOLD, SCENARIOS, One, rel, sd_of, tol          # noqa: E402
from realpdebench_amd.model.deeponet import DeepONet, point_weights        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MSG = "DeepONet training step is not built yet"


def _model(case):
    shape_in, shape_out, p, _ = DC.CASES[case]
    m = DeepONet(shape_in, shape_out, shape_in[-1], shape_out[-1], p)
    m.load_state_dict(sd_of(case))
    return m.to(DEV).eval()


def _u(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _check(got, want, what):
    e = rel(got.cpu(), want)
    print(f"{what}: Rel-L2 {e:.2e}")
    if e >= 1e-5:                                 # localise: which rows (points / cells) and which channels are off
        d = (got.cpu().double() - want).reshape(-1, want.shape[-1]).abs()
        rows = (d.max(1).values > 1e-4).nonzero().flatten()
        cols = (d.max(0).values > 1e-4).nonzero().flatten()
        print(f"  {what}: {len(rows)}/{d.shape[0]} rows off, first {rows[:24].tolist()}; channels off {cols.tolist()}")
    assert e < 1e-5, what


@pytest.mark.parametrize("p,cout,N,B", [(64, 3, 4400, 2), (128, 16, 1024, 3), (256, 2, 193, 1)])
def test_point_mlp_kernel(p, cout, N, B):
    """Tail tiles (4400 = 34 x 128 + 48, 193 = 128 + 65), the widest C_out, every p; two calls are bit-equal."""
    W1, b1, W2, b2, W3, b3 = (_u(1, 512, p) * (3 / p) ** 0.5, _u(2, 512) * 0.2, _u(3, 128, 512) * (3 / 512) ** 0.5, _u(4, 128) * 0.2,
                              _u(5, cout, 128) * (3 / 128) ** 0.5, _u(6, cout) * 0.2)
    t, b = _u(7, N, p), _u(8, B, p) * 2
    pw = point_weights(*(w.to(DEV) for w in (W1, b1, W2, b2, W3, b3)))
    out = DeepONet.k_point_mlp(t.to(DEV), b.to(DEV), pw)
    out2 = DeepONet.k_point_mlp(t.to(DEV), b.to(DEV), pw)
    sd = {"output_net.0.weight": W1, "output_net.0.bias": b1, "output_net.3.weight": W2, "output_net.3.bias": b2,
          "output_net.6.weight": W3, "output_net.6.bias": b3}
    assert tuple(out.shape) == (B, N, cout)
    assert torch.equal(out, out2), "two calls must give bit-equal outputs"
    _check(out, R.point_mlp(sd, t.double(), b.double()), f"point_mlp p={p} C_out={cout} N={N} B={B}")


@pytest.mark.parametrize("p", [64, 256])
def test_trunk_kernel(p):
    T, H, W = 5, 20, 44                              # N = 4400: 68 full 64-point blocks and a tail of 48
    sd = sd_of("a" if p == 64 else "c")
    wt = [sd[f"trunk.fc.{i}.weight"].t().contiguous().to(DEV) for i in (0, 2, 4)]
    bs = [sd[f"trunk.fc.{i}.bias"].to(DEV) for i in (0, 2, 4)]
    _check(DeepONet.k_trunk(T, H, W, wt, bs, DEV), R.trunk(sd, T, H, W), f"trunk p={p}")


@pytest.mark.parametrize("B,T,H,W,C,ld", [(2, 5, 11, 6, 32, 64), (1, 2, 2, 5, 256, 256)])
def test_bn_relu_pool_kernel(B, T, H, W, C, ld):
    """Odd extents (the trailing frame / row is dropped), a leading dimension above the channel count (its upper channels leave as
    zeros), overlapping and replicated adaptive bins."""
    x = _u(1, B, T, H, W, ld)
    bn = (_u(2, C) * 0.25 + 1, _u(3, C) * 0.3, _u(4, C) * 0.45, _u(5, C) * 0.7 + 1.25)
    sc64 = bn[0].double() / torch.sqrt(bn[3].double() + 1e-5)
    sc, sh = sc64.float().to(DEV), (bn[1].double() - bn[2].double() * sc64).float().to(DEV)
    y = R.bn_relu(x[..., :C].double(), bn)
    for mode, want in ((0, R.max_pool(y)), (1, R.adaptive_pool(y))):
        got = DeepONet.k_bn_relu_pool(x.reshape(-1, ld).to(DEV), sc, sh, B, T, H, W, C, ld, mode).view(*want.shape[:4], ld)
        _check(got[..., :C], want, f"bn_relu_pool mode {mode} C={C} ld={ld}")
        assert not bool(got[..., C:].any()), "channels C..ld-1 must leave as zeros"


@pytest.mark.parametrize("case", list(DC.CASES))
def test_branch(case):
    m = _model(case)
    x, _ = DC.case_inputs(case)
    keep, keep_r = [], []
    with torch.no_grad():
        b = m.branch_forward(x.to(DEV), m._prep(torch.device(DEV)), keep=keep)
        br = R.branch(sd_of(case), x.double(), keep=keep_r)
    for i in range(4):
        _check(keep[i], keep_r[i], f"case {case} pooled stage {i + 1}")
    _check(b, br, f"case {case} branch b")
    assert rel(b.cpu(), GOLD[f"{case}_b"]) < tol(case + "_b")


@pytest.mark.parametrize("case", list(DC.CASES))
def test_model_matches_reference(case, tmp_path):
    from realpdebench_amd.data_normalizer import GaussianNormalizer
    from realpdebench_amd.rollout import autoregressive_rollout
    shape_in, shape_out, p, _ = DC.CASES[case]
    m = _model(case)
    x, y = DC.case_inputs(case)
    with torch.no_grad():
        out = m(x.to(DEV))
        out2 = m(x.to(DEV))
        loss = float(m.train_loss(x.to(DEV), y.to(DEV)).double().mean())
        tr = m.train()(x.to(DEV))                  # no batch-statistics path: train mode still runs on the running statistics
        m.eval()
    e = rel(DC.stored(case, out.cpu()), GOLD[f"{case}_out"])
    el = abs(loss - float(GOLD[f"{case}_loss"])) / float(GOLD[f"{case}_loss"])
    print(f"case {case}: eval Rel-L2 {e:.2e} (tol {tol(case + '_out'):.1e}), loss rel {el:.2e} (tol {tol(case + '_loss'):.1e})")
    assert tuple(out.shape[1:]) == shape_out
    assert torch.equal(out, out2), "two calls must give bit-equal outputs"
    assert torch.equal(out, tr), "train() under no_grad must use the running statistics"
    ero = None
    if case in DC.ROLLOUT_CASES:                   # 3-step rollout through rollout.py with the Gaussian normaliser (eval.py:311-319)
        norm = GaussianNormalizer(*DC.normalizer_stats(case), device=DEV)
        co = shape_out[-1]
        para = x[..., co:].contiguous() if shape_in[-1] != co else None
        xin, _ = norm.preprocess(x, y)
        roll = autoregressive_rollout(m, xin, DC.ROLLOUT_STEPS, normalizer=norm, para_input=para)
        ero = rel(DC.roll_stored(case, roll.cpu()), GOLD[f"{case}_roll"])
        print(f"case {case}: rollout Rel-L2 {ero:.2e} (tol {tol(case + '_roll'):.1e})")
    # checkpoint in the reference's format (train.py: model_state_dict + bookkeeping) loads and the output is unchanged
    path = str(tmp_path / "model_7.pth")
    ref_sd = {k: v.cpu() for k, v in m.state_dict().items()}
    torch.save({"model_state_dict": ref_sd, "train_losses": [1.0], "val_losses": {}, "iteration": 7, "best_iteration": 7,
                "best_val_loss": 0.5}, path)
    m2 = DeepONet(shape_in, shape_out, shape_in[-1], shape_out[-1], p)
    meta = m2.load_checkpoint(path, DEV)
    assert meta["iteration"] == 7
    with torch.no_grad():
        assert torch.equal(m2.eval()(x.to(DEV)), out)
        # a stale trunk cache would hand back the same output after a trunk weight changed
        ref_sd["trunk.fc.4.weight"] = ref_sd["trunk.fc.4.weight"] * 1.5
        m2.load_state_dict(ref_sd)
        assert not torch.equal(m2(x.to(DEV)), out), "the cached trunk output must be rebuilt when a trunk weight changes"
    assert e < tol(case + "_out")
    assert el < tol(case + "_loss")
    if ero is not None:
        assert ero < tol(case + "_roll")


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_native_shape_through_yaml(scenario):
    from realpdebench_amd.model import load_model
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", scenario, "deeponet.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    shape_in, shape_out = tuple(cfg["shape_in"]), tuple(cfg["shape_out"])
    assert list(shape_in) == CFG["native_shapes"][scenario]["shape_in"]
    torch.manual_seed(0)
    m = load_model(One(shape_in, shape_out), device=DEV, **cfg).eval()
    with torch.no_grad():
        out = m(torch.randn(1, *shape_in, device=DEV))
    assert tuple(out.shape) == (1,) + shape_out and bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0


def test_backward_is_refused():
    from realpdebench_amd.trainer import make_trainer
    m = _model("a")
    x, y = (t.to(DEV) for t in DC.case_inputs("a"))
    with pytest.raises(NotImplementedError, match=MSG):
        m.train_loss(x, y)
    with pytest.raises(NotImplementedError, match=MSG):
        m(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match=MSG):
        make_trainer(m.train(), lr=1e-3, num_update=10)


def test_eval_and_train_entrypoints(tmp_path):
    """`python -m realpdebench_amd.eval --config configs/cylinder/deeponet.yaml` (the shipped YAML, results redirected, a bare-weights
    checkpoint): the rollout runs on the synthetic data path.  `realpdebench_amd.train` with the same YAML stops at trainer construction."""
    from realpdebench_amd import eval as ev
    from realpdebench_amd import train as tr
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", "cylinder", "deeponet.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    cfg.update(results_path=str(tmp_path), n_train=2, n_val=2, test_batch_size=2, train_batch_size=2)
    path = tmp_path / "deeponet.yaml"
    path.write_text(yaml.safe_dump(cfg))
    torch.manual_seed(0)
    m = DeepONet(cfg["shape_in"], cfg["shape_out"], cfg["shape_in"][-1], cfg["shape_out"][-1], cfg["p"], cfg["dropout_rate"])
    torch.save(m.state_dict(), str(tmp_path / "model_0.pth"))
    res = ev.main(["--config", str(path), "--checkpoint_path", str(tmp_path / "model_0.pth")])
    assert isinstance(res, dict)
    with pytest.raises(NotImplementedError, match=MSG):
        tr.main(["--config", str(path), "--max_updates", "1"])
