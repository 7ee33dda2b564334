"""DeepONet.set_arith("f16x2") on the GPU.

rpb_don_point_mlp_f16x2 against the fp64 restatement (tests/deeponet_restatement.py) at the shapes and seeded inputs of
tests/test_gpu_deeponet.py::test_point_mlp_kernel -- every p, the widest C_out, tails of 48 and 65 points -- with Rel-L2 < 2e-6, the
project's f16x2 kernel bound (hi planes alone give ~5e-4, so a dropped lo term fails): plain inputs, t scaled by
2^-20 and 2^12, W1 scaled by 2^-10, one zero point among non-zero ones, all-zero t (absolutely, against output_net(0)) and the
adversarial column whose h1 reaches the exponent rule's bound (tests/deeponet_arith_helpers.py); two calls bit-equal; an output view
inside a sentinel-filled buffer.

Whole model, cases of ``deeponet_common.CASES``: against the reference's vectors within ``deeponet_helpers.tol`` and against the default
path (forward < 5e-6, rollout < 2e-5: the bounds of tests/test_gpu_mwt_arith.py); ``set_arith("f32")`` reproduces the default bits; the
planes follow an in-place weight change; the training step is untouched; the native shapes; the eval entry point.

Measured on an MI355X (profiles/deeponet_arith_probe.txt holds the output): kernel 1.0-3.6e-7 over all cases, the zero point alone
0.4-1.0e-7, the adversarial point alone 0.8-4.9e-7, all-zero t 4e-8 absolute; model forward against the default path 0.9-1.1e-6, rollout
1.5-2.1e-6, against the reference's vectors 1.4-1.7e-6 / 2.4e-6; native fsi 1.1e-7, foil 4.9e-8."""
import functools
import os
import sys

import pytest
import torch
import yaml

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeponet_arith_helpers as AH               # noqa: E402
import deeponet_common as DC                      # noqa: E402
import deeponet_restatement as R                  # noqa: E402
import deeponet_train_common as TC                # noqa: E402
import deeponet_train_helpers as TH               # noqa: E402
from deeponet_helpers import GOLD, One, rel, sd_of, tol          # noqa: E402
from realpdebench_amd import ops                  # noqa: E402
from realpdebench_amd.model.deeponet import DeepONet, point_weights_f16x2        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-6
SHAPES = [(64, 3, 4400, 2), (128, 16, 1024, 3), (256, 2, 193, 1)]
VARIANTS = ["plain", "t_small", "t_large", "w1_small", "zero_row", "adversarial"]


@functools.lru_cache(maxsize=None)
def _case(p, cout, N, B, variant):
    """(weights, t, b, the fp64 restatement's output), computed once per case"""
    ws, t, b = AH.point_inputs(p, cout, N, B)
    if variant == "t_small":
        t = t * 2.0 ** -20
    elif variant == "t_large":
        t = t * 2.0 ** 12
    elif variant == "w1_small":
        ws = (ws[0] * 2.0 ** -10,) + ws[1:]
    elif variant == "zero_row":
        t = t.clone()
        t[N - 2] = 0                                   # in the tail tile, between non-zero points
    elif variant == "zero":
        t = torch.zeros_like(t)
    elif variant == "adversarial":
        t, b = AH.adversarial(ws[0], t, b, row=N - 1)
    return ws, t, b, R.point_mlp(AH.sd_of(ws), t.double(), b.double())


def _run(ws, t, b, out=None):
    pw = point_weights_f16x2(*(w.to(DEV) for w in ws))
    return DeepONet.k_point_mlp_f16x2(t.to(DEV), b.to(DEV), pw, out=out)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("p,cout,N,B", SHAPES)
def test_point_mlp_f16x2_kernel(p, cout, N, B, variant):
    ws, t, b, want = _case(p, cout, N, B, variant)
    out = _run(ws, t, b)
    assert tuple(out.shape) == (B, N, cout)
    assert torch.equal(out, _run(ws, t, b)), "two calls must give bit-equal outputs"
    e = rel(out.cpu(), want)
    print(f"point_mlp_f16x2 p={p} C_out={cout} N={N} B={B} [{variant}]: Rel-L2 {e:.2e} (bound {BOUND:.0e})")
    assert bool(torch.isfinite(out).all())
    assert e < BOUND
    if variant in ("zero_row", "adversarial"):
        # The one special point on its own (a Rel-L2 over all points would hide it), against its own norm or, where cancellation in the
        # last layer leaves that smaller, the tensor's RMS point norm: a point's error scales with its hidden activations, not its output.
        n = N - 2 if variant == "zero_row" else N - 1
        s = 0 if variant == "adversarial" else slice(None)
        got_n, want_n = out[s, n].cpu().double().reshape(-1, cout), want[s, n].reshape(-1, cout)
        rms = float(want.reshape(-1, cout).norm(dim=1).pow(2).mean().sqrt())
        ep = float(((got_n - want_n).norm(dim=1) / want_n.norm(dim=1).clamp_min(rms)).max())
        print(f"  point {n} alone: {ep:.2e}")
        assert ep < BOUND


@pytest.mark.parametrize("p,cout,N,B", SHAPES)
def test_point_mlp_f16x2_all_zero_input(p, cout, N, B):
    ws, t, b, want = _case(p, cout, N, B, "zero")
    out = _run(ws, t, b).cpu().double()
    d = float((out - want).abs().max())
    print(f"all-zero t, p={p}: max |out - output_net(0)| {d:.2e} (|output_net(0)| max {float(want.abs().max()):.2e})")
    assert d < BOUND * float(want.abs().max())


def test_point_mlp_f16x2_writes_only_its_output():
    """The output as a view inside a larger buffer: the sentinels before and after it stay."""
    p, cout, N, B = SHAPES[2]                          # N = 193: a tail tile of 65 points, C_out = 2
    ws, t, b, want = _case(p, cout, N, B, "plain")
    pad, n = 1024, B * N * cout
    buf = torch.full((pad + n + pad,), -7.5, device=DEV)
    _run(ws, t, b, out=ops.Sub(buf, pad))
    torch.cuda.synchronize()
    assert bool((buf[:pad] == -7.5).all()) and bool((buf[pad + n:] == -7.5).all())
    assert rel(buf[pad:pad + n].view(B, N, cout).cpu(), want) < BOUND


# ----------------------------------------------------------------------------------------------------------- whole model
def _model(case):
    shape_in, shape_out, p, _ = DC.CASES[case]
    m = DeepONet(shape_in, shape_out, shape_in[-1], shape_out[-1], p)
    m.load_state_dict(sd_of(case))
    return m.to(DEV).eval()


@pytest.mark.parametrize("case", list(DC.CASES))
def test_model_f16x2_matches_reference_and_default(case):
    from realpdebench_amd.data_normalizer import GaussianNormalizer
    from realpdebench_amd.rollout import autoregressive_rollout
    shape_in, shape_out, p, _ = DC.CASES[case]
    m = _model(case)
    x, y = DC.case_inputs(case)

    def rollout():
        norm = GaussianNormalizer(*DC.normalizer_stats(case), device=DEV)
        co = shape_out[-1]
        para = x[..., co:].contiguous() if shape_in[-1] != co else None
        xin, _ = norm.preprocess(x, y)
        return autoregressive_rollout(m, xin, DC.ROLLOUT_STEPS, normalizer=norm, para_input=para)

    with torch.no_grad():
        out0 = m(x.to(DEV))
        loss0 = float(m.train_loss(x.to(DEV), y.to(DEV)).double().mean())
        roll0 = rollout() if case in DC.ROLLOUT_CASES else None
        assert m.set_arith("f16x2") is m
        out = m(x.to(DEV))
        assert torch.equal(m(x.to(DEV)), out), "two f16x2 calls must give bit-equal outputs"
        loss = float(m.train_loss(x.to(DEV), y.to(DEV)).double().mean())
        roll = rollout() if case in DC.ROLLOUT_CASES else None
        assert torch.equal(m.set_arith("f32")(x.to(DEV)), out0), "set_arith('f32') must reproduce the default output bit for bit"
        m.set_arith("f16x2").output_net[3].weight.mul_(1.25)      # in place: same storage, new version -> the planes are rebuilt
        out_w = m(x.to(DEV))
        want_w = m.set_arith("f32")(x.to(DEV))
    e = rel(DC.stored(case, out.cpu()), GOLD[f"{case}_out"])
    el = abs(loss - float(GOLD[f"{case}_loss"])) / float(GOLD[f"{case}_loss"])
    d, dw = rel(out.cpu(), out0.cpu()), rel(out_w.cpu(), want_w.cpu())
    print(f"case {case} [f16x2]: eval Rel-L2 {e:.2e} (tol {tol(case + '_out'):.1e}), loss rel {el:.2e} (tol {tol(case + '_loss'):.1e}), "
          f"loss against the default {abs(loss - loss0) / loss0:.2e}, forward against the default path {d:.2e} (bound 5e-6), after the "
          f"weight change {dw:.2e}")
    assert tuple(out.shape[1:]) == shape_out
    assert not torch.equal(out, out0), "the switch must reach the kernels"
    assert not torch.equal(out_w, out), "the planes must be rebuilt when an output_net weight changes in place"
    assert e < tol(case + "_out")
    assert el < tol(case + "_loss")
    assert abs(loss - loss0) / loss0 < 5e-6
    assert d < 5e-6 and dw < 5e-6
    if roll is not None:
        ero, dr = rel(DC.roll_stored(case, roll.cpu()), GOLD[f"{case}_roll"]), rel(roll.cpu(), roll0.cpu())
        print(f"case {case} [f16x2]: rollout Rel-L2 {ero:.2e} (tol {tol(case + '_roll'):.1e}), against the default path {dr:.2e} (bound 2e-5)")
        assert ero < tol(case + "_roll")
        assert dr < 2e-5


def test_training_step_is_untouched_by_set_arith():
    """With enable_training(): one training step (dropout on, one seed) under "f16x2" gives the default's loss and every gradient bit
    for bit; the no_grad forward of the same instance in eval() mode takes the selected arithmetic."""
    case = "d"
    assert TC.CASES[case][4] > 0
    x, y = (t.to(DEV) for t in TC.case_inputs(case))
    res = []
    for arith in ("f32", "f16x2"):
        m = TH.new_model(case).to(DEV).enable_training(seed=77).train().set_arith(arith)
        loss = m.train_loss(x, y).mean()
        loss.backward()
        with torch.no_grad():
            ev = m.eval()(x)
        res.append((loss.detach(), {n: p.grad for n, p in m.named_parameters()}, {k: v.clone() for k, v in m.state_dict().items()}, ev))
    (l0, g0, s0, e0), (l1, g1, s1, e1) = res
    assert torch.equal(l0, l1)
    assert sum(g is not None for g in g0.values()) > 20
    for n in g0:
        assert (g0[n] is None and g1[n] is None) or torch.equal(g0[n], g1[n]), n
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
    d = rel(e1.cpu(), e0.cpu())
    print(f"eval forward of the enabled instance, f16x2 against f32: {d:.2e}")
    assert not torch.equal(e0, e1) and d < 5e-6


@pytest.mark.parametrize("scenario", ["fsi", "foil"])
def test_native_shape_through_yaml_f16x2(scenario):
    """p = 64 (fsi) and p = 256 (foil) at B = 1, from the shipped YAMLs"""
    from realpdebench_amd.model import load_model
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", scenario, "deeponet.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    shape_in, shape_out = tuple(cfg["shape_in"]), tuple(cfg["shape_out"])
    assert cfg["p"] == {"fsi": 64, "foil": 256}[scenario] and "eval_arith" not in cfg
    torch.manual_seed(0)
    m = load_model(One(shape_in, shape_out), device=DEV, **cfg).eval()
    x = torch.randn(1, *shape_in, device=DEV)
    with torch.no_grad():
        want = m(x)
        out = m.set_arith("f16x2")(x)
    d = rel(out.cpu(), want.cpu())
    print(f"{scenario} (p = {cfg['p']}), B = 1: f16x2 against the default path {d:.2e} (bound 5e-6)")
    assert tuple(out.shape) == (1,) + shape_out and bool(torch.isfinite(out).all())
    assert not torch.equal(out, want) and d < 5e-6


def test_eval_entrypoint_takes_eval_arith_deeponet(tmp_path):
    """`python -m realpdebench_amd.eval` with `eval_arith: f16x2` on a small synthetic DeepONet YAML: the metrics agree with the default
    arithmetic's to 1e-4 relative; a value the model rejects ends the run with its ValueError (a non-zero exit of the command)."""
    from realpdebench_amd import eval as ev
    shape_in, shape_out, p, _ = DC.CASES["a"]
    cfg = dict(exp_name="t", gpu=0, seed=0, results_path=str(tmp_path), dataset_name="synthetic", dataset_root="", num_workers=0,
               normalizer="none", shape_in=list(shape_in), shape_out=list(shape_out), n_train=4, n_val=4, model_name="deeponet",
               checkpoint_path="", p=p, dropout_rate=0.1, is_use_tb=None, scheduler="cosine", step_size=10, num_update=100,
               train_batch_size=2, test_batch_size=2, lr=1e-3, clip_grad_norm=0.0, N_autoregressive=1)
    ck = str(tmp_path / "model_0.pth")
    torch.save(sd_of("a"), ck)
    path = tmp_path / "deeponet.yaml"
    path.write_text(yaml.safe_dump(cfg))
    base = ev.main(["--config", str(path), "--checkpoint_path", ck])
    path2 = tmp_path / "deeponet_f16x2.yaml"
    path2.write_text(yaml.safe_dump(dict(cfg, eval_arith="f16x2")))
    fast = ev.main(["--config", str(path2), "--checkpoint_path", ck])
    assert set(base) == set(fast)
    n = 0
    for k in base:
        if not isinstance(base[k], (int, float)):
            assert base[k] == fast[k]
            continue
        a, b = float(base[k]), float(fast[k])
        if a == a and b == b:
            assert abs(a - b) <= 1e-4 * max(abs(a), 1e-12), (k, a, b)
            n += 1
    assert n >= 5
    path3 = tmp_path / "bad.yaml"
    path3.write_text(yaml.safe_dump(dict(cfg, eval_arith="fp8")))
    with pytest.raises((ValueError, SystemExit)) as exc:
        ev.main(["--config", str(path3), "--checkpoint_path", ck])
    assert not (isinstance(exc.value, SystemExit) and exc.value.code in (0, None))
