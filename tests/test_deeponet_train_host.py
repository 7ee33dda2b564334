"""DeepONet training step, host side (no GPU): the plain-torch fp64 restatement of the training forward and backward
(tests/deeponet_train_restatement.py) against the reference's vectors (tests/golden/deeponet_train_small.npz, written by
tests/golden/make_golden_deeponet_train.py) and against ``torch.autograd`` of ``torch.nn`` modules, the opt-in surface
(``enable_training()`` / ``hip_training: true``) and the dropout seed rule.

The tolerance rule is in tests/deeponet_train_helpers.py: Rel-L2 < max(1e-5, 4 x the stored selferr); zero-gradient biases:
max |g| <= 64 x ``bias_noise``."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeponet_train_common as TC                # noqa: E402
import deeponet_train_restatement as TR           # noqa: E402
from deeponet_helpers import SCENARIOS, One       # noqa: E402
from deeponet_train_helpers import GOLD, TRAIN_MSG, compare_gradients, compare_outputs, new_model          # noqa: E402
from realpdebench_amd.model import deeponet as M  # noqa: E402

_STEP = {}


def _step(case):
    """The restated fp64 step of a case, computed once and shared."""
    if case not in _STEP:
        x, y = (t.double() for t in TC.case_inputs(case))
        _STEP[case] = TR.step(TC.weights(case), x, y, TC.CASES[case][1], TC.dropout_masks(case))
    return _STEP[case]


@pytest.mark.parametrize("case", list(TC.CASES))
def test_restated_step_matches_reference(case):
    r = _step(case)
    report = []
    misses = compare_outputs(case, r["out"], r["loss"], r["stats"], report)
    ws, wn, gm = compare_gradients(case, r["grads"], report)
    print("\n".join(report))
    print(f"case {case}: worst gradient samples / norm at {ws:.2f} / {wn:.2f} of their bounds")
    assert tuple(r["out"].shape[1:]) == TC.CASES[case][1]
    assert not misses and not gm, (misses, gm)


def test_fixture_covers_the_cases_the_kernels_need():
    c = TC.CASES
    assert any(v[3] >= 2 and v[3] % 2 for v in c.values()) and any(v[3] == 1 for v in c.values())
    assert {v[2] for v in c.values()} == {64, 128, 256}
    assert c["b"][0][-1] == 5 and c["b"][1][-1] == 3 and c["b"][0][0] != c["b"][1][0]
    assert [e[0] for e in M.pooled_extents(*c["b"][0][:3])] == [10, 5, 2, 1]
    pools = [e for v in c.values() for e in M.pooled_extents(*v[0][:3])[:3]]
    assert all(any(e[ax] % 2 for e in pools) for ax in range(3)), "a dropped frame, row and column"
    assert all(e % 2 for e in M.pooled_extents(*c["c"][0][:3])[0])
    last = [M.pooled_extents(*v[0][:3])[3] for v in c.values()]
    assert any(5 in e[1:] for e in last) and any(2 in e[1:] for e in last), "overlapping (5 -> 4) and replicated (2 -> 4) bins"
    assert any((v[1][0] * v[0][1] * v[0][2]) % 32 for v in c.values())
    assert sum(v[4] > 0 for v in c.values()) == 1
    assert all(int(GOLD[f"{k}_seed"]) == TC.SEEDS[k] for k in c)


@pytest.mark.parametrize("n", range(1, 10))
def test_pool_backwards_are_autograds(n):
    """Both pool backwards at In = 1..9 (overlapping, replicated and identity bins; odd extents with a dropped frame / row / column)
    against torch.autograd of the torch.nn modules behind a ReLU.  Values are distinct, so the arg-max is unique."""
    g = torch.Generator().manual_seed(n)
    z = (torch.rand(2, 3, n, 10 - n, 5, generator=g, dtype=torch.float64) - 0.4).requires_grad_()
    pooled = torch.nn.AdaptiveAvgPool3d((1, 4, 4))(torch.relu(z).permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
    go = torch.rand(pooled.shape, generator=g, dtype=torch.float64)
    pooled.backward(go)
    assert torch.allclose(TR.adaptive_pool_bwd(z.detach(), go), z.grad, rtol=0, atol=1e-14)
    if n >= 2 and 10 - n >= 2:
        z = (torch.rand(2, n, 10 - n, n + 1, 5, generator=g, dtype=torch.float64) - 0.4).requires_grad_()
        pooled = torch.nn.MaxPool3d(2)(torch.relu(z).permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
        go = torch.rand(pooled.shape, generator=g, dtype=torch.float64)
        pooled.backward(go)
        got = TR.max_pool_bwd(torch.relu(z.detach()), go)
        assert torch.equal(got, z.grad)
        if n % 2:
            assert not got[:, n - 1].any(), "the frame the flooring pool drops gets no gradient"


def test_max_pool_backward_takes_the_first_maximum_and_nothing_at_zero():
    v = torch.zeros(1, 2, 2, 2, 2, dtype=torch.float64)
    v[0, 0, 1, 0, 0] = v[0, 1, 0, 1, 0] = 3.0                        # channel 0: a tie, (0, 1, 0) comes first in (t, h, w) order
    g = torch.ones(1, 1, 1, 1, 2, dtype=torch.float64)
    gz = TR.max_pool_bwd(v, g)
    assert gz[0, 0, 1, 0, 0] == 1 and gz[..., 0].sum() == 1
    assert not gz[..., 1].any(), "a window whose maximum is 0 (every ReLU closed) passes nothing"


def test_batchnorm_and_conv_backward_are_autograds():
    g = torch.Generator().manual_seed(5)
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1
    x, w, gamma, beta = u(2, 3, 4, 5, 6).requires_grad_(), u(7, 6, 3, 3, 3).requires_grad_(), u(7).requires_grad_(), u(7).requires_grad_()
    bn = torch.nn.BatchNorm3d(7).double().train()
    bn.weight.data, bn.bias.data = gamma.detach().clone(), beta.detach().clone()
    y = torch.nn.functional.conv3d(x.permute(0, 4, 1, 2, 3), w, None, padding=1)
    z = bn(y).permute(0, 2, 3, 4, 1)
    go = u(*z.shape)
    z.backward(go)
    yc = y.detach().permute(0, 2, 3, 4, 1)
    zz, (mean, var, rstd, xhat) = TR.bn_train(yc, gamma.detach(), beta.detach())
    assert torch.allclose(zz, z.detach(), rtol=0, atol=1e-12)
    rm, rv = TR.running_update(torch.zeros(7), torch.ones(7), mean, var, yc.numel() // 7)
    assert torch.allclose(rm, bn.running_mean, rtol=0, atol=1e-14) and torch.allclose(rv, bn.running_var, rtol=0, atol=1e-14)
    dy, dgamma, dbeta = TR.bn_backward(go, gamma.detach(), rstd, xhat)
    dx, dW, _ = TR.conv_bwd(x.detach(), w.detach(), dy)
    assert torch.allclose(dgamma, bn.weight.grad, rtol=0, atol=1e-12) and torch.allclose(dbeta, bn.bias.grad, rtol=0, atol=1e-12)
    assert torch.allclose(dx, x.grad, rtol=0, atol=1e-12) and torch.allclose(dW, w.grad, rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="more than 1 value"):
        TR.batch_stats(torch.zeros(1, 1, 1, 1, 4))


def test_opt_in_surface(monkeypatch):
    from realpdebench_amd.model import load_model
    from realpdebench_amd.trainer import ArenaTrainer, make_trainer
    shape_in, shape_out, p, _, _ = TC.CASES["a"]
    x, y = torch.zeros(1, *shape_in), torch.zeros(1, *shape_out)
    m = new_model("a")
    assert m.batch_independent is True and not m.hip_training and TRAIN_MSG in m.training_unavailable and m.dp_unavailable is None
    # a default instance still refuses everything tests/test_deeponet_host.py lists
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        m.train_loss(x, y)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        m(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        m.eval()(x)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        make_trainer(m, lr=1e-3, num_update=10)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x)
    assert m.enable_training() is m
    assert m.hip_training and m.training_unavailable is None and m.batch_independent is False
    assert "SyncBN" in m.dp_unavailable and "one rank" in m.dp_unavailable
    cls = type(m)
    assert cls.batch_independent is True and TRAIN_MSG in cls.training_unavailable and cls.hip_training is False and cls.dp_unavailable is None, \
        "the class, and every other instance, is unchanged"
    other = new_model("a")
    assert not other.hip_training and TRAIN_MSG in other.training_unavailable
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):       # eval() under grad mode still refuses
        m.eval()(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # train(): the HIP path, which has no CPU fallback
        m.train()(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.train().train_loss(x, y)
    with pytest.raises(ValueError, match="micro_batch"):
        make_trainer(m, lr=1e-3, num_update=10, micro_batch=1)
    tr = make_trainer(m, lr=1e-3, num_update=10)                     # constructed on the CPU as far as that goes: the arenas exist
    assert isinstance(tr, ArenaTrainer) and len(tr.params) == len(list(m.parameters()))
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    with pytest.raises(NotImplementedError, match="SyncBN"):
        make_trainer(new_model("a").enable_training(), lr=1e-3, num_update=10)
    monkeypatch.undo()
    cfg = dict(model_name="deeponet", p=p, dropout_rate=0.1)
    assert not load_model(One(shape_in, shape_out), **cfg).hip_training
    assert not load_model(One(shape_in, shape_out), hip_training=False, **cfg).hip_training
    on = load_model(One(shape_in, shape_out), hip_training=True, **cfg)
    assert on.hip_training and on.batch_independent is False and on.training_unavailable is None and on.dropout_rate == 0.1


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_shipped_yamls_do_not_opt_in(scenario):
    import yaml
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", scenario, "deeponet.yaml")) as fh:
        assert "hip_training" not in yaml.safe_load(fh)


def test_dropout_seed_rule():
    """Distinct seeds for distinct (step, layer, chunk): Philox is keyed on the element index within a GEMM call, so a seed without the
    chunk would repeat one mask in every chunk."""
    seeds = {(s, l, c): M.drop_seed(12345, s, l, c) for s in range(40) for l in range(3) for c in (0, 1, 2, 77, (1 << 22) - 1)}
    assert len(set(seeds.values())) == len(seeds)
    assert all(0 <= v < 1 << 62 for v in seeds.values())
    assert M.drop_seed(12345, 3, 1, 2) == 12345 + (3 << 24) + (1 << 22) + 2
    assert M.drop_seed((1 << 62) - 1, 0, 0, 1) == 0, "wraps inside 62 bits"
    assert M.drop_seed(1, 0, 1, 0) != M.drop_seed(2, 0, 1, 0)
    m = new_model("d").enable_training(seed=99)
    assert m.dropout_seed == 99 and m.dropout_rate == 0.1 and m._drop_step == 0
    assert m._drop(1, 5, 2) == (M.drop_seed(99, 2, 1, 5), 0.9)
    assert new_model("a").enable_training()._drop(1, 0, 0) is None, "rate 0: nn.Dropout is the identity"
