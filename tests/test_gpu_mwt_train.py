"""MWT3d opt-in training step on the MI355X against the reference's fp64 run (tests/golden/mwt_train_small.npz, written by
tests/golden/make_golden_mwt_train.py): loss and every gradient within the project's MWT rule max(1e-5, 4 x selferr) per tensor (norm and
128 stored samples each; the fixture's seeds keep every ReLU input of the reference at least three times the reference's own fp32 error
from zero, so no gate is ambiguous); the parameters without a gradient; bit-equality of the training forward with the eval forward and
of two backward passes; two Adam steps through ``make_trainer``; micro-batching; the arithmetic switch; eval before and after opting in."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mwt_common as MC                           # noqa: E402
import mwt_train_common as TC                     # noqa: E402
from mwt_train_helpers import GOLD, TRAIN_MSG, compare_gradients, new_model, rel, tol      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def step_grads(m, x, y):
    for p in m.parameters():
        p.grad = None
    loss = m.train_loss(x, y).mean()
    loss.backward()
    return loss.detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def runs():
    """per case: the enabled model in train() mode, its inputs, the loss and the gradients of one backward"""
    out = {}
    for case in TC.CASES:
        m = new_model(case, DEV).enable_training().train()
        x, y = (t.to(DEV) for t in TC.case_inputs(case))
        loss, grads = step_grads(m, x, y)
        out[case] = dict(m=m, x=x, y=y, loss=loss, grads=grads)
    return out


@pytest.mark.parametrize("case", list(TC.CASES))
def test_loss_and_gradients_match_reference(runs, case):
    r = runs[case]
    e = abs(float(r["loss"]) - float(GOLD[f"{case}_loss"])) / float(GOLD[f"{case}_loss"])
    print(f"case {case}: loss rel {e:.2e} (tol {tol(GOLD[case + '_loss_selferr']):.1e})")
    assert e < tol(GOLD[f"{case}_loss_selferr"])
    none = [str(n) for n in GOLD[f"{case}_none"]]
    assert sorted(n for n, p in r["m"].named_parameters() if n not in r["grads"]) == sorted(none), "exactly BN.* has no gradient"
    for n, g in r["grads"].items():
        p = dict(r["m"].named_parameters())[n]
        assert g.dtype == p.dtype and g.shape == p.shape, n
    misses = compare_gradients(case, r["grads"])
    assert not misses, misses


@pytest.mark.parametrize("case", list(TC.CASES))
def test_training_forward_is_bit_equal_to_eval_and_backward_repeats(runs, case):
    m, x, y = runs[case]["m"], runs[case]["x"], runs[case]["y"]
    with torch.no_grad():
        ev = m.eval()(x)
        m.train()
        state = m._new_state()
        tr = m._forward_hip(x, state)
        assert torch.equal(tr, ev), "the keep-variants are the eval kernels with one more store"
        assert torch.equal(m(x), ev), "train() under no_grad records nothing and gives the same output"
        g = (2 * (tr - y) / tr.numel()).contiguous()
        a, b = m._backward_hip(state, g), m._backward_hip(state, g)
    assert set(a) == set(b)
    for p in a:
        assert torch.equal(torch.view_as_real(a[p]) if a[p].is_complex() else a[p],
                           torch.view_as_real(b[p]) if b[p].is_complex() else b[p]), "two backward passes are bit-equal"
    names = {p: n for n, p in m.named_parameters()}
    for p, t in a.items():              # and they are what autograd delivered (which forms 2 (pred - y) / N in another order: not bit-equal)
        ref = runs[case]["grads"][names[p]]
        if bool(ref.abs().sum()):
            assert rel(TC.flat_real(t).cpu(), TC.flat_real(ref).cpu()) < 1e-6, names[p]
        else:
            assert not bool(t.abs().sum()), names[p]


class _One(torch.utils.data.Dataset):
    def __init__(self, shape_in, shape_out):
        self.s = (torch.zeros(*shape_in), torch.zeros(*shape_out))

    def __len__(self):
        return 1

    def __getitem__(self, i):
        return self.s


def configured(case, **extra):
    from realpdebench_amd.model import load_model
    shape_in, shape_out = TC.CASES[case]
    cfg = dict(model_name="mwt", k=MC.K, alpha=MC.ALPHA, c=MC.C, nCZ=TC.NCZ, L=0, base="legendre", config="mwt.yaml", **extra)
    m = load_model(_One(shape_in, shape_out), device=DEV, **cfg)
    m.load_state_dict(TC.weights(case), strict=False)
    return m


def unreached(case):
    """[4][m][m][m] bool: spectral weight entries no level's corner table maps a bin to"""
    import math
    from realpdebench_amd.model.mwt import corner_table
    _, H, W, _ = TC.CASES[case][0]
    hit = torch.zeros(4 * MC.ALPHA ** 3, dtype=torch.bool)
    for i in range(int(math.log2(H))):
        hit[torch.from_numpy(corner_table(H >> (i + 1), W >> (i + 1), MC.ALPHA)[2]).long()] = True
    return ~hit.view(4, MC.ALPHA, MC.ALPHA, MC.ALPHA)


def test_two_adam_steps_through_make_trainer(tmp_path):
    from realpdebench_amd.trainer import make_trainer
    case = TC.ADAM_CASE
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):       # the same config without the key still stops at trainer construction
        make_trainer(configured(case), lr=TC.ADAM_LR, num_update=TC.ADAM_T_MAX)
    m = configured(case, hip_training=True)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    tr = make_trainer(m, lr=TC.ADAM_LR, num_update=TC.ADAM_T_MAX)
    losses = []
    for k in range(TC.ADAM_STEPS):
        x, y = (t.to(DEV) for t in TC.case_inputs(case, k))
        losses.append(float(tr.step(x, y)))
    for k, (got, want, se) in enumerate(zip(losses, GOLD[f"{case}_adam_loss"], GOLD[f"{case}_adam_loss_selferr"])):
        e = abs(got - float(want)) / float(want)
        print(f"adam step {k}: loss {got:.7f} reference {float(want):.7f} rel {e:.2e} (tol {tol(se):.1e})")
        assert e < tol(se)
    after = m.state_dict()
    shapes = MC.state_shapes(*TC.CASES[case], TC.NCZ)
    assert list(after) == list(shapes)
    dead = unreached(case).to(DEV)
    assert bool(dead.any())
    for k, v in after.items():
        assert tuple(v.shape) == tuple(shapes[k][0]) and v.dtype == shapes[k][1], k
        same = torch.equal(torch.view_as_real(v) if v.is_complex() else v, torch.view_as_real(before[k]) if v.is_complex() else before[k])
        if k.startswith("BN.") or k.rsplit(".", 1)[-1] in MC._BUFFERS:
            assert same, f"{k} has no gradient and must not move"
        elif ".A.weights" in k:
            j = int(k[-1]) - 1
            moved = (torch.view_as_real(v) != torch.view_as_real(before[k])).any(-1).any(0).any(0)       # [x][y][t]
            assert not bool((moved & dead[j]).any()), f"{k}: an entry no level reaches moved"
            assert bool(moved[~dead[j]].all()), f"{k}: a reached entry did not move"
        else:
            assert not same, f"{k} did not move"
    path = str(tmp_path / "ck.pth")
    torch.save(tr.checkpoint(), path)
    twin = configured(case, hip_training=True)
    meta = twin.load_checkpoint(path, DEV)
    assert meta["iteration"] == TC.ADAM_STEPS
    for k, v in twin.state_dict().items():
        assert torch.equal(torch.view_as_real(v) if v.is_complex() else v, torch.view_as_real(after[k]) if v.is_complex() else after[k]), k
    x, _ = TC.case_inputs(case)
    with torch.no_grad():
        assert torch.equal(twin.eval()(x.to(DEV)), m.eval()(x.to(DEV)))


def test_micro_batch_gives_the_full_steps_gradients(runs):
    from realpdebench_amd.trainer import ArenaTrainer
    case = "q"
    x, y = runs[case]["x"], runs[case]["y"]
    m = new_model(case, DEV).enable_training()
    tr = ArenaTrainer(m, lr=0.0, num_update=10, micro_batch=1)      # lr 0: the step only fills the gradient arena
    loss = tr.step(x, y)
    assert abs(float(loss) - float(runs[case]["loss"])) < 1e-6 * float(runs[case]["loss"])
    names = {p: n for n, p in m.named_parameters()}
    for p, g in tr.mean_grads().items():
        n = names[p]
        if n.startswith("BN."):
            assert not bool(g.any())
            continue
        ref = runs[case]["grads"][n]
        if not bool(ref.abs().sum()):
            assert not bool(g.abs().sum()), n
            continue
        assert rel(torch.view_as_real(g).cpu() if g.is_complex() else g.cpu(),
                   torch.view_as_real(ref).cpu() if ref.is_complex() else ref.cpu()) < 1e-6, n


def test_training_runs_the_f32_kernels_under_every_arith(runs):
    case = "r"
    m = new_model(case, DEV).enable_training().train().set_arith("f16x2")
    loss, grads = step_grads(m, runs[case]["x"], runs[case]["y"])
    assert torch.equal(loss, runs[case]["loss"])
    for n, g in grads.items():
        ref = runs[case]["grads"][n]
        assert torch.equal(torch.view_as_real(g) if g.is_complex() else g, torch.view_as_real(ref) if ref.is_complex() else ref), n
    with torch.no_grad():                                           # while the eval forward does follow the switch
        x = runs[case]["x"]
        assert not torch.equal(m.eval()(x), runs[case]["m"].eval()(x))
    runs[case]["m"].train()


def test_eval_is_bit_equal_before_and_after_opting_in():
    case = "p"
    m = new_model(case, DEV)
    x = TC.case_inputs(case)[0].to(DEV)
    with torch.no_grad():
        before = m.eval()(x)
        m.enable_training()
        assert torch.equal(m.eval()(x), before)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):       # eval() under grad mode still refuses
        m.eval()(x)
