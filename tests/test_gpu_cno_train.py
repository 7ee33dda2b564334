"""CNO3d training step on the GPU (opt-in: ``CNO3d.enable_training()``).

``train_loss(x, y).mean().backward()`` on an enabled model in ``train()`` against the reference's fp64 run
(tests/golden/cno_train_small.npz), cases d, g, h, c, with the rule of tests/cno_helpers.py: Rel-L2 < max(1e-5, 4 x the reference's own
fp32-vs-fp64 deviation); the factor 4 allows for another summation order and the bf16x3 split.  Output, loss, every running statistic,
every sampled gradient and every gradient norm of the parameters with a non-zero gradient follow that rule.  The 31 convolution biases
in front of a BatchNorm have a zero gradient; the reference's fp32 autograd returns rounding noise there (``bias_noise``) and so does
this port: max |g| <= 64 x ``bias_noise`` -- the noise of another summation order is not reproducible, only its scale is, and the bound
still sits five orders of magnitude below the smallest real gradient.

Measured on an MI355X (profiles/cno_train_pytest.txt holds the full output).  Output 1.8-1.9e-6, loss < 1e-7, running statistics 1.3-1.6e-7,
zero-gradient biases 0.6-1.9e-8 (bounds 3.7-5.4e-7), every sampled gradient 1-5e-6 (worst 0.48-0.52 of its bound in the four cases),
every gradient norm below 0.10 of its bound, Adam losses 6e-8 and 6e-7.

Why seven data gradients run on the exact-fp32 implicit GEMM (model/cno.py ``EXACT_DGRAD``).  With every data gradient on the bf16x3
kernel this test failed for cases d and h on the BatchNorm shift gradients at the end of the neck's backward residual chain
(res_nets.6 / 7 / 8.batch_norm2.bias: 1.17e-5 / 1.30e-5 / 1.64e-5 in d, 1.03e-5 / 1.15e-5 / 1.03e-5 in h, against 1e-5; g and c at 0.86
and 0.95 of the bound), with every other gradient at 2-4e-6.  Such a gradient is a column sum of the data gradient, and a column sum
sees a per-channel BIAS of the error sqrt(M) times stronger than its unbiased part: unbiased noise of the convolution's measured size
(3-5e-7 per layer) injected into the fp64 restatement moves these tensors by 3e-6 like all the others, while the GPU moved them by 6e-6
at the first block of the chain and more with every block.  tests/test_gpu_cno_train_kernels.py prints the bias: the error of
rpb_cno_conv3x as a data gradient has a column mean 2.8-4.1 times what unbiased rounding leaves (0.8); sum_m dy of the BatchNorm
backward is at 2.3-3.2 units of ONE rounding, so the row kernels are not the source.  Only the gradients that ADD INTO the chain carry
the bias from block to block (every other path goes through a BatchNorm backward, which removes a per-channel offset), so those seven
-- ED_expansion.3 and convolution1 of the six neck blocks -- take the exact kernel; the same six tensors then measure 2.8-4.2e-6."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cno_train_common as TC                     # noqa: E402
from cno_train_helpers import GOLD, TRAIN_MSG, compare_gradients, new_model, rel, stat_slices, tol          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _enabled(case):
    return new_model(case).to(DEV).enable_training().train()


def _named_grads(m):
    return {n: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("case", list(TC.CASES))
def test_training_step_matches_reference(case):
    shape_in, shape_out, _ = TC.CASES[case]
    m = _enabled(case)
    x, y = (t.to(DEV) for t in TC.case_inputs(case))
    seen, forward = {}, m.forward
    m.forward = lambda x_: seen.__setitem__("out", forward(x_)) or seen["out"]      # train_loss calls self.forward: one forward, its output kept
    loss = m.train_loss(x, y).mean()
    del m.forward
    loss.backward()
    out = seen["out"].detach()
    real, zero_bias, none = TC.param_names(case)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    eo = rel(out.cpu(), GOLD[f"{case}_out"])
    el = abs(float(loss.detach()) - float(GOLD[f"{case}_loss"])) / float(GOLD[f"{case}_loss"])
    print(f"case {case}: output Rel-L2 {eo:.2e} (tol {tol(GOLD[case + '_out_selferr']):.1e}), loss rel {el:.2e} "
          f"(tol {tol(GOLD[case + '_loss_selferr']):.1e})")
    worst_stat = 0.0
    for j, (k, sl) in enumerate(stat_slices(case).items()):
        e = rel(sd[k], GOLD[f"{case}_stats"][sl])
        worst_stat = max(worst_stat, e)
        assert e < tol(GOLD[f"{case}_stats_selferr"][j]), (k, e)
    print(f"case {case}: worst running statistic Rel-L2 {worst_stat:.2e} (tol 1.0e-05)")
    report = []
    *worst, misses = compare_gradients(case, _named_grads(m), tol, report)
    print("\n".join(report))
    print(f"case {case}: worst gradient samples / norm at {worst[0]:.2f} / {worst[1]:.2f} of their bounds")
    noise, bound = max(float(_named_grads(m)[n].abs().max()) for n in zero_bias), 64 * float(GOLD[f"{case}_bias_noise"])
    print(f"case {case}: zero-gradient biases max |g| {noise:.1e} (bound {bound:.1e}; smallest real gradient norm "
          f"{float(GOLD[case + '_gnorm'].min()):.1e})")
    assert tuple(out.shape[1:]) == shape_out
    assert eo < tol(GOLD[f"{case}_out_selferr"])
    assert el < tol(GOLD[f"{case}_loss_selferr"])
    assert not misses, misses
    assert noise <= bound
    tracked = [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked") and not k.startswith("decoder_inv.3.")]
    assert len(tracked) == 31 and all(v == TC.TRACKED_BEFORE + 1 for v in tracked), "num_batches_tracked == 8"
    assert int(sd["decoder_inv.3.batch_norm.num_batches_tracked"]) == TC.TRACKED_BEFORE
    assert all(_named_grads(m)[n] is None for n in none), "decoder_inv.3 never runs: grad is None"
    # after that one training forward, eval() equals a fresh eval model loaded with the updated state_dict, bit for bit: the layout
    # cache saw the new running statistics
    with torch.no_grad():
        ev = m.eval()(x)
        fresh = new_model(case)
        fresh.load_state_dict(sd)
        assert torch.equal(fresh.to(DEV).eval()(x), ev)
        stale = new_model(case).to(DEV).eval()(x)
    assert not torch.equal(stale, ev), "the running statistics moved, so must the eval output"


def test_backward_twice_is_bit_equal():
    m = _enabled("d")
    x, y = (t.to(DEV) for t in TC.case_inputs("d"))
    state = m._new_state()
    out = m._forward_hip(x, state)
    g_out = (2.0 / out.numel()) * (out - y)
    first = m._backward_hip(state, g_out.contiguous())
    first = {p: g.clone() for p, g in first.items()}
    again = m._backward_hip(state, g_out.contiguous())
    assert len(first) == len(again) == 2 * 35 + 2 * 31
    for p, g in first.items():
        assert torch.equal(g, again[p])
    # ... and a second model gives the same forward and gradients (no atomics, fixed summation order)
    m2 = _enabled("d")
    m2.train_loss(x, y).mean().backward()
    m3 = _enabled("d")
    m3.train_loss(x, y).mean().backward()
    for (n, p), q in zip(m2.named_parameters(), m3.parameters()):
        assert (p.grad is None and q.grad is None) or torch.equal(p.grad, q.grad), n
    for (n, b), c in zip(m2.named_buffers(), m3.buffers()):
        assert torch.equal(b, c), n


def test_two_adam_steps_through_make_trainer(tmp_path):
    from realpdebench_amd.trainer import ArenaTrainer, make_trainer
    case = TC.ADAM_CASE
    m, twin = _enabled(case), _enabled(case)
    tr = make_trainer(m, lr=TC.ADAM_LR, num_update=TC.ADAM_T_MAX)
    assert isinstance(tr, ArenaTrainer)
    opt = torch.optim.Adam(twin.parameters(), lr=TC.ADAM_LR)
    for k in range(TC.ADAM_STEPS):
        x, y = (t.to(DEV) for t in TC.case_inputs(case, k))
        loss = float(tr.step(x, y))
        e, bound = abs(loss - float(GOLD[f"{case}_adam_loss"][k])) / float(GOLD[f"{case}_adam_loss"][k]), tol(GOLD[f"{case}_adam_loss_selferr"][k])
        print(f"step {k}: loss {loss:.8f} rel {e:.2e} (tol {bound:.1e})")
        assert e < bound
        if k == 0:
            # the arena step == torch.optim.Adam on a twin that received the port's own gradients (the comparison of tests/test_gpu_dp.py)
            twin.train_loss(x, y).mean().backward()
            opt.step()
            for (n, p), q in zip(m.named_parameters(), twin.parameters()):
                assert float((p.data - q.data).abs().max()) <= 0.05 * TC.ADAM_LR, n
    # enabled, stepped, saved, reloaded: the reference's 232 keys round-trip
    path = str(tmp_path / "model_2.pth")
    ck = tr.checkpoint({"train_losses": [1.0], "val_losses": {}, "best_iteration": 2, "best_val_loss": 0.5})
    assert len(ck["model_state_dict"]) == 232 and ck["iteration"] == TC.ADAM_STEPS
    torch.save({k: ({n: v.cpu() for n, v in val.items()} if k == "model_state_dict" else val) for k, val in ck.items()}, path)
    m2 = new_model(case)
    meta = m2.load_checkpoint(path, DEV)
    assert meta["iteration"] == TC.ADAM_STEPS
    sd, sd2 = m.state_dict(), m2.state_dict()
    assert list(sd) == list(sd2) == list(TC.weights(case))
    for k in sd:
        assert torch.equal(sd[k], sd2[k]) and sd[k].dtype == TC.weights(case)[k].dtype, k
    x = TC.case_inputs(case)[0].to(DEV)
    with torch.no_grad():
        assert torch.equal(m.eval()(x), m2.eval()(x))


def test_refusals_and_opt_in():
    from realpdebench_amd.trainer import make_trainer
    x, y = (t.to(DEV) for t in TC.case_inputs("c"))
    m = new_model("c").to(DEV)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):       # the default model still refuses
        m.train().train_loss(x, y)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        m(x)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        make_trainer(m, lr=1e-3, num_update=10)
    m.enable_training()
    with pytest.raises(ValueError, match="micro_batch"):
        make_trainer(m, lr=1e-3, num_update=10, micro_batch=1)
    with pytest.raises(NotImplementedError, match="no input gradient"):
        m.train()(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):       # eval() under grad mode still refuses
        m.eval()(x)
    with torch.no_grad():                                            # train() without a graph: batch statistics, statistics updated
        before = m.res_nets[8].batch_norm2.running_mean.clone()
        a = m.train()(x)
        assert not torch.equal(m.res_nets[8].batch_norm2.running_mean, before)
        assert not torch.equal(a, m.eval()(x))
