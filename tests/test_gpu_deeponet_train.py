"""DeepONet training step on the GPU (opt-in: ``DeepONet.enable_training()``).

``train_loss(x, y).mean().backward()`` on an enabled model in ``train()`` against the reference's fp64 run
(tests/golden/deeponet_train_small.npz), cases a, b, c (dropout rate 0) and d (rate 0.1, explicit seeded masks), with the rule of
tests/deeponet_train_helpers.py: Rel-L2 < max(1e-5, 4 x the reference's own fp32-vs-fp64 deviation); the factor 4 allows for another
summation order and the bf16x3 split.  Output samples, loss, every running statistic, every sampled gradient and every gradient norm
follow that rule.  The four convolution biases in front of a BatchNorm have a zero gradient; the reference's fp32 autograd returns
rounding noise there (``bias_noise``) and so does this port: max |g| <= 64 x ``bias_noise``.

In-kernel dropout (Philox in the GEMM epilogue) is checked against the explicit-mask path: the masks the step used are materialised
with rpb_dropout_mul on ones from the recorded seeds and fed back through the ``mask`` argument; the two routes multiply the same fp32
value by the same fp32 factor (0 or 1 / keep) in the same epilogue, so outputs and gradients are required to be bit-equal.

Measured on an MI355X (profiles/deeponet_train_pytest.txt holds the full output).  Output 1.7-2.0e-6, loss 0.2-1.0e-6, running statistics
0.5-1.0e-7, zero-gradient biases 0.5-10e-6 (bounds 0.3-4e-4), every sampled gradient 1-7e-6 (worst 0.31 / 0.45 / 0.60 / 0.33 of its bound
in cases a / b / c / d), every gradient norm below 0.19 of its bound, Adam losses 8e-7 and 7e-7.  In-kernel against explicit-mask
dropout: output and every gradient bit-equal (max |diff| 0); kept fractions 0.9023 / 0.8996 / 0.8991.  Every data gradient runs on
the bf16x3 kernels (rpb_gemm3x, rpb_conv3x): none of the column-sum gradients (BatchNorm shifts, gb, gt) needed the exact path.

The trunk of the training forward (three rpb_gemm3x launches over the zero-padded coordinate matrix) against rpb_don_trunk at the
bound of tests/test_gpu_deeponet.py::test_trunk_kernel (Rel-L2 < 1e-5): measured 2.5e-7 / 2.7e-7 / 2.8e-7 at p = 64 / 128 / 256
(1.5-2.1e-7 from fp64, where rpb_don_trunk itself is at 1.9e-7).  The step in small chunks against the one-chunk
step, every parameter under the tolerance rule: measured worst at 0.068 (case b, chunks of 350) and 0.041 (case d, chunks of 60) of its bound.

The dropout case is small for the margin argument of deeponet_train_common.CASES."""
import glob
import os
import sys

import pytest
import torch
import yaml

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeponet_train_common as TC                # noqa: E402
from deeponet_train_helpers import GOLD, TRAIN_MSG, compare_gradients, compare_outputs, new_model, rel, tol          # noqa: E402
from realpdebench_amd import ops                  # noqa: E402
from realpdebench_amd.model import deeponet as M  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _enabled(case, seed=1234):
    m = new_model(case).to(DEV).enable_training(seed=seed).train()
    masks = TC.dropout_masks(case)
    if masks is not None:
        m._mask_override = [t.to(DEV) for t in masks]
    return m


def _named_grads(m):
    return {n: p.grad for n, p in m.named_parameters()}


def _step(m, x, y):
    """One forward / backward; returns (output, loss) with the gradients left on the parameters."""
    seen, forward = {}, m.forward
    m.forward = lambda x_: seen.__setitem__("out", forward(x_)) or seen["out"]      # train_loss calls self.forward: one forward, its output kept
    loss = m.train_loss(x, y).mean()
    del m.forward
    loss.backward()
    return seen["out"].detach(), loss.detach()


@pytest.mark.parametrize("case", list(TC.CASES))
def test_training_step_matches_reference(case):
    """Cases a, b, c at dropout rate 0; case d: the explicit-mask dropout case."""
    m = _enabled(case)
    x, y = (t.to(DEV) for t in TC.case_inputs(case))
    out, loss = _step(m, x, y)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    report = []
    misses = compare_outputs(case, out, loss, sd, report)
    ws, wn, gm = compare_gradients(case, _named_grads(m), report)
    print("\n".join(report))
    print(f"case {case}: worst gradient samples / norm at {ws:.2f} / {wn:.2f} of their bounds")
    assert tuple(out.shape[1:]) == TC.CASES[case][1]
    assert not misses, misses
    assert not gm, gm
    tracked = [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")]
    assert len(tracked) == 4 and all(v == TC.TRACKED_BEFORE + 1 for v in tracked), "num_batches_tracked == 8"
    # after that one training forward, eval() equals a fresh eval model loaded with the updated state_dict, bit for bit: the layout
    # cache saw the new running statistics
    with torch.no_grad():
        ev = m.eval()(x)
        fresh = new_model(case)
        fresh.load_state_dict(sd)
        assert torch.equal(fresh.to(DEV).eval()(x), ev)
        stale = new_model(case).to(DEV).eval()(x)
    assert not torch.equal(stale, ev), "the running statistics moved, so must the eval output"


@pytest.mark.parametrize("case,rows", [("b", 350), ("d", 60)])
def test_small_chunks_give_the_same_step(case, rows):
    """The output net in chunks of ``rows`` points: several chunks, a tail chunk and chunk boundaries inside a sample (N = 480 / 128).
    The forward output is bit-equal to the one-chunk run (a GEMM row does not depend on its tile).  The gradients -- of EVERY parameter --
    equal the one-chunk run's and the fixture's to the tolerance rule: the output net's weight gradients and ``gt`` / ``gb`` are summed
    chunk after chunk, i.e. in another order, and everything in the trunk and the branch hangs off those two."""
    x, y = (t.to(DEV) for t in TC.case_inputs(case))
    one, many = _enabled(case), _enabled(case)
    many._point_rows = rows
    B, N = TC.CASES[case][3], TC.CASES[case][1][0] * TC.CASES[case][0][1] * TC.CASES[case][0][2]
    assert B * N > 3 * rows and (B * N) % rows and N % rows, "several chunks, a tail, a boundary inside a sample"
    out1, _ = _step(one, x, y)
    out2, _ = _step(many, x, y)
    assert torch.equal(out1, out2)
    report = []
    ws, wn, gm = compare_gradients(case, _named_grads(many), report)
    print("\n".join(report))
    print(f"case {case} in chunks of {rows}: worst gradient samples / norm at {ws:.2f} / {wn:.2f} of their bounds")
    assert not gm, gm
    g1, gm_ = _named_grads(one), _named_grads(many)
    real, zero_bias = TC.param_names(case)
    worst, misses = 0.0, []
    for i, n in enumerate(real):
        e, bound = float((gm_[n] - g1[n]).norm() / g1[n].norm()), tol(GOLD[f"{case}_g_selferr"][i])
        worst = max(worst, e / bound)
        print(f"  {n:28s} chunked vs one chunk Rel-L2 {e:.2e} (tol {bound:.1e})")
        if not e < bound:
            misses.append((n, e, bound))
    noise, nb = max(float(gm_[n].abs().max()) for n in zero_bias), 64 * float(GOLD[f"{case}_bias_noise"])
    print(f"case {case} in chunks of {rows} vs one chunk: worst gradient at {worst:.3f} of its bound; zero-gradient biases {noise:.1e} (bound {nb:.1e})")
    assert not misses, misses
    assert noise <= nb


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_training_trunk_is_the_eval_trunk(case):
    """``t`` of the training forward (rpb_gemm3x x 3 over the [N][64] coordinate matrix, W1 zero-padded to K = 64) against rpb_don_trunk
    (the cached eval trunk) and against the fp64 restatement, at the bound of tests/test_gpu_deeponet.py::test_trunk_kernel:
    Rel-L2 < 1e-5.  p = 64 / 128 / 256; N = 1024, 480 and 2475 (no multiple of 32)."""
    import deeponet_restatement as R
    shape_in, shape_out, p, _, _ = TC.CASES[case]
    m = _enabled(case)
    x = TC.case_inputs(case)[0].to(DEV)
    state = m._new_state()
    m._forward_hip(x, state)
    T_out, H, W = shape_out[0], shape_in[1], shape_in[2]
    with torch.no_grad():
        t_eval = m._trunk(T_out, H, W, torch.device(DEV))
    want = R.trunk(TC.weights(case), T_out, H, W)
    t = state["t"]
    e_k, e_t, e_e = rel(t.cpu(), t_eval.cpu()), rel(t.cpu(), want), rel(t_eval.cpu(), want)
    print(f"case {case} p={p} N={t.shape[0]}: training trunk vs rpb_don_trunk Rel-L2 {e_k:.2e}; vs fp64 {e_t:.2e} (rpb_don_trunk vs fp64 {e_e:.2e})")
    assert tuple(t.shape) == tuple(t_eval.shape) == (T_out * H * W, p)
    assert e_k < 1e-5 and e_t < 1e-5


def _used_masks(m, state, B, N, rows):
    """The masks of one step of in-kernel dropout, materialised by rpb_dropout_mul on ones with the seeds of the step."""
    keep, step = 1.0 - m.dropout_rate, state["step"]
    def mask(layer, chunk, n_rows, width):
        ones, out = torch.ones(n_rows, width, device=DEV), torch.empty(n_rows, width, device=DEV)
        ops.dropout_mul(ones, out, n_rows * width, M.drop_seed(m.dropout_seed, step, layer, chunk), keep)
        return out
    chunks = [(ci, q0, min(rows, B * N - q0)) for ci, q0 in enumerate(range(0, B * N, rows))]
    return [mask(0, 0, B, 512), torch.cat([mask(1, ci, R, 512) for ci, _, R in chunks]), torch.cat([mask(2, ci, R, 128) for ci, _, R in chunks])]


def test_in_kernel_dropout_is_the_explicit_mask_path():
    case, rows = "d", 100
    B, N = TC.CASES[case][3], TC.CASES[case][1][0] * TC.CASES[case][0][1] * TC.CASES[case][0][2]
    x, y = (t.to(DEV) for t in TC.case_inputs(case))

    def run(seed, masks=None):
        m = new_model(case).to(DEV).enable_training(seed=seed).train()
        m._point_rows, m._mask_override = rows, masks
        state = m._new_state()
        out = m._forward_hip(x, state)
        grads = m._backward_hip(state, ((2.0 / out.numel()) * (out - y)).contiguous())
        return m, state, out, {n: grads[p] for n, p in m.named_parameters()}

    m, state, out, grads = run(77)
    masks = _used_masks(m, state, B, N, rows)
    for k, mk in enumerate(masks):
        vals = set(mk.unique().tolist())
        frac = float((mk > 0).float().mean())
        print(f"dropout site {k}: kept fraction {frac:.4f}, values {sorted(vals)}")
        assert vals == {0.0, float(torch.tensor(1.0) / torch.tensor(0.9))}
        assert abs(frac - 0.9) < 4 * (0.09 / mk.numel()) ** 0.5, "the kept fraction within four standard deviations of a Bernoulli(0.9) sample"
    assert not torch.equal(masks[1][:rows], masks[1][rows:2 * rows]), "the masks of two chunks differ (the seed includes the chunk)"
    assert not torch.equal(masks[2][:rows], masks[2][rows:2 * rows])
    _, _, out_m, grads_m = run(77, masks)
    print("in-kernel vs explicit masks: output max |diff| %.3e, worst gradient Rel-L2 %.3e" % (
        float((out - out_m).abs().max()), max(float((grads[n] - grads_m[n]).norm() / grads[n].norm()) for n in grads)))
    assert torch.equal(out, out_m), "in-kernel Philox == the explicit mask of the same seeds, bit for bit"
    for n in grads:
        assert torch.equal(grads[n], grads_m[n]), n
    _, _, out_again, grads_again = run(77)
    assert torch.equal(out, out_again) and all(torch.equal(grads[n], grads_again[n]) for n in grads), "the same seed: the same step"
    _, _, out_other, _ = run(78)
    assert not torch.equal(out, out_other), "another seed: other masks"
    # a second step of one model draws new masks (the seed includes the step)
    state2 = m._new_state()
    assert not torch.equal(m._forward_hip(x, state2), out) and state2["step"] == state["step"] + 1


def test_backward_twice_is_bit_equal():
    m = _enabled("c")
    x, y = (t.to(DEV) for t in TC.case_inputs("c"))
    state = m._new_state()
    out = m._forward_hip(x, state)
    g_out = (2.0 / out.numel()) * (out - y)
    first = {p: g.clone() for p, g in m._backward_hip(state, g_out.contiguous()).items()}
    again = m._backward_hip(state, g_out.contiguous())
    assert len(first) == len(again) == len(list(m.parameters())) == 32
    for p, g in first.items():
        assert torch.equal(g, again[p])
    # ... and a second model gives the same forward and gradients (no atomics, fixed summation order)
    m2, m3 = _enabled("c"), _enabled("c")
    _step(m2, x, y)
    _step(m3, x, y)
    for (n, p), q in zip(m2.named_parameters(), m3.parameters()):
        assert torch.equal(p.grad, q.grad), n
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
    path = str(tmp_path / "model_2.pth")
    ck = tr.checkpoint({"train_losses": [1.0], "val_losses": {}, "best_iteration": 2, "best_val_loss": 0.5})
    assert list(ck["model_state_dict"]) == list(TC.weights(case)) and ck["iteration"] == TC.ADAM_STEPS
    torch.save({k: ({n: v.cpu() for n, v in val.items()} if k == "model_state_dict" else val) for k, val in ck.items()}, path)
    m2 = new_model(case)
    meta = m2.load_checkpoint(path, DEV)
    assert meta["iteration"] == TC.ADAM_STEPS
    sd, sd2 = m.state_dict(), m2.state_dict()
    for k in sd:
        assert torch.equal(sd[k], sd2[k]) and sd[k].dtype == TC.weights(case)[k].dtype, k
    x = TC.case_inputs(case)[0].to(DEV)
    with torch.no_grad():
        assert torch.equal(m.eval()(x), m2.eval()(x))


def test_refusals_and_opt_in(tmp_path):
    from realpdebench_amd import eval as ev
    from realpdebench_amd import train as trn
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
        before = m.branch.conv4[1].running_mean.clone()
        a = m.train()(x)
        assert not torch.equal(m.branch.conv4[1].running_mean, before)
        assert not torch.equal(a, m.eval()(x))
    loss = m.train().train_loss(x, y)
    assert loss.requires_grad and loss.grad_fn is not None, "train_loss of an enabled instance in train() carries a graph"
    # a BatchNorm that would see a single value per channel: B T H W == 1 at stage 4 (torch raises the same ValueError)
    one = M.DeepONet((8, 8, 8, 3), (8, 8, 8, 3), 3, 3, 64).to(DEV).enable_training().train()
    with torch.no_grad(), pytest.raises(ValueError, match="more than 1 value per channel"):
        one(torch.zeros(1, 8, 8, 8, 3, device=DEV))
    # `python -m realpdebench_amd.train` on a small synthetic YAML with `hip_training: true`: a few updates, a checkpoint, eval loads it
    shape = [8, 16, 16, 3]
    cfg = dict(exp_name="t", gpu=0, seed=0, results_path=str(tmp_path), dataset_name="synthetic", dataset_root="", num_workers=0,
               normalizer="none", shape_in=shape, shape_out=shape, n_train=4, n_val=2, model_name="deeponet", checkpoint_path="", p=64,
               dropout_rate=0.1, hip_training=True, is_use_tb=None, scheduler="cosine", step_size=10, num_update=100, train_batch_size=2,
               test_batch_size=2, lr=1e-3, clip_grad_norm=0.0, N_autoregressive=1)
    path = tmp_path / "deeponet.yaml"
    path.write_text(yaml.safe_dump(cfg))
    exp = trn.main(["--config", str(path), "--max_updates", "3"])
    ckpts = sorted(glob.glob(os.path.join(exp, "model_*.pth")))
    assert ckpts, "no checkpoint written"
    ck = torch.load(ckpts[-1], map_location="cpu")
    assert ck["iteration"] == 3 and all(l == l and l < 1e3 for l in ck["train_losses"])
    assert int(ck["model_state_dict"]["branch.conv1.1.num_batches_tracked"]) == 3
    res = ev.main(["--config", str(path), "--checkpoint_path", ckpts[-1]])
    assert isinstance(res, dict)
    off = tmp_path / "off.yaml"
    off.write_text(yaml.safe_dump({k: v for k, v in cfg.items() if k != "hip_training"}))
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):       # without the key: still refused at trainer construction
        trn.main(["--config", str(off), "--max_updates", "1"])
