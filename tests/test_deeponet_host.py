"""DeepONet host side (no GPU): the plain-torch restatement of the forward against the reference's vectors
(tests/golden/deeponet_small.npz, written by tests/golden/make_golden_deeponet.py), the adaptive-pool bin rule, state_dict
compatibility, the operand layout of the point kernel, the YAMLs and the refusals.

The tolerance rule is in tests/deeponet_helpers.py."""
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeponet_common as DC                      # noqa: E402
import deeponet_restatement as R                  # noqa: E402
from deeponet_helpers import CFG, GOLD, SCENARIOS, One, rel, sd_of, tol          # noqa: E402
from realpdebench_amd.model import deeponet as M  # noqa: E402


def _new(case):
    shape_in, shape_out, p, _ = DC.CASES[case]
    return M.DeepONet(shape_in, shape_out, shape_in[-1], shape_out[-1], p)


@pytest.mark.parametrize("case", list(DC.CASES))
def test_restatement_matches_reference(case):
    shape_in, shape_out, p, _ = DC.CASES[case]
    x, y = DC.case_inputs(case)
    keep = []
    with torch.no_grad():
        out = R.forward(sd_of(case), x.double(), shape_out, keep=keep)
    e = rel(DC.stored(case, out), GOLD[f"{case}_out"])
    eb = rel(keep[4], GOLD[f"{case}_b"])
    loss = float(((out - y) ** 2).mean())
    el = abs(loss - float(GOLD[f"{case}_loss"])) / float(GOLD[f"{case}_loss"])
    print(f"case {case}: out Rel-L2 {e:.2e} (tol {tol(case + '_out'):.1e}); b {eb:.2e}; loss rel {el:.2e}")
    assert tuple(out.shape[1:]) == shape_out
    if case == "a":
        for i in range(4):
            ei = rel(DC.pool_stored(keep[i]), GOLD[f"a_pool{i + 1}"])
            print(f"  pooled stage {i + 1}: {ei:.2e}")
            assert ei < tol(f"a_pool{i + 1}"), i
    assert eb < tol(case + "_b")
    assert e < tol(case + "_out")
    assert el < tol(case + "_loss")


@pytest.mark.parametrize("case", DC.ROLLOUT_CASES)
def test_restatement_rollout_matches_reference(case):
    """The 3-step rollout with the Gaussian normaliser (eval.py:305-321), restated: normalise, predict, de-normalise, append the
    control channels of the raw input, normalise again."""
    shape_in, shape_out, _, _ = DC.CASES[case]
    sd = sd_of(case)
    x = DC.case_inputs(case)[0].double()
    mi, mt, si, st = (t.double() for t in DC.normalizer_stats(case))
    co = shape_out[-1]
    cur, preds = (x - mi) / si, []
    with torch.no_grad():
        for _ in range(DC.ROLLOUT_STEPS):
            pr = R.forward(sd, cur, shape_out) * st + mt
            if shape_in[-1] != co:
                pr = torch.cat([pr, x[..., co:]], -1)
            cur = (pr - mi) / si
            preds.append(cur)
    e = rel(DC.roll_stored(case, torch.cat(preds, 1)), GOLD[f"{case}_roll"])
    print(f"case {case}: rollout Rel-L2 {e:.2e} (tol {tol(case + '_roll'):.1e})")
    assert e < tol(case + "_roll")


@pytest.mark.parametrize("n_in", range(1, 10))
def test_adaptive_bins_are_torchs(n_in):
    """[floor(i In / Out), ceil((i + 1) In / Out)): overlapping when In % 4 != 0, replicated when In < 4 -- both the model's rule and
    the restatement's against torch.nn.AdaptiveAvgPool3d."""
    assert M.adaptive_bins(n_in, 4) == R.bins(n_in, 4)
    x = torch.rand(2, 3, n_in, 10 - n_in, 5, generator=torch.Generator().manual_seed(n_in), dtype=torch.float64)
    want = torch.nn.AdaptiveAvgPool3d((1, 4, 4))(x.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
    assert torch.allclose(R.adaptive_pool(x), want, rtol=0, atol=1e-13)


def test_flooring_pools_drop_the_trailing_frame():
    assert M.pooled_extents(20, 64, 128) == [(20, 64, 128), (10, 32, 64), (5, 16, 32), (2, 8, 16)]
    assert M.pooled_extents(10, 64, 128)[3] == (1, 8, 16)
    x = torch.rand(1, 5, 11, 6, 2, dtype=torch.float64)
    want = torch.nn.MaxPool3d(2)(x.permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1)
    assert torch.equal(R.max_pool(x), want)


@pytest.mark.parametrize("case", list(DC.CASES))
def test_state_dict_is_the_references(case):
    sd = _new(case).state_dict()
    assert [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()] == CFG["state_dict"][case]
    shape_in, shape_out, p, _ = DC.CASES[case]
    assert list(sd) == list(DC.state_shapes(shape_in, shape_out, p))


def test_reference_layout_round_trip():
    """A reference-layout dict goes in, the same dict comes out: the (c, h, w) -> (h, w, c) column permutation of branch.fc.0 is a
    derived kernel-side tensor and never reaches ``state_dict``."""
    m = _new("a")
    new = sd_of("a")
    m.load_state_dict(new)
    back = m.state_dict()
    assert list(back) == list(new)
    for k, v in new.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k


def _emulate_point_kernel(t, b, pw):
    """rpb_don_point_mlp's data flow in numpy, from the operands ``point_weights`` builds and the register layout of
    v_mfma_f32_32x32x16_bf16 (A / B lane (row or column = lane % 32, kg = lane // 32) holds k = 8 kg + e; accumulator register r of
    lane (column, kg) is row 8 (r // 4) + 4 kg + r % 4), for one 32-point tile."""
    w1z, b1z, w2z, b2z, w3z, b3 = pw
    val = lambda z: sum((pl.to(torch.int32) << 16).view(torch.float32).double() for pl in z.unbind(-3)).numpy()    # [..., 64, 8]
    w1, w2, w3 = val(w1z), val(w2z), val(w3z)
    b1z, b2z = b1z.double().numpy(), b2z.double().numpy()
    lanes = np.arange(64)
    col, kg = lanes % 32, lanes // 32
    rows = np.array([[8 * (r // 4) + 4 * g + r % 4 for r in range(16)] for g in range(2)])      # [kg][r]

    def mfma(A, Bop, D):                       # A, Bop [64 lanes][8]; D [64 lanes][16]
        a = np.zeros((32, 16)); bm = np.zeros((16, 32))
        for l in range(64):
            a[col[l], 8 * kg[l]:8 * kg[l] + 8] = A[l]
            bm[8 * kg[l]:8 * kg[l] + 8, col[l]] = Bop[l]
        prod = a @ bm
        for l in range(64):
            D[l] += prod[rows[kg[l]], col[l]]

    def act(D, bias):                          # bias [2][16] -> B operands of the two k-steps
        v = np.maximum(D + bias[kg], 0)
        return [v[:, 8 * s:8 * s + 8] for s in range(2)]

    p = t.shape[1]
    x = (t.double() * b.double()).numpy()      # [32 points][p]
    acc2 = [np.zeros((64, 16)) for _ in range(4)]
    for blk in range(16):
        acc1 = np.zeros((64, 16))
        for ks in range(p // 16):
            xop = np.stack([x[col[l], 16 * ks + 8 * kg[l]:16 * ks + 8 * kg[l] + 8] for l in range(64)])
            mfma(w1[blk, ks], xop, acc1)
        hp = act(acc1, b1z[blk])
        for s in range(2):
            for mt in range(4):
                mfma(w2[blk, s, mt], hp[s], acc2[mt])
    acc3 = np.zeros((64, 16))
    for mt in range(4):
        hp = act(acc2[mt], b2z[mt])
        for s in range(2):
            mfma(w3[mt, s], hp[s], acc3)
    out = np.zeros((32, b3.shape[0]))
    for l in range(64):
        for r in range(8):
            c = rows[kg[l]][r]
            if c < b3.shape[0]:
                out[col[l], c] = acc3[l, r] + float(b3[c])
    return out


@pytest.mark.parametrize("p,cout", [(64, 3), (128, 16)])
def test_point_kernel_operand_layout(p, cout):
    """The lane-ordered bf16 planes and register-ordered biases of ``point_weights`` reproduce output_net when they are pushed through
    the MFMA register layout the kernel relies on (a numpy emulation; the planes sum to the fp32 weights exactly)."""
    g = torch.Generator().manual_seed(p + cout)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    W1, b1, W2, b2, W3, b3 = u(512, p) * 0.2, u(512) * 0.2, u(128, 512) * 0.1, u(128) * 0.2, u(cout, 128) * 0.2, u(cout)
    pw = M.point_weights(W1, b1, W2, b2, W3, b3)
    h, m, l = M.bf16_planes(W1)
    back = sum((v.to(torch.int32) << 16).view(torch.float32).double() for v in (h, m, l))
    assert torch.equal(back, W1.double())
    t, b = u(32, p), u(1, p)
    sd = {"output_net.0.weight": W1, "output_net.0.bias": b1, "output_net.3.weight": W2, "output_net.3.bias": b2,
          "output_net.6.weight": W3, "output_net.6.bias": b3}
    want = R.point_mlp(sd, t.double(), b.double())[0]
    assert rel(_emulate_point_kernel(t, b, pw), want) < 1e-12


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_yaml_parses_with_reference_values(scenario):
    with open(os.path.join(ROOT, "realpdebench_amd", "configs", scenario, "deeponet.yaml")) as fh:
        cfg = yaml.safe_load(fh)
    for k, v in CFG["model_keys"][scenario].items():
        assert cfg[k] == v, (scenario, k)
    assert cfg["shape_in"] == CFG["native_shapes"][scenario]["shape_in"] and cfg["shape_out"] == CFG["native_shapes"][scenario]["shape_out"]
    assert cfg["p"] == {"cylinder": 128, "combustion": 128, "controlled_cylinder": 256, "foil": 256, "fsi": 64}[scenario]


def test_load_model_returns_the_class():
    from realpdebench_amd.model import load_model
    shape_in, shape_out, p, _ = DC.CASES["b"]
    m = load_model(One(shape_in, shape_out), model_name="deeponet", p=p, dropout_rate=0.1, config="x.yaml", lr=1e-3)
    assert isinstance(m, M.DeepONet) and m.p == p and m.input_channels == 5 and m.output_channels == 3
    with pytest.raises(ValueError, match="deeponet"):
        load_model(One(shape_in, shape_out), model_name="no_such_model")


def test_unsupported_configurations_are_refused_loudly():
    with pytest.raises(NotImplementedError, match="p=100"):
        M.DeepONet((8, 32, 32, 3), (8, 32, 32, 3), 3, 3, 100)
    with pytest.raises(NotImplementedError, match="empty extent"):
        M.DeepONet((4, 32, 32, 3), (4, 32, 32, 3), 3, 3, 64)


def test_backward_is_refused_without_a_gpu_too():
    m = _new("a")
    x = torch.zeros(1, *DC.CASES["a"][0])
    msg = "DeepONet training step is not built yet"
    with pytest.raises(NotImplementedError, match=msg):
        m.train_loss(x, x)
    with pytest.raises(NotImplementedError, match=msg):
        m(x.requires_grad_())
    with pytest.raises(NotImplementedError, match=msg):
        m.eval()(x.detach())                       # eval mode under grad mode with trainable parameters: no graph-less tensor comes back
    from realpdebench_amd.trainer import make_trainer
    with pytest.raises(NotImplementedError, match=msg):
        make_trainer(m, lr=1e-3, num_update=10)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(x.detach())


def test_checkpoint_formats(tmp_path):
    m = _new("a")
    m.load_state_dict(sd_of("a"))
    torch.save(m.state_dict(), str(tmp_path / "w.pth"))
    torch.save({"model_state_dict": m.state_dict(), "train_losses": [2.0], "val_losses": {}, "iteration": 3, "best_iteration": 2,
                "best_val_loss": 0.25}, str(tmp_path / "full.pth"))
    m2 = _new("a")
    meta = m2.load_checkpoint(str(tmp_path / "w.pth"), "cpu")
    assert meta["iteration"] == 0 and meta["all_train_losses"] == []
    assert torch.equal(m2.branch.fc[0].weight, m.branch.fc[0].weight)
    meta = _new("a").load_checkpoint(str(tmp_path / "full.pth"), "cpu")
    assert meta["iteration"] == 3 and meta["best_val_loss"] == 0.25 and meta["all_train_losses"] == [2.0]
