"""CNO3d training step, host side (no GPU).

tests/cno_train_restatement.py -- the formulas the HIP training step implements, in fp64 without autograd -- against the reference's fp64
run (tests/golden/cno_train_small.npz): Rel-L2 < 1e-9 for the output, the loss, every running statistic and every sampled gradient and
gradient norm.  Both sides are fp64 and differ only in summation order; the LeakyReLU gates have margins of ~1e-7 of a standard
deviation, far above fp64 noise.  The 31 convolution biases in front of a BatchNorm have |g| <= 1e-12.
The opt-in plumbing that needs no GPU, and the flipped-weight layout of the data gradient against ``conv_transpose3d``."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cno_train_common as TC                     # noqa: E402
import cno_train_restatement as R                 # noqa: E402
from cno_helpers import One                       # noqa: E402
from cno_train_helpers import GOLD, TRAIN_MSG, compare_gradients, new_model, rel, stat_slices      # noqa: E402

HOST_TOL = 1e-9


@pytest.mark.parametrize("case", list(TC.CASES))
def test_restatement_matches_reference_fp64(case):
    x, y = TC.case_inputs(case)
    out, loss, stats, grads = R.train_step(TC.weights(case), x, y)
    real, zero_bias, none = TC.param_names(case)
    assert rel(out, GOLD[f"{case}_out"]) < HOST_TOL
    assert abs(float(loss) - float(GOLD[f"{case}_loss"])) < HOST_TOL * float(GOLD[f"{case}_loss"])
    for k, sl in stat_slices(case).items():
        assert rel(stats[k], GOLD[f"{case}_stats"][sl]) < HOST_TOL, k
    assert all(int(v) == TC.TRACKED_BEFORE + 1 for k, v in stats.items() if k.endswith("num_batches_tracked"))
    assert sum(k.endswith("num_batches_tracked") for k in stats) == 31
    *worst, misses = compare_gradients(case, grads, lambda _selferr: HOST_TOL)
    assert not misses, misses
    noise = max(float(grads[n].abs().max()) for n in zero_bias)
    print(f"case {case}: worst sampled gradient / norm {worst[0] * HOST_TOL:.1e} / {worst[1] * HOST_TOL:.1e}, zero-gradient biases {noise:.1e}")
    assert noise <= 1e-12
    assert not any(n in grads for n in none), "decoder_inv.3 never runs: no gradient"
    assert sorted(grads) == sorted(real + zero_bias)


def test_opt_in_plumbing():
    from realpdebench_amd.model import load_model
    from realpdebench_amd.trainer import make_trainer
    shape_in, shape_out, _ = TC.CASES["d"]
    m = new_model("d")
    assert m.batch_independent is True and not m.hip_training and TRAIN_MSG in m.training_unavailable
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        make_trainer(m, lr=1e-3, num_update=10)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        m.train_loss(torch.zeros(1, *shape_in), torch.zeros(1, *shape_out))
    assert m.enable_training() is m
    assert m.hip_training and m.training_unavailable is None and m.batch_independent is False
    assert type(m).batch_independent is True and TRAIN_MSG in type(m).training_unavailable, "the class, and every other instance, is unchanged"
    with pytest.raises(ValueError, match="micro_batch"):
        make_trainer(m, lr=1e-3, num_update=10, micro_batch=2)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):       # eval() under grad mode still refuses
        m.eval()(torch.zeros(1, *shape_in))
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        m.eval().train_loss(torch.zeros(1, *shape_in), torch.zeros(1, *shape_out))
    with pytest.raises(RuntimeError, match="MI355X only"):          # train(): the HIP path, which has no CPU fallback
        m.train()(torch.zeros(1, *shape_in))
    cfg = dict(model_name="cno", N_layers=3)
    assert not load_model(One(shape_in, shape_out), **cfg).hip_training
    assert not load_model(One(shape_in, shape_out), hip_training=False, **cfg).hip_training
    on = load_model(One(shape_in, shape_out), hip_training=True, **cfg)
    assert on.hip_training and on.batch_independent is False and on.training_unavailable is None


@pytest.mark.parametrize("Ci,Co", [(3, 64), (16, 32), (64, 128), (128, 64)])
def test_flipped_weight_is_conv_transpose(Ci, Co):
    """``flipped_weight`` laid out as ``padded_weight`` lays out the forward weights: a convolution with it is the data gradient."""
    from realpdebench_amd.model._common import flipped_weight, padded_weight
    g = torch.Generator().manual_seed(Ci * 1000 + Co)
    conv = torch.nn.Conv3d(Ci, Co, 3, padding=1).double()
    with torch.no_grad():
        conv.weight.copy_(torch.rand(Co, Ci, 3, 3, 3, generator=g, dtype=torch.float64) - 0.5)
    N, K = max(Co, 64), max(Ci, 64)
    wd = flipped_weight(conv, N, K).double()                          # (built in fp32: compare against the fp32-rounded weights)
    w32 = conv.weight.detach().float().double()
    dy = torch.rand(2, Co, 3, 4, 5, generator=g, dtype=torch.float64) - 0.5
    want = F.conv_transpose3d(dy, w32, padding=1)
    dyp = F.pad(dy, (0, 0, 0, 0, 0, 0, 0, N - Co))
    got = F.conv3d(dyp, wd.view(K, 3, 3, 3, N).permute(0, 4, 1, 2, 3), padding=1)
    assert rel(got[:, :Ci], want) < 1e-12
    assert not bool(got[:, Ci:].any()), "pad rows are zero"
    # the layout convention is padded_weight's: [out][27 taps][in]
    assert tuple(wd.shape) == (K, 27 * N) and tuple(padded_weight(conv, N, K).shape) == (N, 27 * K)
