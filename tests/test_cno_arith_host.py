"""CNO3d.set_arith on the host (no GPU): validation, the training refusal and the opt-in under "f16x2", and the f16x2 arithmetic of
rpb_cno_conv3x_f16x2 restated in fp64 (tests/cno_arith_cases.py) against the exact fp64 result at the operands of the GPU kernel
cases: it must stay under one eighth of the GPU bound (2e-6 / 8 = 2.5e-7).  Measured: 4.7e-8 to 6.5e-8 over the
sixteen (Ci, N, epilogue) cases.  The exponent rule at the boundary values of tests/test_gpu_conv3h.py; tests/test_gpu_cno_arith.py
compares rpb_amax_exp_finish with the same function."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cno_arith_cases as AC                      # noqa: E402
import cno_common as CC                           # noqa: E402
from cno_helpers import TRAIN_MSG, new_model      # noqa: E402


def test_set_arith_validates_defaults_and_returns_the_model():
    m = new_model("a")
    assert m.arith == "f32"
    assert m.set_arith("f16x2") is m and m.arith == "f16x2"
    assert m.set_arith("f32") is m and m.arith == "f32"
    for bad in ("fp8", "bf16x3", "F16X2", "", None):
        with pytest.raises(ValueError, match="arith must be 'f32' or 'f16x2'"):
            m.set_arith(bad)
    assert m.arith == "f32", "a refused value leaves the setting alone"


def test_training_refusal_and_opt_in_are_unchanged_under_f16x2():
    from realpdebench_amd.trainer import make_trainer
    shape_in, shape_out, _ = CC.CASES["a"]
    x, y = torch.zeros(1, *shape_in), torch.zeros(1, *shape_out)
    m = new_model("a").set_arith("f16x2")
    assert m.batch_independent is True and not m.hip_training and TRAIN_MSG in m.training_unavailable
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        make_trainer(m, lr=1e-3, num_update=10)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        m.train_loss(x, y)
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):
        m(x)
    assert m.enable_training() is m and m.arith == "f16x2"
    assert m.hip_training and m.training_unavailable is None and m.batch_independent is False
    with pytest.raises(NotImplementedError, match=TRAIN_MSG):       # eval() under grad mode still refuses
        m.eval()(x)
    with pytest.raises(RuntimeError, match="MI355X only"):          # train(): the HIP path, which has no CPU fallback
        m.train()(x)
    with torch.no_grad(), pytest.raises(RuntimeError, match="MI355X only"):     # eval forward: no CPU fallback under either setting
        m.eval()(x)


@pytest.mark.parametrize("act,with_res,narrow", AC.EPILOGUES)
@pytest.mark.parametrize("Ci,N", AC.SHAPES)
def test_restated_arithmetic_stays_under_an_eighth_of_the_gpu_bound(Ci, N, act, with_res, narrow):
    c = AC.kernel_case(Ci, N)
    nv = 16 if narrow else N
    e = AC.rel(AC.restated(c, Ci, N, act, with_res, nv), AC.expected(c, act, with_res, nv))
    print(f"Ci={Ci} N={N} act={act} res={with_res} nvalid={nv}: restatement Rel-L2 {e:.2e} (bound {AC.HOST_BOUND:.1e})")
    assert e < AC.HOST_BOUND


def test_planes_reconstruct_the_scaled_operand():
    """hi + lo is x * 2^e to 2^-23 relative for every element within 2^-16 of the maximum; the maximum lands in [2^14, 2^15)"""
    for Ci, N in AC.SHAPES:
        c = AC.kernel_case(Ci, N)
        for t in (c["x"], c["w"]):
            e = AC.exponent(t)
            xs = t.double() * 2.0 ** e
            assert 2.0 ** 14 <= float(xs.abs().max()) < 2.0 ** 15
            hi, lo = AC.split2h(t, e)
            big = xs.abs() >= 2.0 ** -16 * xs.abs().max()
            assert float(((hi + lo - xs).abs() / xs.abs().clamp_min(1e-300))[big].max()) <= 2.0 ** -23


def test_exponent_rule_at_the_boundary_values():
    for v in AC.BOUNDARY_VALUES:
        e = AC.exponent_of_bits(AC.f32_bits(v))
        assert 2.0 ** 14 <= v * 2.0 ** e < 2.0 ** 15, (v, e)
        assert AC.exponent(torch.tensor([0.0, -v, v / 3])) == e
    assert AC.exponent_of_bits(0) == 0
    for nonfinite in (float("inf"), float("nan")):
        assert AC.exponent_of_bits(AC.f32_bits(nonfinite) & 0x7FFFFFFF) == 0
