"""MWT3d.set_arith on the host (no GPU): validation, the C ABI of the split-operand convolution, and the training refusal under the
opt-in modes."""
import os
import re

import pytest
import torch

from conftest import ROOT
from realpdebench_amd.model import mwt as M

SYMBOLS = ("rpb_mwt_conv3x_wprep", "rpb_mwt_conv3x")


def _model():
    return M.MWT3d(k=3, alpha=5, c=4, nCZ=1, shape_in=(8, 4, 4, 3), shape_out=(8, 4, 4, 3))


def test_set_arith_validates_and_returns_the_model():
    m = _model()
    assert m.arith == "f32"
    for a in ("bf16x3", "f16x2", "f32"):
        assert m.set_arith(a) is m and m.arith == a
    for bad in ("fp8", "bf16", "", None, 3):
        with pytest.raises(ValueError, match="arith must be 'f32', 'bf16x3' or 'f16x2'"):
            m.set_arith(bad)
    assert m.arith == "f32"


def test_symbols_declared_and_bound():
    from realpdebench_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpb.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, txt), f"{s} is not declared in include/rpb.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[s][1]), s


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
def test_training_stays_refused(arith):
    from realpdebench_amd.trainer import make_trainer
    m = _model().set_arith(arith)
    x = torch.zeros(1, 8, 4, 4, 3)
    with pytest.raises(NotImplementedError, match="MWT training step is not built yet"):
        m.train_loss(x, x)
    with pytest.raises(NotImplementedError, match="MWT training step is not built yet"):
        m(x.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="MWT training step is not built yet"):
        make_trainer(m, lr=1e-3, num_update=10)
