"""Host side of the opt-in f16x2 convolution arithmetic (no GPU needed): the four entry points are exported and bound, and
Transolver / Unet3d .set_arith check their argument, default to "f32" and return the model."""
import pytest

SYMBOLS = ("rpb_amax_exp", "rpb_split2h", "rpb_conv3x_wprep_f16x2", "rpb_conv3x_f16x2")


def test_conv3h_symbols_exported_and_bound():
    from realpdebench_amd import _lib
    lib = _lib.load()
    for n in SYMBOLS:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n


def _models():
    from realpdebench_amd.model.transolver import Transolver
    from realpdebench_amd.model.unet import Unet3d
    return [Transolver(space_dim=3, n_layers=1, n_hidden=64, n_head=2, fun_dim=0, out_dim=3, slice_num=16, mlp_ratio=2, H=8, W=6, D=4),
            Unet3d(dim=64, out_channels=3, dim_mults=[1, 2], channels=3, in_time=2, out_time=2)]


@pytest.mark.parametrize("idx", [0, 1])
def test_set_arith_checks_and_default(idx):
    m = _models()[idx]
    assert m.arith == "f32"
    assert m.set_arith("f16x2") is m and m.arith == "f16x2"
    assert m.set_arith("f32") is m and m.arith == "f32"
    for bad in ("fp8", "F16X2", "", None):
        with pytest.raises(ValueError):
            m.set_arith(bad)
    assert m.arith == "f32"


def test_conv3_rejects_unknown_arith():
    import torch
    from realpdebench_amd import ops
    x = torch.zeros(8, 64)
    with pytest.raises(ValueError):
        ops.conv3(x, torch.zeros(64, 27 * 64), torch.zeros(8, 64), 8, 64, 64, (2, 2, 2), arith="bf16")
