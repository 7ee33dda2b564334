"""DPOT.set_arith on the host (no GPU): the C ABI of the large-K f16x2 token GEMM and of the f16x2 AFNO block MLP, the switch's surface
on a CPU-built model from the ``dpot_golden()`` configuration, and what the two ``_supported`` queries accept."""
import os
import re

import pytest
import torch

from conftest import ROOT, dpot_golden

SYMBOLS = ("rpb_gemm3hk_supported", "rpb_gemm3hk_rowexp", "rpb_gemm3hk", "rpb_afno_mlp_f16x2_supported", "rpb_afno_wprep_f16x2",
           "rpb_afno_mlp_f16x2")


def _model():
    from realpdebench_amd.model.dpot import DPOT
    g = dpot_golden()
    cfg = {k: v for k, v in g["cfg"].items() if k != "data_out_channels"}
    m = DPOT(shape_in=tuple(g["x"].shape[1:]), shape_out=tuple(g["y"].shape[1:]), normalize=False, act="gelu", **cfg)
    m.load_state_dict(g["sd"], strict=True)
    return m, g


def test_symbols_declared_and_bound():
    from realpdebench_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpb.h")).read(), flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, txt), f"{s} is not declared in include/rpb.h"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature"
        decl = re.search(r"\b%s\s*\((.*?)\)\s*;" % s, txt, flags=re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[s][1]), s


def test_set_arith_surface():
    from realpdebench_amd.model import dpot
    m, g = _model()
    assert dpot.DPOT.ARITHS == ("f32", "f16x2")
    assert m.arith == "f32"
    keys = set(m.state_dict())
    assert m.set_arith("f16x2") is m and m.arith == "f16x2"
    assert set(m.state_dict()) == keys == set(g["sd"])
    for bad in ("fp8", "bf16x3", "", None, 3):
        with pytest.raises(ValueError, match="arith must be 'f32' or 'f16x2'"):
            m.set_arith(bad)
    assert m.arith == "f16x2"
    assert m.set_arith("f32") is m and m.arith == "f32"
    assert set(m.F16X2_SITES) <= set(m.ALL_F16X2_SITES) == {"mlp0", "mlp2", "out0", "out2", "tagg", "afno"}


@pytest.mark.parametrize("arith", ["f32", "f16x2"])
def test_cpu_forward_still_refuses(arith):
    m, g = _model()
    m.set_arith(arith).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        m(g["x"])


@pytest.mark.parametrize("M,N,K,lda,ldo,want", [
    (16384, 6144, 1536, None, None, True),        # dpot_l mlp0
    (16384, 1536, 6144, None, None, True),        # dpot_l mlp2
    (4096, 98304, 1536, None, None, True),        # dpot_l out0
    (1 << 20, 1536, 1536, None, None, True),      # dpot_l out2
    (16384, 1536, 1280, None, None, True),        # tagg at 20 frames
    (4096, 1024, 1024, None, None, True),         # dpot_s FeedForward
    (1, 256, 576, None, None, True),
    (300, 256, 1536, 3 * 1536, 512, True),        # column ranges of wider tensors
    (256, 256, 96, None, None, False),            # K % 64
    (256, 96, 1536, None, None, False),           # N % 256
    (256, 256, 1536, 1538, None, False),          # lda % 4
    (256, 256, 256, 258, None, False),
    (256, 256, 1536, None, 258, False),           # ldo % 4
    (256, 256, 1536, 1024, None, False),          # lda < K
    (256, 256, 512, None, None, False),           # K <= 512 is rpb_gemm3h's
    (256, 32, 32, None, None, False),             # dpot_s out2
    (0, 256, 1536, None, None, False),
])
def test_gemm3hk_supported_truth_table(M, N, K, lda, ldo, want):
    from realpdebench_amd import ops
    assert ops.gemm3hk_supported(M, N, K, lda, ldo) is want


@pytest.mark.parametrize("nb,bs,want", [(16, 96, True), (8, 128, True), (8, 16, True), (8, 32, True), (8, 24, False), (8, 144, False),
                                        (0, 96, False), (8, 0, False)])
def test_afno_f16x2_supported_truth_table(nb, bs, want):
    from realpdebench_amd import ops
    assert ops.afno_f16x2_supported(nb, bs) is want
