"""Every rpb_conv7x* / rpb_wdno_* entry point declared in include/rpb.h is exported by the built library and bound in _lib."""
import os
import re

from conftest import ROOT


def test_wdno_symbols_exported_and_bound():
    from realpdebench_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpb.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(rpb_(?:wdno|conv7x)_?[a-z0-9_]*)\s*\(", txt)))
    assert names == ["rpb_conv7x", "rpb_conv7x_supported", "rpb_conv7x_wprep", "rpb_conv7x_wz_elems", "rpb_wdno_dec", "rpb_wdno_dec_rows",
                     "rpb_wdno_rec", "rpb_wdno_step"], names
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/rpb.h but not exported by librpb_hip.so"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
    assert lib.rpb_wdno_dec_rows() == 128
    # what the implicit GEMM takes, asked without a launch: the five configs' channel counts at dim 128 / 256, and what it refuses
    for ci in (48, 64, 256):
        for n in (128, 256):
            assert lib.rpb_conv7x_supported(24576, n, ci, 7) == 1
    assert lib.rpb_conv7x_supported(24576, 256, 3, 7) == 0 and lib.rpb_conv7x_supported(24576, 192, 48, 7) == 0
    assert lib.rpb_conv7x_wz_elems(256, 48, 7) == 49 * 21 * 3 * 8 * 512 and lib.rpb_conv7x_wz_elems(256, 50, 7) == -1
