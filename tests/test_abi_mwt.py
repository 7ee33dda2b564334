"""Every rpb_mwt_* entry point declared in include/rpb.h is exported by the built library and bound in _lib."""
import os
import re

from conftest import ROOT


def test_mwt_symbols_exported_and_bound():
    from realpdebench_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rpb.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(rpb_mwt_[a-z0-9_]+)\s*\(", txt)))
    assert len(names) >= 10, names
    lib = _lib.load()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/rpb.h but not exported by librpb_hip.so"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature"
