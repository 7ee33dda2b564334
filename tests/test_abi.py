"""The C-ABI library loads on a CPU-only box and exports every symbol include/rpb.h declares."""
import os
import re

from conftest import ROOT


def _header():
    txt = open(os.path.join(ROOT, "include", "rpb.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def declared_symbols():
    return sorted(set(re.findall(r"\b(rpb_[a-z0-9_]+)\s*\(", _header())))


def declared_signatures():
    """name -> (return type, argument codes of ``_lib.SIGNATURES``) parsed from the declarations of include/rpb.h."""
    def code(param):
        if "*" in param or "hipStream_t" in param:
            return "p"
        words = [w for w in param.split()[:-1] if w not in ("const", "unsigned", "signed")]      # the last word is the name
        return {"int": "i", "long": "l", "float": "f", "double": "d"}[" ".join(words)]

    out = {}
    for ret, name, params in re.findall(r"\b([a-z][a-z ]*?\*?)\s*\b(rpb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header()):
        params = params.strip()
        out[name] = (" ".join(ret.split()), "" if params == "void" else "".join(code(q.strip()) for q in params.split(",")))
    return out


def test_header_symbols_exported_and_bound():
    from realpdebench_amd import _lib
    lib = _lib.load()
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/rpb.h but not exported by librpb_hip.so"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in realpdebench_amd/_lib.py"
    assert set(_lib.SIGNATURES) == set(names)
    # every hand-typed row against the declaration: callers pass bare Python ints, so a wrong l / i would truncate silently
    import ctypes
    restypes = {"int": ctypes.c_int, "long": ctypes.c_long, "const char*": ctypes.c_char_p}
    decl = declared_signatures()
    assert set(decl) == set(names)
    for n in names:
        ret, codes = decl[n]
        assert _lib.SIGNATURES[n] == (restypes[ret], codes), f"{n}: include/rpb.h declares {ret} ({codes}), _lib.SIGNATURES has {_lib.SIGNATURES[n]}"
    hdr = open(os.path.join(ROOT, "include", "rpb.h")).read()
    assert lib.rpb_abi_version() == int(re.search(r"#define RPB_ABI_VERSION (\d+)", hdr).group(1)) == _lib.ABI_VERSION


def test_no_gpu_means_loud_failure_not_fallback():
    import pytest
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from realpdebench_amd.model.fno import FNO3d
    m = FNO3d(2, 3, 3, 1, 32, (4, 8, 8, 2), (4, 8, 8, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 4, 8, 8, 2))


def test_product_never_imports_oracle():
    bad = []
    for d, _, files in os.walk(os.path.join(ROOT, "realpdebench_amd")):
        for f in files:
            if f.endswith(".py") and re.search(r"^\s*(from|import)\s+oracle\b", open(os.path.join(d, f)).read(), re.M):
                bad.append(f)
    assert not bad, bad
