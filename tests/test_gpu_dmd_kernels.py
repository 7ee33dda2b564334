"""rpb_dmd_gram and rpb_dmd_predict (csrc/rpb_dmd.hip), one call at a time against the references of tests/dmd_kernel_cases.py, every call
on guard-banded operands (tests/guarded.py): a stray write (row S of the prediction, the upper triangle of ``part``), an element never
written (elements 240..251 of a 252-element chunk, the mirrored triangle of G) and a stray read that reaches a result (a point at P,
a channel c >= f, frame 0 of the prediction: all NaN) are assertions of ``Arena.check()``, not GPU faults.  Shapes, inputs, bounds and
drivers live in tests/dmd_kernel_cases.py (its docstring derives the bounds), shared with tests/test_dmd_kernels_host.py, which proves
without a GPU that the same drivers fail on a stand-in with one wrong term or one out-of-range access.

The cases reach what tests/test_gpu_dmd.py (f = 2 throughout) does not: the partial last tile of the prediction (pts f = 252), float4
staging loads that straddle 3- and 7-wide cells, the 4-byte staging through a misaligned base, T and S of 2, 16, 17 and 32, the Gram
kernel's second and third trip over the chunks, and coefficients that cancel.  The measured figures (``pytest -s`` of this file on the
MI355X) are in profiles/dmd_deeponet_kernels_pytest.txt."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmd_kernel_cases as K                 # noqa: E402

pytestmark = pytest.mark.gpu


class HipKernels:
    """the entry points the drivers of tests/dmd_kernel_cases.py call, on the library (``ops.dmd_gram`` / ``ops.dmd_predict`` allocate
    their outputs: the arena operands go to the C ABI directly)"""
    dev = "cuda"

    def __init__(self, ops):
        self.ops = ops

    def dmd_gram_groups(self, B, P, f):
        return self.ops._lib.query("rpb_dmd_gram_groups", B, P, f)

    def dmd_gram(self, x, G, part, B, T, P, C, f):
        o = self.ops
        o._lib.call("rpb_dmd_gram", o._p(x), o._ptr(G, torch.float64), o._ptr(part, torch.float64), B, T, P, C, f, o._stream(), label="dmd_gram")

    def dmd_predict(self, x, M, out, B, T, P, C, f, S):
        o = self.ops
        o._lib.call("rpb_dmd_predict", o._p(x), o._ptr(M, torch.float64), o._p(out), B, T, P, C, f, S, o._stream(), label="dmd_predict")


@pytest.fixture(scope="module")
def kern():
    from realpdebench_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels(ops)


@pytest.fixture(scope="module")
def cus(kern):
    """the restated group count of the cases module is the library's, on this device; the gram-only cases take their second trip"""
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    for B, T, P, C, f in [c[:5] for c in K.CASES] + K.GRAM_ONLY:
        assert kern.dmd_gram_groups(B, P, f) == K.gram_groups(B, P, f, n), (B, P, f)
    for B, T, P, C, f in K.GRAM_ONLY:
        assert K.nchunk(P, f) > K.gram_groups(B, P, f, n), (B, P, f)
    return n


def _ids(v):
    return "-".join(str(a) for a in v)


@pytest.mark.parametrize("dims", [c[:5] for c in K.CASES], ids=_ids)
def test_gram(kern, cus, dims):
    K.run_gram_twice(kern, K.gram_case(*dims))


@pytest.mark.parametrize("dims", K.GRAM_ONLY, ids=_ids)
def test_gram_workgroups_take_a_second_trip(kern, cus, dims):
    """66, 69 and 130 chunks against at most 64 workgroups per sample: the restaging barrier, and a third trip in the last case"""
    K.run_gram_twice(kern, K.gram_case(*dims))


def test_gram_misaligned_base(kern, cus):
    """the 4-byte staging through the base address: G bit-equal to the 16-byte staging's"""
    K.run_gram_misaligned(kern, K.gram_case(*K.MISALIGNED[:5]))


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("dims", K.CASES, ids=_ids)
def test_predict(kern, dims, family):
    K.run_predict_twice(kern, K.predict_case(*dims, family))


@pytest.mark.parametrize("family", K.FAMILIES)
def test_predict_misaligned_base(kern, family):
    K.run_predict_misaligned(kern, K.predict_case(*K.MISALIGNED, family))
