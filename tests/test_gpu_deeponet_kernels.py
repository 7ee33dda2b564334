"""The DeepONet evaluation kernels -- rpb_don_bn_relu_pool, rpb_don_trunk, rpb_don_point_mlp (csrc/rpb_deeponet.hip) and
rpb_don_point_mlp_f16x2 (csrc/rpb_deeponet_h.hip) -- one launch at a time against the fp64 restatements of
tests/deeponet_restatement.py, every call on guard-banded operands (tests/guarded.py): a stray write (column C_out of the last point,
row N of the trunk output), an element never written (the last tail point, columns C..ldo-1 of a pooled cell, the items of the pool's
second grid trip) and a stray read that reaches a result (row N of ``t``, column C of a strided ``x``, a weight plane past its operand:
all NaN) are assertions of ``Arena.check()``, not GPU faults.  Shapes, inputs, bounds and drivers live in
tests/deeponet_kernel_cases.py (its docstring lists what each case reaches), shared with tests/test_deeponet_kernels_host.py, which
proves without a GPU that every case is well conditioned and that the same drivers fail on a stand-in with one wrong term or one
out-of-range access.

Bounds: each output on Rel-L2 and on max |error| / max |reference| against max(8 * e32, 1e-6), e32 being the same measure of the fp32
CPU restatement; the f16x2 point MLP against 2e-6 (Rel-L2, the bound of tests/test_gpu_deeponet_arith.py) and 1e-5 (maximum).
``EXISTING`` names, for a kernel whose MI355X result needs more, the bound tests/test_gpu_deeponet.py already asserts for it.  The
measured figures (``pytest -s`` of this file on the MI355X) are in profiles/dmd_deeponet_kernels_pytest.txt."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeponet_kernel_cases as K            # noqa: E402

pytestmark = pytest.mark.gpu

# kernel -> the bound an existing test asserts for it, used INSTEAD of max(8 * e32, 1e-6); each entry names the measured figure that
# needs it (profiles/dmd_deeponet_kernels_pytest.txt)
EXISTING = {}


class HipKernels:
    """the entry points the drivers of tests/deeponet_kernel_cases.py call, on the library (the ``DeepONet.k_*`` wrappers allocate their
    outputs: the arena operands go to the C ABI directly)"""
    dev = "cuda"

    def __init__(self, ops):
        self.ops = ops

    def don_point_mlp(self, t, b, w, sc, out, B, N, p, cout):
        o = self.ops
        P, I = o._p, lambda z: o._p(z, torch.int32)               # (the planes: int16 pairs in an int32 arena)
        w1z, b1z, w2z, b2z, w3z, b3 = w
        if sc is None:
            o._lib.call("rpb_don_point_mlp", P(t), P(b), I(w1z), P(b1z), I(w2z), P(b2z), I(w3z), P(b3), P(out), B, N, p, cout, o._stream(),
                        label="don_point_mlp")
        else:
            o._lib.call("rpb_don_point_mlp_f16x2", P(t), P(b), I(w1z), P(b1z), I(w2z), P(b2z), I(w3z), P(b3), P(sc), P(out), B, N, p, cout,
                        o._stream(), label="don_point_mlp_f16x2")

    def don_trunk(self, axes, wb, out, T, H, W, p):
        o = self.ops
        o._lib.call("rpb_don_trunk", *(o._p(z) for z in axes), *(o._p(z) for z in wb), o._p(out), T, H, W, p, o._stream(), label="don_trunk")

    def don_bn_relu_pool(self, x, sc, sh, out, B, T, H, W, C, ldx, ldo, mode):
        o = self.ops
        o._lib.call("rpb_don_bn_relu_pool", o._p(x), o._p(sc), o._p(sh), o._p(out), B, T, H, W, C, ldx, ldo, mode, o._stream(),
                    label="don_bn_relu_pool")


@pytest.fixture(scope="module")
def kern():
    from realpdebench_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels(ops)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _ids(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("arith", ["f32", "f16x2"])
@pytest.mark.parametrize("shape", K.POINT_CASES, ids=_ids)
def test_point_mlp(kern, shape, arith):
    """N = 1, N < 32, N = 128 exactly, tails of 33 and 65, C_out = 1 and 16, every p; two calls bit-equal"""
    K.run_point_mlp_twice(kern, K.point_case(*shape), arith, EXISTING)


@pytest.mark.parametrize("shape", K.TRUNK_CASES, ids=_ids)
def test_trunk(kern, shape):
    """N = 1, N = 63, N = 64 exactly, a tail of 3; every p"""
    K.run_trunk(kern, K.trunk_case(*shape), EXISTING)


@pytest.mark.parametrize("dims,mode", [r for r in K.POOL_RUNS if r != K.POOL_SECOND_TRIP], ids=_ids)
def test_bn_relu_pool(kern, dims, mode):
    K.run_pool(kern, K.pool_case(*dims), mode, EXISTING)


def test_bn_relu_pool_refuses_max_pool_of_one_cell(kern):
    K.run_pool_refused(kern, K.pool_case(*K.POOL_REFUSED[0]), K.POOL_REFUSED[1])


@pytest.mark.parametrize("at", K.NAN_AT, ids=_ids)
@pytest.mark.parametrize("mode", [0, 1])
def test_bn_relu_pool_keeps_a_nan(kern, mode, at):
    """ReLU and max keep a NaN, as torch's do: exactly the windows / bins that contain it, in its channel"""
    K.run_pool_nan(kern, mode, at)


def test_bn_relu_pool_threads_take_a_second_trip(kern, cus):
    """(last: the 17 MB output) 1 064 960 float4 items against 16 blocks of 256 threads per compute unit"""
    dims, mode = K.POOL_SECOND_TRIP
    total, grid = K.pool_grid(dims, mode, cus)
    assert total > grid * 256 and K.pool_trips(dims, mode, cus) == 2, (total, grid, cus)
    K.run_pool(kern, K.pool_case(*dims), mode, EXISTING)
