"""The step plumbing kernels -- the lift and its backward, lift_feat, feat_mix, feat_mix_wgrad and small_gemm (csrc/rpb_feat.hip), the cell
BatchNorm passes, mse, Adam (plain and ranged), the normaliser affines, mul, the reducers (csrc/rpb_pointwise.hip), pair_pack and
window_pack (csrc/rpb_io.hip) and the spectrum bins of ``eval_metrics`` (csrc/rpb_metrics.hip) -- one launch at a time against the
fp64 restatements of tests/plumbing_kernel_cases.py, every call on guard-banded operands (tests/guarded.py): a stray write, an element
never written (a partial row of an idle block: no partial buffer is pre-zeroed here) and a stray read that reaches a result (the
padding columns of ``Phi``, the margin of the lift's gradient, the gaps of a strided operand all hold NaN) are assertions of
``Arena.check()``, not GPU faults.  Shapes, inputs and the drivers live in tests/plumbing_kernel_cases.py, shared with
tests/test_plumbing_kernels_host.py, which proves without a GPU that the restatements agree with autograd / torch.optim.Adam / a
triple loop with ``math.isqrt``, that every case is well conditioned and that the same drivers fail on a stand-in with one wrong term
or one out-of-range access.

Bounds: each output against the fp64 restatement on Rel-L2 and on max |error| / max |reference|, bounded by max(8 * e32, 1e-6), e32
being the same measure of the fp32 CPU restatement that partitions its sums into per-block partial rows as the launcher does and
accumulates in fp64 where the kernel does; a case with 8 * e32 > 1e-5 is rejected as badly conditioned; the kernel's output never
enters a bound.  Adam is judged on its update p_out - p_in, on m and on v, against a reference computed from the hyperparameters as the
ABI receives them.  Kernels that only move data (mul, lift_feat, the zero margin of the lift, the zero fill of window_pack, the
elements outside Adam's ranges) are asserted bit-equal, and so is the ranged Adam launch against the plain one.  ``EXISTING`` names, for
a kernel whose MI355X result needs more, the bound tests/test_gpu_kernels.py already asserts for it.  The measured figures
(``pytest -s`` of this file on the MI355X) are in profiles/plumbing_kernels_pytest.txt.

The second-trip shapes are computed from the device's compute-unit count (``cus``) and come last."""
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import plumbing_kernel_cases as K           # noqa: E402

pytestmark = pytest.mark.gpu

# kernel -> the bound an existing test asserts for it, used INSTEAD of max(8 * e32, 1e-6); each entry names the measured figure that
# needs it (profiles/plumbing_kernels_pytest.txt)
EXISTING = {}


class HipKernels:
    """the entry points the drivers of tests/plumbing_kernel_cases.py call, on the library"""
    dev = "cuda"

    def __init__(self, ops):
        self.ops = ops

    def _dims(self, dims):
        B, T, H, W, Cin, C, pad = dims
        return self.ops.Dims(B, T, H, W, Cin, C, pad)

    def lift_pad_fwd(self, x, grids, w0, b0, out, dims):
        self.ops.lift_pad_fwd(x, grids, w0, b0, out, self._dims(dims))

    def lift_bwd_rows(self):
        return self.ops._lib.query("rpb_lift_bwd_rows")

    def lift_bwd(self, g, x, grids, part, dims):
        self.ops.lift_bwd(g, x, grids, part, self._dims(dims))

    def lift_feat(self, x, grids, out, dims, FW):
        self.ops.lift_feat(x, grids, out, self._dims(dims), FW)

    def feat_mix(self, Phi, w0, b0, Xh, B, M2, NB, Cin, C):
        self.ops.feat_mix(Phi, w0, b0, Xh, B, M2, NB, Cin, C)

    def feat_mix_wgrad_rows(self):
        return self.ops.feat_mix_wgrad_rows()

    def feat_mix_wgrad(self, G, Phi, part, B, M2, NB, Cin, C):
        self.ops.feat_mix_wgrad(G, Phi, part, B, M2, NB, Cin, C)

    def small_gemm(self, A, Bm, out, M, N, K_, a_rs, a_cs, b_rs, b_cs, ldo, accumulate):
        self.ops.small_gemm(A, Bm, out, M, N, K_, a_rs, a_cs, b_rs, b_cs, ldo, accumulate=accumulate)

    def bn_finalize(self, sums, count, eps, momentum, mean, invstd, rmean, rvar, C):
        self.ops.bn_finalize(sums, count, eps, momentum, mean, invstd, rmean, rvar, C)

    def bn_eval_prep(self, rvar, eps, invstd, C):
        self.ops.bn_eval_prep(rvar, eps, invstd, C)

    def bn_act_fwd(self, s, stat, y, ncell, C, gelu):
        self.ops.bn_act_fwd(s, *stat, y, ncell, C, gelu)

    def bn_bwd_rows(self):
        return self.ops.bn_bwd_rows()

    def bn_bwd_reduce(self, s, gy, stat, part, ncell, C, gelu):
        self.ops.bn_bwd_reduce(s, gy, *stat, part, ncell, C, gelu)

    def bn_bwd_apply(self, s, gy, stat, sums, count, gs, ncell, C, gelu):
        self.ops.bn_bwd_apply(s, gy, *stat, sums, count, gs, ncell, C, gelu)

    def mse_rows(self):
        return self.ops.mse_rows()

    def mse(self, pred, tgt, elem, gout, part, n, gscale):
        self.ops.mse(pred, tgt, elem, gout, part, n, gscale)

    def adam_step(self, p, g, m, v, n, lr, b1, b2, eps, step, gscale):
        self.ops.adam_step(p, g, m, v, n, lr, b1, b2, eps, step, gscale)

    def adam_step_ranges(self, p, g, m, v, tab, nr, total, lr, b1, b2, eps, step, gscale):
        self.ops.adam_step_ranges(p, g, m, v, tab, nr, total, lr, b1, b2, eps, step, gscale)

    def rollout_affine(self, pred, para, out, ncell, Cp, Cx, mean_t, std_t, mean_i, std_i):
        self.ops.rollout_affine(pred, para, out, ncell, Cp, Cx, mean_t, std_t, mean_i, std_i)

    def channel_affine(self, x, out, n, C, mean, std, inverse):
        self.ops.channel_affine(x, out, n, C, mean, std, inverse)

    def mul(self, a, b, out, n):
        self.ops.mul(a, b, out, n)

    def pair_pack(self, num, real, para, inp, tgt, B, ntok, Cl, n_para, mean_in, mean_tgt, std_in, std_tgt):
        from realpdebench_amd import _lib
        p = self.ops._p                                           # (ops.pair_pack counts the bytes of tensors: a Sub has no numel)
        _lib.call("rpb_pair_pack", p(num), p(real), p(para), p(inp), p(tgt), B, ntok, Cl, n_para, p(mean_in), p(mean_tgt), p(std_in),
                  p(std_tgt), self.ops._stream(), label="pair_pack")

    def window_pack(self, planar, cl, flags, inp, tgt, B, horizon, in_step, Hf, Wf, sub_s, n_para, Cp, Cl, mean_in, mean_tgt, std_in,
                    std_tgt, rows_subsampled):
        from realpdebench_amd import _lib
        p = self.ops._p
        _lib.call("rpb_window_pack", p(planar), p(cl), p(flags), p(inp), p(tgt), B, horizon, in_step, Hf, Wf, sub_s, int(rows_subsampled),
                  n_para, Cp, Cl, p(mean_in), p(mean_tgt), p(std_in), p(std_tgt), self.ops._stream(), label="window_pack")

    def reduce_partials(self, part, rows, L, stride, outf, outd, scale, accumulate):
        self.ops.reduce_partials(part, rows, L, out_f32=outf, out_f64=outd, scale=scale, accumulate=accumulate, row_stride=stride)

    def reduce_partials_batched(self, part, nbatch, rows, L, stride, batch_stride, out):
        from realpdebench_amd import _lib                         # (ops.reduce_partials_batched passes contiguous blocks only)
        _lib.call("rpb_reduce_partials_batched", self.ops._p(part), nbatch, rows, L, stride, batch_stride, self.ops._p(out), self.ops._stream())

    def reduce_grouped_cols(self):
        return self.ops._lib.query("rpb_reduce_partials_grouped_cols")

    def addr(self, operand):
        return self.ops._p(operand.op)

    def reduce_partials_grouped(self, tab, n, total_chunks):
        from realpdebench_amd import _lib
        _lib.call("rpb_reduce_partials_grouped", tab.data_ptr(), n, total_chunks, self.ops._stream(), label="reduce_partials_grouped")

    def spectrum_bin(self, Y, out, R, NB):
        self.ops.spectrum_bin(Y, out, R, NB)


@pytest.fixture(scope="module")
def kern():
    from realpdebench_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels(ops)


@pytest.fixture(scope="module")
def cus(kern):
    """the restated slot and row counts of the cases module are the library's, on this device"""
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert kern.mse_rows() == K.mse_rows(n)
    assert kern.bn_bwd_rows() == K.bn_bwd_rows(n)
    assert kern.lift_bwd_rows() == K.lift_bwd_rows(n)
    assert kern.feat_mix_wgrad_rows() == K.feat_mix_wgrad_rows(n)
    assert kern.reduce_grouped_cols() == K.GROUPED_COLS
    return n


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)                        # one case, one pair of references, however many tests look at it


def _ids(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


# ================================================================================================ lift
@pytest.mark.parametrize("dims", K.LIFT_CASES, ids=_ids)
def test_lift_pad_fwd(kern, cus, dims):
    """F = 5, 6, 8, 19 and the generic instantiation, one of them past the 2048-input prefetch; exact zeros in the margin"""
    K.run_lift_fwd(kern, case_of(K.lift_case, dims + (cus,)), EXISTING)


@pytest.mark.parametrize("dims", K.LIFT_CASES, ids=_ids)
def test_lift_bwd(kern, cus, dims):
    """F = 3, 5, 6, 8, 19 and the generic instantiation; every row of ``part`` written, the margin of the gradient (NaN) never read"""
    K.run_lift_bwd(kern, case_of(K.lift_case, dims + (cus,)), EXISTING)


@pytest.mark.parametrize("dims", K.LIFT_FEAT_CASES, ids=_ids)
def test_lift_feat(kern, dims):
    K.run_lift_feat(kern, case_of(K.lift_feat_case, dims), EXISTING)


# ================================================================================================ layer-0 feature algebra
@pytest.mark.parametrize("shape", K.FEAT_MIX_CASES, ids=_ids)
def test_feat_mix(kern, cus, shape):
    K.run_feat_mix(kern, case_of(K.feat_case, shape + (cus,)), EXISTING)


@pytest.mark.parametrize("shape", K.FEAT_WGRAD_CASES, ids=_ids)
def test_feat_mix_wgrad(kern, cus, shape):
    K.run_feat_mix_wgrad(kern, case_of(K.feat_case, shape + (cus,)), EXISTING)


@pytest.mark.parametrize("shape", K.SMALL_GEMM_CASES, ids=_ids)
def test_small_gemm(kern, shape):
    K.run_small_gemm(kern, case_of(K.small_gemm_case, shape), EXISTING)


# ================================================================================================ cell BatchNorm
@pytest.mark.parametrize("gelu", [True, False])
@pytest.mark.parametrize("ncell", [1, 257])
@pytest.mark.parametrize("C", K.BN_C)
def test_batchnorm_passes(kern, cus, C, ncell, gelu):
    c = case_of(K.bn_case, (C, ncell, gelu, cus))
    K.run_bn_act_fwd(kern, c, EXISTING)
    K.run_bn_bwd_reduce(kern, c, EXISTING)
    K.run_bn_bwd_apply(kern, c, EXISTING)


@pytest.mark.parametrize("shape", K.BN_FINALIZE_CASES, ids=_ids)
def test_bn_finalize_and_eval_prep(kern, shape):
    K.run_bn_finalize(kern, case_of(K.bn_finalize_case, shape), EXISTING)
    K.run_bn_eval_prep(kern, case_of(K.bn_eval_prep_case, (shape[0],)), EXISTING)


# ================================================================================================ loss and optimizer
@pytest.mark.parametrize("with_elem,with_gout", K.MSE_OUTPUTS)
@pytest.mark.parametrize("n", [1, 255])
def test_mse(kern, cus, n, with_elem, with_gout):
    K.run_mse(kern, case_of(K.mse_case, (n, cus)), with_elem, with_gout, EXISTING)


@pytest.mark.parametrize("run", [r for r in K.adam_runs() if r[0] <= 1003], ids=_ids)
def test_adam_step(kern, run):
    """single calls from a preloaded state (n, step, |g| regime); the update, m and v are judged, p is not"""
    K.run_adam(kern, case_of(K.adam_case, run), EXISTING)


def test_adam_step_chained_with_a_changing_lr(kern):
    K.run_adam_chain(kern, case_of(K.adam_chain_case, ()), EXISTING)


@pytest.mark.parametrize("name", [n for n in K.adam_range_tables() if n != "past a grid trip"])
def test_adam_step_ranges(kern, cus, name):
    """bit-equal to rpb_adam_step over the same elements, everything outside the ranges bit-identical to its preload"""
    K.run_adam_ranges(kern, case_of(K.adam_ranges_case, (name, cus)), EXISTING)


# ================================================================================================ normaliser affines and small movers
@pytest.mark.parametrize("stats", K.AFFINE_STATS, ids=_ids)
@pytest.mark.parametrize("shape", K.rollout_shapes()[:2], ids=_ids)
def test_rollout_affine(kern, shape, stats):
    K.run_rollout_affine(kern, case_of(K.rollout_case, shape + stats), EXISTING)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("C", [1, 3, 16])
def test_channel_affine(kern, C, inverse):
    K.run_channel_affine(kern, case_of(K.channel_affine_case, (350 * C, C, inverse)), EXISTING)


@pytest.mark.parametrize("n", K.MUL_SIZES)
def test_mul(kern, n):
    K.run_mul(kern, case_of(K.mul_case, (n,)), EXISTING)


@pytest.mark.parametrize("shape", K.PAIR_PACK_CASES, ids=_ids)
def test_pair_pack(kern, shape):
    K.run_pair_pack(kern, case_of(K.pair_pack_case, shape), EXISTING)


@pytest.mark.parametrize("spec", K.WINDOW_PACK_CASES, ids=lambda s: s[0].replace(" ", "_"))
def test_window_pack(kern, spec):
    K.run_window_pack(kern, K.window_pack_case(spec), EXISTING)


# ================================================================================================ reducers
@pytest.mark.parametrize("shape", K.REDUCE_CASES, ids=_ids)
def test_reduce_partials(kern, shape):
    """the wide / tall switch at 256 rows, gapped rows, accumulating launches; the fp32 output, the fp64 output, and both"""
    K.run_reduce_partials(kern, case_of(K.reduce_case, shape), EXISTING)


@pytest.mark.parametrize("shape", K.REDUCE_BATCHED_CASES, ids=_ids)
def test_reduce_partials_batched(kern, shape):
    K.run_reduce_batched(kern, case_of(K.reduce_batched_case, shape), EXISTING)


def test_reduce_partials_grouped(kern, cus):
    K.run_reduce_grouped(kern, K.reduce_grouped_case(), EXISTING)


# ================================================================================================ spectrum bins
@pytest.mark.parametrize("shape", K.SPECTRUM_CASES, ids=_ids)
def test_spectrum_bin(kern, shape):
    K.run_spectrum_bin(kern, case_of(K.spectrum_case, shape), EXISTING)


# ================================================================================================ second trips (last: the large shapes)
def test_lift_blocks_take_a_second_row(kern, cus):
    """the forward: a live row after a live one (prefetched), a pad row after a live one, a live row after a pad one; the backward: 4 CUs + 3
    rows of the data"""
    dims = K.lift_fwd_trip_dims(cus)
    assert {"live>live", "live>pad", "pad>live"} <= K.lift_fwd_handoffs(dims, cus)
    K.run_lift_fwd(kern, K.lift_case(*dims, cus), EXISTING)
    dims = K.lift_bwd_trip_dims(cus)
    assert K.trips(dims[0] * dims[1] * dims[2], K.lift_bwd_rows(cus)).count(2) >= 3
    K.run_lift_bwd(kern, K.lift_case(*dims, cus), EXISTING)


def test_lift_feat_waves_take_a_second_row(kern, cus):
    dims = K.lift_feat_trip_dims(cus)
    assert K.trips(dims[0] * (dims[1] + dims[5]) * (dims[2] + dims[5]), 32 * cus).count(2) >= 5
    K.run_lift_feat(kern, K.lift_feat_case(*dims), EXISTING)


def test_feat_mix_threads_take_a_second_trip(kern, cus):
    C, Cin, B, M2 = K.feat_mix_trip_case(cus)
    assert B * M2 * C // 4 >= 8 * cus * 256 + 5
    K.run_feat_mix(kern, K.feat_case(C, Cin, B, M2, cus), EXISTING)


def test_feat_mix_wgrad_blocks_take_a_second_trip(kern, cus):
    for shape in K.feat_wgrad_trip_cases(cus):
        K.run_feat_mix_wgrad(kern, K.feat_case(*shape, cus), EXISTING)


@pytest.mark.parametrize("gelu", [True, False])
@pytest.mark.parametrize("C", K.BN_C)
def test_batchnorm_passes_take_a_second_trip(kern, cus, C, gelu):
    c = K.bn_case(C, K.bn_ncells(C, cus)[-1], gelu, cus)
    K.run_bn_act_fwd(kern, c, EXISTING)
    K.run_bn_bwd_reduce(kern, c, EXISTING)
    K.run_bn_bwd_apply(kern, c, EXISTING)


def test_mse_blocks_take_a_third_trip(kern, cus):
    c = K.mse_case(K.mse_sizes(cus)[-1], cus)
    for with_elem, with_gout in K.MSE_OUTPUTS:
        K.run_mse(kern, c, with_elem, with_gout, EXISTING)


def test_adam_step_second_trip_with_a_scalar_tail(kern, cus):
    n = K.adam_sizes(cus)[-1]
    K.run_adam(kern, K.adam_case(n, 2, "unit"), EXISTING)
    K.run_adam(kern, K.adam_case(n, 1000, "tiny"), EXISTING)


def test_adam_step_ranges_past_a_grid_trip(kern, cus):
    K.run_adam_ranges(kern, K.adam_ranges_case("past a grid trip", cus), EXISTING)


def test_affines_take_a_second_trip(kern, cus):
    for stats in K.AFFINE_STATS:
        K.run_rollout_affine(kern, K.rollout_case(*K.rollout_shapes(cus)[-1], *stats), EXISTING)
    for shape in K.channel_affine_cases(cus)[-2:]:
        K.run_channel_affine(kern, K.channel_affine_case(*shape), EXISTING)
