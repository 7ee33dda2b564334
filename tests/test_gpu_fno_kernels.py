"""The FNO3d step kernels -- axis_gemm (csrc/rpb_axg.hip, rpb_axis_gemm.hip), mode_contract (rpb_mode_contract.hip), cell_mix at widths 64
and 128, cell_mix_feat and cell_mix_wgrad (rpb_cmx.hip), the fp32 cell_mix and its gather launch (rpb_cell.hip), bn_bwd_row /
bn_bwd_row_c128 (rpb_bwr.hip), the fp32 bn_bwd_row and bn_bwd_row_feat (rpb_bwd_row.hip), the head (rpb_pjf.hip, rpb_pjg.hip: head_bwd,
head_fwd_bwd, head_bwd_finalize) -- one launch at a time against the fp64 restatements of
tests/fno_kernel_cases.py, every call on guard-banded operands (tests/guarded.py): a stray write, an element never written (a partial
row of an idle wave, say) and a stray read that reaches a result are assertions of ``Arena.check()``, not GPU faults.  Shapes, inputs
and the drivers live in tests/fno_kernel_cases.py, shared with tests/test_fno_kernels_host.py, which proves without a GPU that the
restatements agree with autograd / torch.fft, that every case is well conditioned and that the same drivers fail on a stand-in with
one wrong term.

Bounds: each output against the fp64 restatement on Rel-L2 and on max |error| / max |reference|, bounded by max(8 * e32, 1e-6), e32
being the same measure of the fp32 CPU restatement that partitions its sums into per-wave partial rows as the launcher does; a case
with 8 * e32 > 1e-5 is rejected as badly conditioned; the kernel's output never enters a bound.  ``EXISTING`` names, for a kernel whose
MI355X result needs more, the bound tests/test_gpu_kernels.py already asserts for it.  The measured figures (``pytest -s`` of this file
on the MI355X) are in profiles/fno_kernels_pytest.txt.

The second-trip shapes are computed from the device's compute-unit count (``cus``) and come last."""
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                              # noqa: E402
import fno_kernel_cases as K                # noqa: E402

pytestmark = pytest.mark.gpu

# kernel -> the bound an existing test asserts for it, used INSTEAD of max(8 * e32, 1e-6); each entry names the measured figure that
# needs it (profiles/fno_kernels_pytest.txt)
EXISTING = {}


class HipKernels:
    """the entry points the drivers of tests/fno_kernel_cases.py call, on the library"""
    dev = "cuda"

    def __init__(self, ops):
        self.ops = ops

    def axis_gemm(self, x, out, Mt, G, K_, O, N, in_g, in_k, out_g, out_o, kv, accumulate, xf):
        from realpdebench_amd import _lib
        p = self.ops._p                                           # (ops.axis_gemm asserts Mt.shape, which a Sub does not have)
        _lib.call("rpb_axis_gemm", p(x), p(out), p(Mt), G, K_, O, N, in_g, in_k, out_g, out_o, K_ if kv is None else kv, int(accumulate),
                  *self.ops._xf(xf), self.ops._stream(), label=f"axis_gemm[K{K_}xO{O}]")

    def mode_contract_fwd(self, X, W, Y, B, M, C):
        self.ops.mode_contract_fwd(X, W, Y, B, M, C)

    def mode_contract_dgrad(self, GY, W, GX, B, M, C):
        self.ops.mode_contract_dgrad(GY, W, GX, B, M, C)

    def mode_contract_wgrad(self, X, GY, GW, B, M, C, accumulate):
        self.ops.mode_contract_wgrad(X, GY, GW, B, M, C, accumulate=accumulate)

    def cell_mix_writes_gz(self, ncell, KC, CO, K2, Wp):
        return self.ops.cell_mix_writes_gz(ncell, KC, CO, K2, Wp, True)

    def cell_mix_stat_rows(self, ncell, C, K2, Wp, bwd):
        return self.ops.cell_mix_stat_rows(ncell, C, C, K2, Wp, True, bwd)

    def cell_mix(self, x, Wc, bias, z2, GW, out, part, ncell, C, K2, Wp, transpose_w, xf, bnb, oxf, write_gz):
        self.ops.cell_mix(x, Wc, bias, z2, GW, out, part, ncell, C, C, K2, Wp, transpose_w=transpose_w, xf=xf, bnb=bnb, oxf=oxf,
                          write_gz=write_gz)

    def cell_mix_gather_rows(self, ncell, KC, CO):
        return self.ops.cell_mix_stat_rows(ncell, KC, CO, 0, 1, False, True)

    def cell_mix_gather(self, gu, Wm, out, part, ncell, KC, CO, dims, bnb):
        B, T, H, W, pad = dims
        self.ops.cell_mix(gu, Wm, None, None, None, out, part, ncell, KC, CO, 0, 1, transpose_w=True, gather=True,
                          crop6=(T, H, W, T + pad, H + pad, W + pad), bnb=bnb)

    def cell_mix_feat(self, phi, Wcomp, bias, z2, GW, out, part, ncell, FW, K2, Wp, oxf):
        self.ops.cell_mix_feat(phi, Wcomp, bias, z2, GW, out, part, ncell, FW, K2, Wp, oxf=oxf)

    def bn_bwd_row_feat(self, s, gy, phi, gs, stat, sums, count, gelu, GW, Y1, part, G, Wp, C, K2, FW):
        self.ops.bn_bwd_row_feat(s, gy, phi, gs, *stat, sums, count, gelu, GW, Y1, part, G, Wp, C, K2, FW)

    def cell_mix_wgrad_slots(self, ncell, Wp):
        return self.ops.cell_mix_wgrad_slots(ncell, Wp)

    def cell_mix_wgrad(self, gs, Wc, z2, GW, out, sp, wp, ncell, K2, Wp, bnb, write_gz):
        assert self.ops.cell_mix_wgrad_supported(ncell, K2, Wp)
        self.ops.cell_mix_wgrad(gs, Wc, z2, GW, out, sp, wp, ncell, K2, Wp, bnb, write_gz=write_gz)

    def bn_bwd_row_slots(self, G):
        return self.ops.bn_bwd_row_slots(G)

    def bn_bwd_row(self, s, gy, x, gs, stat, sums, count, gelu, xf, GW, Y1, part, G, Wp, C, K2):
        self.ops.bn_bwd_row(s, gy, x, gs, *stat, sums, count, gelu, xf, GW, Y1, part, G, Wp, C, K2)

    def bn_bwd_row_c128_supported(self, Wp, K2):
        return self.ops.bn_bwd_row_c128_supported(Wp, K2)

    def bn_bwd_row_c128(self, s, gy, gs, stat, sums, count, gelu, GW, Y1, part, G, Wp, K2):
        self.ops.bn_bwd_row_c128(s, gy, gs, *stat, sums, count, gelu, GW, Y1, part, G, Wp, K2)

    def _dims(self, dims):
        B, T, H, W, pad, DO = dims
        return self.ops.Dims(B, T, H, W, DO, 64, pad)

    def head_bwd_slots(self, dims):
        return self.ops.head_bwd_slots(self._dims(dims))

    def head_bwd_row(self, DO):
        return self.ops.head_bwd_row(DO)

    def head_bwd(self, s, w1, b1, w2, gout, g, part, dims, DO, stat):
        d = self._dims(dims)
        assert self.ops.head_bwd_supported(64, DO, d.W, d.Wp, False, 0)
        self.ops.head_bwd(s, w1, b1, w2, gout, g, part, d, DO, tuple(stat) + (False,))

    def head_fwd_bwd(self, s, w1, b1, w2, b2, target, gscale, g, part, lpart, dims, DO, stat):
        self.ops.head_fwd_bwd(s, w1, b1, w2, b2, target, gscale, g, part, lpart, self._dims(dims), DO, tuple(stat) + (False,))

    def reduce_partials(self, part, rows, L, out):
        self.ops.reduce_partials(part, rows, L, out_f32=out)

    def head_bwd_finalize(self, tot, w1, gamma, beta, DO, dw1, dw2, db1, db2, bn_sums):
        self.ops.head_bwd_finalize(tot, w1, gamma, beta, DO, dw1, dw2, db1, db2, bn_sums)


@pytest.fixture(scope="module")
def kern():
    from realpdebench_amd import ops
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return HipKernels(ops)


@pytest.fixture(scope="module")
def cus(kern):
    """the restated slot counts of the cases module are the library's, on this device"""
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    ops = kern.ops
    for lines in (1, 3, 9, 8 * n - 1, 8 * n + 5, 10 ** 6):
        for bwd in (False, True):
            assert ops.cell_mix_stat_rows(32 * lines, 64, 64, 32, 32, True, bwd) == K.cmx_stat_rows(lines, n)
            assert ops.cell_mix_stat_rows(134 * lines, 128, 128, 32, 134, True, bwd) == K.cmx128_stat_rows(lines, 134, n)
            assert ops.cell_mix_stat_rows(70 * lines, 128, 128, 32, 70, True, bwd) == K.cmx128_stat_rows(lines, 70, n)
        assert ops.cell_mix_wgrad_slots(32 * lines, 32) == K.cmx_wg_slots(lines, n)
        assert ops.bn_bwd_row_slots(lines) == K.bn_bwd_row_slots(lines, n)
        assert ops.head_bwd_slots(ops.Dims(1, 1, lines, 4, 2, 64, 2)) == K.head_slots(lines, n)
        for bwd in (False, True):                                 # the fp32 kernel: 32-cell tiles, fewer waves with the BN-backward sums
            assert ops.cell_mix_stat_rows(18 * lines, 32, 32, 8, 18, True, bwd) == K.cell_fp32_rows(18 * lines, 32, 32, 8, 18, True, bwd, n)
        assert ops.cell_mix_stat_rows(630 * lines, 128, 64, 0, 1, False, True) == K.cell_fp32_rows(630 * lines, 128, 64, 0, 1, False, True, n)
    return n


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)                        # one case, one pair of references, however many tests look at it


def _ids(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


# ================================================================================================ axis_gemm
@pytest.mark.parametrize("shape", K.AXG_CASES, ids=_ids)
def test_axis_gemm(kern, shape):
    K.run_axis_gemm(kern, case_of(K.axg_case, shape), EXISTING)


# ================================================================================================ mode_contract
@pytest.mark.parametrize("shape", K.MODE_CASES, ids=_ids)
def test_mode_contract(kern, shape):
    K.run_mode_contract(kern, case_of(K.mode_case, shape), EXISTING)


# ================================================================================================ cell_mix
@pytest.mark.parametrize("mode", K.CMX_MODES)
@pytest.mark.parametrize("shape", K.CMX_SHAPES, ids=_ids)
def test_cell_mix(kern, cus, shape, mode):
    K.run_cell_mix(kern, case_of(K.cmx_case, shape + (cus,)), mode, EXISTING)


@pytest.mark.parametrize("mode", K.CMX_MODES)
@pytest.mark.parametrize("shape", K.CMX128_SHAPES, ids=_ids)
def test_cell_mix_c128(kern, cus, shape, mode):
    """width 128: workgroup pairs, one 64-channel output half each"""
    K.run_cell_mix(kern, case_of(K.cmx_case, shape + (cus, 128)), mode, EXISTING)


@pytest.mark.parametrize("mode", K.CELL_FP32_MODES)
@pytest.mark.parametrize("shape", K.CELL_FP32_SHAPES, ids=_ids)
def test_cell_mix_fp32_kernel(kern, cus, shape, mode):
    """csrc/rpb_cell.hip (C = 32, or lines shorter than a tile): 32-cell tiles that straddle lines, a ragged last tile"""
    K.run_cell_mix(kern, case_of(K.cmx_case, shape[:3] + (cus, shape[3])), mode, EXISTING)


@pytest.mark.parametrize("gelu", [True, False])
def test_cell_mix_gather_with_bn_backward_sums(kern, cus, gelu):
    K.run_cell_mix_gather(kern, case_of(K.gather_case, (gelu, cus)), EXISTING)


@pytest.mark.parametrize("mode", ["fwd", "oxf"])
@pytest.mark.parametrize("shape", K.FEAT_SHAPES, ids=_ids)
def test_cell_mix_feat(kern, cus, shape, mode):
    K.run_cell_mix_feat(kern, case_of(K.feat_case, shape + (cus,)), mode, EXISTING)


@pytest.mark.parametrize("gelu,write_gz", K.WG_MODES)
@pytest.mark.parametrize("shape", K.WG_SHAPES, ids=_ids)
def test_cell_mix_wgrad(kern, cus, shape, gelu, write_gz):
    K.run_cell_mix_wgrad(kern, case_of(K.wg_case, shape + (gelu, write_gz, cus)), EXISTING)


# ================================================================================================ bn_bwd_row
@pytest.mark.parametrize("variant", K.BWR_VARIANTS, ids=_ids)
@pytest.mark.parametrize("shape", K.BWR_SHAPES, ids=_ids)
def test_bn_bwd_row(kern, cus, shape, variant):
    K.run_bn_bwd_row(kern, case_of(K.bwr_case, shape + variant + (cus,)), EXISTING)


@pytest.mark.parametrize("variant", K.BWR32_VARIANTS, ids=_ids)
def test_bn_bwd_row_c32_fp32_kernel(kern, cus, variant):
    K.run_bn_bwd_row(kern, case_of(K.bwr_case, K.BWR32_SHAPE + variant + (cus, 32)), EXISTING)


@pytest.mark.parametrize("FW,gelu,inplace", K.BWRF_VARIANTS)
def test_bn_bwd_row_feat(kern, cus, FW, gelu, inplace):
    """layer 0: the field moments in columns < FW of the block, zeros up to column 31, the rest unwritten; gs in place, or not stored"""
    K.run_bn_bwd_row(kern, case_of(K.bwr_case, K.BWRF_SHAPE + ("x", None, gelu, inplace, cus, 64, FW)), EXISTING)


@pytest.mark.parametrize("gelu,inplace", K.BWR128_VARIANTS)
@pytest.mark.parametrize("shape", K.BWR128_SHAPES, ids=_ids)
def test_bn_bwd_row_c128(kern, cus, shape, gelu, inplace):
    K.run_bn_bwd_row_c128(kern, case_of(K.bwr128_case, shape + (gelu, inplace, cus)), EXISTING)


# ================================================================================================ the head
@pytest.mark.parametrize("shape", K.HEAD_SHAPES, ids=_ids)
def test_head(kern, cus, shape):
    K.run_head(kern, case_of(K.head_case, shape + (cus,)), EXISTING)


# ================================================================================================ refusals
def _all(*shape):
    return torch.ones(shape, dtype=torch.bool)


def test_refusals_leave_everything_untouched(kern):
    """what include/rpb.h and the RPB_REQUIRE texts document: an error code before any launch"""
    from realpdebench_amd._lib import RpbError
    ops, C = kern.ops, 64

    def refused(match, build):
        a = guarded.Arena("cuda")
        call = build(a)
        with pytest.raises(RpbError, match=match):
            call()
        a.check()                                                 # every guard and every output sentinel is intact

    def axg(N, K_, kv, xf):
        def build(a):
            x, Mt, out = a.inp(torch.ones(2, K_, N)), a.inp(torch.ones(K_, 4)), a.out(2, 4, N, unwritten=_all(2, 4, N))
            v = tuple(a.inp(torch.ones(N)) for _ in range(4)) if xf else None
            return lambda: kern.axis_gemm(x.op, out.op, Mt.op, 2, K_, 4, N, K_ * N, N, 4 * N, N, kv, False,
                                          tuple(t.op for t in v) + (True,) if v else None)
        return build
    refused("axis_gemm: N=", axg(33, 4, None, False))
    refused("axis_gemm: k_valid", axg(64, 4, 5, False))
    refused("axis_gemm: input transform", axg(256, 4, None, True))

    # (the C entry point of cell_mix_wgrad has no bias argument -- "no bias" is a requirement of the launcher behind it that the ABI
    # cannot violate; what the entry point itself refuses: a missing partial buffer, K2 > 32, a line shorter than a tile)
    def wgrad(K2, Wp, with_wg_part):
        def build(a):
            n = 2 * Wp
            gs, Wc, z2, FW, s = (a.inp(torch.ones(*sh)) for sh in ((n, C), (C, C), (2, K2, C), (K2, Wp), (n, C)))
            v = [a.inp(torch.ones(C)) for _ in range(4)]
            out, sp, wp = a.out(n, C, unwritten=_all(n, C)), a.out(4, 2, C, unwritten=_all(4, 2, C)), a.out(4, C, C, unwritten=_all(4, C, C))
            return lambda: ops.cell_mix_wgrad(gs.op, Wc.op, z2.op, FW.op, out.op, sp.op, wp.op if with_wg_part else None, n, K2, Wp,
                                              (s.op, v[0].op, v[1].op, v[2].op, v[3].op, True))
        return build
    refused("cell_mix_wgrad: null pointer", wgrad(8, 32, False))
    refused("cell_mix_wgrad: needs C = 64", wgrad(33, 32, True))
    refused("cell_mix_wgrad: needs C = 64", wgrad(8, 31, True))

    def head(a):
        d, DO = ops.Dims(1, 1, 2, 4, 5, C, 2), 5
        s, w1, b1, w2, gout = (a.inp(torch.ones(*sh)) for sh in ((d.ncell, C), (128, C), (128,), (DO, 128), (d.ncrop, DO)))
        v = [a.inp(torch.ones(C)) for _ in range(4)]
        g, part = a.out(d.ncell, C, unwritten=_all(d.ncell, C)), a.out(4, 128 * C + 6 * 128 + 5, unwritten=_all(4, 128 * C + 6 * 128 + 5))
        return lambda: ops.head_bwd(s.op, w1.op, b1.op, w2.op, gout.op, g.op, part.op, d, DO, (v[0].op, v[1].op, v[2].op, v[3].op, False))
    refused("head_bwd: unsupported shape", head)

    def c128(a):
        G, Wp, K2 = 2, 32, 49
        s, gy, GW = a.inp(torch.ones(G * Wp, 128)), a.inp(torch.ones(G * Wp, 128)), a.inp(torch.ones(Wp, K2))
        v = [a.inp(torch.ones(128)) for _ in range(4)] + [a.inp(torch.ones(256))]
        gs, Y1 = a.out(G * Wp, 128, unwritten=_all(G * Wp, 128)), a.out(G, K2, 128, unwritten=_all(G, K2, 128))
        part = a.out(16, C * C + C, unwritten=_all(16, C * C + C))
        return lambda: ops.bn_bwd_row_c128(s.op, gy.op, gs.op, v[0].op, v[1].op, v[2].op, v[3].op, v[4].op, G * Wp, False, GW.op, Y1.op,
                                           part.op, G, Wp, K2)
    refused("bn_bwd_row_c128: unsupported", c128)

    def mode(entry, Cc):
        def build(a):
            B, M = 2, 3
            X, W, Y = a.inp(torch.ones(B, 2, M, Cc)), a.inp(torch.ones(M, Cc, Cc, 2)), a.out(B, 2, M, Cc, unwritten=_all(B, 2, M, Cc))
            return lambda: getattr(ops, entry)(X.op, W.op, Y.op, B, M, Cc)
        return build
    refused("mode_contract: C=", mode("mode_contract_fwd", 48))
    refused("mode_contract: C=", mode("mode_contract_dgrad", 48))

    def mode_wgrad(a):
        B, M, Cc = 2, 3, 48
        X, GY, GW = a.inp(torch.ones(B, 2, M, Cc)), a.inp(torch.ones(B, 2, M, Cc)), a.out(M, Cc, Cc, 2, unwritten=_all(M, Cc, Cc, 2))
        return lambda: ops.mode_contract_wgrad(X.op, GY.op, GW.op, B, M, Cc)
    refused("mode_contract: C=", mode_wgrad)


# ================================================================================================ second trips (last: the large shapes)
def test_axis_gemm_waves_take_a_second_trip(kern, cus):
    for shape in K.axg_trip_cases(cus):
        G, K_, O, N = shape[:4]
        t = K.trips(G * (N // 64), K.axg_slots(G, N, cus))
        assert t.count(2) == 3 and t.count(1) == len(t) - 3
        K.run_axis_gemm(kern, K.axg_case(*shape), EXISTING)


def test_mode_contract_persistent_workgroups_take_a_second_mode(kern, cus):
    C, B, M = K.mode_trip_case(cus)
    assert K.trips(M, K.mode_grid(M, cus)).count(2) == 5
    K.run_mode_contract(kern, K.mode_case(C, B, M), EXISTING)


def test_bn_bwd_row_waves_take_a_second_trip(kern, cus):
    G, Wp, K2 = K.bwr_trip_shape(cus)
    assert K.trips(G, K.bwr_slots(G, cus)).count(2) == 3
    for variant in K.BWR_TRIP_VARIANTS:
        K.run_bn_bwd_row(kern, K.bwr_case(G, Wp, K2, *variant, cus), EXISTING)


def test_head_waves_take_a_second_line(kern, cus):
    for shape in K.head_trip_shapes(cus):
        lines = shape[1] * shape[2]
        assert K.trips(lines, K.head_slots(lines, cus)).count(2) == 3
        K.run_head(kern, K.head_case(*shape, cus), EXISTING)


def test_cell_mix_wgrad_wave_pairs_take_a_second_trip(kern, cus):
    Wp, lines, K2 = K.wg_trip_shape(cus)
    assert K.trips(lines, K.cmx_wg_slots(lines, cus)).count(2) == 3
    K.run_cell_mix_wgrad(kern, K.wg_case(Wp, lines, K2, True, True, cus), EXISTING)


def test_cell_mix_c128_waves_take_a_second_trip(kern, cus):
    Wp, lines, K2 = K.cmx128_trip_shape(cus)
    assert K.trips(lines, K.cmx128_stat_rows(lines, Wp, cus)).count(2) == 5
    c = K.cmx_case(Wp, lines, K2, cus, 128)
    for mode in ("fwd+bn+gelu", "bwd+gelu+gz", "plain"):
        K.run_cell_mix(kern, c, mode, EXISTING)


def test_cell_mix_waves_take_a_second_trip_in_every_claim_mode(kern, cus):
    """with statistics the dealt walk is used in every mode (the partial rows are sums over the lines a wave walked); without, the lines
    are dealt (0), claimed from the workgroup's LDS counter (1) or from one counter in HBM (2): each against fp64, not against each other"""
    from realpdebench_amd import _lib
    Wp, lines, K2 = K.cmx_trip_shape(cus)
    assert K.trips(lines, K.cmx_stat_rows(lines, cus)).count(2) == 5
    c = K.cmx_case(Wp, lines, K2, cus)
    K.run_cell_mix(kern, c, "fwd+bn+gelu", EXISTING)
    K.run_cell_mix(kern, c, "bwd+gelu+gz", EXISTING)
    try:
        for mode in K.CLAIM_MODES:
            _lib.call("rpb_line_claim_set", mode)
            print(f"[fno-kernels] line claim mode {mode}")
            K.run_cell_mix(kern, c, "fwd+bn+gelu", EXISTING, with_stats=False)
            K.run_cell_mix(kern, c, "plain", EXISTING)
    finally:
        _lib.call("rpb_line_claim_set", -1)
