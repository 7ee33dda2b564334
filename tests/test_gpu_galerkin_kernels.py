"""The Galerkin Transformer kernels (csrc/rpb_galerkin.hip) and the token GEMMs / weight gradients in the combinations its training step
issues, one launch at a time against tests/galerkin_restatement.py, every call on guard-banded operands (tests/guarded.py): a stray
write, an element never written and a stray read that reaches a result are assertions of ``Arena.check()``, not GPU faults.  Shapes,
inputs and the drivers (arena layout, ``check()``, verdict) live in tests/galerkin_kernel_cases.py, shared with
tests/test_galerkin_kernels_host.py, which proves without a GPU that the restatements agree with autograd, that every case is well
conditioned and that the same drivers fail on a stand-in with one wrong term.

Bounds: each output against the fp64 restatement on Rel-L2 and on max |error| / max |reference|, bounded by max(8 * e32, 1e-6), e32
being the same measure of the fp32 CPU restatement; a case with 8 * e32 > 1e-5 is rejected as badly conditioned; the kernel's output
never enters a bound.  ``EXISTING`` names, for a kernel whose MI355X result needs more, the bound another test already asserts for it.
The measured figures (``pytest -s`` of this file on the MI355X) are in profiles/galerkin_kernels_pytest.txt.

Dropout has an independent reference here: the host's Philox4x32-10 (galerkin_restatement.dropout_mask).  ``dropout_mul`` and
``head_apply`` equal ``x * host mask`` bit for bit; at the GEMM sites an element the host mask drops (at the documented index
m * ldo + n) is exactly 0.0 before the residual, a kept one is not, and the values pass the bound against the fp64 reference formed with
the host mask -- on the exact-fp32 kernel and on the 64-row-tile split kernel, at ldo == N and ldo != N.

The token GEMMs go through ``ops.gemm_nt``; the test records the entry point from the ``label`` of ``_lib.call`` and asserts the kernel
the dispatch must choose, so that a moved threshold cannot turn two cases into duplicates.  Which split kernel ``rpb_gemm3x`` runs is
the rule of rpb_gemm3x2_supported (csrc/rpb_gemm3x2.hip), restated in the cases module because the C ABI does not export it.  No
Galerkin site reaches the 128-row split kernel through ``ops.gemm_nt`` (a mask tensor with K, N <= 256 stays on the exact-fp32 kernel
at any row count -- M = 65 613 included, which is asserted -- and without a mask tensor the 64-row-tile kernel takes N % 128 == 0):
``test_token_gemm_sites_with_the_row_threshold_lowered`` asserts that with ``ops.GEMM_SPLIT_MIN_ROWS`` at 0 as well, and
``test_split128_kernel_direct`` runs that kernel on the three mask-tensor epilogues through its own entry point."""
import contextlib
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                              # noqa: E402
import galerkin_kernel_cases as K           # noqa: E402

pytestmark = pytest.mark.gpu

C = K.C
# kernel -> the bound an existing test asserts for it, used INSTEAD of max(8 * e32, 1e-6); each entry names the measured figure that
# needs it (profiles/galerkin_kernels_pytest.txt)
EXISTING = {}


class HipKernels:
    """the entry points the drivers of tests/galerkin_kernel_cases.py call, on the library"""
    dev = "cuda"

    def __init__(self, ops):
        from realpdebench_amd import _lib
        self.ops, self.lib = ops, _lib

    @contextlib.contextmanager
    def labels(self):
        """the ``label`` of every ``_lib.call`` made inside"""
        seen, call = [], self.lib.call

        def recording(name, *args, label=None, **kw):
            seen.append(label or name)
            return call(name, *args, label=label, **kw)
        self.lib.call = recording
        try:
            yield seen
        finally:
            self.lib.call = call

    def headnorm_bwd_rows(self, M):
        return self.ops.headnorm_bwd_rows(M)

    def headnorm_fwd(self, x, ldx, gamma, beta, out, ldo, M, Cc, eps):
        self.ops.headnorm_fwd(x, ldx, gamma, beta, out, ldo, M, Cc, eps)

    def headnorm_bwd(self, x, ldx, gamma, gy, ldg, gx, ldgx, part, M, Cc, eps):
        self.ops.headnorm_bwd(x, ldx, gamma, gy, ldg, gx, ldgx, part, M, Cc, eps)

    def _dims(self, dims):
        B, T, H, W, Cc, pad = dims
        return self.ops.Dims(B, T, H, W, 0, Cc, pad)

    def pad_grid_fwd(self, U, gt, gh, gw, Wg, bias, out, dims):
        self.ops.pad_grid_fwd(U, [gt, gh, gw], Wg, bias, out, self._dims(dims))

    def crop_gather(self, g, out, dims):
        self.ops.crop_gather(g, out, self._dims(dims))

    def head_scores_chunks(self, B, n):
        return self.ops.head_scores_chunks(B, n)

    def head_scores(self, G, ldg, A, lda, part, B, n, nh):
        self.ops.head_scores(G, ldg, A, lda, part, B, n, nheads=nh)

    def head_apply(self, X, ldx, Wm, out, ldo, B, n, nh, residual, ldr, mask, ldm, drop):
        self.ops.head_apply(X, ldx, Wm, out, ldo, B, n, residual=residual, ldr=ldr, mask=mask, ldm=ldm, nheads=nh, drop=drop)

    def dropout_mul(self, g, out, n, seed, keep):
        self.ops.dropout_mul(g, out, n, seed, keep)

    def gemm_nt(self, A, W, out, M, N, Kk, bias, residual, act, aux, mask, drop, lda, ldo):
        with self.labels() as seen:
            self.ops.gemm_nt(A, W, out, M, N, Kk, bias=bias, residual=residual, act=act, lda=lda, ldo=ldo, aux=aux, mask=mask, drop=drop)
        gemms = [s for s in seen if s.startswith(("gemm_nt[", "gemm3x["))]
        assert len(gemms) == 1, seen
        return gemms[0]

    def gemm3x_direct(self, A, W, out, M, N, Kk, bias, residual, act, aux, mask, drop, lda, ldo):
        """the split branch of ops.gemm_nt, whatever its thresholds say"""
        p, st = self.ops._p, self.ops._stream()
        wz = torch.empty(3 * N * Kk, dtype=torch.int16, device=W.t.device)
        self.lib.call("rpb_gemm3x_wprep", p(W), p(wz, torch.int16), N, Kk, st, label="gemm3x_wprep")
        self.lib.call("rpb_gemm3x", p(A), p(wz, torch.int16), p(bias), None, p(residual), p(out), M, N, Kk, lda, ldo, int(act), p(aux), None,
                      p(mask), int(drop[0]) if drop else 0, float(drop[1]) if drop else 0.0, st, label=f"gemm3x[N{N},K{Kk}]")
        return f"gemm3x[N{N},K{Kk}]"

    def gemm_tn_splits(self, M, N, Kk, ldg, lda):
        return self.ops.gemm_tn_splits(M, N, Kk, ldg=ldg, lda=lda)

    def gemm_tn(self, G, A, part, M, N, Kk, ldg, lda):
        splits, L = self.gemm_tn_splits(M, N, Kk, ldg, lda), N * Kk + N
        rows = part.t[part.offset:part.offset + splits * L].view(splits, L)          # ops.gemm_tn sizes the partials by their shape
        with self.labels() as seen:
            self.ops.gemm_tn(G, A, rows, M, N, Kk, ldg=ldg, lda=lda)
        assert len(seen) == 1, seen
        return seen[0]


@pytest.fixture(scope="module")
def kern():
    from realpdebench_amd import ops
    return HipKernels(ops)


@pytest.fixture(scope="module")
def cus(kern):
    """the restated block counts of the cases module are the library's, on this device"""
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    ops = kern.ops
    assert ops.headnorm_bwd_rows(10 ** 9) == K.headnorm_rows(10 ** 9, n) and ops.headnorm_bwd_rows(5) == K.headnorm_rows(5, n)
    assert all(ops.head_scores_chunks(B, m) == K.head_scores_chunks(B, m, n) for B, m in K.HS_SHAPES)
    assert all(ops.gemm_tn_splits(M, N, Kk) == K.tn_splits(M, N, Kk, n) for N, Kk in K.TN_SHAPES for M in K.TN_M)
    return n


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)                        # one case, one pair of references, however many tests look at it


# ================================================================================================ per-head LayerNorm
@pytest.mark.parametrize("M,flat", [(M, 0) for M in K.HEADNORM_M] + [(5, 1)])
def test_headnorm(kern, cus, M, flat):
    rows = K.run_headnorm(kern, case_of(K.headnorm_case, (M, flat)), EXISTING)
    assert rows == K.headnorm_rows(M, cus)


def test_headnorm_waves_take_a_second_trip(kern, cus):
    rows0 = kern.headnorm_bwd_rows(10 ** 9)
    M = K.headnorm_trip_M(rows0)
    rows = K.run_headnorm(kern, case_of(K.headnorm_case, (M, 0)), EXISTING)
    assert rows == rows0 and M == rows + 5


# ================================================================================================ tokens <-> padded cells
@pytest.mark.parametrize("shape", K.PAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pad_grid_and_crop_gather(kern, shape):
    K.run_pad_grid(kern, case_of(K.pad_case, shape), EXISTING)


# ================================================================================================ per-head products
@pytest.mark.parametrize("nh", K.HS_HEADS)
@pytest.mark.parametrize("B,n", K.HS_SHAPES)
def test_head_scores(kern, cus, nh, B, n):
    chunks = K.run_head_scores(kern, case_of(K.scores_case, (nh, B, n)), EXISTING)
    assert chunks == K.head_scores_chunks(B, n, cus)


@pytest.mark.parametrize("nh", K.HA_HEADS)
@pytest.mark.parametrize("B,n", K.HA_SHAPES)
def test_head_apply(kern, nh, B, n):
    K.run_head_apply(kern, case_of(K.apply_case, (nh, B, n)), EXISTING)


# ================================================================================================ dropout against the host's Philox
@pytest.mark.parametrize("seed", K.DROP_SEEDS)
@pytest.mark.parametrize("keep", K.DROP_KEEPS)
def test_dropout_mul_is_the_host_mask(kern, cus, keep, seed):
    sizes = K.dropout_sizes(K.stream_blocks(10 ** 12, cus))
    assert sizes[-1] // 4 == 16 * cus * 256 + 1                   # one float4 past a full grid: a thread takes a second trip
    for n in sizes:
        K.run_dropout_mul(kern, n, seed, keep)


# ================================================================================================ token GEMMs
@pytest.mark.parametrize("M", K.GEMM_M_FP32 + K.GEMM_M_SPLIT64)
@pytest.mark.parametrize("site,mode,pad", K.GEMM_VARIANTS, ids=lambda v: str(v))
def test_token_gemm_sites(kern, site, mode, pad, M):
    K.run_gemm(kern, case_of(K.gemm_case, (site, mode, pad, M)), EXISTING, expect=K.expected_gemm_kernel(site, mode, M))


def test_token_gemm_mask_route_above_the_split_threshold(kern):
    """the one large case, unpatched: lr2 with a mask tensor at M = 65 536 + 77 stays on the exact-fp32 kernel"""
    site, mode, pad, M = K.GEMM_BIG
    assert M >= kern.ops.GEMM_SPLIT_MIN_ROWS
    label, kernel = K.run_gemm(kern, K.gemm_case(site, mode, pad, M), EXISTING, expect="fp32")
    assert label.startswith("gemm_nt[")


@pytest.mark.parametrize("M", K.GEMM_M_FP32)
@pytest.mark.parametrize("site,mode,pad", K.GEMM_LOWERED, ids=lambda v: str(v))
def test_token_gemm_sites_with_the_row_threshold_lowered(kern, monkeypatch, site, mode, pad, M):
    """ops.GEMM_SPLIT_MIN_ROWS = 0, as tests/test_gpu_conv3x.py sets it: the 64-row-tile kernel on one row, on two tiles and a row, on a
    ragged fifth tile; the mask-tensor sites stay on the exact-fp32 kernel even so (no Galerkin site reaches the 128-row split kernel)"""
    monkeypatch.setattr(kern.ops, "GEMM_SPLIT_MIN_ROWS", 0)
    K.run_gemm(kern, case_of(K.gemm_case, (site, mode, pad, M)), EXISTING, expect="fp32" if mode == "mask" else "split64")


@pytest.mark.parametrize("site,mode,pad,M", K.GEMM_DIRECT_128, ids=lambda v: str(v))
def test_split128_kernel_direct(kern, site, mode, pad, M):
    K.run_gemm(kern, case_of(K.gemm_case, (site, mode, pad, M)), EXISTING, expect="split128", entry="gemm3x_direct")


# ================================================================================================ weight gradients
@pytest.mark.parametrize("M", K.TN_M)
@pytest.mark.parametrize("N,Kk", K.TN_SHAPES)
def test_weight_gradients(kern, cus, N, Kk, M):
    path, splits = K.run_gemm_tn(kern, case_of(K.tn_case, (N, Kk, M)), EXISTING)
    assert splits == K.tn_splits(M, N, Kk, cus)
    if M in (1000, 1025) and (N, M) != (K.REG, 1000):
        assert splits >= 2


# ================================================================================================ refusals
def _all(shape):
    return torch.ones(shape, dtype=torch.bool)


def test_refusals_leave_everything_untouched(kern):
    """what include/rpb.h and the RPB_REQUIRE texts document: an error code before any launch"""
    from realpdebench_amd._lib import RpbError
    ops, M = kern.ops, 8

    def refused(match, build):
        a = guarded.Arena("cuda")
        call = build(a)
        with pytest.raises(RpbError, match=match):
            call()
        a.check()                                                 # every guard and every output sentinel is intact

    x, one = torch.ones(M, 3 * C), torch.ones(C)

    def hn_fwd(Cc, ldx):
        def build(a):
            xi, g, b, o = a.inp(torch.ones(M, ldx)), a.inp(one), a.inp(one), a.out(M, 2 * C, unwritten=_all((M, 2 * C)))
            return lambda: ops.headnorm_fwd(xi.op, ldx, g.op, b.op, o.op, 2 * C, M, Cc, K.EPS)
        return build
    refused("headnorm", hn_fwd(128, 3 * C))
    refused("headnorm", hn_fwd(C, 3 * C + 2))

    def hn_bwd(Cc, ldg):
        def build(a):
            xi, g, gy = a.inp(x), a.inp(one), a.inp(torch.ones(M, ldg))
            gx, part = a.out(M, 3 * C, unwritten=_all((M, 3 * C))), a.out(4, 2 * C, unwritten=_all((4, 2 * C)))
            return lambda: ops.headnorm_bwd(xi.op, 3 * C, g.op, gy.op, ldg, gx.op, 3 * C, part.op, M, Cc, K.EPS)
        return build
    refused("headnorm", hn_bwd(192, 2 * C))
    refused("headnorm", hn_bwd(C, 2 * C + 2))

    def scores(nh, ldg):
        def build(a):
            G, A, part = a.inp(torch.ones(M, ldg)), a.inp(torch.ones(M, 320)), a.out(1, 5 * 4096, unwritten=_all((1, 5 * 4096)))
            return lambda: ops.head_scores(G.op, ldg, A.op, 320, part.op, 1, M, nheads=nh)
        return build
    refused("head_scores", scores(0, 320))
    refused("head_scores", scores(5, 320))
    refused("head_scores", scores(4, 257))

    def apply(nh, with_mask, drop):
        def build(a):
            X, Wm, out = a.inp(torch.ones(M, 256)), a.inp(torch.ones(4, 64, 64)), a.out(M, 256, unwritten=_all((M, 256)))
            mask = a.inp(torch.ones(M, 256)) if with_mask else None
            return lambda: ops.head_apply(X.op, 256, Wm.op, out.op, 256, 1, M, mask=mask.op if mask else None, ldm=256 if mask else 0,
                                          nheads=nh, drop=drop)
        return build
    refused("head_apply", apply(3, False, None))
    refused("head_apply", apply(4, True, (55, 0.8)))

    def dropmul(n, keep):
        def build(a):
            g, out = a.inp(torch.ones(16)), a.out(16, unwritten=_all((16,)))
            return lambda: ops.dropout_mul(g.op, out.op, n, 55, keep)
        return build
    refused("dropout_mul", dropmul(6, 0.5))
    refused("dropout_mul", dropmul(8, 0.0))
    refused("dropout_mul", dropmul(8, 1.0))
    refused("dropout_mul", dropmul(8, 1.5))
