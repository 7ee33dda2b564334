"""rpb_gemm3h (csrc/rpb_gemm3h.hip): the token GEMM of the opt-in "f16x2" eval arithmetic against ``A.double() @ W.double().T`` with the
epilogue in fp64.

Bound: Rel-L2 < 2e-6, the project's f16x2 kernel bound (``BOUND`` of tests/test_gpu_deeponet_arith.py); the hi
planes alone give about 5e-4, so a dropped lo term fails.  Shapes: the Q|K|V shape with tiles of 64 rows and a ragged one, one full tile
and one row, a single row at the regressor's N = 128, one 64-column stage at N = 64, K = 512 (the one-workgroup-per-CU build).  For the
``row_scales`` (row i times 2^((7 i) % 45 - 30)) and ``zero_row`` variants every row is also checked on its own -- the case a per-tensor
activation scale cannot pass -- and the zero row's output is exactly zero.

Measured on an MI355X: 0.5-2.6e-7 over all shapes and variants (largest at K = 512), the worst single row 1.8-3.2e-7, all-zero A at most
2.4e-7 absolute (the fp32 rounding of bias + residual; exactly the bias / ReLU result otherwise)."""
import functools

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-6
SHAPES = [(300, 768, 256), (129, 256, 256), (1, 128, 256), (777, 64, 64), (260, 256, 512)]
VARIANTS = ["plain", "bias_relu", "bias_residual", "row_scales", "zero_row", "w_small"]


@functools.lru_cache(maxsize=None)
def _case(M, N, K, variant):
    """(A, W, bias, residual, act, the fp64 result), computed once per case"""
    gen = torch.Generator().manual_seed(1000 * M + N + K)
    A = torch.randn(M, K, generator=gen)
    W = torch.randn(N, K, generator=gen) / 16
    bias = torch.randn(N, generator=gen) if variant in ("bias_relu", "bias_residual") else None
    res = torch.randn(M, N, generator=gen) if variant == "bias_residual" else None
    act = 3 if variant == "bias_relu" else 0
    if variant == "row_scales":
        A = A * torch.tensor([2.0 ** ((7 * i) % 45 - 30) for i in range(M)]).unsqueeze(1)
    elif variant == "zero_row":
        A = A.clone()
        A[M - 2 if M > 1 else 0] = 0
    elif variant == "zero":
        A = torch.zeros_like(A)
    elif variant == "w_small":
        W = W * 2.0 ** -10
    return A, W, bias, res, act, _want(A, W, bias, res, act)


def _want(A, W, bias, res, act):
    want = A.double() @ W.double().t()
    if bias is not None:
        want = want + bias.double()
    if act == 3:
        want = torch.relu(want)
    if res is not None:
        want = want + res.double()
    return want


def _d(t):
    return None if t is None else t.to(DEV).contiguous()


def _run(A, W, bias, res, act):
    from realpdebench_amd import ops
    M, K = A.shape
    N = W.shape[0]
    wz = ops.gemm3h_wprep(_d(W))
    out = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm_nt_f16x2(_d(A), wz, out, M, N, K, bias=_d(bias), residual=_d(res), act=act)
    return out


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm3h_against_fp64(M, N, K, variant):
    A, W, bias, res, act, want = _case(M, N, K, variant)
    out = _run(A, W, bias, res, act)
    assert torch.equal(out, _run(A, W, bias, res, act)), "two calls must give bit-equal outputs"
    assert bool(torch.isfinite(out).all())
    e = rel_l2(out.cpu(), want)
    print(f"gemm3h M={M} N={N} K={K} [{variant}]: Rel-L2 {e:.2e} (bound {BOUND:.0e})")
    assert e < BOUND
    if variant in ("row_scales", "zero_row"):
        got = out.cpu().double()
        wn = want.norm(dim=1)
        live = wn > 0
        if bool(live.any()):
            er = float(((got - want).norm(dim=1)[live] / wn[live]).max())
            print(f"  worst row on its own: {er:.2e}")
            assert er < BOUND
        if variant == "zero_row":
            z = M - 2 if M > 1 else 0
            assert not bool(live[z]) and bool((got[z] == 0).all()), "the zero row's output is exactly zero"


@pytest.mark.parametrize("epilogue", ["plain", "bias_relu", "bias_residual"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm3h_all_zero_input(M, N, K, epilogue):
    _, W, bias, res, act, _ = _case(M, N, K, epilogue)
    A = torch.zeros(M, K)
    want = _want(A, W, bias, res, act)
    out = _run(A, W, bias, res, act)
    assert bool(torch.isfinite(out).all())
    d = float((out.cpu().double() - want).abs().max())
    print(f"all-zero A M={M} N={N} K={K} [{epilogue}]: max |out - epilogue(0)| {d:.2e} (max |want| {float(want.abs().max()):.2e})")
    assert d <= BOUND * float(want.abs().max())


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm3h_strided_operands_write_only_their_output(M, N, K):
    """A = columns [K, 2K) of an [M][3K] tensor; out = columns [N, 2N) of a sentinel-filled [M][2N] tensor inside a sentinel-padded
    buffer: the sentinels before it, after it and in the other columns stay."""
    from realpdebench_amd import ops
    A, W, _, _, _, want = _case(M, N, K, "plain")
    wide = torch.full((M, 3 * K), 3.25, device=DEV)
    wide[:, K:2 * K] = _d(A)
    pad, S = 1024, -7.5
    buf = torch.full((pad + M * 2 * N + pad,), S, device=DEV)
    wz = ops.gemm3h_wprep(_d(W))
    assert ops.gemm3h_supported(M, N, K, 3 * K, 2 * N)
    ops.gemm_nt_f16x2(ops.Sub(wide, K), wz, ops.Sub(buf, pad + N), M, N, K, lda=3 * K, ldo=2 * N)
    torch.cuda.synchronize()
    body = buf[pad:pad + M * 2 * N].view(M, 2 * N)
    assert bool((buf[:pad] == S).all()) and bool((buf[pad + M * 2 * N:] == S).all())
    assert bool((body[:, :N] == S).all())
    assert rel_l2(body[:, N:].cpu(), want) < BOUND


@pytest.mark.parametrize("M,N,K,lda", [(256, 256, 96, None), (256, 96, 256, None), (256, 256, 256, 258)])
def test_gemm3h_refuses_unsupported_shapes(M, N, K, lda):
    """K = 96, N = 96, lda = K + 2: rpb_gemm3h_supported is false and the call returns the library's error without launching"""
    from realpdebench_amd import _lib, ops
    assert not ops.gemm3h_supported(M, N, K, lda)
    ld = K if lda is None else lda
    A = torch.zeros(M, ld, device=DEV)
    out = torch.full((M, N), -7.5, device=DEV)
    wz = (torch.zeros(2 * N * K, dtype=torch.int16, device=DEV), torch.ones(2, device=DEV))
    with pytest.raises(_lib.RpbError):
        ops.gemm_nt_f16x2(A, wz, out, M, N, K, lda=lda)
    with pytest.raises(_lib.RpbError):
        ops.gemm_nt_f16x2(torch.zeros(M, 256, device=DEV), wz, torch.empty(M, 256, device=DEV), M, 256, 256, act=1)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())
