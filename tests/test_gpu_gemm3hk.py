"""rpb_gemm3hk (csrc/rpb_gemm3hk.hip): the large-K token GEMM of the opt-in "f16x2" eval arithmetic against ``A.double() @ W.double().T``
with the epilogue in fp64.

Bound: Rel-L2 < max(2e-6, 2 e_default).  2e-6 is the project's f16x2 kernel bound (tests/test_gpu_gemm3h.py), measured there only up to
K = 512; e_default is the error, against the same fp64 result, of the existing ``ops.gemm_nt`` on the same operands, computed here.
fp32 accumulation error grows with K for both kernels, so the default kernel -- not the kernel under test -- sets the yardstick.  Both
figures are printed.  Shapes: ragged row tiles at every tile height the launcher picks (M = 1, 70, 129, 260, 300 are too few rows for
the taller instances and run the 64-row one; ``test_gemm3hk_tall`` runs the 128- and 256-row instances), K = 576 (not a multiple of
512), K = 6144.  Variants: the three epilogues and plain; ``row_scales`` (row i times 2^((7 i) % 45 - 30)) and ``zero_row``, where every
row is also checked on its own -- the case a per-tensor activation scale cannot pass -- and the zero row's output is exactly the
epilogue of zero; ``w_small`` (W 2^-10); ``k_block_scales`` (columns [512 j, 512 j + 512) times 2^(10 j) for even j, 2^(-10 j) for odd j).

Measured on an MI355X: 1.9e-7 to 8.8e-7 over all shapes and variants against 2.9e-7 to 1.4e-6 of the default kernel on the same
operands (never above 0.70 of the default's error); the largest at K = 6144, 8.8e-7 against 1.4e-6; the worst single row 2.7e-7 to
9.6e-7; all-zero A with bias + GELU 3.6e-8 to 4.0e-8, the same as the default kernel; every case below half its bound."""
import functools

import pytest
import torch

from conftest import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOUND = 2e-6
SHAPES = [(300, 256, 1536), (129, 512, 1024), (1, 256, 576), (260, 1536, 6144), (70, 2048, 1280)]
VARIANTS = ["plain", "bias_gelu", "bias_relu", "bias_residual", "row_scales", "zero_row", "w_small", "k_block_scales"]
ACT = {"bias_gelu": 1, "bias_relu": 3}


@functools.lru_cache(maxsize=None)
def _case(M, N, K, variant):
    """(A, W, bias, residual, act, the fp64 result), computed once per case"""
    gen = torch.Generator().manual_seed(1000 * M + N + K)
    A = torch.randn(M, K, generator=gen)
    W = torch.randn(N, K, generator=gen) / 16
    bias = torch.randn(N, generator=gen) if variant in ("bias_gelu", "bias_relu", "bias_residual") else None
    res = torch.randn(M, N, generator=gen) if variant == "bias_residual" else None
    act = ACT.get(variant, 0)
    if variant == "row_scales":
        A = A * torch.tensor([2.0 ** ((7 * i) % 45 - 30) for i in range(M)]).unsqueeze(1)
    elif variant == "zero_row":
        A = A.clone()
        A[M - 2 if M > 1 else 0] = 0
    elif variant == "w_small":
        W = W * 2.0 ** -10
    elif variant == "k_block_scales":
        j = torch.arange(K) // 512
        A = A * (2.0 ** (10.0 * j * (1 - 2 * (j % 2)))).unsqueeze(0)
    return A, W, bias, res, act, _want(A, W, bias, res, act)


def _want(A, W, bias, res, act):
    want = A.double() @ W.double().t()
    if bias is not None:
        want = want + bias.double()
    if act == 1:
        want = torch.nn.functional.gelu(want)
    elif act == 3:
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
    ops.gemm_nt_f16x2k(_d(A), wz, out, M, N, K, bias=_d(bias), residual=_d(res), act=act)
    return out


def _run_default(A, W, bias, res, act):
    from realpdebench_amd import ops
    M, K = A.shape
    N = W.shape[0]
    out = torch.full((M, N), float("nan"), device=DEV)
    ops.gemm_nt(_d(A), _d(W), out, M, N, K, bias=_d(bias), residual=_d(res), act=act)
    return out


def _check(M, N, K, variant):
    A, W, bias, res, act, want = _case(M, N, K, variant)
    out = _run(A, W, bias, res, act)
    assert torch.equal(out, _run(A, W, bias, res, act)), "two calls must give bit-equal outputs"
    assert bool(torch.isfinite(out).all())
    e, e0 = rel_l2(out.cpu(), want), rel_l2(_run_default(A, W, bias, res, act).cpu(), want)
    bound = max(BOUND, 2 * e0)
    print(f"gemm3hk M={M} N={N} K={K} [{variant}]: Rel-L2 {e:.2e}, default kernel {e0:.2e} (bound {bound:.1e})")
    assert e < bound
    return out.cpu().double(), want


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm3hk_against_fp64(M, N, K, variant):
    got, want = _check(M, N, K, variant)
    if variant in ("row_scales", "zero_row"):
        wn = want.norm(dim=1)
        live = wn > 0
        if bool(live.any()):
            er = float(((got - want).norm(dim=1)[live] / wn[live]).max())
            print(f"  worst row on its own: {er:.2e}")
            assert er < BOUND
        if variant == "zero_row":
            z = M - 2 if M > 1 else 0
            assert not bool(live[z]) and bool((got[z] == 0).all()), "the zero row's output is exactly zero"


@pytest.mark.parametrize("M,N,variant", [(4000, 2048, "bias_gelu"), (4000, 2048, "bias_residual"), (4000, 2048, "row_scales"),
                                         (300, 65536, "bias_gelu"), (300, 65536, "row_scales")])
def test_gemm3hk_tall(M, N, variant):
    """The launcher's other two instances on the 256 CUs of an MI355X (``SHAPES`` all run the 64-row one).  128 rows wherever such
    items keep three quarters of the CUs busy: M = 4000, N = 2048 is 32 row tiles (the last with 32 rows) x 8 column blocks = 256
    items.  256 rows where the weight planes exceed half the Infinity Cache and there is an item per CU: N = 65536 at K = 576 is 151 MB
    of planes, M = 300 two row tiles (the second with 44 rows) x 256 column blocks."""
    got, want = _check(M, N, 576, variant)
    if variant == "row_scales":
        er = float(((got - want).norm(dim=1) / want.norm(dim=1)).max())
        print(f"  worst row on its own: {er:.2e}")
        assert er < BOUND


@pytest.mark.parametrize("epilogue", ["plain", "bias_gelu", "bias_relu", "bias_residual"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm3hk_all_zero_input(M, N, K, epilogue):
    """Exactly the epilogue of zero: 0, relu(bias) and relu-free bias + residual are single fp32 operations and must match torch's fp32
    bit for bit; GELU of the bias goes through the kernels' erf approximation and is held to the bound against fp64"""
    _, W, bias, res, act, _ = _case(M, N, K, epilogue)
    A = torch.zeros(M, K)
    out = _run(A, W, bias, res, act).cpu()
    assert bool(torch.isfinite(out).all())
    if epilogue == "bias_gelu":
        want = _want(A, W, bias, res, act)
        e, e0 = rel_l2(out, want), rel_l2(_run_default(A, W, bias, res, act).cpu(), want)
        print(f"all-zero A M={M} N={N} K={K} [{epilogue}]: Rel-L2 {e:.2e}, default kernel {e0:.2e}")
        assert e < max(BOUND, 2 * e0)
        return
    want = torch.zeros(M, N)
    if bias is not None:
        want = want + bias
    if act == 3:
        want = torch.relu(want)
    if res is not None:
        want = want + res
    assert torch.equal(out, want)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm3hk_strided_operands_write_only_their_output(M, N, K):
    """A = columns [K, 2K) of an [M][3K] tensor; out = columns [N, 2N) of a NaN-filled [M][2N] tensor inside a NaN-padded buffer: the
    NaNs before it, after it and in the other columns stay."""
    from realpdebench_amd import ops
    A, W, _, _, _, want = _case(M, N, K, "plain")
    wide = torch.full((M, 3 * K), 3.25, device=DEV)
    wide[:, K:2 * K] = _d(A)
    pad = 1024
    buf = torch.full((pad + M * 2 * N + pad,), float("nan"), device=DEV)
    wz = ops.gemm3h_wprep(_d(W))
    assert ops.gemm3hk_supported(M, N, K, 3 * K, 2 * N)
    ops.gemm_nt_f16x2k(ops.Sub(wide, K), wz, ops.Sub(buf, pad + N), M, N, K, lda=3 * K, ldo=2 * N)
    torch.cuda.synchronize()
    body = buf[pad:pad + M * 2 * N].view(M, 2 * N)
    assert bool(torch.isnan(buf[:pad]).all()) and bool(torch.isnan(buf[pad + M * 2 * N:]).all())
    assert bool(torch.isnan(body[:, :N]).all())
    assert bool(torch.isfinite(body[:, N:]).all())
    e0 = rel_l2(_run_default(A, W, None, None, 0).cpu(), want)
    assert rel_l2(body[:, N:].cpu(), want) < max(BOUND, 2 * e0)


@pytest.mark.parametrize("M,N,K,lda", [(256, 256, 96, None), (256, 96, 1536, None), (256, 256, 1536, 1538), (256, 256, 256, 258)])
def test_gemm3hk_refuses_unsupported_shapes(M, N, K, lda):
    """K = 96, N = 96, lda = K + 2: rpb_gemm3hk_supported is false and the call returns the library's error without launching; so does an
    activation code the kernel does not have"""
    from realpdebench_amd import _lib, ops
    assert not ops.gemm3hk_supported(M, N, K, lda)
    ld = K if lda is None else lda
    A = torch.zeros(M, ld, device=DEV)
    out = torch.full((M, N), -7.5, device=DEV)
    wz = (torch.zeros(2 * N * K, dtype=torch.int16, device=DEV), torch.ones(2, device=DEV))
    with pytest.raises(_lib.RpbError):
        ops.gemm_nt_f16x2k(A, wz, out, M, N, K, lda=lda)
    wz2 = (torch.zeros(2 * 256 * 1024, dtype=torch.int16, device=DEV), torch.ones(2, device=DEV))
    with pytest.raises(_lib.RpbError):
        ops.gemm_nt_f16x2k(torch.zeros(M, 1024, device=DEV), wz2, torch.empty(M, 256, device=DEV), M, 256, 1024, act=2)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())
