"""TEST INFRASTRUCTURE ONLY -- the shapes, inputs, restatements, restated launch arithmetic and drivers of the per-kernel tests of the
DMD kernels ``rpb_dmd_gram`` and ``rpb_dmd_predict`` (csrc/rpb_dmd.hip).  Shared by tests/test_gpu_dmd_kernels.py (which runs the HIP
kernels) and tests/test_dmd_kernels_host.py (which proves, without a GPU, that every case is well conditioned, that the restated launch
arithmetic gives the second trips and that a wrong kernel would be noticed).  A plain helper module: no conftest, no fixture.  The two
measures are those of tests/unet_kernel_cases.py, the verdict is tests/kernel_verdict.py, the arenas are tests/guarded.py.

A DRIVER (``run_gram``, ``run_predict``) lays the operands of ONE launch out in guard-banded arenas -- ``x`` in an fp32 arena with NaN
around it, the fp64 operands ``M``, ``G`` and ``part`` in an fp64 arena, handed over as ``Operand.tensor()`` --, calls ``kern.<entry>``,
runs ``Arena.check()`` and judges the outputs.  Beyond its guards ``x`` holds NaN wherever the kernels' contract says nothing is read
for a result: the channels ``c >= f`` of every cell and, for the prediction, frame 0.

Cases ``(B, T, P, C, f, S)`` and what they reach (``dmd_pts(f) = (256 / f) & ~3`` points per chunk; the staging reads 16 bytes at a time,
VEC = 4, when ``P C % 4 == 0`` and the base is 16-byte aligned, else 4 bytes):
  (2, 17, 88, 3, 3, 17)  f = 3: pts = 84, pts f = 252 = 15 tiles of 16 columns + a partial one; two chunks, the second with 4 points;
                         P C = 264: VEC 4 with float4s that straddle 3-wide cells; T = S = 17: one live row in the second tile row
  (1, 16, 84, 3, 3, 16)  exactly one tile (``two`` false), exactly one full chunk, K = 15
  (1, 2, 5, 1, 1, 1)     T = 2, K = 1, C = f = 1, the 4-byte path through P C % 4
  (2, 5, 9, 64, 64, 16)  f = 64: pts = 4, three chunks, a tail of one point; S = 16
  (1, 32, 40, 7, 6, 32)  pts f = 240 = 15 tiles; C = 7 with VEC 4; T = S = 32, K = 31: the padded k = 31
  (1, 9, 61, 5, 4, 3)    P C = 305: the 4-byte path; f = 4
  the first, misaligned  ``x`` declared with one extra leading float and handed over from element 1: the 4-byte path through the base
                         address.  Only the staging differs, the LDS image is the same: G and out equal the aligned run bit for bit.
  gram only              (1, 3, 8321, 3, 2), (3, 6, 1100, 16, 16), (1, 5, 518, 64, 64): 66, 69 and 130 chunks against at most 64
                         workgroups per sample -- ``for (ch = g; ch < nchunk; ch += NG)`` takes a second trip, a third in the last.

Inputs.  Gram: N(0, 1), frame t scaled by 2^-t, so that the entries of G span 2 T binades.  Predict, two families: ``random``, the inputs
of tests/test_gpu_dmd.py (x ~ N(0, 1), M of mixed sign up to 1e3), and ``cancelling``: x[b, k] = base[b] + 1e-3 noise[b, k],
M = U(-1, 1) 10^U(2, 3) with the last row replaced so that every column sums to a weight in [0.5, 1.5] -- the result is of order 1, the
terms of order 1e3: coefficients that cancel, which is why the kernel accumulates in fp64.

Bounds -- derived, none measured on a kernel.
  Gram, both measures: max(1e-12, 2 P f 2^-53).  The product of two fp32 values is exact in fp64; any summation order of n = P f terms
  errs by at most n 2^-53 sum |terms| to first order (the factor 2 covers the rest), and sum |x_i x_j| <= sqrt(G_ii G_jj) <= max |G|.
  Per entry |error_ij| <= bound sqrt(G_ii G_jj) is asserted too: the maximum measure alone would hide a wrong small row.  The reference
  is the exactly rounded sum (``math.fsum`` over the exact fp64 products), so it adds no error of its own.
  Predict, both measures, both families: 1e-6, the bound tests/test_gpu_dmd.py asserts (``existing=``): fp64 accumulation and one
  rounding to fp32, 2^-24 per element.  On the cancelling family K 2^-53 sum |M| |x| is about 1e-10 of the result, so correct
  arithmetic measures 2.5e-8 (Rel-L2) / 3-5e-8 (maximum) while M rounded to fp32 gives 1.3-2.4e-5 / 2.3-5.2e-5 and fp32 accumulation
  1.8-6.7e-5 / 0.4-1.7e-4 (tests/test_dmd_kernels_host.py asserts both sides of the bound, and that on the random family both wrong
  variants pass it: those inputs cannot tell them apart).
The figure printed as ``e32`` is the restatement's own error: the fp64 matrix product against the exact sum (Gram), the fp64 product
rounded once to fp32 as the kernel rounds (predict)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

import guarded
from kernel_verdict import verdict
from unet_kernel_cases import F32, F64, MEASURES, MI355X_CUS, _gen, measures          # noqa: F401

TAG = "dmd-kernels"
NAN = float("nan")
KC, MAX_GROUPS = 256, 64                                          # DMD_KC; the cap of rpb_dmd_gram_groups
PREDICT_BOUND = 1e-6                                              # tests/test_gpu_dmd.py::test_predict_kernel

# (B, T, P, C, f, S)
CASES = [(2, 17, 88, 3, 3, 17), (1, 16, 84, 3, 3, 16), (1, 2, 5, 1, 1, 1), (2, 5, 9, 64, 64, 16), (1, 32, 40, 7, 6, 32), (1, 9, 61, 5, 4, 3)]
MISALIGNED = CASES[0]
# (B, T, P, C, f): more chunks than workgroups
GRAM_ONLY = [(1, 3, 8321, 3, 2), (3, 6, 1100, 16, 16), (1, 5, 518, 64, 64)]
FAMILIES = ["random", "cancelling"]


def ceil_div(a, b):
    return (a + b - 1) // b


# ================================================================================================ launch arithmetic (restated)
def dmd_pts(f):
    """points per chunk: a multiple of 4, so that pts * f is one too"""
    return (KC // f) & ~3


def nchunk(P, f):
    return ceil_div(P, dmd_pts(f))


def gram_groups(B, P, f, cus=MI355X_CUS):
    """rpb_dmd_gram_groups: about two workgroups per compute unit over the batch, 64 and the chunk count at the most"""
    return max(1, min(MAX_GROUPS, ceil_div(2 * cus, B), nchunk(P, f)))


def vec(P, C, misaligned=False):
    """floats per staging load"""
    return 4 if (P * C) % 4 == 0 and not misaligned else 1


def gram_bound(P, f):
    return max(1e-12, 2 * P * f * 2.0 ** -53)


# ================================================================================================ shared pieces
def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def exact(name, got, want):
    """bit equality"""
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (name, got.shape, want.shape)
    bad = (_bits(got) != _bits(want)).reshape(-1).nonzero()
    print(f"[{TAG}] {name}: {got.numel()} element(s) compared bit for bit, {bad.numel()} differ")
    assert not bad.numel(), f"{name}: {bad.numel()} element(s) differ in their bits, the first at flat index {int(bad[0])}"


def _mask_unread(x, f, frame0=False):
    """NaN where no result may depend on x: channels c >= f, and frame 0 for the prediction"""
    x = x.clone()
    x[..., f:] = NAN
    if frame0:
        x[:, 0] = NAN
    return x


def _x_operand(a, x, P, C, misaligned):
    """``x`` in arena ``a`` and the element the kernel gets it from: 0, or -- misaligned -- 1 of an operand with one more leading float
    (``Operand.at``, once every operand of the arena is declared)"""
    if not misaligned:
        return a.inp(x, "x", ld=P * C), 0
    return a.inp(torch.cat((torch.full((1,), NAN), x.reshape(-1))), "x", ld=P * C), 1


# ================================================================================================ Gram
def exact_gram(x, f):
    """G[b][i][j] = the correctly rounded sum over (p, c < f) of the exact fp64 products x[b][i][p][c] x[b][j][p][c]"""
    B, T, P, _ = x.shape
    X = x[..., :f].double().reshape(B, T, P * f).numpy()
    G = np.empty((B, T, T))
    for b in range(B):
        for i in range(T):
            for j in range(i + 1):
                G[b, i, j] = G[b, j, i] = math.fsum(X[b, i] * X[b, j])
    return torch.from_numpy(G)


@functools.lru_cache(maxsize=None)
def gram_case(B, T, P, C, f):
    g = _gen(81, B, T, P, C, f)
    x = torch.randn(B, T, P, C, generator=g) * (2.0 ** -torch.arange(T, dtype=F32)).view(1, T, 1, 1)
    want = exact_gram(x, f)
    X = x[..., :f].double().reshape(B, T, P * f)
    return SimpleNamespace(name=f"gram B={B} T={T} P={P} C={C} f={f}", dims=(B, T, P, C, f), x=_mask_unread(x, f), want=want,
                           restated=X @ X.transpose(1, 2))


def run_gram(kern, c, misaligned=False):
    """one rpb_dmd_gram call (its two launches) on guarded operands; returns G as the host sees it"""
    B, T, P, C, f = c.dims
    NG = kern.dmd_gram_groups(B, P, f)
    name = f"{c.name} VEC={vec(P, C, misaligned)} chunks={nchunk(P, f)} groups={NG}" + (" misaligned" if misaligned else "")
    a, a64 = guarded.Arena(kern.dev), guarded.Arena(kern.dev, dtype=F64)
    x, x0 = _x_operand(a, c.x, P, C, misaligned)
    upper = torch.ones(T, T, dtype=torch.bool).triu(1).expand(B, NG, T, T).contiguous()
    part = a64.out(B, NG, T, T, name="part", ld=T * T, unwritten=upper)      # the finish reads the lower triangle only
    G = a64.out(B, T, T, name="G", ld=T * T)
    kern.dmd_gram(x.at(x0), G.tensor(), part.tensor(), B, T, P, C, f)
    a.check()
    a64.check()
    got, pt = G.get(), part.get()
    exact(f"{name} G against its transpose", got, got.transpose(1, 2).contiguous())
    s = pt[:, 0].clone()                                          # the finish: the partials summed in order
    for g in range(1, NG):
        s = s + pt[:, g]
    low = torch.ones(T, T, dtype=torch.bool).tril()
    exact(f"{name} G against the partials summed in order", got[:, low], s[:, low])
    bound = gram_bound(P, f)
    verdict(TAG, name, zip(MEASURES, measures(c.restated, c.want), measures(got, c.want)), existing=bound)
    d = torch.diagonal(c.want, dim1=1, dim2=2)
    scale = torch.sqrt(d[:, :, None] * d[:, None, :])
    worst = float(((got - c.want).abs() / scale).max())
    print(f"[{TAG}] {name} per entry: max |error_ij| / sqrt(G_ii G_jj) {worst:.3e} bound {bound:.3e}")
    assert worst <= bound, f"{name}: an entry is off by {worst:.3e} of sqrt(G_ii G_jj) > {bound:.3e}"
    return got


def run_gram_twice(kern, c):
    exact(f"{c.name} second call", run_gram(kern, c), run_gram(kern, c))


def run_gram_misaligned(kern, c):
    exact(f"{c.name} misaligned against aligned", run_gram(kern, c, misaligned=True), run_gram(kern, c))


# ================================================================================================ predict
def predict_inputs(B, T, P, C, S, family):
    """(x [B][T][P][C] fp32, M [B][T-1][S] fp64)"""
    K = T - 1
    if family == "random":                                        # tests/test_gpu_dmd.py's
        x = torch.from_numpy(np.random.default_rng(B * 1000 + T).standard_normal((B, T, P, C), dtype=np.float32))
        rng = np.random.default_rng(S)
        return x, torch.from_numpy(rng.uniform(-1, 1, (B, K, S)) * 10.0 ** rng.uniform(0, 3, (B, K, S)))
    rng = np.random.default_rng(7000 + 100 * B + 10 * T + S)
    base = rng.standard_normal((B, 1, P, C))
    x = torch.from_numpy((base + 1e-3 * rng.standard_normal((B, T, P, C))).astype(np.float32))
    M = rng.uniform(-1, 1, (B, K, S)) * 10.0 ** rng.uniform(2, 3, (B, K, S))
    M[:, K - 1] = rng.uniform(0.5, 1.5, (B, S)) - M[:, :K - 1].sum(1)        # every column sums to a weight in [0.5, 1.5]
    return x, torch.from_numpy(M)


def predict(x, M, f, dt=F64):
    """out[b][s][p][c] = sum_k M[b][k][s] x[b][k + 1][p][c], c < f"""
    B, T, P, _ = x.shape
    return torch.einsum("bks,bkn->bsn", M.to(dt), x[:, 1:, :, :f].to(dt).reshape(B, T - 1, P * f)).reshape(B, M.shape[2], P, f)


@functools.lru_cache(maxsize=None)
def predict_case(B, T, P, C, f, S, family):
    x, M = predict_inputs(B, T, P, C, S, family)
    want = predict(x, M, f)
    return SimpleNamespace(name=f"predict B={B} T={T} P={P} C={C} f={f} S={S} [{family}]", dims=(B, T, P, C, f, S),
                           x=_mask_unread(x, f, frame0=True), M=M, want=want, rounded=want.float())


def run_predict(kern, c, misaligned=False):
    """one rpb_dmd_predict launch on guarded operands; returns out as the host sees it"""
    B, T, P, C, f, S = c.dims
    name = f"{c.name} VEC={vec(P, C, misaligned)} chunks={nchunk(P, f)}" + (" misaligned" if misaligned else "")
    a, a64 = guarded.Arena(kern.dev), guarded.Arena(kern.dev, dtype=F64)
    x, x0 = _x_operand(a, c.x, P, C, misaligned)
    M = a64.inp(c.M, "M", ld=S)
    out = a.out(B, S, P, f, name="out", ld=P * f, guard=P * f + 256)        # a write of row S lands in memory the test owns
    kern.dmd_predict(x.at(x0), M.tensor(), out.op, B, T, P, C, f, S)
    a64.check()
    a.check()
    got = out.get()
    verdict(TAG, name, zip(MEASURES, measures(c.rounded, c.want), measures(got, c.want)), existing=PREDICT_BOUND)
    return got


def run_predict_twice(kern, c):
    exact(f"{c.name} second call", run_predict(kern, c), run_predict(kern, c))


def run_predict_misaligned(kern, c):
    exact(f"{c.name} misaligned against aligned", run_predict(kern, c, misaligned=True), run_predict(kern, c))
