"""TEST INFRASTRUCTURE ONLY -- the shapes, inputs, restated launch arithmetic and drivers of the per-kernel tests of the DeepONet
EVALUATION kernels: ``rpb_don_bn_relu_pool``, ``rpb_don_trunk``, ``rpb_don_point_mlp`` (csrc/rpb_deeponet.hip) and
``rpb_don_point_mlp_f16x2`` (csrc/rpb_deeponet_h.hip).  Shared by tests/test_gpu_deeponet_kernels.py (which runs the HIP kernels) and
tests/test_deeponet_kernels_host.py (which proves, without a GPU, that every case is well conditioned, that the restated pool grid
takes its second trip and that a wrong kernel would be noticed).  A plain helper module: no conftest, no fixture.  ``Case``, the two
measures and the conditioning cap are those of tests/unet_kernel_cases.py, the verdict is tests/kernel_verdict.py, the restatements are
tests/deeponet_restatement.py (run in fp64 for the reference and in fp32 for e32), the arenas are tests/guarded.py.

A DRIVER (``run_*``) lays the operands of ONE launch out in guard-banded arenas, calls ``kern.<entry>``, runs ``Arena.check()`` and judges
the outputs.  The int16 weight planes of the point MLP sit in an int32 arena, two halves per element, whose guard value is a pair of
NaN halves (0x7FC07FC0 for the bf16 planes, 0x7E007E00 for the fp16 planes): a weight read past an operand poisons the result.

Cases and what they reach.
  point MLP (p, C_out, N, B), both kernels; weights and inputs of ``deeponet_arith_helpers.point_inputs``:
    (64, 1, 31, 1)     N < 32: three of the four waves are all-tail and read row N - 1; C_out = 1
    (64, 3, 128, 2)    N = 128 exactly: one workgroup, no tail
    (128, 16, 161, 2)  a tail of 33 points: one full wave, one wave with one point, two all-tail waves; the widest C_out
    (256, 2, 193, 1)   p = 256 (the one-wave-per-SIMD build), a tail of 65
    (128, 5, 1, 3)     N = 1
  trunk (T, H, W, p), seeded synthetic weights scaled like nn.Linear's, axes np.linspace cast to fp32 as ``k_trunk`` does:
    (1, 1, 1, 64) N = 1, T = 1;  (1, 7, 9, 128) N = 63 < 64, p = 128;  (2, 4, 8, 128) N = 64 exactly;  (3, 5, 13, 256) N = 195: a tail of 3
  pool (B, T, H, W, C, ldx, ldo), both modes unless noted; columns C..ldx-1 of x hold NaN (a strided input's gaps), columns C..ldo-1
  of the output must be exactly zero, channels c % 4 == 1 are shifted negative everywhere (their result must be exactly +0.0):
    (2, 5, 11, 6, 32, 64, 64), (1, 2, 2, 5, 256, 256, 256)   the shapes of tests/test_gpu_deeponet.py
    (1, 2, 2, 2, 4, 4, 4)                                    one window, one float4
    (2, 3, 5, 7, 8, 12, 16)                                  ldx != ldo, both above C; odd extents
    (1, 1, 1, 1, 4, 4, 8)                                    mode 1 only (replicated bins); mode 0 must raise the library's error
    (1, 2, 128, 130, 8, 8, 1024)                             mode 0 only: 4160 cells x 256 float4s = 1 064 960 items against the grid's
                                                             16 blocks x 256 CUs x 256 threads = 1 048 576: the grid-stride second trip
  pool, NaN rule (plain tensors: ``check()`` refuses NaN outputs): one NaN planted in x; exactly the windows / bins that contain it are
  NaN in that channel, as torch's max_pool3d(relu) and adaptive_avg_pool3d(relu) in fp64 say, and nothing else is.

Bounds.  The verdict's default max(8 * e32, 1e-6) on both measures for the trunk, the pool and the f32 point MLP.  The f16x2 point MLP:
Rel-L2 against 2e-6, the bound tests/test_gpu_deeponet_arith.py asserts (``existing=``); max |error| / max |reference| against 1e-5, the
project's per-kernel cap (hi planes alone give about 5e-4).  Two calls of a point kernel must be bit-equal."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deeponet_arith_helpers as AH
import deeponet_restatement as R
import guarded
from kernel_verdict import verdict
from unet_kernel_cases import F32, F64, MEASURES, MI355X_CUS, Case, _gen, measures          # noqa: F401

TAG = "deeponet-kernels"
NAN = float("nan")
BF16_NAN_PAIR, F16_NAN_PAIR = 0x7FC07FC0, 0x7E007E00
F16X2_REL_L2, F16X2_MAX = 2e-6, 1e-5

# (p, C_out, N, B)
POINT_CASES = [(64, 1, 31, 1), (64, 3, 128, 2), (128, 16, 161, 2), (256, 2, 193, 1), (128, 5, 1, 3)]
# (T, H, W, p)
TRUNK_CASES = [(1, 1, 1, 64), (1, 7, 9, 128), (2, 4, 8, 128), (3, 5, 13, 256)]
# (B, T, H, W, C, ldx, ldo) -> modes
POOL_CASES = {(2, 5, 11, 6, 32, 64, 64): (0, 1), (1, 2, 2, 5, 256, 256, 256): (0, 1), (1, 2, 2, 2, 4, 4, 4): (0, 1),
              (2, 3, 5, 7, 8, 12, 16): (0, 1), (1, 1, 1, 1, 4, 4, 8): (1,), (1, 2, 128, 130, 8, 8, 1024): (0,)}
POOL_RUNS = [(dims, mode) for dims, modes in POOL_CASES.items() for mode in modes]
POOL_REFUSED = ((1, 1, 1, 1, 4, 4, 8), 0)
POOL_SECOND_TRIP = ((1, 2, 128, 130, 8, 8, 1024), 0)
POOL_ERROR = "MaxPool3d\\(2\\) needs extents >= 2"


def ceil_div(a, b):
    return (a + b - 1) // b


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def exact(name, got, want):
    """bit equality"""
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (name, got.shape, want.shape)
    bad = (_bits(got) != _bits(want)).reshape(-1).nonzero()
    print(f"[{TAG}] {name}: {got.numel()} element(s) compared bit for bit, {bad.numel()} differ")
    assert not bad.numel(), f"{name}: {bad.numel()} element(s) differ in their bits, the first at flat index {int(bad[0])}"


def judge(name, got, ref64, ref32, existing=None):
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    verdict(TAG, name, zip(MEASURES, measures(ref32, ref64), measures(got, ref64)), existing)


# ================================================================================================ point MLP
def as_i32(z):
    """int16 planes -> int32, two halves per element, flat"""
    return z.contiguous().reshape(-1).view(torch.int32)


@functools.lru_cache(maxsize=None)
def point_case(p, cout, N, B):
    ws, t, b = AH.point_inputs(p, cout, N, B)
    sd = AH.sd_of(ws)
    return Case(f"point_mlp p={p} C_out={cout} N={N} B={B}", dict(dims=(p, cout, N, B), ws=ws, t=t, b=b),
                lambda dt: dict(out=R.point_mlp(sd, t.to(dt), b.to(dt))))


def run_point_mlp(kern, c, arith, existing=None):
    """one rpb_don_point_mlp (``arith`` "f32") or rpb_don_point_mlp_f16x2 ("f16x2") launch; returns out as the host sees it"""
    from realpdebench_amd.model.deeponet import point_weights, point_weights_f16x2
    p, cout, N, B = c.dims
    r64, r32 = c.refs()
    half = arith == "f16x2"
    pw = (point_weights_f16x2 if half else point_weights)(*c.ws)
    a = guarded.Arena(kern.dev)
    aw = guarded.Arena(kern.dev, dtype=torch.int32, fill=F16_NAN_PAIR if half else BF16_NAN_PAIR)
    t, b = a.inp(c.t, "t", ld=p), a.inp(c.b, "b", ld=p)
    w1, w2, w3 = (aw.inp(as_i32(pw[i]), n, ld=512) for i, n in ((0, "w1z"), (2, "w2z"), (4, "w3z")))
    b1z, b2z, b3 = a.inp(pw[1], "b1z", ld=16), a.inp(pw[3], "b2z", ld=16), a.inp(pw[5], "b3")
    sc = a.inp(pw[6], "sc") if half else None
    out = a.out(B, N, cout, name="out", ld=cout)
    kern.don_point_mlp(t.op, b.op, (w1.op, b1z.op, w2.op, b2z.op, w3.op, b3.op), None if sc is None else sc.op, out.op, B, N, p, cout)
    aw.check()
    a.check()
    got = out.get()
    name = f"{c.name} [{arith}]"
    if not half:
        judge(name, got, r64["out"], r32["out"], (existing or {}).get("point_mlp"))
    else:
        figures = list(zip(MEASURES, measures(r32["out"], r64["out"]), measures(got, r64["out"])))
        verdict(TAG, name, figures[:1], existing=F16X2_REL_L2)
        verdict(TAG, name, figures[1:], existing=F16X2_MAX)
    return got


def run_point_mlp_twice(kern, c, arith, existing=None):
    exact(f"{c.name} [{arith}] second call", run_point_mlp(kern, c, arith, existing), run_point_mlp(kern, c, arith, existing))


# ================================================================================================ trunk
def _linear(g, n_out, n_in):
    """nn.Linear's scale: U(-1, 1) / sqrt(fan_in) for weight and bias"""
    k = 1.0 / math.sqrt(n_in)
    return (torch.rand(n_out, n_in, generator=g) * 2 - 1) * k, (torch.rand(n_out, generator=g) * 2 - 1) * k


@functools.lru_cache(maxsize=None)
def trunk_case(T, H, W, p):
    g = _gen(91, T, H, W, p)
    sd = {}
    for i, (n_out, n_in) in zip((0, 2, 4), ((64, 3), (128, 64), (p, 128))):
        sd[f"trunk.fc.{i}.weight"], sd[f"trunk.fc.{i}.bias"] = _linear(g, n_out, n_in)
    axes = [torch.tensor(np.linspace(0, 1, n), dtype=torch.float) for n in (T, H, W)]       # get_grid: float64 linspace, cast
    return Case(f"trunk T={T} H={H} W={W} p={p}", dict(dims=(T, H, W, p), sd=sd, axes=axes), lambda dt: dict(t=R.trunk(sd, T, H, W, dt)))


def run_trunk(kern, c, existing=None):
    T, H, W, p = c.dims
    N = T * H * W
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    axes = tuple(a.inp(t, n) for t, n in zip(c.axes, ("grid_t", "grid_h", "grid_w")))
    wb = []
    for i in (0, 2, 4):
        w = c.sd[f"trunk.fc.{i}.weight"]
        wb += [a.inp(w.t().contiguous(), f"w{i}t", ld=w.shape[0]), a.inp(c.sd[f"trunk.fc.{i}.bias"], f"b{i}")]
    out = a.out(N, p, name="t", ld=p)
    kern.don_trunk(tuple(o.op for o in axes), tuple(o.op for o in wb), out.op, T, H, W, p)
    a.check()
    judge(f"{c.name} N={N}", out.get(), r64["t"], r32["t"], (existing or {}).get("trunk"))


# ================================================================================================ BN + ReLU + pooling
def pool_extents(T, H, W, mode):
    return (1, 4, 4) if mode else (T // 2, H // 2, W // 2)


def pool_grid(dims, mode, cus=MI355X_CUS):
    """(work items, blocks) of rpb_don_bn_relu_pool: one thread per float4 of the output, 16 blocks of 256 per compute unit at the most"""
    B, T, H, W, C, ldx, ldo = dims
    To, Ho, Wo = pool_extents(T, H, W, mode)
    total = B * To * Ho * Wo * (ldo // 4)
    return total, min(ceil_div(total, 256), 16 * cus)


def pool_trips(dims, mode, cus=MI355X_CUS):
    total, grid = pool_grid(dims, mode, cus)
    return ceil_div(total, grid * 256)


def negative_channels(C):
    return torch.arange(C) % 4 == 1


@functools.lru_cache(maxsize=None)
def pool_case(B, T, H, W, C, ldx, ldo):
    g = _gen(92, B, T, H, W, C, ldx, ldo)
    u = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    x = torch.full((B, T, H, W, ldx), NAN)                        # columns C..ldx-1: a strided input's gaps
    x[..., :C] = torch.randn(B, T, H, W, C, generator=g)
    bn = [u(C) * 0.25 + 1, u(C) * 0.3, u(C) * 0.45, u(C) * 0.7 + 1.25]      # (weight away from 0, bias, running_mean, running_var)
    bn[1][negative_channels(C)] = -20.0                           # relu(...) == 0 in every cell of these channels
    bn = tuple(bn)
    sc64 = bn[0].double() / torch.sqrt(bn[3].double() + R.EPS)    # as DeepONet._build_prep folds the running statistics
    sc, sh = sc64.float(), (bn[1].double() - bn[2].double() * sc64).float()
    modes = POOL_CASES.get((B, T, H, W, C, ldx, ldo), (0, 1))

    def ref(dt):
        y = R.bn_relu(x[..., :C].to(dt), bn)
        return {m: (R.adaptive_pool(y) if m else R.max_pool(y)) for m in modes}
    return Case(f"bn_relu_pool B={B} T={T} H={H} W={W} C={C} ldx={ldx} ldo={ldo}", dict(dims=(B, T, H, W, C, ldx, ldo), x=x, sc=sc, sh=sh), ref)


def run_pool(kern, c, mode, existing=None):
    B, T, H, W, C, ldx, ldo = c.dims
    To, Ho, Wo = pool_extents(T, H, W, mode)
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    x, sc, sh = a.inp(c.x.reshape(-1, ldx), "x", ld=ldx), a.inp(c.sc, "sc"), a.inp(c.sh, "sh")
    out = a.out(B * To * Ho * Wo, ldo, name="out", ld=ldo)
    kern.don_bn_relu_pool(x.op, sc.op, sh.op, out.op, B, T, H, W, C, ldx, ldo, mode)
    a.check()                                                     # every column of every cell is written, C..ldo-1 included
    got = out.get().view(B, To, Ho, Wo, ldo)
    name = f"{c.name} mode={mode}"
    if ldo > C:
        exact(f"{name} columns C..ldo-1", got[..., C:], torch.zeros(B, To, Ho, Wo, ldo - C))
    neg = got[..., :C][..., negative_channels(C)]
    exact(f"{name} all-negative channels", neg, torch.zeros_like(neg))
    judge(name, got[..., :C], r64[mode], r32[mode], (existing or {}).get("bn_relu_pool"))


def run_pool_refused(kern, c, mode):
    """MaxPool3d(2) of an extent below 2: the library's error, nothing launched"""
    B, T, H, W, C, ldx, ldo = c.dims
    a = guarded.Arena(kern.dev)
    x, sc, sh = a.inp(c.x.reshape(-1, ldx), "x", ld=ldx), a.inp(c.sc, "sc"), a.inp(c.sh, "sh")
    out = a.out(4, ldo, name="out", ld=ldo, unwritten=torch.ones(4, ldo, dtype=torch.bool))
    with pytest.raises(RuntimeError, match=POOL_ERROR):
        kern.don_bn_relu_pool(x.op, sc.op, sh.op, out.op, B, T, H, W, C, ldx, ldo, mode)
    a.check()


# ---- the NaN rule, on plain tensors
NAN_DIMS = (2, 4, 6, 7, 8)                                        # (B, T, H, W, C), ld = C; W odd: column 6 is dropped by MaxPool3d(2)
NAN_AT = [(1, 1, 3, 2, 5), (0, 3, 1, 6, 2)]                       # (b, t, h, w, c): inside a window; in the dropped column / two h bins


def run_pool_nan(kern, mode, at):
    B, T, H, W, C = NAN_DIMS
    g = _gen(93, *NAN_DIMS)
    x = torch.randn(B, T, H, W, C, generator=g)
    x[at] = NAN
    sc, sh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    To, Ho, Wo = pool_extents(T, H, W, mode)
    xd, scd, shd = (t.reshape(-1).to(kern.dev) for t in (x, sc, sh))
    out = torch.full((B * To * Ho * Wo * C,), guarded.SENTINEL, device=kern.dev)
    kern.don_bn_relu_pool(xd, scd, shd, out, B, T, H, W, C, C, C, mode)
    got = out.cpu().view(B, To, Ho, Wo, C)
    y = F.relu(x.double() * sc.double() + sh.double()).permute(0, 4, 1, 2, 3)
    want = (F.adaptive_avg_pool3d(y, (1, 4, 4)) if mode else F.max_pool3d(y, 2)).permute(0, 2, 3, 4, 1)
    b, t, h, w, ch = at
    mask = torch.zeros(B, To, Ho, Wo, C, dtype=torch.bool)        # the windows / bins that contain the planted NaN, stated directly
    if mode:
        for i, (h0, h1) in enumerate(R.bins(H, 4)):
            for j, (w0, w1) in enumerate(R.bins(W, 4)):
                mask[b, 0, i, j, ch] = h0 <= h < h1 and w0 <= w < w1
    elif t < 2 * To and h < 2 * Ho and w < 2 * Wo:
        mask[b, t // 2, h // 2, w // 2, ch] = True
    print(f"[{TAG}] bn_relu_pool NaN rule mode={mode} NaN at {at}: {int(torch.isnan(got).sum())} NaN output(s), {int(mask.sum())} expected")
    assert torch.equal(torch.isnan(want), mask), "torch's pooling disagrees with the windows stated here"
    assert torch.equal(torch.isnan(got), mask), f"NaN outputs at {torch.isnan(got).nonzero().tolist()}, expected at {mask.nonzero().tolist()}"
    e = float((got.double() - want)[~mask].abs().max() / want[~mask].abs().max())
    print(f"[{TAG}] bn_relu_pool NaN rule mode={mode}: the other outputs max-abs {e:.3e} bound 1.000e-06")
    assert e <= 1e-6
