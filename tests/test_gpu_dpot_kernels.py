"""The DPOT kernel family (csrc/rpb_dpot.hip: the sixteen rpb_dpot_* / rpb_rowtable_* / rpb_gn_tokens_* / rpb_afno_* entry points of
include/rpb.h) one kernel at a time against tests/dpot_restatement.py, at the block sizes, token counts and group shapes the
whole-model runs of test_gpu_dpot.py never reach.

Kernels that only move data or do one fp32 addition must equal the fp32 restatement bit for bit.  The arithmetic kernels are compared
with the restatement run in fp64 on two measures -- Rel-L2, and max |error| over max |reference| -- and the bound of each comparison
is max(8 * e32, 1e-6), where e32 is the same measure of the restatement run in fp32 on the CPU against its fp64 run: the kernel may
lose eight times what plain fp32 arithmetic on the same inputs loses (the MFMA sums K-long and token-long sequences in order where
torch's CPU kernels sum blocked / pairwise; the erf and cosine implementations differ), with a floor of 1e-6 where fp32 torch happens
to be nearly exact.  The kernel's own output never enters the bound, and a case whose 8 * e32 would exceed the project's fp32 bound of
1e-5 is rejected as badly conditioned.

Every output buffer is filled with a sentinel and carries 64 more sentinel elements past its end: elements the kernel does not
write and writes past the end are both seen."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dpot_restatement as R                 # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
GUARD = 64
SENTINEL = -3.0e30


@pytest.fixture(scope="module")
def ops():
    from realpdebench_amd import ops as o
    return o


def dev(t):
    return None if t is None else t.float().cuda().contiguous()


class Out:
    """A device output of the given shape, sentinel-filled, followed by GUARD sentinel elements."""

    def __init__(self, *shape):
        self.shape, self.n = shape, math.prod(shape)
        self.buf = torch.full((self.n + GUARD,), SENTINEL, device="cuda", dtype=F32)
        self.t = self.buf[:self.n].view(*shape)

    def get(self):
        """the host copy of the in-range part, after checking that the guard is untouched"""
        torch.cuda.synchronize()
        h = self.buf.cpu()
        assert torch.equal(h[self.n:], torch.full((GUARD,), SENTINEL)), "the kernel wrote past the end of its output"
        return h[:self.n].view(*self.shape)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())


def measures(a, ref):
    a, ref = a.double().flatten(), ref.double().flatten()
    d = a - ref
    return (float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300)))


def check(name, got, ref64, ref32):
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    for kind, e32, ek in zip(("rel-l2", "max-abs"), measures(ref32, ref64), measures(got, ref64)):
        bound = max(8 * e32, 1e-6)
        print(f"[dpot-kernels] {name} {kind}: e32 {e32:.3e} kernel {ek:.3e} bound {bound:.3e}")
        assert 8 * e32 <= 1e-5, f"{name}: badly conditioned inputs, the fp32 restatement itself is off by {e32:.3e} ({kind})"
        assert ek <= bound, f"{name} {kind}: kernel error {ek:.3e} > {bound:.3e} (fp32 restatement: {e32:.3e})"


def _cast(a, dt):
    return a.to(dt) if torch.is_tensor(a) and a.is_floating_point() else a


def ref_pair(fn, *args):
    """the restatement on the same (fp32-representable) inputs in fp64 and in fp32"""
    return fn(*[_cast(a, F64) for a in args]), fn(*[_cast(a, F32) for a in args])


def lin(m):
    return torch.tensor(np.linspace(0, 1, m), dtype=F32)          # the grids as model/dpot.py builds them


# ================================================================================================ exact kernels
@pytest.mark.parametrize("B,T,H,W,Cd,Cm,ps", [(2, 3, 8, 16, 2, 4, 4), (1, 1, 6, 3, 3, 3, 3), (1, 2, 16, 8, 1, 4, 8)])
def test_patch_tokens_and_bwd(ops, B, T, H, W, Cd, Cm, ps):
    torch.manual_seed(H * W)
    u = torch.randn(B, T, H, W, Cd)
    gx, gy, gt = lin(H), lin(W), lin(T)
    rows, Kp = B * (H // ps) * (W // ps) * T, (Cm + 3) * ps * ps
    P = Out(rows, Kp)
    ops.dpot_patch_tokens(dev(u), dev(gx), dev(gy), dev(gt), P.t, B, T, H, W, Cd, Cm, ps)
    assert torch.equal(P.get(), R.patch_tokens(u, gx, gy, gt, Cm, ps))
    gP = torch.randn(rows, Kp)
    gu = Out(B, T, H, W, Cd)
    ops.dpot_patch_tokens_bwd(dev(gP), gu.t, B, T, H, W, Cd, Cm, ps)
    assert torch.equal(gu.get(), R.patch_tokens_bwd(gP, B, T, H, W, Cd, Cm, ps))


@pytest.mark.parametrize("B,T,H,W,Cd,Co,ps,ldo", [(2, 2, 8, 16, 3, 4, 4, 8), (1, 3, 6, 3, 2, 4, 3, 32), (1, 1, 8, 8, 4, 4, 8, 4)])
def test_unpatch_and_bwd(ops, B, T, H, W, Cd, Co, ps, ldo):
    torch.manual_seed(ldo)
    O_ = torch.randn(B * H * W, ldo)
    pred = Out(B, T, H, W, Cd)
    ops.dpot_unpatch(dev(O_), pred.t, B, T, H, W, Cd, Co, ps, ldo)
    assert torch.equal(pred.get(), R.unpatch(O_, B, T, H, W, Cd, Co, ps))
    g = torch.randn(B, T, H, W, Cd)
    gO = Out(B * H * W, ldo)
    ops.dpot_unpatch_bwd(dev(g), gO.t, B, T, H, W, Cd, Co, ps, ldo)
    assert torch.equal(gO.get(), R.unpatch_bwd(g, Co, ps, ldo))


@pytest.mark.parametrize("B,nent,rpe,C", [(3, 5, 4, 4), (2, 7, 1, 36)])
def test_rowtable_add(ops, B, nent, rpe, C):
    torch.manual_seed(C)
    M = B * nent * rpe
    x, table = torch.randn(M, C), torch.randn(nent, C)
    xo = Out(M, C)
    xo.t.copy_(dev(x))
    ops.rowtable_add(xo.t, dev(table), M, C, rpe, nent)
    assert torch.equal(xo.get(), R.rowtable_add(x, table, rpe))


@pytest.mark.parametrize("nb,bs", [(3, 16), (1, 48)])
@pytest.mark.parametrize("transpose", [False, True])
def test_afno_wprep(ops, nb, bs, transpose):
    torch.manual_seed(bs)
    w = torch.randn(2, nb, bs, bs)
    Wc = Out(nb, 2 * bs, 2 * bs)
    ops.afno_wprep(dev(w), Wc.t, nb, bs, transpose)
    assert torch.equal(Wc.get(), R.afno_wprep(w, transpose))


# ================================================================================================ AFNO block MLP
MLP_SHAPES = [(1, 1, 16), (33, 3, 16), (70, 2, 48), (95, 2, 96), (64, 1, 128), (37, 2, 256)]


def _mlp_weights(nb, bs):
    """weights randn / sqrt(2 bs) (unit-variance layer outputs), biases randn: every term of both layers matters"""
    w1, w2 = torch.randn(2, nb, bs, bs) / math.sqrt(2 * bs), torch.randn(2, nb, bs, bs) / math.sqrt(2 * bs)
    return w1, w2, torch.randn(2, nb * bs), torch.randn(2, nb * bs)


@pytest.mark.parametrize("ntok,nb,bs", MLP_SHAPES)
@pytest.mark.parametrize("with_mid", [True, False])
@pytest.mark.parametrize("with_bias", [True, False])
def test_afno_mlp_forward(ops, ntok, nb, bs, with_mid, with_bias):
    torch.manual_seed(1000 * bs + ntok)
    C = nb * bs
    X = torch.randn(ntok, 2, C)
    w1, w2, b1, b2 = _mlp_weights(nb, bs)
    if not with_bias:
        b1 = b2 = None
    Wa, Wb = R.afno_wprep(w1, False), R.afno_wprep(w2, False)
    (mid64, out64), (mid32, out32) = ref_pair(lambda *a: R.afno_mlp(*a, None, nb, bs, 0), X, Wa, b1, Wb, b2)
    mid, out = (Out(ntok, 2, C) if with_mid else None), Out(ntok, 2, C)
    ops.afno_mlp(dev(X), dev(Wa), dev(b1), dev(Wb), dev(b2), None, mid.t if with_mid else None, out.t, ntok, nb, bs, 0)
    tag = f"afno_mlp fwd ntok={ntok} nb={nb} bs={bs} mid={int(with_mid)} bias={int(with_bias)}"
    check(tag + " out", out.get(), out64, out32)
    if with_mid:
        check(tag + " mid", mid.get(), mid64, mid32)


@pytest.mark.parametrize("ntok,nb,bs", MLP_SHAPES)
def test_afno_mlp_backward(ops, ntok, nb, bs):
    """mode 1 with the transposed composites: mid = (g W2c^T) * gelu'(aux), out = mid W1c^T"""
    torch.manual_seed(2000 * bs + ntok)
    C = nb * bs
    g = torch.randn(ntok, 2, C)
    aux = 1.5 * torch.randn(ntok, 2, C)                       # the saved pre-activation: both signs, into both GELU tails
    w1, w2, _, _ = _mlp_weights(nb, bs)
    W2t, W1t = R.afno_wprep(w2, True), R.afno_wprep(w1, True)
    (mid64, out64), (mid32, out32) = ref_pair(lambda g_, a_, b_, x_: R.afno_mlp(g_, a_, None, b_, None, x_, nb, bs, 1), g, W2t, W1t, aux)
    mid, out = Out(ntok, 2, C), Out(ntok, 2, C)
    ops.afno_mlp(dev(g), dev(W2t), None, dev(W1t), None, dev(aux), mid.t, out.t, ntok, nb, bs, 1)
    tag = f"afno_mlp bwd ntok={ntok} nb={nb} bs={bs}"
    check(tag + " mid", mid.get(), mid64, mid32)
    check(tag + " out", out.get(), out64, out32)


WGRAD_CASES = [(ntok, nb, bs) for nb, bs in ((2, 16), (1, 48), (1, 128)) for ntok in (1, 15, 17, 255, 257, 513, 5000)
               if ntok != 5000 or (nb, bs) == (2, 16)]


@pytest.mark.parametrize("ntok,nb,bs", WGRAD_CASES)
@pytest.mark.parametrize("a_gelu", [False, True])
def test_afno_wgrad(ops, ntok, nb, bs, a_gelu):
    torch.manual_seed(3000 * bs + ntok)
    C = nb * bs
    A, G = 1.5 * torch.randn(ntok, 2, C), torch.randn(ntok, 2, C)
    dw64, dw32 = ref_pair(lambda a_, g_: R.afno_wgrad(a_, g_, nb, bs, a_gelu), A, G)
    splits = ops.afno_wgrad_splits(ntok)
    part, dw = Out(splits, nb, 2 * bs, 2 * bs), Out(2, nb, bs, bs)
    ops.afno_wgrad(dev(A), dev(G), part.t, dw.t, ntok, nb, bs, a_gelu)
    part.get()                                                # the guard behind the partials
    check(f"afno_wgrad ntok={ntok} nb={nb} bs={bs} gelu={int(a_gelu)} dw", dw.get(), dw64, dw32)


def test_afno_wgrad_splits(ops):
    assert [ops.afno_wgrad_splits(n) for n in (1, 256, 257, 4096, 4097, 10 ** 6)] == [1, 1, 2, 16, 16, 16]


# ================================================================================================ GroupNorm on token rows
def _grid(t):
    """values on a 2^-10 grid: x + x2 is then exact in fp32, so the fp64 reference, its fp32 run and the kernel all normalise the very
    same numbers (a group with a single element has the exact answers y = beta, pg = 0)"""
    return torch.round(t * 1024) / 1024


@pytest.mark.parametrize("B,P,C,G", [(2, 1, 8, 8), (2, 5, 24, 8), (1, 64, 200, 2), (2, 33, 1024, 8), (1, 17, 1536, 8), (1, 9, 600, 1),
                                     (1, 4, 1024, 1)])
@pytest.mark.parametrize("with_x2", [False, True])
@pytest.mark.parametrize("with_gadd", [False, True])
def test_gn_tokens(ops, B, P, C, G, with_x2, with_gadd):
    """inputs sit at +8 (a one-pass variance would lose them); the backward kernel is handed the fp64 statistics rounded to fp32"""
    torch.manual_seed(C + P)
    eps = 1e-5
    x = _grid(torch.randn(B, P, C) + 8)
    x2 = _grid(torch.randn(B, P, C)) if with_x2 else None
    gadd = torch.randn(B, P, C) if with_gadd else None
    gamma, beta, gy = torch.randn(C), torch.randn(C), torch.randn(B, P, C)
    (y64, st64), (y32, st32) = ref_pair(lambda *a: R.gn_tokens_fwd(*a, G, eps), x, x2, gamma, beta)
    y, stat = Out(B, P, C), Out(B * G, 2)
    ops.gn_tokens_fwd(dev(x), dev(x2), dev(gamma), dev(beta), y.t, stat.t, B, P, C, G, eps)
    tag = f"gn_tokens B={B} P={P} C={C} G={G} x2={int(with_x2)} gadd={int(with_gadd)}"
    check(tag + " y", y.get(), y64, y32)
    st = stat.get()
    check(tag + " mean", st[:, 0], st64[:, 0], st32[:, 0])
    check(tag + " rstd", st[:, 1], st64[:, 1], st32[:, 1])
    stat_in = st64.float()
    r64, r32 = ref_pair(lambda *a: R.gn_tokens_bwd(*a, G), x, x2, gamma, stat_in, gy, gadd)
    gx, pg, pb = Out(B, P, C), Out(B, C), Out(B, C)
    ops.gn_tokens_bwd(dev(x), dev(x2), dev(gamma), dev(stat_in), dev(gy), dev(gadd), gx.t, pg.t, pb.t, B, P, C, G)
    for name, o, a, b in zip(("gx", "pg", "pb"), (gx, pg, pb), r64, r32):
        check(f"{tag} {name}", o.get(), a, b)


# ================================================================================================ TimeAggregator, pos_embed gradient
@pytest.mark.parametrize("T,C", [(1, 32), (4, 96)])
@pytest.mark.parametrize("with_sum", [False, True])
def test_tagg_prep_and_finish(ops, T, C, with_sum):
    torch.manual_seed(T * C)
    w = 1 / (T * C ** 0.5) * torch.randn(T, C, C)             # model/dpot.py: _TimeAgg and the plan's tt
    gamma = 2 ** torch.linspace(-10, 10, C)
    tt = torch.linspace(0, 1, T)
    (Wf64, Wb64, e64), (Wf32, Wb32, e32) = ref_pair(R.tagg_prep, w, gamma, tt)
    Wf, Wb, e = Out(C, T * C), Out(T * C, C), Out(T, C)
    ops.dpot_tagg_prep(dev(w), dev(gamma), dev(tt), Wf.t, Wb.t, e.t, T, C)
    tag = f"tagg T={T} C={C} sum={int(with_sum)}"
    check(tag + " Wf", Wf.get(), Wf64, Wf32)
    check(tag + " Wb", Wb.get(), Wb64, Wb32)
    check(tag + " e", e.get(), e64, e32)
    assert torch.equal(Wf.get(), Wb.get().t())
    dWb = torch.randn(T * C, C)
    dWsum = torch.randn(C, C) if with_sum else None
    (dw64, dg64), (dw32, dg32) = ref_pair(lambda a, b, c, d, s: R.tagg_finish(a, b, c, d, s), dWb, w, gamma, tt, dWsum)
    dw, dgamma = Out(T, C, C), Out(C)
    ops.dpot_tagg_finish(dev(dWb), dev(w), dev(gamma), dev(tt), dw.t, dgamma.t, T, C, dWsum=dev(dWsum))
    check(tag + " dw", dw.get(), dw64, dw32)
    check(tag + " dgamma", dgamma.get(), dg64, dg32)


@pytest.mark.parametrize("B,C,rpe,nent", [(3, 8, 4, 5), (2, 6, 1, 7)])
def test_rowtable_grad(ops, B, C, rpe, nent):
    torch.manual_seed(nent)
    g = torch.randn(B * nent * rpe, C)
    r64, r32 = ref_pair(lambda g_: R.rowtable_grad(g_, B, rpe, nent), g)
    dt = Out(nent, C)
    ops.rowtable_grad(dev(g), dt.t, B, C, rpe, nent)
    check(f"rowtable_grad B={B} C={C} rpe={rpe} nent={nent}", dt.get(), r64, r32)


# ================================================================================================ refusals
def test_refusals_are_loud(ops):
    """arguments outside a kernel's documented range raise and launch nothing: the outputs keep their sentinel"""
    from realpdebench_amd._lib import RpbError
    z = lambda *s: torch.zeros(*s, device="cuda")
    for bs in (24, 272):                                      # not a multiple of 16; above 256
        mid, out = Out(4, 2, bs), Out(4, 2, bs)
        with pytest.raises(RpbError):
            ops.afno_mlp(z(4, 2, bs), z(1, 2 * bs, 2 * bs), None, z(1, 2 * bs, 2 * bs), None, None, mid.t, out.t, 4, 1, bs, 0)
        assert mid.untouched() and out.untouched()
    mid, out = Out(4, 2, 16), Out(4, 2, 16)
    with pytest.raises(RpbError):                             # mode 1 without the saved pre-activation
        ops.afno_mlp(z(4, 2, 16), z(1, 32, 32), None, z(1, 32, 32), None, None, mid.t, out.t, 4, 1, 16, 1)
    assert mid.untouched() and out.untouched()
    y, stat = Out(1, 2, 1025), Out(1, 2)
    with pytest.raises(RpbError):                             # 1025 channels per group
        ops.gn_tokens_fwd(z(1, 2, 1025), None, z(1025), z(1025), y.t, stat.t, 1, 2, 1025, 1)
    assert y.untouched() and stat.untouched()
    x = Out(4, 6)
    with pytest.raises(RpbError):                             # C % 4 != 0
        ops.rowtable_add(x.t, z(2, 6), 4, 6, 1, 2)
    assert x.untouched()
    pred = Out(1, 2, 4, 4, 2)
    with pytest.raises(RpbError):                             # ldo = 4 < T * Co = 8
        ops.dpot_unpatch(z(16, 8), pred.t, 1, 2, 4, 4, 2, 4, 4, 4)
    assert pred.untouched()
