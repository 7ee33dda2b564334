"""The WDNO kernels one at a time against tests/wdno_restatement.py and torch's own ``conv3d``, every call on guard-banded operands
(tests/guarded.py): a stray write, an element never written and a stray read that reaches a result are assertions of ``Arena.check()``,
not GPU faults.

Shapes.  ``rpb_wdno_dec`` / ``_rec`` / ``_step`` run at the two fixture shapes (a: bior1.1, mesh (4,16,24), pad live in T only; b:
bior1.3, (6,10,10) with T_out = 2 T_in, odd coefficient extents, the crop live in ``rec``) and at B = 1, C = 3 with T odd for both
wavelets.  ``rpb_conv7x`` runs at Ci in {8, 24, 48} x N in {64, 256} on the meshes (4,8,12) (B = 2: M = 768, six full tiles) and (3,5,7)
(M = 210: a tail tile, the sample boundary inside a tile, and a halo wider than the mesh), and with KS = 3.

Bounds (tests/kernel_verdict.py): Rel-L2 and max |error| / max |reference| against the fp64 restatement, bounded by max(8 e32, 1e-6),
e32 being the same measure of the fp32 CPU restatement against its fp64 run (for the convolution: fp32 in a blocked summation order,
see ``conv_case``); the kernel's own output never enters a bound.  The
maximum mode of ``rpb_wdno_dec`` is bounded the same way (a maximum of |coefficient| inherits the coefficients' error).  Two calls of
``rpb_conv7x`` must be bit-equal, and it must agree with ``rpb_im2col`` + ``rpb_gemm_nt`` (the path it replaces) within the same bound."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                                    # noqa: E402
import wdno_restatement as R                      # noqa: E402
from kernel_verdict import MEASURES, bound_of, measures, verdict          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64

# name -> (wave, B, (T, H, W), C, r, padded mesh)
TRANSFORM_CASES = {
    "a_in": ("bior1.1", 2, (4, 16, 24), 2, 1, (4, 8, 12)),
    "a_out": ("bior1.1", 2, (4, 16, 24), 1, 1, (4, 8, 12)),
    "b_in": ("bior1.3", 2, (6, 10, 10), 1, 1, (8, 8, 8)),
    "b_out": ("bior1.3", 2, (6, 10, 10), 1, 2, (8, 8, 8)),
    "odd11": ("bior1.1", 1, (5, 6, 9), 3, 1, (4, 4, 8)),
    "odd13": ("bior1.3", 1, (5, 6, 9), 3, 1, (8, 8, 8)),
}


def _u(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def _filt(wave):
    t = R.TABLES[wave]
    return torch.tensor([t["dec_lo"], t["dec_hi"], t["rec_lo"], t["rec_hi"]], dtype=torch.float32)


def figures(got, r64, r32):
    return [(k, e32, ek) for k, e32, ek in zip(MEASURES, measures(r32, r64), measures(got, r64))]


@functools.lru_cache(maxsize=None)
def transform_case(name):
    wave, B, (T, H, W), C, r, padded = TRANSFORM_CASES[name]
    seed = sum(map(ord, name))
    x = _u(seed, B, r * T, H, W, C)
    ncol = 8 * C * r
    resc = torch.rand(ncol + 8, generator=torch.Generator().manual_seed(seed + 1)) * 3 + 0.5       # [8 leading columns | ours]
    cols64 = R.dec_state(x.double(), r, wave, resc[8:].double(), padded)
    cols32 = R.dec_state(x, r, wave, resc[8:], padded)
    raw64, raw32 = R.dec_state(x.double(), r, wave, None, padded), R.dec_state(x, r, wave, None, padded)
    state = _u(seed + 2, B, *padded, ncol + 8)
    rec64 = R.rec_state(state[..., 8:].double(), wave, resc[8:].double(), (T, H, W), C, r)
    rec32 = R.rec_state(state[..., 8:], wave, resc[8:], (T, H, W), C, r)
    return dict(x=x, resc=resc, cols64=cols64, cols32=cols32, max64=raw64.abs().reshape(-1, ncol).amax(0),
                max32=raw32.abs().reshape(-1, ncol).amax(0), state=state, rec64=rec64, rec32=rec32)


@pytest.fixture(scope="module")
def ops():
    from realpdebench_amd import ops as o
    return o


@pytest.mark.parametrize("name", list(TRANSFORM_CASES))
def test_dec(ops, name):
    wave, B, (T, H, W), C, r, padded = TRANSFORM_CASES[name]
    c = transform_case(name)
    L, ncol, ld = len(R.TABLES[wave]["dec_lo"]), 8 * C * r, 8 * C * r + 8
    a = guarded.Arena(DEV)
    other = torch.ones(B, *padded, ld, dtype=torch.bool)
    other[..., 8:] = False                                                      # the eight leading columns are not ours
    x, f, rs, st = a.inp(c["x"]), a.inp(_filt(wave)), a.inp(c["resc"]), a.out(B, *padded, ld, unwritten=other)
    ops.wdno_dec(x.op, f.op, rs.op, st.op, B, T, H, W, C, r, L, padded, ld, 8)
    a.check()
    got = st.get()[..., 8:]
    Tc, Hc, Wc = (R.coef_len(n, L) for n in (T, H, W))
    pad = got.clone()
    pad[:, :Tc, :Hc, :Wc] = 0
    assert not pad.any(), "cells outside the coefficient mesh must be exactly zero"
    verdict("wdno-kernels", f"dec {name}", figures(got, c["cols64"], c["cols32"]))
    rows = ops.wdno_dec_rows()
    a = guarded.Arena(DEV)
    x, f, part = a.inp(c["x"]), a.inp(_filt(wave)), a.out(rows, ncol)
    ops.wdno_dec_max(x.op, f.op, part.op, B, T, H, W, C, r, L)
    a.check()
    verdict("wdno-kernels", f"dec max {name}", figures(part.get().amax(0), c["max64"], c["max32"]))


@pytest.mark.parametrize("name", list(TRANSFORM_CASES))
def test_rec(ops, name):
    wave, B, (T, H, W), C, r, padded = TRANSFORM_CASES[name]
    c = transform_case(name)
    L, ld = len(R.TABLES[wave]["dec_lo"]), 8 * C * r + 8
    a = guarded.Arena(DEV)
    st, f, rs, out = a.inp(c["state"]), a.inp(_filt(wave)), a.inp(c["resc"]), a.out(B, r * T, H, W, C)
    ops.wdno_rec(st.op, f.op, rs.op, out.op, B, T, H, W, C, r, L, padded, ld, 8)
    a.check()
    verdict("wdno-kernels", f"rec {name}", figures(out.get(), c["rec64"], c["rec32"]))


# name -> (B, padded, coef, Cs, Ccond)
STEP_CASES = {"a": (2, (4, 8, 12), (2, 8, 12), 24, 16), "b": (2, (8, 8, 8), (5, 7, 7), 24, 8), "odd": (1, (4, 4, 8), (3, 3, 5), 48, 24)}
SCALARS = torch.tensor([1.7, 1.3, 0.8, 0.55, 0.25])


@functools.lru_cache(maxsize=None)
def step_case(name):
    B, padded, coef, Cs, Cc = STEP_CASES[name]
    seed = 700 + sum(map(ord, name))
    t = dict(img=_u(seed, B, *padded, Cs) * 1.5, eps=_u(seed + 1, B, *padded, Cs) * 1.5, cond=_u(seed + 2, B, *padded, Cc),
             noise=_u(seed + 3, B, *padded, Cs) * 2, scb=torch.rand(B, 2, generator=torch.Generator().manual_seed(seed + 4)) + 0.2)
    return t


@pytest.mark.parametrize("mode", [R.DDIM, R.DDIM_LAST, R.ANCESTRAL, "ancestral_t0", R.QSAMPLE, R.START])
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_step(ops, name, mode):
    B, padded, coef, Cs, Cc = STEP_CASES[name]
    c = step_case(name)
    no_noise = mode == "ancestral_t0"
    m = R.ANCESTRAL if no_noise else mode
    sc = c["scb"] if m == R.QSAMPLE else SCALARS
    kw = dict(img=c["img"], eps=c["eps"], cond=c["cond"], noise=None if no_noise else c["noise"], sc=sc)

    def ref(dt):
        return R.step(m, coef, **{k: (v.to(dt) if v is not None else None) for k, v in kw.items()})

    r64, r32 = ref(F64), ref(torch.float32)
    a = guarded.Arena(DEV)
    img, eps, cond, sca = a.inp(c["img"]), a.inp(c["eps"]), a.inp(c["cond"]), a.inp(sc)
    noise = None if no_noise else a.inp(c["noise"])
    out = a.out(B, *padded, Cs)
    out2 = a.out(B, *padded, Cs) if m == R.QSAMPLE else None
    ops.wdno_step(m, out.op, B, padded, coef, Cs, Cc, img=img.op, eps=eps.op, cond=cond.op, noise=noise.op if noise else None, sc=sca.op,
                  out2=out2.op if out2 else None)
    a.check()
    if m == R.QSAMPLE:
        verdict("wdno-kernels", f"step {name} q_sample", figures(out.get(), r64[0], r32[0]))
        assert torch.equal(out2.get(), r32[1]), "the conditioned noise target is a copy"
    else:
        verdict("wdno-kernels", f"step {name} mode {mode}", figures(out.get(), r64, r32))


def test_step_in_place(ops):
    """the sampler updates the state in place: out == img"""
    B, padded, coef, Cs, Cc = STEP_CASES["a"]
    c = step_case("a")
    ref = R.step(R.DDIM, coef, img=c["img"], eps=c["eps"], cond=c["cond"], noise=c["noise"], sc=SCALARS)
    a = guarded.Arena(DEV)
    eps, cond, noise, sca, img = a.inp(c["eps"]), a.inp(c["cond"]), a.inp(c["noise"]), a.inp(SCALARS), a.inout(c["img"])
    ops.wdno_step(R.DDIM, img.op, B, padded, coef, Cs, Cc, img=img.op, eps=eps.op, cond=cond.op, noise=noise.op, sc=sca.op)
    a.check()
    verdict("wdno-kernels", "step in place", figures(img.get(), ref.double(), ref))


# ================================================================================================ rpb_conv7x
MESHES = {"m768": (2, (4, 8, 12)), "m210": (2, (3, 5, 7))}


@functools.lru_cache(maxsize=None)
def conv_case(Ci, N, mesh, KS):
    B, (T, H, W) = MESHES[mesh]
    seed = Ci * 1000 + N + KS
    x = _u(seed, B, T, H, W, Ci)
    w = _u(seed + 1, N, Ci, KS, KS, KS) * (3.0 / (Ci * KS ** 3)) ** 0.5
    b = _u(seed + 2, N) * 0.2

    p = KS // 2
    r64 = F.conv3d(x.double().permute(0, 4, 1, 2, 3), w.double(), b.double(), padding=p).permute(0, 2, 3, 4, 1).reshape(-1, N)
    # the fp32 restatement sums the KS taps along W and the Ci channels of one (kt, kh) in one conv3d and adds the KS^2 partial results in
    # fp32 -- a blocked order, as every fp32 GEMM has one.  (One fp32 conv3d over all K = 343 Ci terms is off by 1e-6 to 3e-6 at these
    # shapes, above what the verdict accepts as a well-conditioned fp32 reference.)
    xp = F.pad(x.permute(0, 4, 1, 2, 3), (0, 0, p, p, p, p))
    acc = None
    for kt in range(KS):
        for kh in range(KS):
            y = F.conv3d(xp[:, :, kt:kt + T, kh:kh + H], w[:, :, kt:kt + 1, kh:kh + 1], padding=(0, 0, p))
            acc = y if acc is None else acc + y
    r32 = (acc + b.view(1, -1, 1, 1, 1)).permute(0, 2, 3, 4, 1).reshape(-1, N)
    return x, w, b, r64, r32


def run_conv7x(ops, x, w, b, B, mesh, Ci, N, KS):
    wz = ops.conv7x_wprep(w.to(DEV).contiguous())
    torch.cuda.synchronize()
    a = guarded.Arena(DEV)
    xi, wi, bi = a.inp(x), a.inp(wz.cpu().view(torch.float32), name="wz"), a.inp(b)
    M = B * mesh[0] * mesh[1] * mesh[2]
    out = a.out(M, N)
    assert ops.conv7x_supported(M, N, Ci, KS)
    ops.conv7x(xi.op, wi.op, out.op, B, mesh, Ci, N, KS, bias=bi.op)
    a.check()
    return out.get()


@pytest.mark.parametrize("mesh", list(MESHES))
@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("Ci", [8, 24, 48])
def test_conv7x(ops, Ci, N, mesh):
    B, m3 = MESHES[mesh]
    x, w, b, r64, r32 = conv_case(Ci, N, mesh, 7)
    got = run_conv7x(ops, x, w, b, B, m3, Ci, N, 7)
    verdict("wdno-kernels", f"conv7x Ci{Ci} N{N} {mesh}", figures(got, r64, r32))
    again = run_conv7x(ops, x, w, b, B, m3, Ci, N, 7)
    assert torch.equal(got, again), "two calls must be bit-equal"
    # the path it replaces: rpb_im2col + rpb_gemm_nt with the [N][tap Ci + ci] weight
    M, cols = r64.shape[0], 343 * Ci
    ldc = (cols + 127) // 128 * 128
    wi = torch.zeros(N, ldc)
    wi[:, :cols] = w.permute(0, 2, 3, 4, 1).reshape(N, cols)
    col, old = torch.empty(M, ldc, device=DEV), torch.empty(M, N, device=DEV)
    ops.im2col(x.reshape(M, Ci).to(DEV), col, B, *m3, Ci, 7, ldc)
    ops.gemm_nt(col, wi.to(DEV), old, M, N, ldc, bias=b.to(DEV))
    # both stand within max(8 e32, 1e-6) of the fp64 convolution (the old path's own tests hold it there): twice that between them
    for kind, e32, e in zip(MEASURES, measures(r32, r64), measures(got, old.cpu())):
        print(f"[wdno-kernels] conv7x Ci{Ci} N{N} {mesh} vs im2col + gemm {kind}: {e:.3e} bound {2 * bound_of(e32):.3e}")
        assert e <= 2 * bound_of(e32), (kind, e, e32)


@pytest.mark.parametrize("Ci,N,mesh", [(8, 64, "m210"), (72, 128, "m210")])
def test_conv7x_ks3(ops, Ci, N, mesh):
    """KS = 3, and Ci = 72: a second, partial 64-channel chunk"""
    B, m3 = MESHES[mesh]
    x, w, b, r64, r32 = conv_case(Ci, N, mesh, 3)
    verdict("wdno-kernels", f"conv7x KS3 Ci{Ci} N{N}", figures(run_conv7x(ops, x, w, b, B, m3, Ci, N, 3), r64, r32))


def test_conv7x_refuses(ops):
    from realpdebench_amd._lib import RpbError
    assert not ops.conv7x_supported(100, 96, 48, 7) and not ops.conv7x_supported(100, 64, 12, 7) and not ops.conv7x_supported(100, 64, 8, 4)
    assert not ops.conv7x_supported(100, 64, 264, 7) and ops.conv7x_supported(100, 128, 256, 5)
    x, out = torch.zeros(1, 2, 2, 2, 12, device=DEV), torch.zeros(8, 64, device=DEV)
    with pytest.raises(RpbError, match="unsupported"):
        ops.conv7x(x, torch.zeros(8, dtype=torch.int16, device=DEV), out, 1, (2, 2, 2), 12, 64, 7)
