"""The two SyncBN entry points of the row BatchNorm family (csrc/rpb_rowbn.hip): ``ops.rowbn_finish_sums`` (the statistics from reduced
sums) and ``ops.rowbn_act_bwd_apply_sync`` (the backward apply from this rank's and all ranks' sums).

Two contracts each.  On one rank they ARE their siblings: with sums = rowbn_sum64(part), M_total = M (and sums_global = sums_local) every
output is bit-equal to ``rowbn_finish`` / ``rowbn_act_bwd_apply``.  On two "ranks" -- the two halves, 360 + 360 rows, of one block of
M = 720 rows whose sums are added in fp64 on the device, which is what the all-reduce does -- they give the BatchNorm of the whole
block: compared with fp64 on the CPU under the verdict of tests/kernel_verdict.py (8 times the error of the fp32 restatement, floor 1e-6).

Operands live in the guard-banded arenas of tests/guarded.py; rows arrive in buffers wider than C whose other columns are NaN.
C = 16 and 128; Cpad = C (runs of 8 channels per thread) and C + 4 (runs of 4); with and without LeakyReLU, whose inputs are drawn at
least 1e-3 from zero (closer elements are redrawn), so fp32 and fp64 agree on every gate.  The in-place operands (running statistics)
are plain tensors: an arena operand is either input or output."""
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                                    # noqa: E402
from kernel_verdict import measures, verdict      # noqa: E402
from realpdebench_amd import ops                  # noqa: E402
from realpdebench_amd._lib import RpbError        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I16, F64 = torch.int16, torch.float64
M_K, HALF = 720, 360
EPS, MOM = 1e-5, 0.1
VEC = ("a", "b", "mean", "rstd")
KINDS = ("rel-l2", "max-abs")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rows_in(a, block, ld, name):
    """block [M][C] as the first columns of an [M][ld] input operand whose other columns are NaN"""
    full = torch.full((block.shape[0], ld), float("nan"))
    full[:, :block.shape[1]] = block
    return a.inp(full, name)


def _stats64(y64, gamma, beta):
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    a = gamma.double() * rstd
    return dict(mean=mean, var=var, rstd=rstd, a=a, b=beta.double() - mean * a)


@functools.lru_cache(maxsize=None)
def _case(C):
    """y, gv, the BatchNorm parameters and the fp64 statistics of the whole block, computed once per channel count"""
    g = _g(4000 + C)
    scale = torch.rand(C, generator=g) * 1.5 + 0.5
    y = torch.randn(M_K, C, generator=g) * scale + torch.randn(C, generator=g)
    gamma, beta = torch.rand(C, generator=g) * 0.5 + 0.75, torch.rand(C, generator=g) * 0.6 - 0.3
    rm, rv = torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) * 1.4 + 0.55
    s = _stats64(y.double(), gamma, beta)
    for _ in range(50):                           # gate robustness: redraw what lies within 1e-3 of a LeakyReLU's zero
        close = (y.double() * s["a"] + s["b"]).abs() < 1e-3
        if not bool(close.any()):
            break
        y = torch.where(close, y + 0.01 * torch.randn(M_K, C, generator=g), y)
        s = _stats64(y.double(), gamma, beta)
    f32 = {k: s[k].float() for k in VEC}
    assert not bool(((y.double() * f32["a"].double() + f32["b"].double()).abs() < 5e-4).any())
    new_rm = (1 - MOM) * rm.double() + MOM * s["mean"]
    new_rv = (1 - MOM) * rv.double() + MOM * s["var"] * M_K / (M_K - 1)              # the unbiased factor 720 / 719
    # the fp32 restatement of the same statistics (what the verdict measures the kernel against)
    y32 = y.float()
    m32, v32 = y32.mean(0), y32.var(0, unbiased=False)
    r32 = 1.0 / torch.sqrt(v32 + torch.tensor(EPS))
    a32 = gamma * r32
    rest = dict(mean=m32, rstd=r32, a=a32, b=beta - m32 * a32, rm=(1 - MOM) * rm + MOM * m32,
                rv=(1 - MOM) * rv + MOM * v32 * torch.tensor(M_K / (M_K - 1.0)))
    return dict(y=y, gv=torch.randn(M_K, C, generator=g) * 1e-3, gamma=gamma, beta=beta, rm=rm, rv=rv, f32=f32, rest=rest,
                want=dict(mean=s["mean"], rstd=s["rstd"], a=s["a"], b=s["b"], rm=new_rm, rv=new_rv))


def _partials(y, ld, C):
    """rowbn_stats of y [m][C] (in an [m][ld] operand) -> the fp64 partials on the host"""
    a32, a64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    o_y, o_part = _rows_in(a32, y, ld, "y"), a64.out(ops.rowbn_rows(), 2 * C, name="part")
    ops.rowbn_stats(o_y.op, ld, y.shape[0], C, o_part.tensor())
    a32.check()
    a64.check()
    return o_part.get()


def _sum64(part, C):
    a = guarded.Arena(DEV, dtype=F64)
    i_part, o_sums = a.inp(part, "part"), a.out(2 * C, name="sums")
    ops.rowbn_sum64(i_part.tensor(), part.shape[0], C, o_sums.tensor())
    a.check()
    return o_sums.get()


def _finish(c, C, M, part=None, sums=None):
    """``rowbn_finish`` (``part``) or ``rowbn_finish_sums`` (``sums``) on arenas -> the six outputs"""
    a32, a64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    o_gamma, o_beta = a32.inp(c["gamma"], "gamma"), a32.inp(c["beta"], "beta")
    outs = {k: a32.out(C, name=k) for k in VEC}
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    tail = (o_gamma.op, o_beta.op, rm, rv, EPS, MOM, *(outs[k].op for k in VEC))
    if sums is None:
        ops.rowbn_finish(a64.inp(part, "part").tensor(), part.shape[0], M, C, *tail)
    else:
        ops.rowbn_finish_sums(a64.inp(sums, "sums").tensor(), M, C, *tail)
    a32.check()
    a64.check()
    return dict({k: outs[k].get() for k in VEC}, rm=rm.cpu(), rv=rv.cpu())


# ----------------------------------------------------------------------------------------------------------- finish from sums
@pytest.mark.parametrize("rows", [13, "all"])
@pytest.mark.parametrize("C", [16, 128])
def test_finish_from_sums_is_the_finish_on_one_rank(C, rows):
    """sums = rowbn_sum64(part), M_total = M: all six outputs have the bits of rowbn_finish(part, rows, M).  rows = 13: the partials of
    rowbn_stats folded onto 13 rows in fp64 (a row count that is no multiple of the eight row groups)."""
    c = _case(C)
    part = _partials(c["y"], C + 8, C)
    if rows == 13:
        part = torch.stack([part[r::13].sum(0) for r in range(13)])
    assert part.shape[0] == (13 if rows == 13 else ops.rowbn_rows())
    plain = _finish(c, C, M_K, part=part)
    synced = _finish(c, C, M_K, sums=_sum64(part, C))
    for k in plain:
        assert torch.equal(plain[k], synced[k]), f"{k}: {int((plain[k] != synced[k]).sum())} of {C} differ"
        assert not torch.equal(plain[k], c[k] if k in ("rm", "rv") else torch.zeros(C)), f"{k} was written"


@pytest.mark.parametrize("C", [16, 128])
def test_finish_from_the_sums_of_two_halves(C):
    """Each half: rowbn_stats, rowbn_sum64.  The two sums added in fp64 on the device and finished with M_total = 720 give the statistics
    of the whole block, the running variance with 720 / 719."""
    c = _case(C)
    halves = [_sum64(_partials(c["y"][r0:r0 + HALF], C + 8, C), C) for r0 in (0, HALF)]
    total = (halves[0].to(DEV) + halves[1].to(DEV)).cpu()
    got = _finish(c, C, M_K, sums=total)
    for k in ("mean", "rstd", "a", "b", "rm", "rv"):
        figures = [(kind, e32, ek) for kind, e32, ek in zip(KINDS, measures(c["rest"][k], c["want"][k]), measures(got[k], c["want"][k]))]
        verdict(f"C={C} two halves", f"rowbn_finish_sums {k}", figures)
    one = _finish(c, C, HALF, sums=halves[0])     # what a rank without the reduction would hold: far outside the bound
    assert measures(one["mean"], c["want"]["mean"])[0] > 1e-3


# ----------------------------------------------------------------------------------------------------------- backward apply
def _bwd_sums(c, C, act, r0, m):
    """rowbn_act_bwd_stats + rowbn_sum64 of the rows r0 .. r0 + m - 1 under the whole block's statistics -> sums [2 C] (host, fp64)"""
    a32, a64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    o_gv, o_y = _rows_in(a32, c["gv"][r0:r0 + m], C + 8, "gv"), _rows_in(a32, c["y"][r0:r0 + m], C + 8, "y")
    vec = [a32.inp(c["f32"][k], k) for k in VEC]
    o_part = a64.out(ops.rowbn_rows(), 2 * C, name="part")
    ops.rowbn_act_bwd_stats(o_gv.op, C + 8, o_y.op, C + 8, *(v.op for v in vec), m, C, act, o_part.tensor())
    a32.check()
    a64.check()
    return _sum64(o_part.get(), C)


def _apply(c, C, Cpad, act, r0, m, sums_local, sums_global=None, m_total=None, inplace=False):
    """One backward apply on arenas: the sibling when ``sums_global`` is None, else the SyncBN form -> (dy [m][Cpad], planes or None,
    dgamma, dbeta).  ``inplace``: dy is gv itself, a [m][Cpad] buffer whose pad columns hold NaN before the call."""
    a32, a64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    ld = C + 8
    gv, y = c["gv"][r0:r0 + m], c["y"][r0:r0 + m]
    if inplace:
        full = torch.full((m, Cpad), float("nan"))
        full[:, :C] = gv
        o_gv, ldg = a32.inout(full, "gv"), Cpad
        o_dy = o_gv
    else:
        o_gv, ldg = _rows_in(a32, gv, ld, "gv"), ld
        o_dy = a32.out(m, Cpad, name="dy")
    o_y = _rows_in(a32, y, ld, "y")
    vec = {k: a32.inp(c["f32"][k], k) for k in VEC}
    o_dp = a32.out(3, m, Cpad // 2, name="dy_planes") if Cpad % 8 == 0 else None
    o_dg, o_db = a32.out(C, name="dgamma"), a32.out(C, name="dbeta")
    i_loc = a64.inp(sums_local, "sums_local")
    kw = dict(dy=o_dy.op, ldd=Cpad, dy_planes=None if o_dp is None else o_dp.op, ldp=Cpad if o_dp is not None else 0, dgamma=o_dg.op,
              dbeta=o_db.op)
    if sums_global is None:
        ops.rowbn_act_bwd_apply(o_gv.op, ldg, m, C, Cpad, act, y=o_y.op, ldy=ld, **{k: v.op for k, v in vec.items()}, sums=i_loc.tensor(), **kw)
    else:
        i_glob = a64.inp(sums_global, "sums_global")
        ops.rowbn_act_bwd_apply_sync(o_gv.op, ldg, m, m_total, C, Cpad, act, o_y.op, ld, *(vec[k].op for k in VEC), i_loc.tensor(),
                                     i_glob.tensor(), **kw)
    a32.check()
    a64.check()
    planes = None if o_dp is None else o_dp.get().view(I16).view(3, m, Cpad)
    return o_dy.get(), planes, o_dg.get(), o_db.get()


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("C", [16, 128])
def test_sync_apply_is_the_apply_on_one_rank(C, pad, act, inplace):
    """sums_global = sums_local, M_total = M: rows, planes (Cpad % 8 == 0), dgamma and dbeta have the bits of rowbn_act_bwd_apply; both run
    lengths, and the in-place form."""
    c, Cpad = _case(C), C + pad
    sums = _bwd_sums(c, C, act, 0, M_K)
    plain = _apply(c, C, Cpad, act, 0, M_K, sums, inplace=inplace)
    synced = _apply(c, C, Cpad, act, 0, M_K, sums, sums_global=sums, m_total=M_K, inplace=inplace)
    assert bool(plain[0][:, :C].any()) and not bool(plain[0][:, C:].any()), "dy is written, its pad columns are exactly zero"
    assert (plain[1] is None) == (Cpad % 8 != 0)
    for name, p, s in zip(("dy", "dy_planes", "dgamma", "dbeta"), plain, synced):
        if p is not None:
            assert torch.equal(p, s), f"{name}: {int((p != s).sum())} elements differ"


def _bwd_reference(c, C, act, dtype):
    """BatchNorm + LeakyReLU backward of the whole block from the fp32 operands the kernels read, in ``dtype`` -> (dy, dgamma, dbeta)"""
    gv, y = c["gv"].to(dtype), c["y"].to(dtype)
    a, b, mu, rs = (c["f32"][k].to(dtype) for k in VEC)
    z = y * a + b
    dz = torch.where(z > 0, gv, 0.2 * gv) if act else gv
    xh = (y - mu) * rs
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    return a * (dz - dbeta / M_K - xh * dgamma / M_K), dgamma, dbeta


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("C", [16, 128])
def test_sync_apply_on_two_halves(C, pad, act):
    """Each half applies with the summed sums and M_total = 720: its dy is the whole block's; its dgamma and dbeta are its own sums
    rounded to fp32, and the two add up to the whole block's."""
    c, Cpad = _case(C), C + pad
    local = [_bwd_sums(c, C, act, r0, HALF) for r0 in (0, HALF)]
    total = (local[0].to(DEV) + local[1].to(DEV)).cpu()
    out = [_apply(c, C, Cpad, act, r0, HALF, local[i], sums_global=total, m_total=M_K) for i, r0 in enumerate((0, HALF))]
    dy = torch.cat([o[0] for o in out])
    want, rest = _bwd_reference(c, C, act, F64), _bwd_reference(c, C, act, torch.float32)
    tag = f"C={C} Cpad={Cpad} act={act} two halves"
    verdict(tag, "rowbn_act_bwd_apply_sync dy", [(k, e32, ek) for k, e32, ek in zip(KINDS, measures(rest[0], want[0]), measures(dy[:, :C], want[0]))])
    assert not bool(dy[:, C:].any()), "pad columns must be exactly zero"
    for i in range(2):
        assert torch.equal(out[i][2], local[i][C:].float()) and torch.equal(out[i][3], local[i][:C].float()), "dgamma, dbeta: the rank's own sums"
    for j, name in ((2, "dgamma"), (3, "dbeta")):
        both = out[0][j].double() + out[1][j].double()
        verdict(tag, f"rowbn_act_bwd_apply_sync {name} of both halves",
                [(k, e32, ek) for k, e32, ek in zip(KINDS, measures(rest[j - 1], want[j - 1]), measures(both, want[j - 1]))])
    # a half that keeps its own sums and M is far outside the bound: the reduction is what the figures above test
    alone = _apply(c, C, Cpad, act, 0, HALF, local[0])[0]
    assert measures(alone[:, :C], want[0][:HALF])[0] > 1e-3
    if Cpad % 8 == 0:                             # planes: the split of the rows, as for the sibling
        for o in out:
            ref = torch.empty(3 * HALF * Cpad, dtype=I16, device=DEV)
            ops.split3(o[0].to(DEV), ref, HALF, Cpad)
            assert torch.equal(ref.view(3, HALF, Cpad).cpu(), o[1])


# ----------------------------------------------------------------------------------------------------------- refusals
def _untouched(arena, *shape, name):
    return arena.out(*shape, name=name, unwritten=torch.ones(*shape, dtype=torch.bool))


def test_new_refusals_leave_the_outputs_untouched():
    """Each returns RPB_ERR_ARG (-1) before any launch: every output operand still holds the arena's sentinel."""
    M, C = 8, 32
    z, v = torch.zeros(M, 64, device=DEV), torch.zeros(4, 64, device=DEV)
    s = torch.zeros(128, dtype=F64, device=DEV)
    rm, rv = torch.full((C,), 0.25, device=DEV), torch.full((C,), 0.75, device=DEV)
    a = guarded.Arena(DEV)
    outs = [_untouched(a, C, name=k) for k in VEC]
    for m_total, Cx, why in ((1, C, "M_total > 1"), (16, 24, "C in")):      # one value per channel; a channel count that is no power of two
        with pytest.raises(RpbError, match=r"rpb_rowbn_finish_sums failed \(-1\).*" + why):
            ops.rowbn_finish_sums(s, m_total, Cx, v[0], v[1], rm, rv, EPS, MOM, *(o.op for o in outs))
    a.check()
    assert bool((rm == 0.25).all()) and bool((rv == 0.75).all()), "the running statistics did not move"
    a = guarded.Arena(DEV)
    o_dy, o_dp, o_dg, o_db = (_untouched(a, M, 64, name="dy"), _untouched(a, 3, M, 32, name="dy_planes"), _untouched(a, C, name="dgamma"),
                              _untouched(a, C, name="dbeta"))
    vec = (v[0], v[1], v[2], v[3])
    with pytest.raises(RpbError, match=r"rpb_rowbn_act_bwd_apply_sync failed \(-1\).*M_total=7 must be >= M=8"):      # fewer rows than this rank's
        ops.rowbn_act_bwd_apply_sync(z, 64, M, 7, C, 64, 0, z, 64, *vec, s, s, dy=o_dy.op, ldd=64, dy_planes=o_dp.op, ldp=64, dgamma=o_dg.op,
                                     dbeta=o_db.op)
    with pytest.raises(RpbError, match=r"rpb_rowbn_act_bwd_apply_sync failed \(-1\).*has_bn needs"):                   # no global sums
        ops.rowbn_act_bwd_apply_sync(z, 64, M, 16, C, 64, 0, z, 64, *vec, s, None, dy=o_dy.op, ldd=64, dgamma=o_dg.op, dbeta=o_db.op)
    with pytest.raises(RpbError, match=r"rpb_rowbn_act_bwd_apply_sync failed \(-1\).*plane output.*Cpad=36 ldp=64"):   # planes at Cpad % 8 == 4
        ops.rowbn_act_bwd_apply_sync(z, 64, M, 16, C, 36, 0, z, 64, *vec, s, s, dy=o_dy.op, ldd=64, dy_planes=o_dp.op, ldp=64)
    with pytest.raises(RpbError, match=r"rpb_rowbn_act_bwd_apply_sync failed \(-1\)"):                                 # C = 24
        ops.rowbn_act_bwd_apply_sync(z, 64, M, 16, 24, 64, 0, z, 64, *vec, s, s, dy=o_dy.op, ldd=64)
    a.check()
