"""The row kernels of the CNO3d training step (csrc/rpb_rowbn.hip, through the ``ops.rowbn_*`` wrappers) one by one, and the data gradient through rpb_cno_conv3x.

Operands live in the guard-banded arena of tests/guarded.py (fp64 partials and sums in an fp64 arena of their own); references are fp64
torch on the CPU, computed once per shape.  M = 720 = B 3 x mesh (5, 6, 8): five full 128-row tiles and a tail, more rows than one
workgroup takes.  Channel layouts: C = 16 in a 64-wide buffer, 64, 128, and C = 64 at column 64 of a 128-wide buffer.
Bounds (u = 2^-24):
  statistics            mean, rstd, a, b and the updated running statistics within 4 u relative of fp64: the kernel forms them in fp64
                        from fp64 sums and rounds once; one case has channel mean / std = 30 (cancellation in sum y^2 - mean^2)
  forward apply         fp32 rows within 16 u (|y a| + |b| + |res|) elementwise; planes bit-equal to rpb_split3 of the rows
  backward              dgamma, dbeta within 4 u relative of the fp64 sums of the same fp32 inputs; dy within 16 u of the sum of the
                        magnitudes of its three terms; pad columns exactly zero; planes bit-equal to the split of the rows
  data gradient         the rule of tests/test_gpu_cno.py::test_cno_conv3x_kernel: Rel-L2 < 1e-6, < 2e-6 with a residual
LeakyReLU inputs are drawn with |y a + b| >= 1e-3 (closer elements are redrawn, none is excluded), so fp32 and fp64 agree on every gate.
The in-place operands (running statistics; ``res`` aliasing ``out``) are plain tensors: an arena operand is either input or output.
Two calls of every kernel are bit-equal."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                                    # noqa: E402
from realpdebench_amd import ops                  # noqa: E402
from realpdebench_amd.model._common import flipped_weight      # noqa: E402
from realpdebench_amd.model.cno import CNO3d      # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I16, F64 = torch.int16, torch.float64
U = 2.0 ** -24
B_K, MESH_K = 3, (5, 6, 8)
M_K = B_K * MESH_K[0] * MESH_K[1] * MESH_K[2]
EPS, MOM = 1e-5, 0.1
LAYOUTS = [(16, 64, 0), (64, 64, 0), (128, 128, 0), (64, 128, 64)]      # (C, ld, first column)


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _within(got, want, bound, what):
    err = (got.double() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst error / bound {worst:.3f}")
    assert bool((err <= bound).all()), (what, worst)


def _rows_in(a, block, ld, col, name):
    """a [M][C] block as the columns col.. of an [M][ld] input operand whose other columns are NaN"""
    full = torch.full((block.shape[0], ld), float("nan"))
    full[:, col:col + block.shape[1]] = block
    return a.inp(full, name)


def _planes(op_f32, M, ld):
    return op_f32.view(I16).view(3, M, ld)


def _split3(rows):
    M, C = rows.shape
    want = torch.empty(3 * M * C, dtype=I16, device=DEV)
    ops.split3(rows.contiguous().to(DEV), want, M, C)
    return want.view(3, M, C).cpu()


@functools.lru_cache(maxsize=None)
def _case(C, shifted=False):
    """y, BatchNorm parameters and the fp64 statistics of one channel count; ``shifted``: channel mean = 30 standard deviations"""
    g = _g(C + (1000 if shifted else 0))
    scale = torch.rand(C, generator=g) * 1.5 + 0.5
    y = torch.randn(M_K, C, generator=g) * scale + (30.0 * scale if shifted else torch.randn(C, generator=g))
    gamma, beta = torch.rand(C, generator=g) * 0.5 + 0.75, torch.rand(C, generator=g) * 0.6 - 0.3
    rm, rv = torch.rand(C, generator=g) - 0.5, torch.rand(C, generator=g) * 1.4 + 0.55
    y64 = y.double()
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + EPS)
    a = gamma.double() * rstd
    b = beta.double() - mean * a
    # gate robustness: redraw every element whose LeakyReLU input is within 1e-3 of zero (the statistics above are then recomputed)
    for _ in range(50):
        close = (y64 * a + b).abs() < 1e-3
        if not bool(close.any()):
            break
        y = torch.where(close, y + 0.01 * torch.randn(M_K, C, generator=g), y)
        y64 = y.double()
        mean, var = y64.mean(0), y64.var(0, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + EPS)
        a = gamma.double() * rstd
        b = beta.double() - mean * a
    assert not bool(((y64 * a + b).abs() < 1e-3).any())
    f32 = dict(a=a.float(), b=b.float(), mean=mean.float(), rstd=rstd.float())
    assert not bool(((y64 * f32["a"].double() + f32["b"].double()).abs() < 5e-4).any())
    new_rm = (1 - MOM) * rm.double() + MOM * mean
    new_rv = (1 - MOM) * rv.double() + MOM * var * M_K / (M_K - 1)
    return dict(y=y, gamma=gamma, beta=beta, rm=rm, rv=rv, mean=mean, rstd=rstd, a=a, b=b, new_rm=new_rm, new_rv=new_rv,
                res=torch.randn(M_K, C, generator=g), gv=torch.randn(M_K, C, generator=g) * 1e-3, **{k + "32": v for k, v in f32.items()})


# ----------------------------------------------------------------------------------------------------------- statistics
@pytest.mark.parametrize("C,ld,col,shifted", [(*l, False) for l in LAYOUTS] + [(64, 64, 0, True)])
def test_bn_stats_and_finish(C, ld, col, shifted):
    c = _case(C, shifted)
    rows = ops.rowbn_rows()
    a32, a64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    o_y = _rows_in(a32, c["y"], ld, col, "y")
    o_gamma, o_beta = a32.inp(c["gamma"], "gamma"), a32.inp(c["beta"], "beta")
    outs = {k: a32.out(C, name=k) for k in ("a", "b", "mean", "rstd")}
    o_part = a64.out(rows, 2 * C, name="part")
    rm, rv = c["rm"].to(DEV), c["rv"].to(DEV)
    ops.rowbn_stats(o_y.at(col), ld, M_K, C, o_part.tensor())
    a64.check()
    # (the finish reads the partials: a second fp64 arena holds them as an input)
    b64 = guarded.Arena(DEV, dtype=F64)
    i_part = b64.inp(o_part.get(), "part")
    ops.rowbn_finish(i_part.tensor(), rows, M_K, C, o_gamma.op, o_beta.op, rm, rv, EPS, MOM, *(outs[k].op for k in ("a", "b", "mean", "rstd")))
    a32.check()
    b64.check()
    part = o_part.get()
    y64 = c["y"].double()
    assert abs(float(part[:, :C].sum()) - float(y64.sum())) <= 1e-12 * float(y64.abs().sum())
    assert abs(float(part[:, C:].sum()) - float((y64 * y64).sum())) <= 1e-12 * float((y64 * y64).sum())
    for k in ("mean", "rstd", "a", "b"):
        _within(outs[k].get(), c[k], 4 * U * c[k].abs(), f"C={C} col={col} shifted={shifted} {k}")
    _within(rm.cpu(), c["new_rm"], 4 * U * c["new_rm"].abs(), "running_mean")
    _within(rv.cpu(), c["new_rv"], 4 * U * c["new_rv"].abs(), "running_var")
    # a second call, into plain tensors, is bit-equal
    yb = torch.zeros(M_K, ld)
    yb[:, col:col + C] = c["y"]
    yb, part2, ab2 = yb.to(DEV), torch.empty(rows, 2 * C, dtype=F64, device=DEV), torch.empty(4, C, device=DEV)
    rm2, rv2 = c["rm"].to(DEV), c["rv"].to(DEV)
    ops.rowbn_stats(ops.Sub(yb, col), ld, M_K, C, part2)
    ops.rowbn_finish(part2, rows, M_K, C, c["gamma"].to(DEV), c["beta"].to(DEV), rm2, rv2, EPS, MOM, *ab2)
    assert torch.equal(part2.cpu(), part) and torch.equal(rm2, rm) and torch.equal(rv2, rv)
    for i, k in enumerate(("a", "b", "mean", "rstd")):
        assert torch.equal(ab2[i].cpu(), outs[k].get()), k


# ----------------------------------------------------------------------------------------------------------- forward apply
@pytest.mark.parametrize("act,with_res,outs", [(1, False, "both"), (0, True, "both"), (1, True, "planes"), (0, False, "f32")])
@pytest.mark.parametrize("C,ld,col", LAYOUTS)
def test_bn_act_fwd(C, ld, col, act, with_res, outs):
    c = _case(C)
    a = guarded.Arena(DEV)
    o_y = a.inp(c["y"], "y")
    o_a, o_b = a.inp(c["a32"], "a"), a.inp(c["b32"], "b")
    o_res = _rows_in(a, c["res"], ld, col, "res") if with_res else None
    un = torch.ones(M_K, ld, dtype=torch.bool)
    un[:, col:col + C] = False
    unp = torch.ones(3, M_K, ld // 2, dtype=torch.bool)
    unp[:, :, col // 2:(col + C) // 2] = False
    o_out = a.out(M_K, ld, name="out", unwritten=un if C < ld else None) if outs in ("both", "f32") else None
    o_op = a.out(3, M_K, ld // 2, name="planes", unwritten=unp if C < ld else None) if outs in ("both", "planes") else None
    kw = dict(res=None if o_res is None else o_res.at(col), ldr=ld, out=None if o_out is None else o_out.at(col), ldo=ld,
              out_planes=None if o_op is None else o_op.at(col // 2), ldp=ld)
    ops.rowbn_act_fwd(o_y.op, C, o_a.op, o_b.op, M_K, C, act, **kw)
    a.check()
    y64, a64, b64 = c["y"].double(), c["a32"].double(), c["b32"].double()
    v = y64 * a64 + b64
    if act:
        v = torch.where(v > 0, v, 0.2 * v)
    bound = 16 * U * ((y64 * a64).abs() + b64.abs())
    if with_res:
        v, bound = v + c["res"].double(), bound + 16 * U * c["res"].double().abs()
    rows = None
    if o_out is not None:
        rows = o_out.get()[:, col:col + C].contiguous()
        _within(rows, v, bound, f"C={C} col={col} act={act} res={with_res} rows")
    if o_op is not None:
        pl = _planes(o_op.get(), M_K, ld)[:, :, col:col + C].contiguous()
        if rows is None:
            rows = ((pl.to(torch.int32) << 16).view(torch.float32).double().sum(0)).float()
            _within(rows, v, bound, f"C={C} col={col} act={act} res={with_res} planes")
        assert torch.equal(_split3(rows), pl), "planes must be bit-equal to rpb_split3 of the fp32 rows"
    if outs == "both":                            # a second call, into plain tensors, is bit-equal
        out2, op2 = torch.zeros(M_K, ld, device=DEV), torch.zeros(3 * M_K * ld, dtype=I16, device=DEV)
        resb = torch.zeros(M_K, ld)
        resb[:, col:col + C] = c["res"]
        ops.rowbn_act_fwd(c["y"].to(DEV), C, c["a32"].to(DEV), c["b32"].to(DEV), M_K, C, act, res=ops.Sub(resb.to(DEV), col) if with_res else None,
                           ldr=ld, out=ops.Sub(out2, col), ldo=ld, out_planes=op2.data_ptr() + 2 * col, ldp=ld)
        assert torch.equal(out2.cpu()[:, col:col + C], rows)
        assert torch.equal(op2.view(3, M_K, ld).cpu()[:, :, col:col + C], _planes(o_op.get(), M_K, ld)[:, :, col:col + C])


# ----------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C,ld,col", LAYOUTS)
def test_bn_act_bwd(C, ld, col, act):
    """gv arrives at column ``col`` of an ld-wide gradient buffer (the concat); dy leaves max(C, 64) wide with zero pad columns."""
    c = _case(C)
    rows, Cpad = ops.rowbn_rows(), max(C, 64)
    a32, a64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    o_gv, o_y = _rows_in(a32, c["gv"], ld, col, "gv"), a32.inp(c["y"], "y")
    vec = {k: a32.inp(c[k + "32"], k) for k in ("a", "b", "mean", "rstd")}
    o_dy, o_dp = a32.out(M_K, Cpad, name="dy"), a32.out(3, M_K, Cpad // 2, name="dy_planes")
    o_dg, o_db = a32.out(C, name="dgamma"), a32.out(C, name="dbeta")
    o_part = a64.out(rows, 2 * C, name="part")
    ops.rowbn_act_bwd_stats(o_gv.at(col), ld, o_y.op, C, vec["a"].op, vec["b"].op, vec["mean"].op, vec["rstd"].op, M_K, C, act, o_part.tensor())
    a64.check()
    b64 = guarded.Arena(DEV, dtype=F64)
    i_part, o_sums = b64.inp(o_part.get(), "part"), b64.out(2 * C, name="sums")
    ops.rowbn_sum64(i_part.tensor(), rows, C, o_sums.tensor())
    b64.check()
    c64 = guarded.Arena(DEV, dtype=F64)
    i_sums = c64.inp(o_sums.get(), "sums")
    ops.rowbn_act_bwd_apply(o_gv.at(col), ld, M_K, C, Cpad, act, y=o_y.op, ldy=C, a=vec["a"].op, b=vec["b"].op, mean=vec["mean"].op,
                             rstd=vec["rstd"].op, sums=i_sums.tensor(), dy=o_dy.op, ldd=Cpad, dy_planes=o_dp.op, ldp=Cpad, dgamma=o_dg.op,
                             dbeta=o_db.op)
    a32.check()
    c64.check()
    # fp64 reference from the same fp32 inputs
    gv, y64 = c["gv"].double(), c["y"].double()
    a_, b_, mu, rs = (c[k + "32"].double() for k in ("a", "b", "mean", "rstd"))
    z = y64 * a_ + b_
    dz = torch.where(z > 0, gv, 0.2 * gv) if act else gv
    xh = (y64 - mu) * rs
    dbeta, dgamma = dz.sum(0), (dz * xh).sum(0)
    sums = o_sums.get()
    tot = o_part.get().sum(0)
    assert float((sums - tot).abs().max()) <= 1e-14 * float(o_part.get().abs().sum(0).max()), "sum64 adds the rows of the partials"
    _within(o_db.get(), dbeta, 4 * U * dbeta.abs(), f"C={C} col={col} act={act} dbeta")
    _within(o_dg.get(), dgamma, 4 * U * dgamma.abs(), f"C={C} col={col} act={act} dgamma")
    t1, t2, t3 = a_ * dz, a_ * dbeta / M_K, a_ * xh * dgamma / M_K
    dy = o_dy.get()
    _within(dy[:, :C], t1 - t2 - t3, 16 * U * (t1.abs() + t2.abs() + t3.abs()), f"C={C} col={col} act={act} dy")
    assert not bool(dy[:, C:].any()), "pad columns must be exactly zero"
    # a figure, not an assertion: sum_m dy is zero in exact arithmetic; what is left, against unbiased rounding of one u per element
    print(f"C={C} col={col} act={act}: |sum_m dy| / (sqrt(M) u rms dy) = "
          f"{float((dy[:, :C].double().sum(0).abs() / (M_K ** 0.5 * U * dy[:, :C].double().pow(2).mean(0).sqrt())).mean()):.2f}")
    pl = _planes(o_dp.get(), M_K, Cpad)
    assert torch.equal(_split3(dy), pl), "planes must be bit-equal to rpb_split3 of the rows (zero pad columns included)"
    # a second pass, into plain tensors, is bit-equal
    gb = torch.zeros(M_K, ld)
    gb[:, col:col + C] = c["gv"]
    gb, yd = gb.to(DEV), c["y"].to(DEV)
    v32 = [c[k + "32"].to(DEV) for k in ("a", "b", "mean", "rstd")]
    part2, sums2 = torch.empty(rows, 2 * C, dtype=F64, device=DEV), torch.empty(2 * C, dtype=F64, device=DEV)
    dy2, dp2, dgb2 = torch.empty(M_K, Cpad, device=DEV), torch.empty(3 * M_K * Cpad, dtype=I16, device=DEV), torch.empty(2, C, device=DEV)
    ops.rowbn_act_bwd_stats(ops.Sub(gb, col), ld, yd, C, *v32, M_K, C, act, part2)
    ops.rowbn_sum64(part2, rows, C, sums2)
    ops.rowbn_act_bwd_apply(ops.Sub(gb, col), ld, M_K, C, Cpad, act, y=yd, ldy=C, a=v32[0], b=v32[1], mean=v32[2], rstd=v32[3], sums=sums2,
                             dy=dy2, ldd=Cpad, dy_planes=dp2, ldp=Cpad, dgamma=dgb2[0], dbeta=dgb2[1])
    assert torch.equal(part2.cpu(), o_part.get()) and torch.equal(sums2.cpu(), sums) and torch.equal(dy2.cpu(), dy)
    assert torch.equal(dp2.view(3, M_K, Cpad).cpu(), pl) and torch.equal(dgb2[0].cpu(), o_dg.get()) and torch.equal(dgb2[1].cpu(), o_db.get())


def test_gate_only_backward():
    """has_bn = 0 (lift.0 / project.0): dy = gv (v > 0 ? 1 : 0.2) from the sign of the saved LeakyReLU output; rows only (lift.0 needs
    no data gradient) and rows + planes."""
    c = _case(64)
    z = c["y"].double() * c["a32"].double() + c["b32"].double()
    v = torch.where(z > 0, z, 0.2 * z).float()
    for planes in (False, True):
        a = guarded.Arena(DEV)
        o_gv, o_v = a.inp(c["gv"], "gv"), a.inp(v, "v")
        o_dy = a.out(M_K, 64, name="dy")
        o_dp = a.out(3, M_K, 32, name="dy_planes") if planes else None
        ops.rowbn_act_bwd_apply(o_gv.op, 64, M_K, 64, 64, 1, y=o_v.op, ldy=64, dy=o_dy.op, ldd=64, dy_planes=None if o_dp is None else o_dp.op,
                                 ldp=64 if planes else 0)
        a.check()
        want = torch.where(v > 0, c["gv"].double(), 0.2 * c["gv"].double())     # (one rounded product with the fp32 constant 0.2f: 1.125 u)
        _within(o_dy.get(), want, 2 * U * want.abs(), f"gate-only planes={planes}")
        if planes:
            assert torch.equal(_split3(o_dy.get()), _planes(o_dp.get(), M_K, 64))


def test_row_kernels_refuse_what_they_do_not_cover():
    from realpdebench_amd import _lib
    y, p = torch.zeros(8, 64, device=DEV), torch.zeros(ops.rowbn_rows(), 128, dtype=F64, device=DEV)
    v = torch.zeros(4, 64, device=DEV)
    with pytest.raises(_lib.RpbError, match="rowbn_stats"):
        ops.rowbn_stats(y, 64, 8, 24, p)
    with pytest.raises(_lib.RpbError, match="rowbn_stats"):
        ops.rowbn_stats(y, 62, 8, 16, p)
    with pytest.raises(_lib.RpbError, match="rowbn_finish"):
        ops.rowbn_finish(p, 4, 1, 64, v[0], v[1], v[2], v[3], EPS, MOM, *torch.zeros(4, 64, device=DEV))       # M = 1: no batch statistics
    with pytest.raises(_lib.RpbError, match="rowbn_act_fwd"):
        ops.rowbn_act_fwd(y, 64, v[0], v[1], 8, 64, 1)                                                       # no output
    with pytest.raises(_lib.RpbError, match="rowbn_act_fwd"):
        ops.rowbn_act_fwd(y, 64, v[0], v[1], 8, 64, 1, out_planes=torch.zeros(3 * 8 * 64, dtype=I16, device=DEV), ldp=60)
    with pytest.raises(_lib.RpbError, match="rowbn_act_bwd_apply"):
        ops.rowbn_act_bwd_apply(y, 64, 8, 64, 32, 1, y=y, ldy=64, dy=torch.zeros(8, 64, device=DEV), ldd=64)   # Cpad < C
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------- data gradient
@functools.lru_cache(maxsize=None)
def _dgrad_case(Ci, Co):
    """dy, the weights and the fp64 ``conv_transpose3d`` of one Conv3d(Ci, Co, 3, padding=1)"""
    T, H, W = MESH_K
    g = _g(Ci * 7 + Co)
    conv = torch.nn.Conv3d(Ci, Co, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_((torch.rand(Co, Ci, 3, 3, 3, generator=g) * 2 - 1) * (3.0 / (27 * Ci)) ** 0.5 * 1.4)
    dy = torch.rand(M_K, Co, generator=g) * 2 - 1
    res = torch.rand(M_K, Ci, generator=g) * 2 - 1
    want = F.conv_transpose3d(dy.view(B_K, T, H, W, Co).permute(0, 4, 1, 2, 3).double(), conv.weight.detach().double(), padding=1)
    want = want.permute(0, 2, 3, 4, 1).reshape(M_K, Ci)
    planes = torch.empty(3 * M_K * Co, dtype=I16, device=DEV)
    ops.split3(dy.to(DEV), planes, M_K, Co)
    wd = CNO3d.k_wprep(flipped_weight(conv, Co, Ci).to(DEV), Ci, Co)
    torch.cuda.synchronize()
    return dict(res=res, want=want, planes=planes.cpu().view(torch.float32), wd=wd.cpu().view(torch.float32))


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("Ci,Co", [(64, 64), (128, 64), (64, 128)])
def test_data_gradient_through_cno_conv3x(Ci, Co):
    """The data gradient of Conv3d(Ci, Co) is rpb_cno_conv3x with N = Ci, Ci = Co on the flipped, transposed taps, sc = 1, sh = 0.
    Written plainly, written at a column offset of a wider buffer, and accumulated with ``res`` aliasing ``out``."""
    c = _dgrad_case(Ci, Co)
    one, zero = torch.ones(Ci), torch.zeros(Ci)
    ldo, col = 2 * Ci, Ci                          # the gradient buffer of a concat: this launch owns columns Ci..2 Ci - 1
    a = guarded.Arena(DEV)
    o_pl, o_wd = a.inp(c["planes"], "planes", ld=Co // 2), a.inp(c["wd"], "wd", ld=512)
    o_sc, o_sh = a.inp(one, "sc"), a.inp(zero, "sh")
    un = torch.ones(M_K, ldo, dtype=torch.bool)
    un[:, col:] = False
    o_out = a.out(M_K, ldo, name="out", unwritten=un)
    CNO3d.k_conv(o_pl.op, o_wd.op, o_sc.op, o_sh.op, M_K, Ci, Co, MESH_K, Ci, 0, out=o_out.at(col), ldo=ldo)
    a.check()
    plain = o_out.get()[:, col:].contiguous()
    e = _rel(plain, c["want"])
    print(f"Ci={Ci} Co={Co}: data gradient Rel-L2 {e:.2e} (bound 1e-06)")
    # a figure, not an assertion: the column mean of the error against what unbiased rounding of this size would leave (a bias gradient
    # is a column sum of such a tensor, so a biased error would show there first)
    err = plain.double() - c["want"]
    print(f"Ci={Ci} Co={Co}: |column mean of the error| / (rms error / sqrt(M)) = "
          f"{float((err.mean(0).abs() / (err.pow(2).mean(0).sqrt() / M_K ** 0.5)).mean()):.2f} (about 0.8 when unbiased)")
    assert e < 1e-6
    # accumulation: res aliases out element for element
    pl, wd = c["planes"].to(DEV).view(I16), c["wd"].to(DEV).view(I16)
    buf = c["res"].to(DEV).clone()
    CNO3d.k_conv(pl, wd, one.to(DEV), zero.to(DEV), M_K, Ci, Co, MESH_K, Ci, 0, res=buf, ldr=Ci, out=buf, ldo=Ci)
    apart = torch.empty(M_K, Ci, device=DEV)
    CNO3d.k_conv(pl, wd, one.to(DEV), zero.to(DEV), M_K, Ci, Co, MESH_K, Ci, 0, res=c["res"].to(DEV), ldr=Ci, out=apart, ldo=Ci)
    e = _rel(buf.cpu(), c["want"] + c["res"].double())
    print(f"Ci={Ci} Co={Co}: accumulated in place Rel-L2 {e:.2e} (bound 2e-06)")
    assert e < 2e-6
    assert torch.equal(buf, apart), "res aliasing out gives what separate buffers give"
    assert torch.equal(apart.cpu(), plain + c["res"]), "sc = 1, sh = 0: the accumulated value is one fp32 add on the plain one"
