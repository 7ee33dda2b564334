"""What the row BatchNorm family (csrc/rpb_rowbn.hip) promises beyond the per-model kernel tests (tests/test_gpu_cno_train_kernels.py,
tests/test_gpu_deeponet_train_kernels.py): the summation order of ``ops.rowbn_sum64``, that the two run lengths of
``ops.rowbn_act_bwd_apply`` (8 channels per thread when Cpad % 8 == 0, else 4) give the same bits, and the refusals.

Operands live in the guard-banded arenas of tests/guarded.py.  The order is restated in fp64 on the CPU and must match bit for bit; the
verdict against the plain fp64 sum is tests/kernel_verdict.py (8 times the error of the fp32 restatement, floor 1e-6)."""
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
F64 = torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rows_in(a, block, ld, name):
    """block [M][C] as the first columns of an [M][ld] input operand whose other columns are NaN"""
    full = torch.full((block.shape[0], ld), float("nan"))
    full[:, :block.shape[1]] = block
    return a.inp(full, name)


# ----------------------------------------------------------------------------------------------------------- rowbn_sum64
def _restated_order(part):
    """eight partial sums over the rows g, g + 8, ... ascending, then added in index order; every addition one fp64 add"""
    groups = []
    for g in range(8):
        s = torch.zeros(part.shape[1], dtype=F64)
        for r in range(g, part.shape[0], 8):
            s = s + part[r]
        groups.append(s)
    t = torch.zeros(part.shape[1], dtype=F64)
    for s in groups:
        t = t + s
    return t


@pytest.mark.parametrize("C", [16, 256])
@pytest.mark.parametrize("rows", [13, 1024])
def test_sum64_order(rows, C):
    """Partials of mixed sign whose magnitudes span six decades: the order of the additions decides the low bits."""
    g = _g(rows + C)
    part = torch.randn(rows, 2 * C, generator=g, dtype=F64) * 10.0 ** (torch.rand(rows, 2 * C, generator=g, dtype=F64) * 6 - 3)
    a = guarded.Arena(DEV, dtype=F64)
    i_part, o_sums = a.inp(part, "part"), a.out(2 * C, name="sums")
    ops.rowbn_sum64(i_part.tensor(), rows, C, o_sums.tensor())
    a.check()
    sums, want = o_sums.get(), _restated_order(part)
    plain, seq = part.sum(0), part.cumsum(0)[-1]
    print(f"rows={rows} C={C}: {int((want != seq).sum())} of {2 * C} columns differ between the restated order and the row-by-row order")
    assert torch.equal(sums, want), f"{int((sums != want).sum())} of {2 * C} sums differ from the restated order"
    figures = [(kind, e32, ek) for kind, e32, ek in zip(("rel-l2", "max-abs"), measures(part.float().sum(0), plain), measures(sums, plain))]
    verdict(f"rows={rows} C={C}", "rowbn_sum64", figures)
    sums2 = torch.empty(2 * C, dtype=F64, device=DEV)
    ops.rowbn_sum64(part.to(DEV), rows, C, sums2)
    assert torch.equal(sums2.cpu(), sums), "a second call is bit-equal"


# ----------------------------------------------------------------------------------------------------------- apply: run length 4 against 8
M_A, C_A = 37, 32


def _apply(ld, has_bn, act):
    """one apply call with Cpad = ld on arenas -> (dy [M][ld], dgamma, dbeta)"""
    g = _g(5)
    y, gv = torch.randn(M_A, C_A, generator=g), torch.randn(M_A, C_A, generator=g) * 1e-3
    vec = dict(a=torch.rand(C_A, generator=g) * 0.5 + 0.75, b=torch.rand(C_A, generator=g) * 0.6 - 0.3,
               mean=torch.randn(C_A, generator=g) * 0.1, rstd=torch.rand(C_A, generator=g) * 0.5 + 0.75)
    sums = torch.randn(2 * C_A, generator=g, dtype=F64) * 1e-2
    a32, a64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    o_gv, o_y = _rows_in(a32, gv, ld, "gv"), _rows_in(a32, y, ld, "y")
    o_dy = a32.out(M_A, ld, name="dy")
    kw = {}
    if has_bn:
        o_vec = {k: a32.inp(v, k) for k, v in vec.items()}
        o_dg, o_db = a32.out(C_A, name="dgamma"), a32.out(C_A, name="dbeta")
        kw = dict({k: o.op for k, o in o_vec.items()}, sums=a64.inp(sums, "sums").tensor(), dgamma=o_dg.op, dbeta=o_db.op)
    ops.rowbn_act_bwd_apply(o_gv.op, ld, M_A, C_A, ld, act, y=o_y.op, ldy=ld, dy=o_dy.op, ldd=ld, **kw)
    a32.check()
    if not has_bn:
        return o_dy.get(), None, None
    a64.check()
    return o_dy.get(), o_dg.get(), o_db.get()


@pytest.mark.parametrize("has_bn,act", [(1, 0), (1, 1), (0, 1)])
def test_apply_run_lengths_agree(has_bn, act):
    """M = 37, C = 32: Cpad = ld = 64 walks runs of 8 channels, Cpad = ld = 68 runs of 4; the expression per element is the same."""
    dy8, dg8, db8 = _apply(64, has_bn, act)
    dy4, dg4, db4 = _apply(68, has_bn, act)
    assert bool(dy8[:, :C_A].any())
    assert torch.equal(dy4[:, :64], dy8), f"{int((dy4[:, :64] != dy8).sum())} elements of dy differ between the run lengths"
    assert not bool(dy8[:, C_A:].any()) and not bool(dy4[:, C_A:].any()), "pad columns (64..67 included) are exactly zero"
    if has_bn:
        assert torch.equal(dg4, dg8) and torch.equal(db4, db8)


# ----------------------------------------------------------------------------------------------------------- refusals
def _untouched(arena, *shape, name):
    return arena.out(*shape, name=name, unwritten=torch.ones(*shape, dtype=torch.bool))


def test_refusals_leave_the_outputs_untouched():
    """Each returns RPB_ERR_ARG (-1) before any launch: every output operand still holds the arena's sentinel."""
    M, rows = 8, ops.rowbn_rows()
    z = torch.zeros(M, 256, device=DEV)
    v = torch.zeros(4, 256, device=DEV)
    s = torch.zeros(512, dtype=F64, device=DEV)
    # plane output at Cpad % 8 == 4
    a = guarded.Arena(DEV)
    o_dy, o_dp = _untouched(a, M, 68, name="dy"), _untouched(a, 3, M, 34, name="dy_planes")
    assert ops._p(o_dp.op) % 16 == 0, "the plane operand is aligned and ldp = 72 is a multiple of 8: only Cpad = 68 is left to refuse"
    with pytest.raises(RpbError, match=r"rpb_rowbn_act_bwd_apply failed \(-1\).*plane output.*Cpad=68 ldp=72"):
        ops.rowbn_act_bwd_apply(z, 256, M, 32, 68, 1, y=z, ldy=256, dy=o_dy.op, ldd=68, dy_planes=o_dp.op, ldp=72)
    a.check()
    # C = 256 for the statistics (the sum and the apply take it, the statistics kernels do not)
    a = guarded.Arena(DEV, dtype=F64)
    o_part = _untouched(a, rows, 512, name="part")
    with pytest.raises(RpbError, match=r"rpb_rowbn_stats failed \(-1\)"):
        ops.rowbn_stats(z, 256, M, 256, o_part.tensor())
    with pytest.raises(RpbError, match=r"rpb_rowbn_act_bwd_stats failed \(-1\)"):
        ops.rowbn_act_bwd_stats(z, 256, z, 256, *v, M, 256, 0, o_part.tensor())
    a.check()
    # C = 24
    a32, a64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    o_dy, o_part, o_sums = _untouched(a32, M, 64, name="dy"), _untouched(a64, rows, 48, name="part"), _untouched(a64, 48, name="sums")
    with pytest.raises(RpbError, match=r"rpb_rowbn_stats failed \(-1\)"):
        ops.rowbn_stats(z, 256, M, 24, o_part.tensor())
    with pytest.raises(RpbError, match=r"rpb_rowbn_sum64 failed \(-1\)"):
        ops.rowbn_sum64(s, 4, 24, o_sums.tensor())
    with pytest.raises(RpbError, match=r"rpb_rowbn_act_bwd_apply failed \(-1\)"):
        ops.rowbn_act_bwd_apply(z, 256, M, 24, 64, 0, y=z, ldy=256, a=v[0], b=v[1], mean=v[2], rstd=v[3], sums=s, dy=o_dy.op, ldd=64)
    a32.check()
    a64.check()
