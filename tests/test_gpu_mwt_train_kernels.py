"""The entry points of the MWT3d training step (csrc/rpb_mwt_train.hip) one launch at a time through ``_lib.call("rpb_mwt_*", ...)``
against fp64 torch autograd of the matching function of tests/mwt_restatement.py, every call on guard-banded operands
(tests/guarded.py): a stray write, an element never written and a stray read that reaches a result are assertions of ``Arena.check()``,
not GPU faults.  Shapes and inputs: tests/mwt_train_cases.py -- (2, 8, 16, 8), (3, 4, 8, 10), (3, 1, 2, 8) and the ragged (1, 3, 5, 9) (135
cells: a partly valid 16-cell column tile, sample borders inside a tile); both accumulate settings; an all-zero g_out, whose results
must be exact zeros.  The gates of lo_bwd come from the supplied z.

Bound: max(8 * e32, 1e-6) on Rel-L2 and on max |error| / max |reference|, e32 the same measure of the fp32 CPU restatement (the rule of
tests/test_gpu_mwt_kernels.py); per-workgroup partials are summed on the host in fp64 (rpb_reduce_partials has its own tests).  The
keep-variants: ``out`` bit-equal to rpb_mwt_conv3 / rpb_mwt_spec_out, the kept tensor within the same bound."""
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                              # noqa: E402
import mwt_kernel_cases as K                # noqa: E402
import mwt_train_cases as TK                # noqa: E402

pytestmark = pytest.mark.gpu

DEV, C, I32 = "cuda", K.C, torch.int32


@pytest.fixture(scope="module")
def ops():
    from realpdebench_amd import _lib, ops as o
    _lib.load()
    return o


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)


def launch(ops, name, *args):
    from realpdebench_amd import _lib

    def arg(a):
        return ops._p(a.op, a.arena.dtype) if isinstance(a, guarded.Operand) else a
    _lib.call(name, *map(arg, args), ops._stream())


def query(name, *args):
    from realpdebench_amd import _lib
    return _lib.query(name, *args)


def check(name, got, r64, r32, kernel):
    K.judge(f"{kernel} {name}", got.reshape(r64.shape), r64, r32, None, 1e-6)


def rows_sum(part):
    return part.get().double().sum(0).float()


# ================================================================================================ lo_bwd
def run_lo(ops, g, z, lo):
    ncell = z.numel() // C
    rows = query("rpb_mwt_lo_bwd_rows", ncell)
    a = guarded.Arena(DEV)
    go, zo, lw = a.inp(g, guard=K.CELL_GUARD), a.inp(z, guard=K.CELL_GUARD), a.inp(lo)
    gz, part = a.out(*z.shape, guard=K.CELL_GUARD), a.out(rows, C * C + C)
    launch(ops, "rpb_mwt_lo_bwd", go, zo, lw, gz, part, ncell)
    a.check()
    return gz.get(), rows_sum(part)


@pytest.mark.parametrize("shape", TK.SHAPES, ids=str)
def test_lo_bwd(ops, shape):
    c = case_of(TK.lo_case, shape)
    r64, r32 = c.refs()
    gz, tot = run_lo(ops, c.g, c.z, c.lo)
    gz2, tot2 = run_lo(ops, c.g, c.z, c.lo)
    assert torch.equal(gz, gz2) and torch.equal(tot, tot2), "two calls must give bit-equal results"
    assert not bool(gz[c.z == 0].any()), "closed gates pass nothing"
    check(c.name + " gz", gz, r64["gz"], r32["gz"], "rpb_mwt_lo_bwd")
    check(c.name + " dLo|dlb", tot, r64["part"], r32["part"], "rpb_mwt_lo_bwd")
    if shape == TK.ZERO_SHAPE:
        gz, tot = run_lo(ops, torch.zeros_like(c.g), c.z, c.lo)
        assert not bool(gz.any()) and not bool(tot.any())


# ================================================================================================ conv3: data and weight gradient
@pytest.fixture(scope="module")
def wpd(ops):
    """the lane-ordered A operand of the data gradient: rpb_mwt_conv3_wprep on the flipped, transposed taps (as MWT3d.k_conv3_dgrad_wprep)"""
    c = case_of(TK.conv_bwd_case, TK.SHAPES[0])
    a = guarded.Arena(DEV)
    w, lo, wp, lop = a.inp(c.wd), a.inp(K.conv_weights("B")[2]), a.out(27 * 9 * 3 * 64), a.out(3 * 4 * 3 * 64)
    launch(ops, "rpb_mwt_conv3_wprep", w, lo, wp, lop)
    a.check()
    return wp.get()


def run_dgrad(ops, wpd, g, base):
    B, Nx, Ny, T, _ = g.shape
    a = guarded.Arena(DEV)
    go, w = a.inp(g, guard=K.CELL_GUARD), a.inp(wpd)
    out = a.out(*g.shape, guard=K.CELL_GUARD) if base is None else a.inout(base, guard=K.CELL_GUARD)
    launch(ops, "rpb_mwt_conv3_dgrad", go, w, out, B, Nx, Ny, T, int(base is not None))
    a.check()
    return out.get()


@pytest.mark.parametrize("shape", TK.SHAPES, ids=str)
def test_conv3_dgrad(ops, wpd, shape):
    c = case_of(TK.conv_bwd_case, shape)
    r64, r32 = c.refs()
    got = run_dgrad(ops, wpd, c.g, None)
    assert torch.equal(got, run_dgrad(ops, wpd, c.g, None)), "two calls must give bit-equal outputs"
    check(c.name + " dgrad", got, r64["dgrad"], r32["dgrad"], "rpb_mwt_conv3_dgrad")
    check(c.name + " dgrad acc", run_dgrad(ops, wpd, c.g, c.base), r64["dgrad_acc"], r32["dgrad_acc"], "rpb_mwt_conv3_dgrad")
    if shape == TK.ZERO_SHAPE:
        assert not bool(run_dgrad(ops, wpd, torch.zeros_like(c.g), None).any())
        assert torch.equal(run_dgrad(ops, wpd, torch.zeros_like(c.g), c.base), c.base)


def run_wgrad(ops, g, x):
    B, Nx, Ny, T, _ = x.shape
    splits = query("rpb_mwt_conv3_wgrad_splits", B * Nx * Ny * T)
    a = guarded.Arena(DEV)
    go, xo, part = a.inp(g, guard=K.CELL_GUARD), a.inp(x, guard=K.CELL_GUARD), a.out(splits, TK.WG_L)
    launch(ops, "rpb_mwt_conv3_wgrad", go, xo, part, B, Nx, Ny, T)
    a.check()
    return rows_sum(part), splits


@pytest.mark.parametrize("shape", TK.SHAPES, ids=str)
def test_conv3_wgrad(ops, shape):
    c = case_of(TK.conv_bwd_case, shape)
    r64, r32 = c.refs()
    got, splits = run_wgrad(ops, c.g, c.x)
    print(f"{c.name}: {splits} split(s)")
    assert torch.equal(got, run_wgrad(ops, c.g, c.x)[0]), "two calls must give bit-equal partials"
    check(c.name + " dW|db", got, r64["wgrad"], r32["wgrad"], "rpb_mwt_conv3_wgrad")
    if shape == TK.ZERO_SHAPE:
        assert not bool(run_wgrad(ops, torch.zeros_like(c.g), c.x)[0].any())


def test_conv3_wgrad_takes_more_than_one_split():
    assert query("rpb_mwt_conv3_wgrad_splits", 2 * 8 * 16 * 8) > 1 and query("rpb_mwt_conv3_wgrad_splits", 135) == 1


# ================================================================================================ the keep-variants
def run_conv(ops, c, keep, base):
    B, Nx, Ny, T, _ = c.v.shape
    a = guarded.Arena(DEV)
    x, w, cb, lop, lb = a.inp(c.v, guard=K.CELL_GUARD), a.inp(c.wp), a.inp(c.cb48), a.inp(c.lop), a.inp(c.lb)
    out = a.out(*c.v.shape, guard=K.CELL_GUARD) if base is None else a.inout(base, guard=K.CELL_GUARD)
    z = a.out(*c.v.shape, guard=K.CELL_GUARD) if keep else None
    if keep:
        launch(ops, "rpb_mwt_conv3_keep", x, w, cb, lop, lb, out, z, B, Nx, Ny, T, int(base is not None))
    else:
        launch(ops, "rpb_mwt_conv3", x, w, cb, lop, lb, out, B, Nx, Ny, T, int(base is not None))
    a.check()
    return out.get(), (z.get() if keep else None)


@pytest.mark.parametrize("shape", TK.SHAPES, ids=str)
def test_conv3_keep(ops, shape):
    c = case_of(TK.keep_case, shape)
    r64, r32 = c.refs()
    for base in (None, c.base):
        out, z = run_conv(ops, c, True, base)
        assert torch.equal(out, run_conv(ops, c, False, base)[0]), "the keep-variant's output is bit-equal to rpb_mwt_conv3's"
        check(f"{c.name} z acc={int(base is not None)}", z, r64["z"], r32["z"], "rpb_mwt_conv3_keep")


def run_spec(ops, c, keep, base):
    n = c.lines * c.T
    a = guarded.Arena(DEV)
    S, GT, loT, lb = a.inp(c.S), a.inp(c.GT), a.inp(c.loT), a.inp(c.lb)
    out = a.out(n, C, guard=K.CELL_GUARD) if base is None else a.inout(base, guard=K.CELL_GUARD)
    rv = a.out(n, C, guard=K.CELL_GUARD) if keep else None
    if keep:
        launch(ops, "rpb_mwt_spec_out_keep", S, GT, loT, lb, out, rv, c.lines, c.T, c.K2, int(base is not None))
    else:
        launch(ops, "rpb_mwt_spec_out", S, GT, loT, lb, out, c.lines, c.T, c.K2, int(base is not None))
    a.check()
    return out.get(), (rv.get() if keep else None)


@pytest.mark.parametrize("shape", TK.SHAPES, ids=str)
def test_spec_out_keep(ops, shape):
    c = case_of(TK.spec_keep_case, shape)
    r64, r32 = c.refs()
    for base in (None, c.base):
        out, rv = run_spec(ops, c, True, base)
        assert torch.equal(out, run_spec(ops, c, False, base)[0]), "the keep-variant's output is bit-equal to rpb_mwt_spec_out's"
        check(f"{c.name} rv acc={int(base is not None)}", rv, r64["rv"], r32["rv"], "rpb_mwt_spec_out_keep")


# ================================================================================================ modes_bwd
def run_modes(ops, c, gY, B):
    a = guarded.Arena(DEV)
    X, g, Wt = a.inp(c.X), a.inp(gY), a.inp(c.Wt)
    gX, dWt = a.out(*c.X.shape), a.inout(c.base)
    ia = guarded.Arena(DEV, I32, fill=K.NAN_BLOCK)
    tab = ia.inp(c.plan.tab)
    launch(ops, "rpb_mwt_modes_bwd", X, g, Wt, tab, gX, dWt, B, c.NB)
    a.check()
    ia.check()
    return gX.get(), dWt.get()


@pytest.mark.parametrize("shape", TK.SHAPES, ids=str)
def test_modes_bwd(ops, shape):
    c = case_of(TK.modes_bwd_case, shape)
    r64, r32 = c.refs()
    gX, dWt = run_modes(ops, c, c.gY, shape[0])
    gX2, dWt2 = run_modes(ops, c, c.gY, shape[0])
    assert torch.equal(gX, gX2) and torch.equal(dWt, dWt2), "two calls must give bit-equal results"
    reached = torch.zeros(4 * K.MODES ** 3, dtype=torch.bool)
    reached[c.plan.tab.long()] = True
    assert torch.equal(dWt[~reached], c.base[~reached]), "weight bins no retained bin maps to keep what they held, bit for bit"
    check(c.name + " gX", gX, r64["gX"], r32["gX"], "rpb_mwt_modes_bwd")
    check(c.name + " dWt (accumulating)", dWt, r64["dWt"], r32["dWt"], "rpb_mwt_modes_bwd")
    if shape == TK.ZERO_SHAPE:
        gX, dWt = run_modes(ops, c, torch.zeros_like(c.gY), shape[0])
        assert not bool(gX.any()) and torch.equal(dWt, c.base)


# ================================================================================================ head_bwd
def run_head(ops, c, g):
    B, Nx, Ny, T, _ = c.v.shape
    dout = c.Cout * c.r
    rows = query("rpb_mwt_head_bwd_rows", B * Nx * Ny * T)
    a = guarded.Arena(DEV)
    x, go, w0t, b0, w1 = a.inp(c.v, guard=K.CELL_GUARD), a.inp(g, guard=K.CELL_GUARD), a.inp(c.w0t), a.inp(c.b0), a.inp(c.w1)
    gx, part = a.out(*c.v.shape, guard=K.CELL_GUARD), a.out(rows, dout * 128 + dout + 128 * C + 128)
    launch(ops, "rpb_mwt_head_bwd", x, go, w0t, b0, w1, gx, part, B, Nx, Ny, T, c.Cout, c.r)
    a.check()
    return gx.get(), rows_sum(part)


@pytest.mark.parametrize("shape", TK.SHAPES, ids=str)
def test_head_bwd(ops, shape):
    c = case_of(TK.head_bwd_case, shape)
    assert TK.head_margin(c) > TK.HEAD_MARGIN, "a hidden unit within fp32 reach of zero: the recomputed gate would be ambiguous"
    r64, r32 = c.refs()
    gx, tot = run_head(ops, c, c.g)
    gx2, tot2 = run_head(ops, c, c.g)
    assert torch.equal(gx, gx2) and torch.equal(tot, tot2), "two calls must give bit-equal results"
    check(c.name + " gx", gx, r64["gx"], r32["gx"], "rpb_mwt_head_bwd")
    check(c.name + " dLc1|db1|dLc0|db0", tot, r64["part"], r32["part"], "rpb_mwt_head_bwd")
    if shape == TK.ZERO_SHAPE:
        gx, tot = run_head(ops, c, torch.zeros_like(c.g))
        assert not bool(gx.any()) and not bool(tot.any())


def test_head_bwd_refuses_more_than_16_outputs(ops):
    from realpdebench_amd import _lib
    t = torch.zeros(4096, device=DEV)
    with pytest.raises(_lib.RpbError, match="at most 16"):
        _lib.call("rpb_mwt_head_bwd", *[ops._p(t)] * 7, 1, 1, 1, 1, 17, 1, ops._stream())


# ================================================================================================ lift_wgrad
@pytest.mark.parametrize("shape", TK.SHAPES, ids=str)
def test_lift_wgrad(ops, shape):
    B, Nx, Ny, T = shape
    c = case_of(TK.lift_wgrad_case, shape)
    r64, r32 = c.refs()
    rows = query("rpb_mwt_lift_wgrad_rows", B * Nx * Ny * T)

    def run(g):
        a = guarded.Arena(DEV)
        go, x, part = a.inp(g, guard=K.CELL_GUARD), a.inp(c.x, guard=K.CELL_GUARD), a.out(rows, C * c.Cin + C)
        launch(ops, "rpb_mwt_lift_wgrad", go, x, part, B, T, Nx, Ny, c.Cin)
        a.check()
        return rows_sum(part)
    got = run(c.g)
    assert torch.equal(got, run(c.g)), "two calls must give bit-equal partials"
    check(c.name + " dLk|db", got, r64["part"], r32["part"], "rpb_mwt_lift_wgrad")
    if shape == TK.ZERO_SHAPE:
        assert not bool(run(torch.zeros_like(c.g)).any())
