"""The twelve MWT3d kernels (csrc/rpb_mwt.hip, csrc/rpb_mwt3x.hip) one launch at a time through ``_lib.call("rpb_mwt_*", ...)`` against
tests/mwt_restatement.py, every call on guard-banded operands (tests/guarded.py): a stray write, an element never written and a stray
read that reaches a result are assertions of ``Arena.check()``, not GPU faults.  The shapes and inputs live in
tests/mwt_kernel_cases.py, shared with tests/test_mwt_kernels_host.py, which proves without a GPU that every case is well conditioned,
that the shapes reach the paths named below and that a wrong formula would fail here.

What the shapes are for: the convolutions (fp32 MFMA, "bf16x3", "f16x2"; plain and accumulating) on 8 to 320 cells, where a 16-cell
MFMA column tile is partly valid inside a live wave, T is odd, 1 or 2, sample borders fall inside a column tile, neither Nx nor Ny is a
power of two, a full block is followed by a block with one live wave of 8 cells or by one full wave next to dead ones -- at two of them
also the zero input and the input scales 2^-20 and 2^12 of the fp16 exponent path; lift with T, H and W distinct and Cin from 1 to 64;
decompose and reconstruct at odd T and non-power-of-two grids, with the broadcast x of the W = 2H configs; coarse at the three K the
configs use; every launch of the spectral kernel on its own (five axis stages, the per-bin contraction through the real corner table
with a NaN weight block behind it, spec_out plain and accumulating) at four levels, (1, 1) to (8, 16); spec_out below, at and above
the 7 cells of a block; the head below, at and above its 8-cell group and once with 129 cells per compute unit, so that some blocks
take a second grid-stride trip; the weight preparations with every output element, pad rows and pad groups included, required
written; and the refusals the C ABI documents, with nothing written.

Bounds: each output against the fp64 restatement on Rel-L2 and on max |error| / max |reference|, bounded by max(8 * e32, 1e-6) (2e-6
in place of 1e-6 for "f16x2"), e32 being the same measure of the fp32 CPU restatement; a case with 8 * e32 > 1e-5 is rejected as badly
conditioned; the kernel's output never enters a bound.  ``EXISTING`` would name a kernel whose MI355X result needs more and hold it to
the bound tests/test_gpu_mwt.py / tests/test_gpu_mwt_arith.py already assert for it.  The measured figures:
profiles/mwt_kernels_pytest.txt."""
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                              # noqa: E402
import mwt_kernel_cases as K                # noqa: E402

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
DEV = "cuda"
C = K.C
ARITHS = ["f32", "bf16x3", "f16x2"]
KERNEL = {"f32": "rpb_mwt_conv3", "bf16x3": "rpb_mwt_conv3x[bf16x3]", "f16x2": "rpb_mwt_conv3x[f16x2]"}

# kernel -> the bound an existing test asserts for it (K.EXISTING_BOUND: 1e-5 for f32 and bf16x3, 2e-6 for f16x2), used INSTEAD of
# max(8 * e32, floor), with the measured figure beside it.
# Empty: on the MI355X no kernel of the family needs it (profiles/mwt_kernels_pytest.txt)
EXISTING = {}


@pytest.fixture(scope="module")
def ops():
    from realpdebench_amd import _lib, ops as o
    _lib.load()
    return o


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)                        # one case, one pair of references, however many tests look at it


def check(name, got, ref64, ref32, kernel, floor=1e-6):
    K.judge(f"{kernel} {name}", got, ref64, ref32, EXISTING.get(kernel), floor)


def launch(ops, name, *args):
    """one kernel through the C ABI; operands are handed over as ``Operand`` (``ops._p(operand.op)``), None stays a null pointer"""
    from realpdebench_amd import _lib

    def arg(a):
        if isinstance(a, guarded.Operand):
            return ops._p(a.op, a.arena.dtype)
        return a
    _lib.call(name, *map(arg, args), ops._stream())


def untouched(*shape):
    return torch.ones(shape, dtype=torch.bool)


def exponent(ops, t, M, Cc):
    """rpb_amax_exp of ``t`` [M][Cc], outside the arena (tests/test_gpu_conv3h.py covers that kernel) -> a host integer"""
    e = torch.empty(1, device=DEV, dtype=I32)
    ops.amax_exp(t.to(DEV).contiguous(), e, M, Cc)
    return int(e.cpu())


def exponents(*values):
    """ea / ew in an int32 arena whose fill (1000) would turn a stray read into a non-finite result"""
    ia = guarded.Arena(DEV, I32, fill=1000)
    return ia, [ia.inp(torch.tensor([v], dtype=I32)) for v in values]


# ================================================================================================ weight preparation
@pytest.fixture(scope="module")
def packs(ops):
    """per weight set (kernel B, kernel C of CZ block 0): the host layouts of the fp32 kernel, and what the two preparation kernels
    wrote on guarded outputs -- every element of an output must have been written, pad rows and pad groups included"""
    out = {}
    for which in ("B", "C"):
        cw, cb, lw, lb = K.conv_weights(which)
        wp, lop = K.conv3_layouts(cw, lw)
        p = dict(wp=wp, lop=lop, cb48=K.cb48(cb), lb=lb, ew=exponent(ops, cw.reshape(C, 972), C, 972))
        a = guarded.Arena(DEV)
        w, lo, kwp, klop = a.inp(cw), a.inp(lw), a.out(27 * 9 * 3 * 64), a.out(3 * 4 * 3 * 64)
        launch(ops, "rpb_mwt_conv3_wprep", w, lo, kwp, klop)
        a.check()
        p["kernel_wp"], p["kernel_lop"] = kwp.get(), klop.get()
        for arith, planes in K.PLANES.items():
            a = guarded.Arena(DEV)
            # the planes are 16-bit patterns; the arena holds them as the fp32 words they occupy (finite operands never give a NaN word)
            w, wpx = a.inp(cw), a.out(31 * 3 * planes * 64 * 4)
            ia, (ew,) = exponents(p["ew"])
            launch(ops, "rpb_mwt_conv3x_wprep", w, wpx, planes, ew if planes == 2 else None)
            a.check()
            ia.check()
            p[arith] = wpx.get()
        out[which] = p
    return out


@pytest.mark.parametrize("which", ["B", "C"])
def test_conv3_wprep_is_the_documented_gather(packs, which):
    p = packs[which]
    assert torch.equal(p["kernel_wp"], p["wp"]) and torch.equal(p["kernel_lop"], p["lop"])


def run_conv(ops, p, arith, shape, v, base):
    B, Nx, Ny, T = shape
    a = guarded.Arena(DEV)
    # x and out are addressed by cell: a kernel off by a whole wave of cells must still land in the guard (K.CELL_GUARD)
    x = a.inp(v, guard=K.CELL_GUARD)
    w, cb, lop, lb = a.inp(p["wp"] if arith == "f32" else p[arith]), a.inp(p["cb48"]), a.inp(p["lop"]), a.inp(p["lb"])
    out = a.out(B, Nx, Ny, T, C, guard=K.CELL_GUARD) if base is None else a.inout(base, guard=K.CELL_GUARD)
    if arith == "f32":
        launch(ops, "rpb_mwt_conv3", x, w, cb, lop, lb, out, B, Nx, Ny, T, int(base is not None))
    else:
        planes = K.PLANES[arith]
        ia, (ea, ew) = exponents(exponent(ops, v.reshape(-1, C), v.numel() // C, C), p["ew"])
        launch(ops, "rpb_mwt_conv3x", x, w, cb, lop, lb, out, B, Nx, Ny, T, int(base is not None), planes, *((ea, ew) if planes == 2 else (None, None)))
        ia.check()
    a.check()
    return out.get()


@pytest.mark.parametrize("arith", ARITHS)
@pytest.mark.parametrize("shape", K.CONV_SHAPES, ids=K.CONV_IDS)
def test_conv3(ops, packs, arith, shape):
    c = case_of(K.conv_case, shape)
    r64, r32 = c.refs()
    runs = [("plain", c.v, None), ("acc", c.v, c.base)]
    if arith != "f32" and shape in K.CONV_SCALED:                 # the exponent path meets the masked lanes
        runs += [("zero", torch.zeros_like(c.v), None)] + [(tag, c.v * s, None) for tag, s in K.SCALES]
    for key, v, base in runs:
        got = run_conv(ops, packs["B"], arith, shape, v, base)
        if key == "plain":
            assert torch.equal(got, run_conv(ops, packs["B"], arith, shape, v, base)), "two calls must give bit-equal outputs"
        check(f"{c.name} {key}", got, r64[key], r32[key], KERNEL[arith], K.FLOOR[arith])


@pytest.mark.parametrize("arith", ["bf16x3", "f16x2"])
def test_conv3x_wprep_planes_through_the_convolution(ops, packs, arith):
    """the content of the 16-bit planes of a second weight set (kernel C), judged through the convolution that consumes them"""
    shape = (3, 2, 4, 11)
    c = case_of(K.conv_case, shape + ("C",))
    r64, r32 = c.refs()
    check(f"{c.name} plain", run_conv(ops, packs["C"], arith, shape, c.v, None), r64["plain"], r32["plain"], KERNEL[arith], K.FLOOR[arith])


# ================================================================================================ lift
@pytest.mark.parametrize("shape", K.LIFT_SHAPES, ids=str)
def test_lift(ops, shape):
    B, T, H, W, Cin = shape
    c = case_of(K.lift_case, shape)
    r64, r32 = c.refs()
    a = guarded.Arena(DEV)
    x, w, b, out = a.inp(c.x), a.inp(c.w), a.inp(c.b), a.out(B, H, W, T, C, guard=K.CELL_GUARD)
    launch(ops, "rpb_mwt_lift", x, w, b, out, B, T, H, W, Cin)
    a.check()
    check(c.name, out.get(), r64["out"], r32["out"], "rpb_mwt_lift")


# ================================================================================================ decompose / reconstruct
@pytest.mark.parametrize("shape", K.DR_SHAPES, ids=str)
def test_decompose_and_reconstruct(ops, shape):
    B, Nx, Ny, T = shape
    c = case_of(K.dr_case, shape)
    r64, r32 = c.refs()
    a = guarded.Arena(DEV)
    # h is addressed on the fine grid: two fine rows of guard if that is more than a wave of cells (K.fine_guard)
    h, ecd, ecs = a.inp(c.h, guard=K.fine_guard(Ny, T)), a.inp(c.ec_d), a.inp(c.ec_s)
    d, s = a.out(B, Nx, Ny, T, C, guard=K.CELL_GUARD), a.out(B, Nx, Ny, T, C, guard=K.CELL_GUARD)
    launch(ops, "rpb_mwt_decompose", h, ecd, ecs, d, s, B, Nx, Ny, T)
    a.check()
    check(c.name + " d", d.get(), r64["d"], r32["d"], "rpb_mwt_decompose")
    check(c.name + " s", s.get(), r64["s"], r32["s"], "rpb_mwt_decompose")
    for key in ("x", "xb"):
        if key not in c.inp:
            continue
        for relu in (0, 1):
            a = guarded.Arena(DEV)
            x, us, ud = (a.inp(t, guard=K.CELL_GUARD) for t in (c.inp[key], c.us, c.ud))
            rc = a.inp(c.rc)
            out = a.out(B, 2 * Nx, 2 * Ny, T, C, guard=K.fine_guard(Ny, T))
            launch(ops, "rpb_mwt_reconstruct", x, us, ud, rc, out, B, Nx, Ny, T, c.inp[key].shape[2], relu)
            a.check()
            k = f"rec_{key}_relu{relu}"
            check(f"{c.name} xNy={c.inp[key].shape[2]} relu={relu}", out.get(), r64[k], r32[k], "rpb_mwt_reconstruct")


# ================================================================================================ coarse
@pytest.mark.parametrize("Kk,rows", K.COARSE_CASES)
def test_coarse(ops, Kk, rows):
    c = case_of(K.coarse_case, (Kk, rows))
    r64, r32 = c.refs()
    a = guarded.Arena(DEV)
    x, w, b, out = a.inp(c.x), a.inp(c.w), a.inp(c.b), a.out(rows, C)
    launch(ops, "rpb_mwt_coarse", x, w, b, out, rows, Kk)
    a.check()
    check(c.name, out.get(), r64["out"], r32["out"], "rpb_mwt_coarse")


# ================================================================================================ the spectral kernel, launch by launch
def run_axis(ops, inp, M, outer, inner):
    O, Kk = M.shape
    a = guarded.Arena(DEV)
    x, m, out = a.inp(inp, ld=inner), a.inp(M), a.out(outer * O * inner, ld=inner)        # two rows of ``inner`` of guard at least
    launch(ops, "rpb_mwt_axis", x, m, out, outer, O, Kk, inner)
    a.check()
    return out.get()


@pytest.mark.parametrize("shape", K.AXIS_CASES, ids=str)
def test_axis(ops, shape):
    outer, O, Kk, inner = shape
    c = case_of(K.axis_case, shape)
    r64, r32 = c.refs()
    check(c.name, run_axis(ops, c.x, c.M, outer, inner), r64["out"], r32["out"], "rpb_mwt_axis")


def run_spec_out(ops, S, GT, lines, T, K2, base):
    _, loT, lb = K.spectral_weights()
    a = guarded.Arena(DEV)
    s, gt, lo, b = a.inp(S, ld=K2 * C), a.inp(GT), a.inp(loT), a.inp(lb)
    out = a.out(lines * T, C, guard=K.CELL_GUARD) if base is None else a.inout(base, guard=K.CELL_GUARD)
    launch(ops, "rpb_mwt_spec_out", s, gt, lo, b, out, lines, T, K2, int(base is not None))
    a.check()
    return out.get().reshape(lines * T, C)


@pytest.mark.parametrize("level", K.LEVELS, ids=str)
def test_spectral_launches(ops, level):
    Nx, Ny, T = level
    c = case_of(K.level_case, level)
    r64, r32 = c.refs()
    plan, B = c.plan, c.B
    for name, (_, outer, inner) in c.calls.items():               # the five axis stages, each judged on its own
        got = run_axis(ops, c.ins[name], getattr(plan, name), outer, inner)
        check(f"{c.name} stage {name} outer={outer} inner={inner}", got, r64[name], r32[name], "rpb_mwt_axis")
    # the per-bin contraction: a stray ``tab`` entry reads the arena's fill, which selects the NaN block behind the 500 real ones
    Wt = torch.cat([K.spectral_weights()[0], torch.full((1, C, C, 2), float("nan"))])
    a = guarded.Arena(DEV)
    X, W, Y = a.inp(c.ins["modes"], ld=C), a.inp(Wt, ld=C * C * 2), a.out(B * 2 * c.NB * C, ld=C)
    ia = guarded.Arena(DEV, I32, fill=K.NAN_BLOCK)
    tab = ia.inp(plan.tab)
    launch(ops, "rpb_mwt_modes", X, W, tab, Y, B, c.NB)
    a.check()
    ia.check()
    check(f"{c.name} modes NB={c.NB}", Y.get(), r64["modes"], r32["modes"], "rpb_mwt_modes")
    lines = B * Nx * Ny
    for key, base in (("spec_out", None), ("spec_out_acc", c.base.reshape(-1, C))):
        got = run_spec_out(ops, c.ins["spec_out"], plan.GT, lines, T, 2 * K.MODES, base)
        check(f"{c.name} {key}", got, r64[key], r32[key], "rpb_mwt_spec_out")


@pytest.mark.parametrize("lines,T", K.SPEC_OUT_CASES)
def test_spec_out(ops, lines, T):
    c = case_of(K.spec_out_case, (lines, T))
    r64, r32 = c.refs()
    for key, base in (("out", None), ("acc", c.base)):
        check(f"{c.name} {key}", run_spec_out(ops, c.S, c.GT, lines, T, c.K2, base), r64[key], r32[key], "rpb_mwt_spec_out")


# ================================================================================================ head
def run_head(ops, c, mesh, Cout, r):
    B, Nx, Ny, T = mesh
    a = guarded.Arena(DEV)
    x = a.inp(c.v, guard=K.CELL_GUARD)
    w0t, b0, w1, b1 = a.inp(c.w0t), a.inp(c.b0), a.inp(c.w1), a.inp(c.b1)
    out = a.out(B, T * r, Nx, Ny, Cout, ld=Nx * Ny * Cout)        # two output time planes of guard at least
    launch(ops, "rpb_mwt_head", x, w0t, b0, w1, b1, out, B, Nx, Ny, T, Cout, r)
    a.check()
    return out.get()


@pytest.mark.parametrize("Cout,r", K.HEAD_DOUT)
@pytest.mark.parametrize("mesh", K.HEAD_MESHES, ids=str)
def test_head(ops, mesh, Cout, r):
    c = case_of(K.head_case, (*mesh, Cout, r))
    r64, r32 = c.refs()
    check(c.name, run_head(ops, c, mesh, Cout, r), r64["out"], r32["out"], "rpb_mwt_head")


def test_head_grid_stride(ops, cus):
    mesh = K.head_stride_mesh(cus)
    ncell = mesh[0] * mesh[1] * mesh[2] * mesh[3]
    trips = K.head_trips(ncell, cus)
    assert len(trips) == 16 * cus and set(trips) == {1, 2}        # some blocks take a second trip, the rest do not
    Cout, r = K.HEAD_STRIDE_DOUT
    c = case_of(K.head_case, (*mesh, Cout, r))
    r64, r32 = c.refs()
    check(f"{c.name} CUs={cus} blocks with two trips={trips.count(2)}", run_head(ops, c, mesh, Cout, r), r64["out"], r32["out"], "rpb_mwt_head")


# ================================================================================================ refusals
def test_documented_refusals_write_nothing(ops, packs):
    from realpdebench_amd._lib import RpbError
    p = packs["B"]

    def refused(name, arena, *args, others=()):
        with pytest.raises(RpbError):
            launch(ops, name, *args)
        arena.check()
        for o in others:
            o.check()

    shape = B, Nx, Ny, T = (3, 2, 4, 11)
    c = case_of(K.conv_case, shape)
    for arith in ARITHS:                                          # x == out
        a = guarded.Arena(DEV)
        w, cb, lop, lb = a.inp(p["wp"] if arith == "f32" else p[arith]), a.inp(p["cb48"]), a.inp(p["lop"]), a.inp(p["lb"])
        out = a.out(B, Nx, Ny, T, C, guard=K.CELL_GUARD, unwritten=untouched(B, Nx, Ny, T, C))
        ia, (ea, ew) = exponents(0, p["ew"])
        if arith == "f32":
            refused("rpb_mwt_conv3", a, out, w, cb, lop, lb, out, B, Nx, Ny, T, 0)
        else:
            refused("rpb_mwt_conv3x", a, out, w, cb, lop, lb, out, B, Nx, Ny, T, 0, K.PLANES[arith], ea, ew, others=(ia,))
    for planes, e in ((4, True), (1, True), (2, False)):          # planes outside {2, 3}; planes = 2 without its exponents
        a = guarded.Arena(DEV)
        x, w, cb, lop, lb = a.inp(c.v, guard=K.CELL_GUARD), a.inp(p["bf16x3"]), a.inp(p["cb48"]), a.inp(p["lop"]), a.inp(p["lb"])
        out = a.out(B, Nx, Ny, T, C, guard=K.CELL_GUARD, unwritten=untouched(B, Nx, Ny, T, C))
        ia, (ea, ew) = exponents(0, p["ew"])
        refused("rpb_mwt_conv3x", a, x, w, cb, lop, lb, out, B, Nx, Ny, T, 0, planes, ea if e else None, ew if e else None, others=(ia,))
        a = guarded.Arena(DEV)
        n = 31 * 3 * 3 * 64 * 4
        cw, wpx = a.inp(K.conv_weights("B")[0]), a.out(n, unwritten=untouched(n))
        refused("rpb_mwt_conv3x_wprep", a, cw, wpx, planes, ew if e else None, others=(ia,))
    # reconstruct: x spans neither Ny columns nor one
    c = case_of(K.dr_case, (2, 2, 4, 11))
    B, Nx, Ny, T = 2, 2, 4, 11
    a = guarded.Arena(DEV)
    x, us, ud, rc = a.inp(c.x, guard=K.CELL_GUARD), a.inp(c.us, guard=K.CELL_GUARD), a.inp(c.ud, guard=K.CELL_GUARD), a.inp(c.rc)
    out = a.out(B, 2 * Nx, 2 * Ny, T, C, guard=K.fine_guard(Ny, T), unwritten=untouched(B, 2 * Nx, 2 * Ny, T, C))
    refused("rpb_mwt_reconstruct", a, x, us, ud, rc, out, B, Nx, Ny, T, 2, 0)
    # coarse: K is no multiple of 36
    a = guarded.Arena(DEV)
    Kk, rows = K.COARSE_REFUSED_K, 9
    x, w, b, out = a.inp(torch.ones(rows, Kk)), a.inp(torch.ones(C, Kk)), a.inp(torch.ones(C)), a.out(rows, C, unwritten=untouched(rows, C))
    refused("rpb_mwt_coarse", a, x, w, b, out, rows, Kk)
    # lift: more input channels than the kernel is built for
    a = guarded.Arena(DEV)
    Cin = K.LIFT_REFUSED_CIN
    x, w, b = a.inp(torch.ones(1, 2, 2, 2, Cin)), a.inp(torch.ones(C, Cin)), a.inp(torch.ones(C))
    out = a.out(1, 2, 2, 2, C, guard=K.CELL_GUARD, unwritten=untouched(1, 2, 2, 2, C))
    refused("rpb_mwt_lift", a, x, w, b, out, 1, 2, 2, 2, Cin)


def test_existing_table():
    """printed last, for profiles/mwt_kernels_pytest.txt; an entry may only name a bound another test already asserts"""
    print(f"[mwt-kernels] EXISTING = {EXISTING!r}")
    known = set(KERNEL.values()) | {"rpb_mwt_" + n for n in ("lift", "decompose", "reconstruct", "coarse", "axis", "modes", "spec_out", "head")}
    for kernel, bound in EXISTING.items():
        assert kernel in known and bound == (K.EXISTING_BOUND["f16x2"] if "f16x2" in kernel else K.EXISTING_BOUND["f32"])
