"""The Transolver kernel family (csrc/rpb_transolver.hip, and rpb_reduce_partials_batched) one kernel at a time against
tests/transolver_restatement.py, backward kernels included, every call on guard-banded operands (tests/guarded.py): a stray write, an
element never written and a stray read that reaches a result are assertions of ``Arena.check()``, not GPU faults.  The shapes and
inputs live in tests/transolver_kernel_cases.py, shared with tests/test_transolver_kernels_host.py, which proves without a GPU that the
restatements agree with autograd and the oracle, that every case is well conditioned and that a wrong formula would fail here.

What the shapes are for: one token; one short of and one past a 32-token tile; all eight head waves with G = 32 (no padded MFMA rows);
an odd head count with G = 12; two B = 16 cases in which every block of slice_fwd_kernel / slice_bwd_kernel walks two or three tiles
(accumulators carried across tiles, wave-private LDS tiles re-used, a ragged tile that is not a block's first) -- at B = 16 most blocks
of the small cases get no tile at all and must still write zero partial rows, which the never-written check sees; every LayerNorm width
the library instantiates, idle waves, and a backward in which every wave accumulates two or three rows; tokens_lift up to K = 32, the
first admitted shape past 64 KiB of dynamic LDS.

Bounds: each output against the fp64 restatement on Rel-L2 and on max |error| / max |reference|, bounded by max(8 * e32, 1e-6), e32
being the same measure of the fp32 CPU restatement; a case with 8 * e32 > 1e-5 is rejected as badly conditioned; the kernel's output
never enters a bound.  The temperature gradient is judged per head on |dtau - dtau64| / sum |terms| (transolver_kernel_cases.py:
dtau_measure).  ``EXISTING`` would name, for a kernel whose hardware exponential needs more, the bound tests/test_gpu_transolver.py
already asserts for it."""
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                              # noqa: E402
import transolver_kernel_cases as K         # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DEV = "cuda"

# kernel -> the bound tests/test_gpu_transolver.py asserts for it (3e-6), used INSTEAD of max(8 * e32, 1e-6).
# Empty: on the MI355X no kernel of the family needs it (profiles/transolver_kernels_pytest.txt)
EXISTING = {}


@pytest.fixture(scope="module")
def ops():
    from realpdebench_amd import ops as o
    return o


@pytest.fixture(scope="module")
def cus(ops):
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert ops.slice_blocks_per_sample(16) == K.slice_bps(16, n) and ops.layernorm_bwd_rows(10 ** 9) == K.ln_bwd_rows(10 ** 9, n)
    return n


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)                        # one case, one pair of references, however many tests look at it


def check(name, got, ref64, ref32, kernel=None):
    K.judge(name, got, ref64, ref32, EXISTING.get(kernel))


def tile(ld):
    """the guard of a token-row operand of the slice kernels: a 32-token tile of rows is how far they can overreach"""
    return 32 * ld + 1024


def reduce_rows(ops, part_host, rows, L, row_stride=None, col0=0):
    """rpb_reduce_partials of a [rows][row_stride] partial buffer (guarded like every other call) -> host [L]"""
    a = guarded.Arena(DEV)
    p, o = a.inp(part_host), a.out(L)
    ops.reduce_partials(p.op, rows, L, out_f32=o.op, row_stride=row_stride, col0=col0)
    a.check()
    return o.get()


def reduce_batched(ops, part_host, nbatch, rows, L):
    """rpb_reduce_partials_batched of [nbatch][rows][L] -> host [nbatch][L], as model/transolver.py reduces the per-sample partials"""
    a = guarded.Arena(DEV)
    p, o = a.inp(part_host), a.out(nbatch, L)
    ops.reduce_partials_batched(p.op, nbatch, rows, L, o.op)
    a.check()
    return o.get()


def untouched(shape):
    return torch.ones(shape, dtype=torch.bool)


# ================================================================================================ slice family
def slice_shape(ops, cus, which):
    shapes = K.slice_shapes(ops.slice_blocks_per_sample(16))
    assert shapes == K.slice_shapes(K.slice_bps(16, cus))
    return shapes[which]


def idle_rows_are_zero(name, part_host, B, bps, ntok):
    """a block whose first tile lies past the sample's end (blk * 32 >= ntok) adds nothing: its partial row is exactly zero"""
    idle = part_host.view(B, bps, -1)[:, (ntok + 31) // 32:]
    assert not idle.any(), f"{name}: {int((idle != 0).sum())} non-zero element(s) in the partial rows of blocks without a tile"


@pytest.mark.parametrize("which", range(8), ids=K.SLICE_IDS)
def test_slice_fwd_and_deslice(ops, cus, which):
    B, ntok, heads, G = shape = slice_shape(ops, cus, which)
    c = case_of(K.slice_case, shape)
    r64, r32 = c.refs()
    C, M, bps = heads * 32, B * ntok, ops.slice_blocks_per_sample(B)
    if which >= 6:
        assert ntok > 32 * bps                                   # every block walks a second tile
    tag = f"{c.name} bps={bps}"
    # ---- weights, token sums and masses
    a = guarded.Arena(DEV)
    xf, Ws, bs, temp = a.inp(c.xf, guard=tile(2 * C)), a.inp(c.Ws), a.inp(c.bs), a.inp(c.temp)
    w, tp, npart = a.out(M, heads, G, ld=heads * G, guard=tile(heads * G)), a.out(B * bps, heads * G * 32), a.out(B * bps, heads * G)
    ops.slice_fwd(xf.op, Ws.op, bs.op, temp.op, w.op, tp.op, npart.op, B, ntok, heads, G, 2 * C)
    a.check()
    check(tag + " slice_fwd w", w.get(), r64["w"], r32["w"], kernel="slice_fwd")
    idle_rows_are_zero(tag + " slice_fwd tok_part", tp.get(), B, bps, ntok)
    idle_rows_are_zero(tag + " slice_fwd norm_part", npart.get(), B, bps, ntok)
    tokS = reduce_batched(ops, tp.get(), B, bps, heads * G * 32).view(B, heads, G, 32)
    check(tag + " slice_fwd tokS", tokS, r64["tokS"], r32["tokS"], kernel="slice_fwd")
    check(tag + " slice_fwd norm", reduce_batched(ops, npart.get(), B, bps, heads * G).view(B, heads, G), r64["norm"], r32["norm"],
          kernel="slice_fwd")
    # ---- given weights: the deslice backward with respect to the attended slice tokens (ldx = C, the optional pointers None)
    a = guarded.Arena(DEV)
    gox, win, tp = a.inp(c.gox, guard=tile(C)), a.inp(c.w, ld=heads * G, guard=tile(heads * G)), a.out(B * bps, heads * G * 32)
    ops.slice_fwd(gox.op, None, None, None, None, tp.op, None, B, ntok, heads, G, C, w_in=win.op)
    a.check()
    idle_rows_are_zero(tag + " slice_fwd(w_in) tok_part", tp.get(), B, bps, ntok)
    check(tag + " slice_fwd(w_in) gtok2", reduce_batched(ops, tp.get(), B, bps, heads * G * 32).view(B, heads, G, 32), r64["gtok2"],
          r32["gtok2"])
    # ---- deslice
    a = guarded.Arena(DEV)
    win, tok2 = a.inp(c.w, ld=heads * G, guard=tile(heads * G)), a.inp(c.tok2)
    if 256 % (heads * 8):                                        # 256 threads are not a whole number of C / 4 column groups: refused
        ox = a.out(M, C, guard=tile(C), unwritten=untouched((M, C)))
        from realpdebench_amd._lib import RpbError
        with pytest.raises(RpbError):
            ops.deslice_fwd(win.op, tok2.op, ox.op, B, ntok, heads, G)
        a.check()
        return
    ox = a.out(M, C, guard=tile(C))
    ops.deslice_fwd(win.op, tok2.op, ox.op, B, ntok, heads, G)
    a.check()
    check(tag + " deslice_fwd", ox.get(), r64["ox"], r32["ox"])


@pytest.mark.parametrize("which", range(8), ids=K.SLICE_IDS)
def test_slice_bwd(ops, cus, which):
    B, ntok, heads, G = shape = slice_shape(ops, cus, which)
    c = case_of(K.slice_case, shape)
    r64, r32 = c.refs()
    C, M, bps, L = heads * 32, B * ntok, ops.slice_blocks_per_sample(B), G * 32 + G + heads
    tag = f"{c.name} bps={bps}"
    a = guarded.Arena(DEV)
    xf, win, gox = a.inp(c.xf, guard=tile(2 * C)), a.inp(c.w, ld=heads * G, guard=tile(heads * G)), a.inp(c.gox, guard=tile(C))
    tok2, gT, gN, Ws, temp = a.inp(c.tok2), a.inp(c.gT), a.inp(c.gN), a.inp(c.Ws), a.inp(c.temp)
    gxf, part = a.out(M, 2 * C, guard=tile(2 * C)), a.out(B * bps, L)
    ops.slice_bwd(xf.op, win.op, gox.op, tok2.op, gT.op, gN.op, Ws.op, temp.op, gxf.op, part.op, B, ntok, heads, G)
    a.check()
    check(tag + " slice_bwd gxf", gxf.get(), r64["gxf"], r32["gxf"], kernel="slice_bwd")
    idle_rows_are_zero(tag + " slice_bwd part", part.get(), B, bps, ntok)
    tot = reduce_rows(ops, part.get(), B * bps, L)                # as _backward: one fp32 row [G*32 dWs | G dbs | heads dtau]
    check(tag + " slice_bwd dWs", tot[:G * 32].view(G, 32), r64["dWs"], r32["dWs"], kernel="slice_bwd")
    check(tag + " slice_bwd dbs", tot[G * 32:G * 32 + G], r64["dbs"], r32["dbs"], kernel="slice_bwd")
    K.judge_dtau(tag + " slice_bwd dtau", tot[G * 32 + G:], r64, r32, EXISTING.get("slice_bwd"))


# ================================================================================================ attention among the slice tokens
@pytest.mark.parametrize("BH,G", K.ATTN_SHAPES)
def test_slice_attn_eval_and_train(ops, BH, G):
    c = case_of(K.attn_case, (BH, G))
    r64, r32 = c.refs()

    def arena(mask, go):
        a = guarded.Arena(DEV)
        ins = [a.inp(c.inp[k]) for k in ("tokS", "norm", "Wq", "Wk", "Wv")]      # operands first, their .op once all are declared
        return a, ins, (a.inp(c.amask) if mask else None), (a.inp(c.go) if go else None)

    def p(o):
        return None if o is None else o.op                      # optional pointers are None, as model/transolver.py passes them

    a, ins, _, _ = arena(False, False)
    out = a.out(BH, G, 32)
    ops.slice_attn(*map(p, ins), out.op, BH, G)
    a.check()
    check(c.name + " slice_attn", out.get(), r64["out"], r32["out"], kernel="slice_attn")
    for mask in (False, True):                                   # the training kernel, forward only
        a, ins, am, _ = arena(mask, False)
        out = a.out(BH, G, 32)
        ops.slice_attn_train(*map(p, ins), p(am), BH, G, out=out.op)
        a.check()
        key = "out_m" if mask else "out"
        check(f"{c.name} slice_attn_train out mask={int(mask)}", out.get(), r64[key], r32[key], kernel="slice_attn_train")
    for mask, with_out in ((False, False), (True, True)):        # the backward alone (out = None: nothing else is written), then both
        a, ins, am, go = arena(mask, True)
        out = a.out(BH, G, 32) if with_out else None
        gT, gN, gW = a.out(BH, G, 32), a.out(BH, G), a.out(BH, 3, 1024)
        ops.slice_attn_train(*map(p, ins), p(am), BH, G, out=p(out), go=p(go), gT=gT.op, gN=gN.op, gW=gW.op)
        a.check()
        s, tag = ("_m" if mask else ""), f"{c.name} slice_attn_train mask={int(mask)} out={int(with_out)}"
        if with_out:
            check(tag + " out", out.get(), r64["out" + s], r32["out" + s], kernel="slice_attn_train")
        check(tag + " gT", gT.get(), r64["gT" + s], r32["gT" + s], kernel="slice_attn_train")
        check(tag + " gN", gN.get(), r64["gN" + s], r32["gN" + s], kernel="slice_attn_train")
        check(tag + " gW per (b,h)", gW.get(), r64["gW" + s], r32["gW" + s], kernel="slice_attn_train")
        check(tag + " dWq|dWk|dWv", reduce_rows(ops, gW.get(), BH, 3 * 1024), r64["dW" + s], r32["dW" + s], kernel="slice_attn_train")


# ================================================================================================ LayerNorm
def layernorm_bwd(ops, c, r64, r32, M, C, with_gadd):
    rows = ops.layernorm_bwd_rows(M)
    a = guarded.Arena(DEV)
    x, gam, gy = a.inp(c.x), a.inp(c.gamma), a.inp(c.gy)
    gadd = a.inp(c.gadd) if with_gadd else None
    gx, part = a.out(M, C), a.out(rows, 2 * C)
    ops.layernorm_bwd(x.op, gam.op, gy.op, gadd.op if with_gadd else None, gx.op, part.op, M, C, K.LN_EPS)
    a.check()
    key, tag = ("gx_add" if with_gadd else "gx"), f"{c.name} bwd gadd={int(with_gadd)} rows={rows}"
    check(tag + " gx", gx.get(), r64[key], r32[key])
    idle = part.get()[M:]
    assert not idle.any(), f"{tag}: {int((idle != 0).sum())} non-zero element(s) in the partial rows of waves without a row"
    check(tag + " dgamma|dbeta", reduce_rows(ops, part.get(), rows, 2 * C), r64["dgb"], r32["dgb"])      # as _ln_bwd
    return rows


@pytest.mark.parametrize("M,C", K.LN_SHAPES)
def test_layernorm_kernels(ops, M, C):
    c = case_of(K.ln_case, (M, C))
    r64, r32 = c.refs()
    a = guarded.Arena(DEV)
    x, gam, beta, y = a.inp(c.x), a.inp(c.gamma), a.inp(c.beta), a.out(M, C)
    ops.layernorm_fwd(x.op, gam.op, beta.op, y.op, M, C, K.LN_EPS)
    a.check()
    check(c.name + " fwd", y.get(), r64["y"], r32["y"])
    for with_gadd in (False, True):
        layernorm_bwd(ops, c, r64, r32, M, C, with_gadd)


def test_layernorm_bwd_waves_walk_rows(ops, cus):
    rows0 = ops.layernorm_bwd_rows(10 ** 9)
    M, C = K.ln_rows_shape(rows0)
    c = case_of(K.ln_case, (M, C))
    r64, r32 = c.refs()
    rows = layernorm_bwd(ops, c, r64, r32, M, C, True)
    assert rows == rows0 and M == 2 * rows + 37                   # every wave accumulates two rows, 37 of them three


# ================================================================================================ tokens_lift
@pytest.mark.parametrize("M,Kk,N,act", K.LIFT_CASES)
def test_tokens_lift(ops, M, Kk, N, act):
    c = case_of(K.lift_case, (M, Kk, N, act))
    r64, r32 = c.refs()
    a = guarded.Arena(DEV)
    x, W, b, out = a.inp(c.x), a.inp(c.W), a.inp(c.b), a.out(M, N)
    ops.tokens_lift(x.op, W.op, b.op, out.op, M, Kk, N, bool(act))
    a.check()
    check(f"{c.name} lds={(Kk + 1) * N * 4}", out.get(), r64["y"], r32["y"], kernel="tokens_lift")


def test_tokens_lift_refuses_more_lds_than_a_compute_unit_has(ops):
    from realpdebench_amd._lib import RpbError
    Kk, N = K.LIFT_REFUSED
    M = 8
    a = guarded.Arena(DEV)
    x, W, b = a.inp(torch.ones(M, Kk)), a.inp(torch.ones(N, Kk)), a.inp(torch.ones(N))
    out = a.out(M, N, unwritten=untouched((M, N)))
    with pytest.raises(RpbError, match="LDS"):
        ops.tokens_lift(x.op, W.op, b.op, out.op, M, Kk, N, True)
    a.check()
