"""The U-Net kernel family one kernel at a time against tests/unet_restatement.py, at the shapes of the configs (T = 20 and beyond, the
16 x 16 bottleneck, the init convolution's 3 / 5 / 16 input channels, 2 x 64-channel heads) and at the edges of each kernel's blocking,
every call on guard-banded operands (tests/guarded.py): a stray write, an element never written and a stray read that reaches a result
are assertions of ``Arena.check()``, not GPU faults.  The shapes and inputs live in tests/unet_kernel_cases.py, shared with
tests/test_unet_kernels_host.py, which proves without a GPU that the guards trip, that the restatements agree with torch's own operators
and oracle/unet_oracle.py, and that every case is well conditioned.

Bounds: the rule of tests/test_gpu_dpot_kernels.py.  Kernels that only move data (im2col, copy_cols, relpos forward, add -- one fp32
addition -- and the column maximum) must equal the fp32 restatement bit for bit.  The arithmetic kernels are compared with the fp64
restatement on two measures -- Rel-L2, and max |error| over max |reference| -- and bounded by max(8 * e32, 1e-6), e32 being the same
measure of the fp32 CPU restatement against its fp64 run; a case with 8 * e32 > 1e-5 is rejected as badly conditioned; the kernel's
output never enters a bound.  Where a kernel's hardware exponential needs more than that, ``EXISTING`` names the bound its test in
tests/test_gpu_unet.py already asserts, with the measured figures next to it."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                              # noqa: E402
import unet_kernel_cases as K               # noqa: E402

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
HID = K.HID
DEV = "cuda"

# kernel output -> the bound tests/test_gpu_unet.py asserts for that kernel, used INSTEAD of max(8 * e32, 1e-6) for it.
# Empty: on the MI355X the hardware-exponential kernels stay below 0.24 of the strict bound (profiles/unet_kernels_pytest.txt)
EXISTING = {}


@pytest.fixture(scope="module")
def ops():
    from realpdebench_amd import ops as o
    return o


@pytest.fixture(scope="module")
def cus(ops):
    n = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    assert ops.tattn_blocks(10 ** 9) == 6 * n                    # the library's own count (rpb_tattn_blocks caps at 6 blocks per compute unit)
    return n


def check(name, got, ref64, ref32, kernel=None):
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    rows = []
    for kind, e32, ek in zip(K.MEASURES, K.measures(ref32, ref64), K.measures(got, ref64)):
        bound = EXISTING.get(kernel, K.bound_of(e32))
        print(f"[unet-kernels] {name} {kind}: e32 {e32:.3e} kernel {ek:.3e} bound {bound:.3e}")
        rows.append((kind, e32, ek, bound))
    for kind, e32, ek, bound in rows:
        assert 8 * e32 <= K.BADLY_CONDITIONED, f"{name}: badly conditioned inputs, the fp32 restatement itself is off by {e32:.3e} ({kind})"
        assert ek <= bound, f"{name} {kind}: kernel error {ek:.3e} > {bound:.3e} (fp32 restatement: {e32:.3e})"


def exact(name, got, ref32):
    assert tuple(got.shape) == tuple(ref32.shape), (name, got.shape, ref32.shape)
    same = torch.equal(got, ref32.float())
    print(f"[unet-kernels] {name}: bit-exact {same}")
    assert same, f"{name}: {int((got != ref32.float()).sum())} element(s) differ from the fp32 restatement"


def reduce_rows(ops, part_host, rows, L, f64=False, row_stride=None, col0=0):
    """rpb_reduce_partials of a [rows][row_stride] partial buffer (guarded like every other call) -> host [L]"""
    a = guarded.Arena(DEV)
    p = a.inp(part_host)
    if f64:
        a64 = guarded.Arena(DEV, F64)                            # the fp64 output has an arena of its own dtype
        o = a64.out(L)
        ops.reduce_partials(p.op, rows, L, out_f64=o.tensor(), row_stride=row_stride, col0=col0)
        a.check()
        a64.check()
        return o.get()
    o = a.out(L)
    ops.reduce_partials(p.op, rows, L, out_f32=o.op, row_stride=row_stride, col0=col0)
    a.check()
    return o.get()


def cols(shape, lo, hi):
    """the ``unwritten`` mask of a column-range output: everything but columns lo..hi-1"""
    m = torch.ones(shape, dtype=torch.bool)
    m[..., lo:hi] = False
    return m


# ================================================================================================ GroupNorm + SiLU channel passes
@pytest.mark.parametrize("B,n,C", K.CHAN_SHAPES)
def test_chan_kernels(ops, B, n, C):
    c = K.chan_case(B, n, C)
    r64, r32 = c.refs()
    nblk = ops.chan_blocks(B, n)
    tag = f"{c.name} nblk={nblk}"
    a = guarded.Arena(DEV)
    x, part = a.inp(c.x), a.out(nblk, B * 2 * C)
    ops.chan_stats(x.op, part.op, B, n, C)
    a.check()
    sums = reduce_rows(ops, part.get(), nblk, B * 2 * C, f64=True)             # as _gn_silu: fp64 sums
    check(tag + " chan_stats", sums.view(B, 2, C), r64["stats"], r32["stats"])
    for with_res in (False, True):
        a = guarded.Arena(DEV)
        x, A, Bc, y = a.inp(c.x), a.inp(c.A), a.inp(c.Bc), a.out(B, n, C)
        res = a.inp(c.res) if with_res else None
        ops.affine_silu_fwd(x.op, A.op, Bc.op, y.op, B, n, C, res=res.op if with_res else None)
        a.check()
        key = "y_res" if with_res else "y"
        check(f"{tag} affine_silu_fwd res={int(with_res)}", y.get(), r64[key], r32[key], kernel="affine_silu_fwd")
    a = guarded.Arena(DEV)
    x, gy, A, Bc, part = a.inp(c.x), a.inp(c.gy), a.inp(c.A), a.inp(c.Bc), a.out(nblk, B * 2 * C)
    ops.affine_silu_bwd_reduce(x.op, gy.op, A.op, Bc.op, part.op, B, n, C)
    a.check()
    check(tag + " affine_silu_bwd_reduce", reduce_rows(ops, part.get(), nblk, B * 2 * C).view(B, 2, C), r64["red"], r32["red"],
          kernel="affine_silu_bwd")
    a = guarded.Arena(DEV)
    x, gy, A, Bc, P, Q, gx = a.inp(c.x), a.inp(c.gy), a.inp(c.A), a.inp(c.Bc), a.inp(c.P), a.inp(c.Q), a.out(B, n, C)
    ops.affine_silu_bwd_apply(x.op, gy.op, A.op, Bc.op, P.op, Q.op, gx.op, B, n, C)
    a.check()
    check(tag + " affine_silu_bwd_apply", gx.get(), r64["gx"], r32["gx"], kernel="affine_silu_bwd")


# ================================================================================================ channel LayerNorm
@pytest.mark.parametrize("M,C", K.LN_SHAPES)
def test_layernorm_kernels(ops, M, C):
    c = K.ln_case(M, C)
    r64, r32 = c.refs()
    a = guarded.Arena(DEV)
    x, gam, beta, y = a.inp(c.x), a.inp(c.gamma), a.inp(torch.zeros(C)), a.out(M, C)
    ops.layernorm_fwd(x.op, gam.op, beta.op, y.op, M, C, K.LN_EPS)
    a.check()
    check(c.name + " fwd", y.get(), r64["y"], r32["y"])
    rows = ops.layernorm_bwd_rows(M)
    a = guarded.Arena(DEV)
    x, gam, gy, gx, part = a.inp(c.x), a.inp(c.gamma), a.inp(c.gy), a.out(M, C), a.out(rows, 2 * C)
    ops.layernorm_bwd(x.op, gam.op, gy.op, None, gx.op, part.op, M, C, K.LN_EPS)
    a.check()
    check(c.name + " bwd gx", gx.get(), r64["gx"], r32["gx"])
    check(f"{c.name} bwd dgamma|dbeta rows={rows}", reduce_rows(ops, part.get(), rows, 2 * C), r64["dgb"], r32["dgb"])


# ================================================================================================ init_conv: im2col and the GEMMs on it
def wgrad(ops, G, A, M, N, Kk, ldg=None, conv=None, conv_mode=1):
    """model/unet.py:_wgrad on guarded operands: the TN GEMM's partials, then the two fp64 reductions -> host (dW [N][K], db [N])"""
    splits = ops.gemm_tn_splits(M, N, Kk, conv is not None, conv_mode, ldg=ldg)
    L = N * Kk + N
    a = guarded.Arena(DEV)
    g, x, part = a.inp(G), a.inp(A), a.out(splits, L)
    ops.gemm_tn(g.op, x.op, part.op, M, N, Kk, ldg=ldg, conv=conv, conv_mode=conv_mode)
    a.check()
    ph = part.get()
    return (reduce_rows(ops, ph, splits, N * Kk, row_stride=L).view(N, Kk), reduce_rows(ops, ph, splits, N, row_stride=L, col0=N * Kk), splits)


@pytest.mark.parametrize("Cin", K.IM2COL_CIN)
@pytest.mark.parametrize("B,T,H,W", K.IM2COL_MESHES)
def test_im2col_and_its_gemms(ops, B, T, H, W, Cin):
    c = K.im2col_case(B, T, H, W, Cin)
    r64, r32 = c.refs()
    M, ldc, ncol = B * T * H * W, K.init_ldc(Cin), K.KS ** 3 * Cin
    a = guarded.Arena(DEV)
    x, col = a.inp(c.x), a.out(M, ldc)
    ops.im2col(x.op, col.op, B, T, H, W, Cin, K.KS, ldc)
    a.check()
    colh = col.get()
    assert not colh[:, ncol:].any(), "im2col: the pad columns must be exactly zero"
    exact(c.name + " im2col", colh, r32["col"])
    a = guarded.Arena(DEV)
    A, Wt, b, y = a.inp(r32["col"]), a.inp(c.W), a.inp(c.bias), a.out(M, 64)
    ops.gemm_nt(A.op, Wt.op, y.op, M, 64, ldc, bias=b.op)
    a.check()
    check(f"{c.name} gemm_nt N=64 K={ldc}", y.get(), r64["y"], r32["y"])
    dW, db, splits = wgrad(ops, c.gy, r32["col"], M, 64, ldc)
    check(f"{c.name} gemm_tn N=64 K={ldc} splits={splits} dW", dW, r64["dW"], r32["dW"])
    check(f"{c.name} gemm_tn N=64 K={ldc} db", db, r64["db"], r32["db"])


# ================================================================================================ final 1x1 convolution
@pytest.mark.parametrize("M,N", K.FINAL_CASES)
def test_final_conv_kernels(ops, M, N):
    c = K.final_case(M, N)
    r64, r32 = c.refs()
    a = guarded.Arena(DEV)
    x, Wt, b, y = a.inp(c.x), a.inp(c.W), a.inp(c.bias), a.out(M, N)
    ops.gemm_nt(x.op, Wt.op, y.op, M, N, 64, bias=b.op)
    a.check()
    check(c.name + " gemm_nt K=64", y.get(), r64["y"], r32["y"])
    ldg = (N + 3) // 4 * 4                                       # model/unet.py:_linear pads the 3-channel gradient to 4 columns of zeros
    gp = torch.zeros(M, ldg)
    gp[:, :N] = c.gy
    dW, db, splits = wgrad(ops, gp, c.x, M, N, 64, ldg=ldg)
    check(f"{c.name} gemm_tn ldg={ldg} splits={splits} dW", dW, r64["dW"], r32["dW"])
    check(f"{c.name} gemm_tn ldg={ldg} db", db, r64["db"], r32["db"])
    a = guarded.Arena(DEV)
    g, Wt, b, gx = a.inp(c.gy), a.inp(c.W.t().contiguous()), a.inp(torch.zeros(64)), a.out(M, 64)
    ops.tokens_lift(g.op, Wt.op, b.op, gx.op, M, N, 64, False)
    a.check()
    check(f"{c.name} tokens_lift K={N} -> 64", gx.get(), r64["gx"], r32["gx"])


# ================================================================================================ strided / transposed gather modes
@pytest.mark.parametrize("C,mesh4", K.GATHER_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gather_modes(ops, C, mesh4):
    B, T, H, W = mesh4
    c = K.gather_case(C, mesh4)
    r64, r32 = c.refs()
    M, Mo = B * T * H * W, B * T * (H // 2) * (W // 2)
    a = guarded.Arena(DEV)
    x, Wd, b, y = a.inp(c.x), a.inp(K.down_layout(c.wd)), a.inp(c.bias), a.out(Mo, C)
    ops.gemm_nt(x.op, Wd.op, y.op, Mo, C, 16 * C, bias=b.op, conv=(T, H, W), conv_mode=2)
    a.check()
    check(c.name + " gemm_nt conv_mode=2", y.get(), r64["down"], r32["down"])
    dW, db, splits = wgrad(ops, c.gy, c.x, Mo, C, 16 * C, conv=(T, H, W), conv_mode=2)
    check(f"{c.name} gemm_tn conv_mode=2 splits={splits} dW", K.down_unlayout(dW, C), r64["dW"], r32["dW"])
    check(f"{c.name} gemm_tn conv_mode=2 db", db, r64["db"], r32["db"])
    Wc = K.up_layout(c.wu)
    for cls in range(4):
        rows = K.up_class_rows(cls, B, T, H, W)
        other = torch.ones(4 * M, C, dtype=torch.bool)
        other[rows] = False                                      # a class writes its own quarter of the (T, 2H, 2W) rows and nothing else
        a = guarded.Arena(DEV)
        x, Wt, b, y = a.inp(c.x), a.inp(Wc[cls]), a.inp(c.bias), a.out(4 * M, C, unwritten=other)
        ops.gemm_nt(x.op, Wt.op, y.op, M, C, 4 * C, bias=b.op, conv=(T, H, W), conv_mode=3, cls=cls)
        a.check()
        check(f"{c.name} gemm_nt conv_mode=3 cls={cls}", y.get()[rows], r64["up"][rows], r32["up"][rows])


# ================================================================================================ temporal attention
TATTN_IDS = ["NI5-full", "NI10-first-odd", "config-T20", "NI16-T21", "NI16-T32", "grid-stride-prefetch"]


@pytest.mark.parametrize("which", range(6), ids=TATTN_IDS)
def test_tattn_kernels(ops, cus, which):
    B, T, HW = K.tattn_shapes(cus)[which]
    blocks = ops.tattn_blocks(B * HW)
    if which == 5:
        assert blocks == 6 * cus and B * HW > blocks             # blocks walk on to a location of the other sample, prefetched
    c = K.tattn_case(B, T, HW)
    r64, r32 = c.refs()
    tag = f"{c.name} blocks={blocks}"
    a = guarded.Arena(DEV)
    qkv, rc, rs, bias, out = a.inp(c.qkv), a.inp(c.rc), a.inp(c.rs), a.inp(c.bias), a.out(B, T, HW, HID)
    ops.tattn_fwd(qkv.op, rc.op, rs.op, bias.op, out.op, B, T, HW)
    a.check()
    check(tag + " tattn_fwd", out.get(), r64["out"], r32["out"], kernel="tattn_fwd")
    a = guarded.Arena(DEV)
    qkv, rc, rs, bias, go = a.inp(c.qkv), a.inp(c.rc), a.inp(c.rs), a.inp(c.bias), a.inp(c.go)
    gq, part = a.out(B, T, HW, 3 * HID), a.out(blocks * 4, T * T)
    ops.tattn_bwd(qkv.op, rc.op, rs.op, bias.op, go.op, gq.op, part.op, B, T, HW)
    a.check()
    check(tag + " tattn_bwd gqkv", gq.get(), r64["gqkv"], r32["gqkv"], kernel="tattn_bwd")
    db = reduce_rows(ops, part.get().view(blocks, 4 * T * T), blocks, 4 * T * T).view(4, T, T)       # row % 4 = head, as _temporal_attn
    check(tag + " tattn_bwd dbias", db, r64["dbias"], r32["dbias"], kernel="tattn_bwd")


# ================================================================================================ bottleneck attention
@pytest.mark.parametrize("Fr,n", K.SATTN_SHAPES)
def test_sattn_kernels(ops, Fr, n):
    c = K.sattn_case(Fr, n)
    r64, r32 = c.refs()
    a = guarded.Arena(DEV)
    qkv, out, lse = a.inp(c.qkv), a.out(Fr, n, HID), a.out(Fr, 4, n)
    ops.sattn_fwd(qkv.op, out.op, lse.op, Fr, n)
    a.check()
    check(c.name + " sattn_fwd out", out.get(), r64["out"], r32["out"], kernel="sattn_fwd")
    check(c.name + " sattn_fwd lse", lse.get(), r64["lse"], r32["lse"], kernel="sattn_fwd")
    a = guarded.Arena(DEV)                                       # the backward gets the fp64 forward results rounded to fp32
    qkv, o, go, lse, gq = a.inp(c.qkv), a.inp(r64["out"]), a.inp(c.go), a.inp(r64["lse"]), a.out(Fr, n, 3 * HID)
    ops.sattn_bwd(qkv.op, o.op, go.op, lse.op, gq.op, Fr, n)
    a.check()
    check(c.name + " sattn_bwd", gq.get(), r64["gqkv"], r32["gqkv"], kernel="sattn_bwd")


# ================================================================================================ spatial linear attention, stage by stage
@pytest.mark.parametrize("Fr,n", K.LINATTN_SHAPES)
def test_linear_attention_stages(ops, Fr, n):
    """the Sub offsets and leading dimensions of model/unet.py:_linear_attn: k = columns 128.. of the 384-wide qkv, E = columns 128.. of
    the 256-wide qe, v = columns 256.. of qkv; outputs into a dense tensor and into column ranges of dqe / gqkv"""
    c = K.linattn_case(Fr, n)
    r64, r32 = c.refs()
    M, nblk, chunks = Fr * n, ops.chan_blocks(Fr, n), ops.head_scores_chunks(Fr, n)
    tag = f"{c.name} nblk={nblk} chunks={chunks}"
    # ---- col_reduce mode 0 (k maxima) and mode 1 (Z = column sums of E)
    a = guarded.Arena(DEV)
    qkv, pm = a.inp(c.qkv), a.out(nblk, Fr * HID)
    ops.col_reduce(qkv.at(HID), 3 * HID, pm.op, Fr, n, HID, 0)
    a.check()
    exact(tag + " col_reduce max", pm.get().amax(0).view(Fr, HID), r32["kmax"])
    a = guarded.Arena(DEV)
    qe, pm = a.inp(c.qe), a.out(nblk, Fr * HID)
    ops.col_reduce(qe.at(HID), 2 * HID, pm.op, Fr, n, HID, 1)
    a.check()
    check(tag + " col_reduce sum", reduce_rows(ops, pm.get(), nblk, Fr * HID).view(Fr, HID), r64["Z"], r32["Z"])
    # ---- linattn_prep forward / backward
    a = guarded.Arena(DEV)
    qkv, kmax, qe = a.inp(c.qkv), a.inp(c.kmax), a.out(Fr, n, 2 * HID)
    ops.linattn_prep_fwd(qkv.op, kmax.op, qe.op, Fr, n)
    a.check()
    check(tag + " linattn_prep_fwd", qe.get(), r64["qe"], r32["qe"], kernel="linattn_prep_fwd")
    a = guarded.Arena(DEV)
    qe, dqe, dz = a.inp(c.qe), a.inp(c.dqe), a.inp(c.dz)
    gq = a.out(Fr, n, 3 * HID, unwritten=cols((Fr, n, 3 * HID), 0, 2 * HID))      # d q | d k; the d v columns belong to head_apply
    ops.linattn_prep_bwd(qe.op, dqe.op, dz.op, gq.op, Fr, n)
    a.check()
    check(tag + " linattn_prep_bwd", gq.get()[..., :2 * HID], r64["gqk"], r32["gqk"], kernel="linattn_prep_bwd")
    # ---- head_scores(nheads=2) + reduce_partials: E^T v and q'^T go
    for key, (G, goff, ldg), (A, aoff, lda) in (("S", (c.qe, HID, 2 * HID), (c.qkv, 2 * HID, 3 * HID)),
                                                ("dctx", (c.qe, 0, 2 * HID), (c.go, 0, HID))):
        a = guarded.Arena(DEV)
        g, x, part = a.inp(G), a.inp(A), a.out(chunks, Fr * 2 * 4096)
        ops.head_scores(g.at(goff), ldg, x.at(aoff), lda, part.op, Fr, n, nheads=2)
        a.check()
        check(f"{tag} head_scores {key}", reduce_rows(ops, part.get(), chunks, Fr * 2 * 4096).view(Fr, 2, 64, 64), r64[key], r32[key])
    # ---- head_apply(nheads=2): dense output; column range 128.. of the 256-wide dqe; column range 256.. of the 384-wide gqkv
    for key, w, (X, xoff, ldx), (ldo, ooff) in (("o", 0, (c.qe, 0, 2 * HID), (HID, 0)),
                                                ("dE", 1, (c.qkv, 2 * HID, 3 * HID), (2 * HID, HID)),
                                                ("dv", 2, (c.qe, HID, 2 * HID), (3 * HID, 2 * HID))):
        a = guarded.Arena(DEV)
        x, Wm = a.inp(X), a.inp(c.Wm[w])
        out = a.out(Fr, n, ldo, unwritten=None if ldo == HID else cols((Fr, n, ldo), ooff, ooff + HID))
        ops.head_apply(x.at(xoff), ldx, Wm.op, out.at(ooff), ldo, Fr, n, nheads=2)
        a.check()
        check(f"{tag} head_apply {key} ldx={ldx} ldo={ldo}", out.get()[..., ooff:ooff + HID], r64[key], r32[key])


# ================================================================================================ copies and sums
@pytest.mark.parametrize("Ca,Cb", K.COPY_SHAPES)
def test_copy_cols(ops, Ca, Cb):
    from unet_restatement import copy_cols as ref
    torch.manual_seed(Ca + Cb)
    M, Ct = K.COPY_M, Ca + Cb
    av, bv, gv = torch.randn(M, Ca), torch.randn(M, Cb), torch.randn(M, Ct)
    sent = torch.full((M, Ct), guarded.SENTINEL)
    # concatenation: two row-block copies into the wide tensor (model/unet.py:_cat) ...
    for src, C, doff in ((av, Ca, 0), (bv, Cb, Ca)):
        a = guarded.Arena(DEV)
        s, d = a.inp(src), a.out(M, Ct, unwritten=cols((M, Ct), doff, doff + C))
        ops.copy_cols(s.op, d.op, M, C, C, Ct, 0, doff)
        a.check()
        exact(f"copy_cols cat C={C} ldd={Ct} doff={doff}", d.get(), ref(src, sent, C, 0, doff, F32))
    # ... and its split
    for C, soff in ((Ca, 0), (Cb, Ca)):
        a = guarded.Arena(DEV)
        s, d = a.inp(gv), a.out(M, C)
        ops.copy_cols(s.op, d.op, M, C, Ct, C, soff, 0)
        a.check()
        exact(f"copy_cols split C={C} lds={Ct} soff={soff}", d.get(), gv[:, soff:soff + C])


@pytest.mark.parametrize("M,N", K.COLSUM_SHAPES)
def test_colsum(ops, M, N):
    """N / 4 must divide 256: wider tensors are summed in power-of-two column chunks with ld = N, as model/_common.py:colsum does"""
    c = K.colsum_case(M, N)
    r64, r32 = c.refs()
    rows, chunk = ops.colsum_rows(), 1024
    while N % chunk:
        chunk //= 2
    got = torch.empty(N)
    for c0 in range(0, N, chunk):
        a = guarded.Arena(DEV)
        x, part = a.inp(c.x), a.out(rows, chunk)
        ops.colsum(x.at(c0), part.op, M, chunk, ld=N)
        a.check()
        got[c0:c0 + chunk] = reduce_rows(ops, part.get(), rows, chunk)
    check(f"{c.name} chunk={chunk}", got, r64["s"], r32["s"])


@pytest.mark.parametrize("n", K.ADD_SIZES)
def test_add(ops, n):
    from realpdebench_amd import _lib
    torch.manual_seed(n)
    x, y = torch.randn(n), torch.randn(n)
    a = guarded.Arena(DEV)
    xa, ya, out = a.inp(x), a.inp(y), a.out(n)
    _lib.call("rpb_add", ops._p(xa.op), ops._p(ya.op), ops._p(out.op), n, ops._stream())      # ops.add allocates its own output
    a.check()
    exact(f"add n={n}", out.get(), x + y)


@pytest.mark.parametrize("T", K.RELPOS_T)
def test_relpos_bias(ops, T):
    """the index guard holds 40: a stray index read would fetch table row 40, inside the NaN guard behind the 32-row table"""
    c = K.relpos_case(T)
    r64, r32 = c.refs()
    a, ai = guarded.Arena(DEV), guarded.Arena(DEV, torch.int32, fill=40)
    table, idx, bias = a.inp(c.table), ai.inp(c.idx), a.out(4, T * T)
    ops.relpos_bias_fwd(table.op, idx.op, bias.op, T * T, 4)
    a.check()
    ai.check()
    exact(c.name + " fwd", bias.get(), r32["bias"])
    a, ai = guarded.Arena(DEV), guarded.Arena(DEV, torch.int32, fill=40)
    g, idx, gt = a.inp(c.g), ai.inp(c.idx), a.out(32, 4)
    ops.relpos_bias_bwd(g.op, idx.op, gt.op, T * T, 4, 32)
    a.check()
    ai.check()
    check(c.name + " bwd", gt.get(), r64["gt"], r32["gt"])


# ================================================================================================ token-GEMM dispatch
@pytest.mark.parametrize("M,N,Kk", K.GEMM_CASES)
def test_token_gemm_dispatch(ops, monkeypatch, M, N, Kk):
    """both sides of the row thresholds of ops.gemm_nt (4096: the 64-row-tile split-operand kernel; 65536: the 128-row one), plain and
    with bias + residual; the entry points ops chose are recorded from its calls into the library, named in every message, and pinned:
    with these N (multiples of 128 take the 64-row-tile kernel, which has no 65536 threshold; N = 64 stays on the fp32 kernel below 65536
    rows) the split-operand entry point must be chosen exactly from 4096 rows on, so that a moved threshold cannot turn the two M of a
    pair into duplicates"""
    from realpdebench_amd import _lib
    c = K.gemm_case(M, N, Kk)
    r64, r32 = c.refs()
    called, real = [], _lib.call

    def spy(name, *args, **kw):
        called.append(kw.get("label") or name)
        return real(name, *args, **kw)

    monkeypatch.setattr(_lib, "call", spy)
    for key in ("plain", "full"):
        del called[:]
        a = guarded.Arena(DEV)
        A, Wt, y = a.inp(c.A), a.inp(c.W), a.out(M, N)
        b, res = (a.inp(c.bias), a.inp(c.res)) if key == "full" else (None, None)
        ops.gemm_nt(A.op, Wt.op, y.op, M, N, Kk, bias=b.op if b else None, residual=res.op if res else None)
        kernel = "+".join(called)
        try:
            a.check()
        except AssertionError as e:
            raise AssertionError(f"{c.name} {key} via {kernel}: {e}") from None
        split = bool(ops.GEMM_SPLIT and M >= 4096 and N % 128 == 0)
        assert any(k.startswith("gemm3x[") for k in called) == split and any(k.startswith("gemm_nt[") for k in called) != split, \
            f"{c.name} {key}: ops chose {kernel}, expected the {'split-operand (gemm3x)' if split else 'fp32 (gemm_nt)'} entry point"
        check(f"{c.name} {key} via {kernel}", y.get(), r64[key], r32[key])
