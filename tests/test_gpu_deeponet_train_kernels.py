"""The row kernels of the DeepONet training step (csrc/rpb_deeponet_train.hip) and the row BatchNorm backward tail they feed
(csrc/rpb_rowbn.hip: ``ops.rowbn_sum64``, ``ops.rowbn_act_bwd_apply``), every entry point called alone.

Operands live in the guard-banded arenas of tests/guarded.py (fp64 partials and sums in fp64 arenas of their own).  References are the
functions of tests/deeponet_train_restatement.py in fp64 on the CPU, computed once per shape; the verdict is tests/kernel_verdict.py: the
error of the same restatement run in fp32, times 8, with floor 1e-6 -- the kernel's own error never enters a bound.  What must be exact is
asserted exactly: zero gradient on the frame / row / column a flooring pool drops, zero pad columns, and bit-equality of a second call.

Ragged shapes: item counts that are no multiple of a workgroup's share, ``ld > C``, C = 32 of ``ld = 64``, meshes with odd extents and
(adaptive pool) an extent of 1, In < 4 bins, B = 1, and for the point kernels N that is no multiple of 32 with a chunk that starts and
ends inside a sample.  ReLU inputs are drawn at least 1e-3 away from zero and the two largest values of every max-pool window at least
1e-3 apart (closer elements are redrawn, none is excluded), so fp32 and fp64 agree on every gate and every arg-max.

Measured on an MI355X (profiles/deeponet_train_pytest.txt): every figure of every kernel lies at 0.6e-8 to 1.0e-7, at or below the fp32
restatement's own error (the partial sums are fp64), against bounds of 1.0-1.2e-6."""
import functools
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeponet_train_restatement as TR           # noqa: E402
import guarded                                    # noqa: E402
from kernel_verdict import measures, verdict      # noqa: E402
from realpdebench_amd import ops                  # noqa: E402
from realpdebench_amd.model.deeponet import DeepONet          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64
# (mode, C, ld, B, T, H, W)
POOL_CASES = [
    (0, 32, 64, 3, 5, 7, 6),          # C = 32 of ld = 64, odd T and H: a dropped frame and row; 108 windows + 54 partial ones
    (0, 64, 64, 1, 2, 9, 4),          # B = 1, the smallest T
    (0, 128, 132, 2, 4, 2, 11),       # ld > C, a dropped column
    (0, 256, 256, 2, 3, 3, 3),        # every extent odd
    (1, 256, 256, 3, 2, 3, 5),        # overlapping bins in both axes (3 -> 4, 5 -> 4), mean over T = 2
    (1, 256, 260, 1, 1, 1, 2),        # B = 1, extents of 1: replicated bins (1 -> 4, 2 -> 4), ld > C
    (1, 64, 64, 2, 1, 9, 4),          # 9 -> 4 and the identity 4 -> 4
]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rows_in(a, block, ld, name):
    """block [M][C] as the first columns of an [M][ld] input operand whose other columns are NaN"""
    full = torch.full((block.shape[0], ld), float("nan"))
    full[:, :block.shape[1]] = block
    return a.inp(full, name)


def _pool_ref(c, dt):
    """(gz, sums [2 C], dy, dgamma, dbeta) of one pool case in ``dt``, from the fp32 operands the kernel gets"""
    mode, C, B, T, H, W = c["mode"], c["C"], *c["mesh"]
    y, g, a, b, mean, rstd = (c[k].to(dt) for k in ("y", "g", "a", "b", "mean", "rstd"))
    y5 = y.view(B, T, H, W, C)
    z = y5 * a + b
    gz = TR.adaptive_pool_bwd(z, g.view(B, 1, 4, 4, C)) if mode else TR.max_pool_bwd(torch.relu(z), g.view(B, T // 2, H // 2, W // 2, C))
    gz = gz.reshape(-1, C)
    xhat = (y - mean) * rstd
    M = y.shape[0]
    s0, s1 = gz.sum(0), (gz * xhat).sum(0)
    dy = a * (gz - s0 / M - xhat * (s1 / M))
    return gz, torch.cat([s0, s1]), dy, s1, s0


@functools.lru_cache(maxsize=None)
def _pool_case(mode, C, B, T, H, W):
    g = _g(1000 * mode + C + 7 * T + 5 * H + 3 * W + B)
    M = B * T * H * W
    y = torch.randn(M, C, generator=g)
    a, b = torch.rand(C, generator=g) * 0.5 + 0.75, torch.rand(C, generator=g) * 0.6 - 0.3
    mean, rstd = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) * 0.5 + 0.75
    for _ in range(200):                       # gate and arg-max robustness: redraw what is closer than 1e-3
        z = (y.double() * a.double() + b.double()).view(B, T, H, W, C)
        close = z.abs() < 1e-3
        if not mode:
            v = torch.relu(z)[:, :T // 2 * 2, :H // 2 * 2, :W // 2 * 2]
            w = v.reshape(B, T // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(B, T // 2, H // 2, W // 2, C, 8)
            top = w.topk(2, dim=-1)
            tie = ((top.values[..., 0] - top.values[..., 1]) < 1e-3) & (top.values[..., 0] > 0)
            hit = torch.zeros_like(w, dtype=torch.bool).scatter_(-1, top.indices[..., 1:2], tie[..., None])
            hit = hit.reshape(B, T // 2, H // 2, W // 2, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(v.shape)
            close[:, :T // 2 * 2, :H // 2 * 2, :W // 2 * 2] |= hit
        if not bool(close.any()):
            break
        y = torch.where(close.view(M, C), y + 0.05 * torch.randn(M, C, generator=g), y)
    else:
        raise AssertionError("could not draw gate-robust inputs")
    cells_out = B * 16 if mode else B * (T // 2) * (H // 2) * (W // 2)
    c = dict(mode=mode, C=C, mesh=(B, T, H, W), y=y, a=a, b=b, mean=mean, rstd=rstd, g=torch.randn(cells_out, C, generator=g))
    c["ref"], c["f32"] = _pool_ref(c, F64), _pool_ref(c, torch.float32)
    return c


def _cols(M, ld, lo):
    """bool [M][ld]: True on the columns from ``lo`` on (what a launch does not write)"""
    u = torch.zeros(M, ld, dtype=torch.bool)
    u[:, lo:] = True
    return u


@pytest.mark.parametrize("mode,C,ld,B,T,H,W", POOL_CASES)
def test_pool_bwd_sum_and_apply(mode, C, ld, B, T, H, W):
    c = _pool_case(mode, C, B, T, H, W)
    M, rows, tag = B * T * H * W, ops.rowbn_rows(), f"pool{mode} C{C} ld{ld} {B}x{T}x{H}x{W}"
    Cpad = min(ld, C + 32) // 4 * 4
    ab = [c[k] for k in ("a", "b", "mean", "rstd")]
    a32, p64, s64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64), guarded.Arena(DEV, dtype=F64)
    o_y, o_g = _rows_in(a32, c["y"], ld, "y"), _rows_in(a32, c["g"], ld, "g")
    o_ab = [a32.inp(t, n) for t, n in zip(ab, ("a", "b", "mean", "rstd"))]
    o_gz = a32.out(M, ld, name="gz", unwritten=_cols(M, ld, C))
    o_part = p64.out(rows, 2 * C, name="part")
    DeepONet.k_pool_bwd(o_y.op, ld, o_g.op, ld, [o.op for o in o_ab], o_gz.op, ld, B, T, H, W, C, mode, o_part.tensor())
    a32.check()
    p64.check()
    gz, part = o_gz.get()[:, :C], o_part.get()
    i_part, o_sums = s64.inp(part, "part"), s64.out(2 * C, name="sums")
    ops.rowbn_sum64(i_part.tensor(), rows, C, o_sums.tensor())
    s64.check()
    sums = o_sums.get()
    # the apply launch, out of place: gz and the sums as inputs of a second arena
    b32, t64 = guarded.Arena(DEV), guarded.Arena(DEV, dtype=F64)
    i_gz, i_y = _rows_in(b32, gz, ld, "gz"), _rows_in(b32, c["y"], ld, "y")
    i_ab = [b32.inp(t, n) for t, n in zip(ab, ("a", "b", "mean", "rstd"))]
    i_sums = t64.inp(sums, "sums")
    o_dy = b32.out(M, ld, name="dy", unwritten=_cols(M, ld, Cpad))
    o_dg, o_db = b32.out(C, name="dgamma"), b32.out(C, name="dbeta")
    v = dict(zip(("a", "b", "mean", "rstd"), (o.op for o in i_ab)))
    ops.rowbn_act_bwd_apply(i_gz.op, ld, M, C, Cpad, 0, y=i_y.op, ldy=ld, **v, sums=i_sums.tensor(), dy=o_dy.op, ldd=ld, dgamma=o_dg.op, dbeta=o_db.op)
    b32.check()
    t64.check()
    dy = o_dy.get()
    r64, r32 = c["ref"], c["f32"]
    figures = []
    for name, got, k in (("gz", gz, 0), ("sums", sums, 1), ("dy", dy[:, :C], 2), ("dgamma", o_dg.get(), 3), ("dbeta", o_db.get(), 4)):
        for kind, e32, ek in zip(("rel-l2", "max-abs"), measures(r32[k], r64[k]), measures(got, r64[k])):
            figures.append((f"{name} {kind}", e32, ek))
    verdict(tag, "don_pool_bwd + rowbn_sum64 + rowbn_act_bwd_apply", figures)
    assert not bool(dy[:, C:Cpad].any()), "pad columns are exactly zero"
    assert torch.equal((gz != 0), (r64[0] != 0)), "the gradient lands on exactly the cells the rule names"
    if not mode:
        g5 = gz.view(B, T, H, W, C)
        assert not bool(g5[:, T // 2 * 2:].any()) and not bool(g5[:, :, H // 2 * 2:].any()) and not bool(g5[:, :, :, W // 2 * 2:].any()), \
            "the trailing frame / row / column the flooring pool drops gets zero gradient"
    # a second call on plain tensors, the apply launch in place: bit-equal
    pad = lambda t: torch.cat([t, torch.zeros(t.shape[0], ld - C)], 1).to(DEV)
    y2, g2, ab2 = pad(c["y"]), pad(c["g"]), torch.stack(ab).to(DEV)
    dy2, part2, sums2 = torch.full((M, ld), 7.0, device=DEV), torch.empty(rows, 2 * C, dtype=F64, device=DEV), torch.empty(2 * C, dtype=F64, device=DEV)
    dgb2 = torch.empty(2, C, device=DEV)
    DeepONet.k_pool_bwd(y2, ld, g2, ld, ab2, dy2, ld, B, T, H, W, C, mode, part2)
    ops.rowbn_sum64(part2, rows, C, sums2)
    ops.rowbn_act_bwd_apply(dy2, ld, M, C, Cpad, 0, y=y2, ldy=ld, a=ab2[0], b=ab2[1], mean=ab2[2], rstd=ab2[3], sums=sums2, dy=dy2, ldd=ld,
                            dgamma=dgb2[0], dbeta=dgb2[1])
    assert torch.equal(part2.cpu(), part) and torch.equal(sums2.cpu(), sums)
    assert torch.equal(dy2.cpu()[:, :Cpad], dy[:, :Cpad]) and torch.equal(dgb2[0].cpu(), o_dg.get()) and torch.equal(dgb2[1].cpu(), o_db.get())
    assert bool((dy2[:, Cpad:] == 7.0).all()), "columns beyond Cpad are not touched"


def test_max_pool_backward_takes_the_first_maximum_on_a_tie():
    """One 2 x 2 x 2 window, a = 1, b = 0.  Channel 0: the same positive maximum in cells k = 3 and k = 5 of the (t, h, w) scan: the gradient
    goes to k = 3 alone.  Channel 1: eight equal positive values: k = 0.  Channel 2: every value <= 0 (the largest exactly 0): nothing.
    Channel 3: a unique maximum in the last cell.  The drawn cases above keep the two largest values 1e-3 apart; this one pins the strict
    comparison of the kernel's scan."""
    C, rows = 32, ops.rowbn_rows()
    y = -torch.rand(8, C, generator=_g(3)) - 0.5
    y[:, 0] = torch.tensor([0.5, 1.0, 0.25, 2.0, 1.5, 2.0, 0.0, -1.0])
    y[:, 1] = 0.75
    y[:, 2] = torch.tensor([-1.0, 0.0, -0.5, -2.0, 0.0, -3.0, -0.25, -0.125])
    y[:, 3] = torch.tensor([0.5, 1.0, 0.25, 2.0, 1.5, 2.0, 0.0, 2.5])
    g = torch.arange(1, C + 1, dtype=torch.float32).view(1, C)
    ab = torch.stack([torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)]).to(DEV)
    gz, part = torch.full((8, C), 7.0, device=DEV), torch.empty(rows, 2 * C, dtype=F64, device=DEV)
    DeepONet.k_pool_bwd(y.to(DEV), C, g.to(DEV), C, ab, gz, C, 1, 2, 2, 2, C, 0, part)
    gz = gz.cpu()
    want = torch.zeros(8, C)
    want[3, 0], want[0, 1], want[7, 3] = 1.0, 2.0, 4.0
    assert torch.equal(gz[:, :4], want[:, :4]), gz[:, :4]
    assert not bool(gz[:, 4:].any()), "channels whose values are all negative pass nothing"
    assert torch.equal(gz, TR.max_pool_bwd(torch.relu(y).view(1, 2, 2, 2, C), g.view(1, 1, 1, 1, C)).view(8, C)), "the restatement's rule"
    sums = part.sum(0).cpu()
    assert float(sums[0]) == 1.0 and float(sums[1]) == 2.0 and float(sums[2]) == 0.0 and float(sums[3]) == 4.0
    assert float(sums[C]) == 2.0 and float(sums[C + 3]) == 4 * 2.5, "sum gz xhat with mean 0, rstd 1: g y at the arg-max"


# (B, N, p, q0, R): N is no multiple of 32
POINT_CASES = [
    (3, 75, 64, 50, 130),             # starts inside sample 0, covers sample 1, ends inside sample 2
    (1, 333, 128, 0, 333),            # B = 1, the whole sample
    (2, 1000, 256, 700, 777),         # more rows than one workgroup's share, a boundary inside
    (2, 45, 256, 44, 1),              # a single row
]


@functools.lru_cache(maxsize=None)
def _point_case(B, N, p):
    g = _g(B + N + p)
    return dict(t=torch.randn(N, p, generator=g), b=torch.randn(B, p, generator=g), gx=torch.randn(B * N, p, generator=g) * 1e-3,
                gt0=torch.randn(N, p, generator=g) * 1e-3, gb0=torch.randn(B, p, generator=g) * 1e-3)


@pytest.mark.parametrize("B,N,p,q0,R", POINT_CASES)
def test_point_mul(B, N, p, q0, R):
    c = _point_case(B, N, p)
    a = guarded.Arena(DEV)
    o_t, o_b, o_x = a.inp(c["t"], "t"), a.inp(c["b"], "b"), a.out(R, p, name="x")
    DeepONet.k_point_mul(o_t.op, o_b.op, o_x.op, q0, R, B, N, p)
    a.check()
    full = lambda dt: (c["b"].to(dt)[:, None, :] * c["t"].to(dt)[None]).reshape(B * N, p)[q0:q0 + R]
    figures = [(kind, e32, ek) for kind, e32, ek in zip(("rel-l2", "max-abs"), measures(full(torch.float32), full(F64)), measures(o_x.get(), full(F64)))]
    verdict(f"B{B} N{N} p{p} q0={q0} R={R}", "don_point_mul", figures)
    x2 = torch.empty(R, p, device=DEV)
    DeepONet.k_point_mul(c["t"].to(DEV), c["b"].to(DEV), x2, q0, R, B, N, p)
    assert torch.equal(x2.cpu(), o_x.get())


@pytest.mark.parametrize("B,N,p,q0,R", POINT_CASES)
def test_point_mul_bwd(B, N, p, q0, R):
    """The chunk's rows, one launch per sample it touches (as the model walks them): gt accumulates over the samples, gb[s] over the
    launches of sample s through rpb_reduce_partials (accumulate)."""
    c = _point_case(B, N, p)
    rows = ops.rowbn_rows()
    gx = c["gx"][q0:q0 + R]
    t_d, b_d = c["t"].to(DEV), c["b"].to(DEV)

    def run(gt, gb, first_arena):
        q, figs = q0, []
        while q < q0 + R:
            s, n0 = divmod(q, N)
            Rs = min(N - n0, q0 + R - q)
            if first_arena and q == q0:                                 # the first launch with every operand in an arena
                a = guarded.Arena(DEV)
                o_gx, o_t, o_b = a.inp(gx[:Rs], "gx"), a.inp(c["t"], "t"), a.inp(c["b"][s], "b")
                o_gt, o_part = a.inout(c["gt0"], "gt"), a.out(rows, p, name="part")
                DeepONet.k_point_mul_bwd(o_gx.op, o_t.op, o_b.op, o_gt.op, o_part.op, n0, Rs, N, p)
                a.check()
                gt.copy_(o_gt.get().to(DEV))
                part = o_part.get().to(DEV)
            else:
                part = torch.empty(rows, p, device=DEV)
                DeepONet.k_point_mul_bwd(ops.Sub(gx.to(DEV).contiguous(), (q - q0) * p), t_d, b_d[s].contiguous(), gt, part, n0, Rs, N, p)
            ops.reduce_partials(part, rows, p, out_f32=ops.Sub(gb, s * p), accumulate=True)
            q += Rs
        return gt, gb

    gt, gb = run(c["gt0"].to(DEV).clone(), c["gb0"].to(DEV).clone(), True)

    def ref(dt):
        full = torch.zeros(B * N, p, dtype=dt)
        full[q0:q0 + R] = gx.to(dt)
        full = full.view(B, N, p)
        return c["gt0"].to(dt) + (full * c["b"].to(dt)[:, None, :]).sum(0), c["gb0"].to(dt) + (full * c["t"].to(dt)[None]).sum(1)

    figures = []
    for name, got, r32, r64 in zip(("gt", "gb"), (gt.cpu(), gb.cpu()), ref(torch.float32), ref(F64)):
        for kind, e32, ek in zip(("rel-l2", "max-abs"), measures(r32, r64), measures(got, r64)):
            figures.append((f"{name} {kind}", e32, ek))
    verdict(f"B{B} N{N} p{p} q0={q0} R={R}", "don_point_mul_bwd", figures)
    gt2, gb2 = run(c["gt0"].to(DEV).clone(), c["gb0"].to(DEV).clone(), False)
    assert torch.equal(gt2, gt) and torch.equal(gb2, gb), "a second pass is bit-equal"


def test_bad_arguments_are_refused():
    from realpdebench_amd._lib import RpbError
    z = torch.zeros(64, 64, device=DEV)
    part = torch.zeros(ops.rowbn_rows(), 128, dtype=F64, device=DEV)
    with pytest.raises(RpbError, match="C in"):
        DeepONet.k_pool_bwd(z, 64, z, 64, z[:4], z, 64, 1, 4, 4, 4, 48, 0, part)
    with pytest.raises(RpbError, match="extents >= 2"):
        DeepONet.k_pool_bwd(z, 64, z, 64, z[:4], z, 64, 1, 1, 8, 8, 64, 0, part)
    with pytest.raises(RpbError, match="q0 \\+ R <= B N"):
        DeepONet.k_point_mul(z, z, z, 60, 10, 1, 64, 64)
    with pytest.raises(RpbError, match="n0 \\+ R <= N"):
        DeepONet.k_point_mul_bwd(z, z, z, z, z, 60, 10, 64, 64)
