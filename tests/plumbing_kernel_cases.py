"""TEST INFRASTRUCTURE ONLY -- the shapes, inputs, restatements and drivers of the per-kernel tests of the step PLUMBING kernels: the lift
and its backward, the layer-0 feature algebra (csrc/rpb_feat.hip), the cell BatchNorm passes, the loss, Adam (plain and ranged), the
normaliser affines and small movers (csrc/rpb_pointwise.hip, csrc/rpb_io.hip), the partial-sum reducers and the spectrum bins of
``eval_metrics`` (csrc/rpb_metrics.hip).  Shared by tests/test_gpu_plumbing_kernels.py (which runs the HIP kernels) and
tests/test_plumbing_kernels_host.py (which proves, without a GPU, that every restatement agrees with an independent statement, that
every case is well conditioned and that a wrong kernel would be noticed).  ``Case``, the two measures and the conditioning cap are those
of tests/unet_kernel_cases.py; the verdict is tests/kernel_verdict.py.

A RESTATEMENT states one launch in plain torch at a given dtype.  The ones with partial rows partition their sums AS THE LAUNCHER DOES:
block ``b`` of ``rows`` adds up the work items b, b + rows, ... into row ``b``; the rows are added up afterwards (in fp64, by the
driver, for the kernel and for the fp32 restatement alike).  Where the kernel accumulates in fp64 and rounds once (the reducers,
small_gemm, bn_finalize) the fp32 restatement does the same.  Scalars enter a restatement AS THE ABI RECEIVES THEM: ``float``
arguments rounded to fp32 (``f32``), Adam's bias corrections in fp64.  The fp32 run gives e32, the fp64 run the reference.

A DRIVER (``run_*``) lays the operands of ONE launch out in a guard-banded arena (tests/guarded.py), calls ``kern.<entry point>``, runs
``Arena.check()`` and judges every output on Rel-L2 and max |error| / max |reference| with the bound max(8 * e32, 1e-6); kernels that
only move data are asserted bit-equal to the fp32 restatement.  Outputs hold the sentinel, the guards around inputs hold NaN, partial
rows are never pre-zeroed, the gaps of a strided operand hold NaN (inputs) or are named ``unwritten`` (outputs).  ``kern`` is the
adapter of the GPU test (realpdebench_amd.ops on a device) or the torch stand-in of the host test on a CPU arena.

Slot and row counts depend on the number of compute units; they are restated here from the launchers (``*_rows``, ``pw_grid``) and the
GPU test asserts that they equal the library's queries on its device."""
import math

import torch

import guarded
from kernel_verdict import verdict
from unet_kernel_cases import (BADLY_CONDITIONED, F32, F64, MEASURES, MI355X_CUS, Case, _gen, _rn,      # noqa: F401
                               measures)

TAG = "plumbing-kernels"
NAN = float("nan")
THREADS = 256                                                      # PW_THREADS


def ceil_div(a, b):
    return (a + b - 1) // b


def f32(x):
    """a ``float`` argument as the C ABI receives it"""
    return float(torch.tensor(float(x), dtype=F32))


# ================================================================================================ slot counts (restated launchers)
def mse_rows(cus=MI355X_CUS):
    return 4 * cus


def bn_bwd_rows(cus=MI355X_CUS):
    return 8 * cus


def lift_bwd_rows(cus=MI355X_CUS):
    return 4 * cus


def feat_mix_wgrad_rows(cus=MI355X_CUS):
    return 2 * cus


def pw_grid(items, cus=MI355X_CUS, per_cu=8):
    """pw_grid of csrc/rpb_pointwise.hip: one 256-thread block per 256 items, ``per_cu`` blocks per compute unit at the most"""
    return max(1, min(ceil_div(items, THREADS), cus * per_cu))


def trips(items, nslots):
    """how many items each slot walks"""
    return [len(range(w, items, nslots)) for w in range(nslots)]


GROUPED_COLS = 1024                                                # rpb_reduce_partials_grouped_cols: 64 columns x RG_SUB = 16 per block


# ================================================================================================ shared pieces
def gelu_grad(z):
    """d/dz of the erf GELU"""
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def _rows(per_item, nslots):
    """[items][...] -> [nslots][...]: block b adds up the items b, b + nslots, ... in that order; blocks without an item hold zeros"""
    out = torch.zeros((nslots,) + tuple(per_item.shape[1:]), dtype=per_item.dtype)
    return out.index_add_(0, torch.arange(per_item.shape[0]) % nslots, per_item)


def _part(per_elem, item, nslots):
    """[n][...] -> [nslots][...]: the work items are runs of ``item`` elements (the last one may be short), dealt as ``_rows`` does"""
    n, items = per_elem.shape[0], ceil_div(per_elem.shape[0], item)
    padded = torch.zeros((items * item,) + tuple(per_elem.shape[1:]), dtype=per_elem.dtype)
    padded[:n] = per_elem
    return _rows(padded.view((items, item) + tuple(per_elem.shape[1:])).sum(1), nslots)


def total(rows):
    """the row sum the trainer's rpb_reduce_partials forms"""
    return rows.double().sum(0)


def judge(name, got, ref64, ref32, existing=None):
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    verdict(TAG, name, zip(MEASURES, measures(ref32, ref64), measures(got, ref64)), existing)


def _bits(t):
    return t.contiguous().view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))


def exact(name, got, want):
    """bit equality (a kernel that only moves data, or one the library promises to agree with another)"""
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (name, got.shape, want.shape)
    bad = (_bits(got) != _bits(want)).reshape(-1).nonzero()
    print(f"[{TAG}] {name}: {got.numel()} element(s) compared bit for bit, {bad.numel()} differ")
    assert not bad.numel(), f"{name}: {bad.numel()} element(s) differ in their bits, the first at flat index {int(bad[0])}"


def _ex(existing, kernel):
    return (existing or {}).get(kernel)


def _stat(g, C):
    """(mean, invstd, gamma, beta) of a BatchNorm layer, none of them near 0"""
    return (_rn(g, C, scale=0.2), torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5, _rn(g, C, scale=0.3))


STAT_NAMES = ("mean", "invstd", "gamma", "beta")


def _ops_of(a, tensors, names):
    return tuple(a.inp(t, n) for t, n in zip(tensors, names))


def _opd(group):
    return None if group is None else tuple(t.op for t in group)


def _op(o):
    return None if o is None else o.op


def _idle_rows_are_zero(name, p, busy):
    idle = p[busy:]
    assert not idle.any(), f"{name}: {int((idle != 0).sum())} non-zero element(s) in the partial rows of blocks without a work item"


# ================================================================================================ lift (rpb_lift_pad_fwd, rpb_lift_bwd)
# (B, T, H, W, Cin, C, pad)
LIFT_CASES = [(2, 3, 4, 5, 2, 64, 2),                              # F = 5: the headline configuration
              (1, 2, 3, 7, 3, 32, 6),                              # F = 6
              (1, 2, 2, 6, 5, 128, 3),                             # F = 8
              (1, 2, 3, 9, 16, 64, 2),                             # F = 19: weights in registers, 16-byte LDS reads
              (1, 1, 2, 129, 16, 32, 1),                           # a row of 2064 inputs: no register prefetch
              (1, 2, 2, 5, 1, 64, 2), (1, 1, 2, 3, 21, 32, 1),     # the generic instantiation; the second at the F = 24 limit
              (1, 2, 2, 4, 0, 64, 2)]                              # rpb_lift_bwd's F = 3 (the forward: generic); x must not be read
LIFT_KERNELS = ["5", "6", "8", "19", "19", "generic", "generic", "3"]


def lift_instantiation(Cin, bwd):
    F = Cin + 3
    return str(F) if F in (5, 6, 8, 19) or (bwd and F == 3) else "generic"


def _live(r, T, H, Tp, Hp):
    return r % Hp < H and (r // Hp) % Tp < T


def lift_fwd_handoffs(dims, cus=MI355X_CUS):
    """the (row -> next row) pairs of the blocks that walk a second row of the padded tensor: which of them are live (read x) or pad"""
    B, T, H, W, Cin, C, pad = dims
    Tp, Hp = T + pad, H + pad
    nrows = B * Tp * Hp
    grid = min(8 * cus, nrows)
    kind = lambda r: "live" if _live(r, T, H, Tp, Hp) else "pad"
    return {f"{kind(r)}>{kind(r + grid)}" for r in range(nrows - grid)}


def lift_fwd_trip_dims(cus=MI355X_CUS):
    """B Tp Hp >= 8 CUs + 3 at W = 3, C = 32: the smallest mesh in whose second trips a live row follows a live row (its inputs were
    prefetched: ``have``), a pad row follows a live row (nothing to prefetch) and a live row follows a pad row (nothing was prefetched)"""
    best = None
    for pad in (1, 2):
        for H in range(2, 24):
            for B in (1, 2, 3):
                for more in range(4):                             # (the last t planes are padding: a live second row needs a few more)
                    Hp = H + pad
                    Tp = ceil_div(8 * cus + 3, B * Hp) + more
                    dims = (B, Tp - pad, H, 3, 2, 32, pad)
                    if Tp - pad >= 1 and {"live>live", "live>pad", "pad>live"} <= lift_fwd_handoffs(dims, cus):
                        if best is None or B * Tp * Hp < best[0]:
                            best = (B * Tp * Hp, dims)
    assert best is not None
    return best[1]


def lift_bwd_trip_dims(cus=MI355X_CUS):
    """B T H >= 4 CUs + 3 rows of the data at W = 3, C = 32 (the backward walks the rows of the data; their gradient rows sit in the
    padded layout, whose margin holds NaN)"""
    H = min(range(2, 17), key=lambda h: ceil_div(4 * cus + 3, h) * h)
    return (1, ceil_div(4 * cus + 3, H), H, 3, 2, 32, 1)


def lift_feats(x, grids, dims, dt):
    """[B][T][H][W][F]: the inputs, then grid_t, grid_h, grid_w"""
    B, T, H, W, Cin = dims[:5]
    gt, gh, gw = (t.to(dt) for t in grids)
    grid = torch.stack((gt.view(1, T, 1, 1).expand(B, T, H, W), gh.view(1, 1, H, 1).expand(B, T, H, W),
                        gw.view(1, 1, 1, W).expand(B, T, H, W)), -1)
    return grid if Cin == 0 else torch.cat((x.to(dt).view(B, T, H, W, Cin), grid), -1)


def lift_fwd(x, grids, w0, b0, dims, dt):
    B, T, H, W, Cin, C, pad = dims
    out = torch.zeros(B, T + pad, H + pad, W + pad, C, dtype=dt)
    out[:, :T, :H, :W] = lift_feats(x, grids, dims, dt) @ w0.to(dt).t() + b0.to(dt)
    return out.view(-1, C)


def lift_bwd(g, x, grids, dims, rows, dt, swap_th=False):
    """part[b] = (d fc0.weight [C][F] | d fc0.bias [C]) over the rows (b, t, h) of the data that block b walks"""
    B, T, H, W, Cin, C, pad = dims
    F = Cin + 3
    feats = lift_feats(x, grids, dims, dt).reshape(B * T * H, W, F)
    if swap_th:                                                   # the host test's wrong term
        feats = feats[..., list(range(Cin)) + [Cin + 1, Cin, Cin + 2]]
    gc = g.to(dt).view(B, T + pad, H + pad, W + pad, C)[:, :T, :H, :W].reshape(B * T * H, W, C)
    per_row = torch.cat((torch.einsum("rwc,rwf->rcf", gc, feats).reshape(B * T * H, C * F), gc.sum(1)), 1)
    return _rows(per_row, rows)


def lift_case(B, T, H, W, Cin, C, pad, cus=MI355X_CUS):
    g = _gen(61, B, T, H, W, Cin, C, pad)
    F, Tp, Hp, Wp = Cin + 3, T + pad, H + pad, W + pad
    dims = (B, T, H, W, Cin, C, pad)
    x = _rn(g, B, T, H, W, Cin) if Cin else torch.full((4,), NAN)    # Cin = 0: a small non-null operand nobody may read
    grids = (torch.linspace(0.2, 1.0, T), torch.linspace(-1.0, -0.1, H), torch.linspace(0.3, 1.3, W))      # three different axes
    w0, b0 = _rn(g, C, F, scale=1 / math.sqrt(F)), _rn(g, C, scale=0.3, shift=1.0)
    gout = torch.full((B, Tp, Hp, Wp, C), NAN)                    # the backward reads the cells of the data only
    gout[:, :T, :H, :W] = _rn(g, B, T, H, W, C, shift=0.3)
    i = dict(dims=dims, x=x, grids=grids, w0=w0, b0=b0, g=gout, rows=lift_bwd_rows(cus))
    return Case(f"lift B={B} T={T} H={H} W={W} Cin={Cin} C={C} pad={pad}", i,
                lambda dt: dict(fwd=lift_fwd(x, grids, w0, b0, dims, dt), bwd=lift_bwd(gout, x, grids, dims, i["rows"], dt)))


def _lift_inputs(a, c):
    W, Cin = c.dims[3], c.dims[4]
    x = a.inp(c.x, "x", ld=max(W * Cin, 4))
    return x, tuple(a.inp(t, n) for t, n in zip(c.grids, ("grid_t", "grid_h", "grid_w")))


def run_lift_fwd(kern, c, existing=None):
    B, T, H, W, Cin, C, pad = c.dims
    Tp, Hp, Wp = T + pad, H + pad, W + pad
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    x, grids = _lift_inputs(a, c)
    w0, b0 = a.inp(c.w0, "w0"), a.inp(c.b0, "b0")
    out = a.out(B * Tp * Hp * Wp, C, name="out", ld=Wp * C)
    kern.lift_pad_fwd(x.op, _opd(grids), w0.op, b0.op, out.op, c.dims)
    a.check()                                                     # every cell of the padded tensor is written, the margin included
    got = out.get()
    inside = torch.zeros(B, Tp, Hp, Wp, dtype=torch.bool)
    inside[:, :T, :H, :W] = True
    margin = got.view(B, Tp, Hp, Wp, C)[~inside]
    exact(f"{c.name} fwd margin", margin, torch.zeros_like(margin))
    judge(f"{c.name} fwd [F={lift_instantiation(Cin, False)}]", got, r64["fwd"], r32["fwd"], _ex(existing, "lift_pad_fwd"))


def run_lift_bwd(kern, c, existing=None):
    B, T, H, W, Cin, C, pad = c.dims
    F = Cin + 3
    r64, r32 = c.refs()
    rows = kern.lift_bwd_rows()
    assert rows == c.rows, (rows, c.rows)
    a = guarded.Arena(kern.dev)
    g = a.inp(c.g, "g", ld=(W + pad) * C)
    x, grids = _lift_inputs(a, c)
    part = a.out(rows, C * F + C, name="part")
    kern.lift_bwd(g.op, x.op, _opd(grids), part.op, c.dims)
    a.check()                                                     # every row is written, those of blocks without a data row included
    p = part.get()
    _idle_rows_are_zero(c.name, p, B * T * H)
    name = f"{c.name} bwd [F={lift_instantiation(Cin, True)}] rows={rows}"
    t64, t32, tk = total(r64["bwd"]), total(r32["bwd"]), total(p)
    judge(f"{name} d weight", tk[:C * F].view(C, F), t64[:C * F].view(C, F), t32[:C * F].view(C, F), _ex(existing, "lift_bwd"))
    judge(f"{name} d bias", tk[C * F:], t64[C * F:], t32[C * F:], _ex(existing, "lift_bwd"))


# ================================================================================================ lift_feat (rpb_lift_feat: a mover)
# (B, T, H, W, Cin, pad, FW)
LIFT_FEAT_CASES = [(2, 2, 3, 3, 2, 2, 8), (1, 2, 2, 37, 2, 3, 8),  # the row-walking kernel: Wp = 5, and Wp = 40 (80 pieces per row)
                   (2, 2, 3, 5, 2, 2, 32),                         # the generic kernel at the headline width
                   (1, 2, 3, 5, 4, 2, 8), (1, 2, 2, 3, 28, 1, 32), # Cin + 4 == FW: every field is filled
                   (1, 2, 3, 5, 16, 2, 32), (2, 2, 3, 5, 3, 2, 8)]


def lift_feat_trip_dims(cus=MI355X_CUS):
    """B Tp Hp >= 32 CUs + 5 rows at Wp = 3: five waves of the row-walking kernel (4 waves x 8 CUs blocks) take a second row"""
    Hp = min(range(3, 24), key=lambda h: ceil_div(32 * cus + 5, h) * h)
    return (1, ceil_div(32 * cus + 5, Hp) - 1, Hp - 1, 2, 2, 1, 8)


def lift_feat(x, grids, dims, dt, ones=1.0):
    B, T, H, W, Cin, pad, FW = dims
    out = torch.zeros(B, T + pad, H + pad, W + pad, FW, dtype=dt)
    out[:, :T, :H, :W, :Cin + 3] = lift_feats(x, grids, dims, dt)
    out[:, :T, :H, :W, Cin + 3] = ones
    return out.view(-1, FW)


def lift_feat_case(B, T, H, W, Cin, pad, FW):
    g = _gen(62, B, T, H, W, Cin, pad, FW)
    dims = (B, T, H, W, Cin, pad, FW)
    x = _rn(g, B, T, H, W, Cin)
    grids = (torch.linspace(0.2, 1.0, T), torch.linspace(-1.0, -0.1, H), torch.linspace(0.3, 1.3, W))
    return Case(f"lift_feat B={B} T={T} H={H} W={W} Cin={Cin} pad={pad} FW={FW}", dict(dims=dims, x=x, grids=grids),
                lambda dt: dict(phi=lift_feat(x, grids, dims, dt)))


def run_lift_feat(kern, c, existing=None):
    B, T, H, W, Cin, pad, FW = c.dims
    a = guarded.Arena(kern.dev)
    x = a.inp(c.x, "x", ld=W * Cin)
    grids = tuple(a.inp(t, n) for t, n in zip(c.grids, ("grid_t", "grid_h", "grid_w")))
    out = a.out(B * (T + pad) * (H + pad) * (W + pad), FW, name="phi", ld=(W + pad) * FW)
    kern.lift_feat(x.op, _opd(grids), out.op, (B, T, H, W, Cin, 64, pad), FW)
    a.check()
    exact(c.name, out.get(), c.refs()[1]["phi"])                  # inputs, grid values, ones and zeros: moved, never computed


# ================================================================================================ feat_mix / feat_mix_wgrad / small_gemm
FEAT_MIX_CASES = [(C, Cin, B, M2) for C in (32, 64, 128) for Cin in (2, 3, 16) for (B, M2) in ((1, 2), (3, 10))]
FEAT_WGRAD_CASES = [(C, Cin, B, M2) for C in (32, 64, 128, 256) for Cin in (2, 16, 20) for (B, M2) in ((1, 1), (3, 5))]


def feat_mix_trip_case(cus=MI355X_CUS):
    """B M2 C / 4 >= 8 CUs x 256 + 5 at C = 64"""
    return (64, 2, 3, ceil_div(ceil_div(4 * (8 * cus * THREADS + 5), 64), 3))


def feat_wgrad_trip_cases(cus=MI355X_CUS):
    """B M2 = 2 CUs x (256 / C) + 3 rows: three row groups take a second trip"""
    return [(C, Cin, 1, 2 * cus * (THREADS // C) + 3) for C in (32, 64, 128, 256) for Cin in (2, 16, 20)]


def feat_nb(B, Cin):
    return 64 * ceil_div(B * Cin + 4, 64)


def feat_fields(Phi, B, Cin, dt):
    """[B][M2][Cin + 4]: the fields of sample b, then the four sample-independent ones"""
    M2 = Phi.shape[0]
    own = Phi[:, :B * Cin].to(dt).reshape(M2, B, Cin).transpose(0, 1)
    return torch.cat((own, Phi[:, B * Cin:B * Cin + 4].to(dt).expand(B, M2, 4)), -1)


def feat_mix(Phi, w0, b0, B, Cin, dt):
    return feat_fields(Phi, B, Cin, dt) @ torch.cat((w0.to(dt), b0.to(dt)[:, None]), 1).t()           # [B][M2][C]


def feat_mix_wgrad(G, Phi, B, Cin, C, rows, dt):
    """part[b][c][j] = sum over block b's (sample, row) pairs of G[.][c] phi_j; a block walks 256 / C pairs at a time"""
    per = torch.einsum("rc,rj->rcj", G.to(dt).view(-1, C), feat_fields(Phi, B, Cin, dt).reshape(-1, Cin + 4))
    return _part(per, THREADS // C, rows)


def feat_case(C, Cin, B, M2, cus=MI355X_CUS):
    g = _gen(63, C, Cin, B, M2)
    NB, F = feat_nb(B, Cin), Cin + 3
    Phi = torch.full((M2, NB), NAN)                               # the padding columns hold NaN: nobody reads them
    Phi[:, :B * Cin + 4] = _rn(g, M2, B * Cin + 4, shift=0.2)
    w0, b0 = _rn(g, C, F, scale=1 / math.sqrt(F)), _rn(g, C, scale=0.3, shift=1.0)
    # the incoming gradient carries a mixed copy of the fields: G^T phi is then a sum of correlated terms, not sqrt(n) noise around 0
    G = _rn(g, B * M2, C) + 0.7 * feat_fields(Phi, B, Cin, F32).reshape(B * M2, Cin + 4) @ _rn(g, Cin + 4, C, scale=1 / math.sqrt(Cin + 4))
    i = dict(dims=(C, Cin, B, M2), NB=NB, Phi=Phi, w0=w0, b0=b0, G=G, rows=feat_mix_wgrad_rows(cus))
    return Case(f"feat C={C} Cin={Cin} B={B} M2={M2}", i,
                lambda dt: dict(mix=feat_mix(Phi, w0, b0, B, Cin, dt), wgrad=feat_mix_wgrad(G, Phi, B, Cin, C, i["rows"], dt)))


def run_feat_mix(kern, c, existing=None):
    C, Cin, B, M2 = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    Phi, w0, b0 = a.inp(c.Phi, "Phi"), a.inp(c.w0, "w0"), a.inp(c.b0, "b0")
    Xh = a.out(B, M2, C, name="Xh")
    kern.feat_mix(Phi.op, w0.op, b0.op, Xh.op, B, M2, c.NB, Cin, C)
    a.check()
    judge(f"{c.name} feat_mix", Xh.get(), r64["mix"], r32["mix"], _ex(existing, "feat_mix"))


def run_feat_mix_wgrad(kern, c, existing=None):
    C, Cin, B, M2 = c.dims
    r64, r32 = c.refs()
    rows = kern.feat_mix_wgrad_rows()
    assert rows == c.rows, (rows, c.rows)
    a = guarded.Arena(kern.dev)
    G, Phi = a.inp(c.G, "G"), a.inp(c.Phi, "Phi")
    part = a.out(rows, C, Cin + 4, name="part", ld=C * (Cin + 4))
    kern.feat_mix_wgrad(G.op, Phi.op, part.op, B, M2, c.NB, Cin, C)
    a.check()                                                     # every partial row is written (B M2 = 1 leaves all blocks but one idle)
    p = part.get()
    _idle_rows_are_zero(c.name, p, ceil_div(B * M2, THREADS // C))
    judge(f"{c.name} feat_mix_wgrad rows={rows}", total(p), total(r64["wgrad"]), total(r32["wgrad"]), _ex(existing, "feat_mix_wgrad"))


# (name, M, N, K, a_rs, a_cs, b_rs, b_cs, ldo): the five call shapes of model/fno.py at C = 32, FW = 8, Cin = 2 (F = 5)
_C, _FW, _F = 32, 8, 5
SMALL_GEMM_SHAPES = [("wcomp = Wc0 W0ext", _C, _FW, _C, _C, 1, _FW, 1, _FW),
                     ("d Wc0 = Mgf W0ext^T", _C, _C, _FW, _C, 1, 1, _FW, _C),
                     ("Wc0^T Mgf[:, :F+1]", _C, _F + 1, _C, 1, _C, _C, 1, _F + 1),
                     ("d fc0.weight += Wc0^T Mgf", _C, _F, _C, 1, _C, _F, 1, _F),
                     ("d fc0.bias += Wc0^T mgf", _C, 1, _C, 1, _C, 1, 1, 1),           # M N = 32 < 256 threads
                     ("K = 1", 7, 5, 1, 1, 1, 5, 1, 5)]
SMALL_GEMM_CASES = [s + (extra, acc) for s in SMALL_GEMM_SHAPES for extra in (0, 3) for acc in (False, True)]


def small_gemm(A, Bm, old, shape, dt):
    """fp64 accumulation, rounded once; then the fp32 add of the accumulating launch"""
    M, N, K, a_rs, a_cs, b_rs, b_cs = shape
    s = A.double().as_strided((M, K), (a_rs, a_cs)) @ Bm.double().as_strided((K, N), (b_rs, b_cs))
    s = s.float().to(dt) if dt == F32 else s
    return s if old is None else old.to(dt) + s


def _strided_buffer(g, rows, cols, rs, cs):
    """a buffer that holds a random [rows][cols] matrix at strides (rs, cs) and NaN everywhere else"""
    buf = torch.full(((rows - 1) * rs + (cols - 1) * cs + 1,), NAN)
    buf.as_strided((rows, cols), (rs, cs))[:] = _rn(g, rows, cols, shift=0.2)
    return buf


def small_gemm_case(name, M, N, K, a_rs, a_cs, b_rs, b_cs, ldo, extra, acc):
    g = _gen(64, M, N, K, a_rs, a_cs, b_rs, b_cs, ldo, extra, acc)
    A, Bm = _strided_buffer(g, M, K, a_rs, a_cs), _strided_buffer(g, K, N, b_rs, b_cs)
    old = _rn(g, M, N) if acc else None
    shape = (M, N, K, a_rs, a_cs, b_rs, b_cs)
    return Case(f"small_gemm {name} M={M} N={N} K={K} ldo={ldo + extra} acc={int(acc)}",
                dict(shape=shape, ldo=ldo + extra, A=A, Bm=Bm, old=old), lambda dt: dict(out=small_gemm(A, Bm, old, shape, dt)))


def run_small_gemm(kern, c, existing=None):
    M, N, K, a_rs, a_cs, b_rs, b_cs = c.shape
    r64, r32 = c.refs()
    ldo, n = c.ldo, (M - 1) * c.ldo + N
    a = guarded.Arena(kern.dev)
    A, Bm = a.inp(c.A, "A"), a.inp(c.Bm, "B")
    gaps = torch.ones(n, dtype=torch.bool)
    gaps.as_strided((M, N), (ldo, 1))[:] = False
    if c.old is None:
        out = a.out(n, name="out", ld=ldo, unwritten=gaps)
    else:
        pre = _rn(_gen(65, M, N, ldo), n)                          # the gaps of the in/out operand: preloaded, and bit-identical afterwards
        pre.as_strided((M, N), (ldo, 1))[:] = c.old
        out = a.inout(pre, "out", ld=ldo)
    kern.small_gemm(A.op, Bm.op, out.op, M, N, K, a_rs, a_cs, b_rs, b_cs, ldo, c.old is not None)
    a.check()
    got = out.get().reshape(-1)
    if c.old is not None and gaps.any():
        exact(f"{c.name} gaps", got[gaps], pre[gaps])
    judge(c.name, got.as_strided((M, N), (ldo, 1)), r64["out"], r32["out"], _ex(existing, "small_gemm"))


# ================================================================================================ cell BatchNorm
BN_C = [32, 64, 128]


def bn_ncells(C, cus=MI355X_CUS):
    """1 cell, 257 cells, and 8 CUs x (1024 / C) + 5: five cells past one trip of the 8-blocks-per-CU grids (a thread owns 4 channels)"""
    return [1, 257, 8 * cus * (1024 // C) + 5]


def bn_shat_z(s, stat, dt):
    mean, invstd, gamma, beta = (t.to(dt) for t in stat)
    sh = (s.to(dt) - mean) * invstd
    return sh, sh * gamma + beta


def bn_act(s, stat, gelu, dt):
    z = bn_shat_z(s, stat, dt)[1]
    return torch.nn.functional.gelu(z) if gelu else z


def bn_gz(s, gy, stat, gelu, dt):
    sh, z = bn_shat_z(s, stat, dt)
    return (gy.to(dt) * gelu_grad(z) if gelu else gy.to(dt)), sh


def bn_bwd_reduce(s, gy, stat, gelu, rows, dt, sums_of_s=False):
    """part[b] = (sum gz | sum gz shat) over block b's cells; a block walks 1024 / C cells at a time"""
    gz, sh = bn_gz(s, gy, stat, gelu, dt)
    second = gz * (s.to(dt) if sums_of_s else sh)                 # sums_of_s: the host test's wrong term
    return _part(torch.cat((gz, second), 1), 1024 // s.shape[1], rows)


def bn_bwd_apply(s, gy, stat, sums, count, gelu, dt, no_shat_term=False):
    gz, sh = bn_gz(s, gy, stat, gelu, dt)
    C = s.shape[1]
    ic = f32(1.0 / count) if dt == F32 else 1.0 / count           # the launcher hands the kernel (float)(1 / count)
    m1, m2 = sums[:C].to(dt) * ic, sums[C:].to(dt) * ic
    return stat[2].to(dt) * stat[1].to(dt) * (gz - m1 - (0 if no_shat_term else sh * m2))


def bn_case(C, ncell, gelu, cus=MI355X_CUS):
    g = _gen(66, C, ncell, gelu)
    s, stat = _rn(g, ncell, C, scale=1.5, shift=0.3), _stat(g, C)
    sh = (s - stat[0]) * stat[1]
    gy = _rn(g, ncell, C) + 0.5 * sh + 0.3                         # sum gz and sum gz shat: sums of terms of one sign mostly
    gz, sh64 = bn_gz(s, gy, stat, gelu, F64)
    sums = torch.cat((gz.sum(0), (gz * sh64).sum(0))).float()     # what the trainer's reduction hands bn_bwd_apply
    i = dict(dims=(C, ncell), gelu=gelu, s=s, gy=gy, stat=stat, sums=sums, rows=bn_bwd_rows(cus))
    return Case(f"bn C={C} ncell={ncell} gelu={int(gelu)}", i,
                lambda dt: dict(act=bn_act(s, stat, gelu, dt), reduce=bn_bwd_reduce(s, gy, stat, gelu, i["rows"], dt),
                                apply=bn_bwd_apply(s, gy, stat, sums, ncell, gelu, dt)))


def run_bn_act_fwd(kern, c, existing=None):
    C, ncell = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    s, st = a.inp(c.s, "s"), _ops_of(a, c.stat, STAT_NAMES)
    y = a.out(ncell, C, name="y")
    kern.bn_act_fwd(s.op, _opd(st), y.op, ncell, C, c.gelu)
    a.check()
    judge(f"{c.name} bn_act_fwd", y.get(), r64["act"], r32["act"], _ex(existing, "bn_act_fwd"))


def run_bn_bwd_reduce(kern, c, existing=None):
    C, ncell = c.dims
    r64, r32 = c.refs()
    rows = kern.bn_bwd_rows()
    assert rows == c.rows, (rows, c.rows)
    a = guarded.Arena(kern.dev)
    s, gy, st = a.inp(c.s, "s"), a.inp(c.gy, "gy"), _ops_of(a, c.stat, STAT_NAMES)
    part = a.out(rows, 2 * C, name="part")
    kern.bn_bwd_reduce(s.op, gy.op, _opd(st), part.op, ncell, C, c.gelu)
    a.check()                                                     # every partial row is written
    p = part.get()
    _idle_rows_are_zero(c.name, p, ceil_div(ncell, 1024 // C))
    t64, t32, tk = total(r64["reduce"]), total(r32["reduce"]), total(p)
    for j, what in enumerate(("sum gz", "sum gz*shat")):
        judge(f"{c.name} bn_bwd_reduce {what} rows={rows}", tk[j * C:(j + 1) * C], t64[j * C:(j + 1) * C], t32[j * C:(j + 1) * C],
              _ex(existing, "bn_bwd_reduce"))


def run_bn_bwd_apply(kern, c, existing=None):
    C, ncell = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    s, gy, st, sums = a.inp(c.s, "s"), a.inp(c.gy, "gy"), _ops_of(a, c.stat, STAT_NAMES), a.inp(c.sums, "sums")
    gs = a.out(ncell, C, name="gs")
    kern.bn_bwd_apply(s.op, gy.op, _opd(st), sums.op, ncell, gs.op, ncell, C, c.gelu)
    a.check()
    judge(f"{c.name} bn_bwd_apply", gs.get(), r64["apply"], r32["apply"], _ex(existing, "bn_bwd_apply"))


# ---- bn_finalize / bn_eval_prep
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
# (C, count, variant): C = 65 needs a second 64-thread block and has a tail; count = 1 is the branch without the unbiased-variance factor
BN_FINALIZE_CASES = [(32, 5000, ""), (64, 5000, ""), (128, 5000, ""), (65, 5000, ""), (64, 1, ""), (64, 5000, "constant channel"),
                     (64, 5000, "no running statistics")]


def bn_finalize(sums, count, rmean, rvar, dt, normalise_unbiased=False):
    """fp64 throughout, as the kernel; rounded once on the store.  eps and momentum as the ABI receives them"""
    eps, mom = f32(BN_EPS), f32(BN_MOMENTUM)
    C = sums.numel() // 2
    m = sums[:C] / count
    var = (sums[C:] / count - m * m).clamp_min(0.0)
    unb = var * count / (count - 1.0) if count > 1 else var
    r = dict(mean=m.to(dt), invstd=(1.0 / torch.sqrt((unb if normalise_unbiased else var) + eps)).to(dt))
    if rmean is not None:
        r["rmean"] = ((1.0 - mom) * rmean.double() + mom * m).to(dt)
        r["rvar"] = ((1.0 - mom) * rvar.double() + mom * unb).to(dt)
    return r


def bn_finalize_case(C, count, variant):
    g = _gen(67, C, count, len(variant))
    s = _rn(g, count, C, scale=1.7, shift=0.4)
    if variant == "constant channel":
        s[:, 3] = 1.7
    sums = torch.cat((s.double().sum(0), (s.double() ** 2).sum(0)))
    if variant == "constant channel":                             # ... whose sum of squares came out 1e-7 low, as a rounded sum may:
        sums[C + 3] *= 1 - 1e-7                                   # E[s^2] - mean^2 = -2.9e-7 against eps = 1e-5; the clamp makes it 0
        assert float(sums[C + 3] / count - (sums[3] / count) ** 2) < -1e-7
    rmean, rvar = (None, None) if variant == "no running statistics" else (_rn(g, C, scale=0.5), torch.rand(C, generator=g) + 0.5)
    i = dict(dims=(C, count), s=s, sums=sums, rmean=rmean, rvar=rvar)
    return Case(f"bn_finalize C={C} count={count} {variant}".rstrip(), i, lambda dt: bn_finalize(sums, float(count), rmean, rvar, dt))


def run_bn_finalize(kern, c, existing=None):
    C, count = c.dims
    r64, r32 = c.refs()
    a64 = guarded.Arena(kern.dev, dtype=F64)
    sums = a64.inp(c.sums, "sums", ld=C)
    a = guarded.Arena(kern.dev)
    mean, invstd = a.out(C, name="mean"), a.out(C, name="invstd")
    run = None if c.rmean is None else (a.inout(c.rmean, "running_mean"), a.inout(c.rvar, "running_var"))
    kern.bn_finalize(sums.tensor(), float(count), BN_EPS, BN_MOMENTUM, mean.op, invstd.op, _op(run and run[0]), _op(run and run[1]), C)
    a64.check()
    a.check()
    outs = dict(mean=mean, invstd=invstd, **(dict(rmean=run[0], rvar=run[1]) if run else {}))
    for k, o in outs.items():                                     # the running statistics are outputs too
        judge(f"{c.name} {k}", o.get(), r64[k], r32[k], _ex(existing, "bn_finalize"))


def bn_eval_prep_case(C):
    rvar = torch.rand(C, generator=_gen(68, C)) + 0.05
    return Case(f"bn_eval_prep C={C}", dict(C=C, rvar=rvar), lambda dt: dict(invstd=1.0 / torch.sqrt(rvar.to(dt) + f32(BN_EPS))))


def run_bn_eval_prep(kern, c, existing=None):
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    rvar, invstd = a.inp(c.rvar, "running_var"), a.out(c.C, name="invstd")
    kern.bn_eval_prep(rvar.op, BN_EPS, invstd.op, c.C)
    a.check()
    judge(c.name, invstd.get(), r64["invstd"], r32["invstd"], _ex(existing, "bn_eval_prep"))


# ================================================================================================ mse
MSE_OUTPUTS = [(True, True), (True, False), (False, True), (False, False)]            # (elem, gout) non-null


def mse_sizes(cus=MI355X_CUS):
    """1, 255, and two whole trips of the 4-blocks-per-CU grid + 257 elements"""
    return [1, 255, 2 * 4 * cus * THREADS + 257]


def mse(pred, tgt, gscale, rows, dt, factor=2.0):
    d = pred.to(dt) - tgt.to(dt)
    e = d * d
    return dict(elem=e, gout=factor * d * f32(gscale), part=_part(e.view(-1, 1), THREADS, rows).view(-1))


def mse_case(n, cus=MI355X_CUS):
    g = _gen(69, n)
    pred, tgt = _rn(g, n), _rn(g, n, scale=0.8, shift=0.1)
    i = dict(n=n, pred=pred, tgt=tgt, gscale=1.0 / n, rows=mse_rows(cus))
    return Case(f"mse n={n}", i, lambda dt: mse(pred, tgt, i["gscale"], i["rows"], dt))


def run_mse(kern, c, with_elem, with_gout, existing=None):
    r64, r32 = c.refs()
    rows = kern.mse_rows()
    assert rows == c.rows, (rows, c.rows)
    a = guarded.Arena(kern.dev)
    pred, tgt = a.inp(c.pred, "pred"), a.inp(c.tgt, "target")
    elem = a.out(c.n, name="elem") if with_elem else None
    gout = a.out(c.n, name="gout") if with_gout else None
    part = a.out(rows, name="part")
    kern.mse(pred.op, tgt.op, _op(elem), _op(gout), part.op, c.n, c.gscale)
    a.check()                                                     # every one of the partials is written
    name = f"{c.name} elem={int(with_elem)} gout={int(with_gout)}"
    p = part.get()
    _idle_rows_are_zero(name, p, ceil_div(c.n, THREADS))
    if elem:
        judge(f"{name} elem", elem.get(), r64["elem"], r32["elem"], _ex(existing, "mse"))
    if gout:
        judge(f"{name} gout", gout.get(), r64["gout"], r32["gout"], _ex(existing, "mse"))
    judge(f"{name} sum rows={rows}", total(p), total(r64["part"]), total(r32["part"]), _ex(existing, "mse"))


# ================================================================================================ Adam
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, gscale=0.25)
ADAM_STEPS = [1, 2, 1000, 100000]
ADAM_REGIMES = ["unit", "tiny"]                                    # |g| ~ 1, and |g| ~ 1e-7: eps is 10 % of the denominator


def adam_sizes(cus=MI355X_CUS):
    """1, 3 (tail only), 4 (one float4 group), 1003, and four float4 trips of the 8-blocks-per-CU grid + 23: a second trip with a tail"""
    return [1, 3, 4, 1003, 4 * (8 * cus * THREADS) + 23]


def adam_runs(cus=MI355X_CUS):
    """(n, step, regime): every size at two (step, regime) pairs, every (step, regime) pair at n = 1003"""
    sizes = adam_sizes(cus)
    runs = [(n, 2, "unit") for n in sizes] + [(n, 1000, "tiny") for n in sizes]
    return runs + [(1003, st, rg) for st in ADAM_STEPS for rg in ADAM_REGIMES if (1003, st, rg) not in runs]


def adam_update(p, g, m, v, step, dt, lr=None, eps_inside_sqrt=False):
    """one rpb_adam_step from the state (p, m, v): the hyperparameters rounded to fp32 as the ABI receives them, the bias corrections in
    fp64 and the two factors made of them handed to the kernel as fp32 numbers"""
    lr, b1, b2, eps, gscale = (f32(x) for x in (ADAM["lr"] if lr is None else lr, ADAM["beta1"], ADAM["beta2"], ADAM["eps"], ADAM["gscale"]))
    step_size, isb2 = lr / (1.0 - b1 ** step), 1.0 / math.sqrt(1.0 - b2 ** step)
    if dt == F32:
        step_size, isb2 = f32(step_size), f32(isb2)
    p, g, m, v = (t.to(dt) for t in (p, g, m, v))
    gk = g * gscale
    m = b1 * m + (1.0 - b1) * gk
    v = b2 * v + (1.0 - b2) * gk * gk
    denom = torch.sqrt(v + eps * eps) * isb2 if eps_inside_sqrt else torch.sqrt(v) * isb2 + eps    # (the host test's misplaced eps)
    return p - step_size * (m / denom), m, v


def adam_state(g, n, step, regime):
    """a state (p, grad, m, v) mid-training: |p| <= lr, so that the update is not lost in p's rounding; in the tiny regime sqrt(v) /
    sqrt(bc2) is about 9e-8, so that eps = 1e-8 is 10 % of the denominator"""
    gs = 4e-7 if regime == "tiny" else 1.0
    sc = gs * ADAM["gscale"]
    isb2 = 1.0 / math.sqrt(1.0 - f32(ADAM["beta2"]) ** step)
    grad, m = _rn(g, n, scale=gs), _rn(g, n, scale=sc)
    v = (0.9 * sc / isb2 if regime == "tiny" else sc) ** 2 * (0.5 + torch.rand(n, generator=g))
    p = (2 * torch.rand(n, generator=g) - 1) * ADAM["lr"]
    return p, grad, m, v


def adam_case(n, step, regime):
    p, grad, m, v = adam_state(_gen(70, n, step, len(regime)), n, step, regime)

    def ref(dt):
        pn, mn, vn = adam_update(p, grad, m, v, step, dt)
        return dict(update=pn - p.to(dt), m=mn, v=vn)
    return Case(f"adam n={n} step={step} |g|~{regime}", dict(n=n, step=step, p=p, g=grad, m=m, v=v), ref)


def _adam_args(step, lr=None):
    return (ADAM["lr"] if lr is None else lr, ADAM["beta1"], ADAM["beta2"], ADAM["eps"], step, ADAM["gscale"])


def _judge_adam(name, c, p, m, v, r64, r32, existing):
    """the update p_out - p_in (p itself is ~100 updates large and would hide an error in one), m and v"""
    judge(f"{name} update", p.get().double() - c.p.double(), r64["update"], r32["update"], _ex(existing, "adam_step"))
    judge(f"{name} m", m.get(), r64["m"], r32["m"], _ex(existing, "adam_step"))
    judge(f"{name} v", v.get(), r64["v"], r32["v"], _ex(existing, "adam_step"))


def run_adam(kern, c, existing=None):
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    p, g, m, v = a.inout(c.p, "p"), a.inp(c.g, "g"), a.inout(c.m, "m"), a.inout(c.v, "v")
    kern.adam_step(p.op, g.op, m.op, v.op, c.n, *_adam_args(c.step))
    a.check()
    _judge_adam(c.name, c, p, m, v, r64, r32, existing)


ADAM_CHAIN_LR = [1e-2 * 0.7 ** k for k in (1, 2, 3)]


def adam_chain_case(n=1003):
    """three steps from zero state with a changing learning rate, as a trainer's first three"""
    g = _gen(71, n)
    p = (2 * torch.rand(n, generator=g) - 1) * ADAM_CHAIN_LR[-1]
    grads = [_rn(g, n) for _ in ADAM_CHAIN_LR]

    def ref(dt):
        pn, mn, vn = p, torch.zeros(n), torch.zeros(n)
        for k, lr in enumerate(ADAM_CHAIN_LR):
            pn, mn, vn = adam_update(pn, grads[k], mn, vn, k + 1, dt, lr=lr)
        return dict(update=pn - p.to(dt), m=mn, v=vn)
    return Case(f"adam chain n={n}", dict(n=n, p=p, grads=grads), ref)


def run_adam_chain(kern, c, existing=None):
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    p, m, v = a.inout(c.p, "p"), a.inout(torch.zeros(c.n), "m"), a.inout(torch.zeros(c.n), "v")
    gs = [a.inp(t, f"g{k}") for k, t in enumerate(c.grads)]
    for k, lr in enumerate(ADAM_CHAIN_LR):
        kern.adam_step(p.op, gs[k].op, m.op, v.op, c.n, *_adam_args(k + 1, lr))
    a.check()
    _judge_adam(c.name, c, p, m, v, r64, r32, existing)


# ---- the ranged launch: (arena elements, [(first element, count)]); starts and counts are multiples of 4
def adam_range_tables(cus=MI355X_CUS):
    trip4 = 8 * cus * THREADS                                      # float4 groups of one grid trip
    half = 4 * (trip4 // 2)
    return {"nr = 1": (64, [(8, 24)]),
            "single float4 groups": (64, [(0, 4), (12, 4), (40, 4), (60, 4)]),
            "adjacent ranges": (96, [(4, 8), (12, 4), (16, 20), (48, 4), (52, 44)]),
            "nr = 257": (257 * 12, [(12 * i + 4 * (i % 2), 4 + 4 * (i % 3 == 0)) for i in range(257)]),      # the binary search
            "past a grid trip": (2 * half + 64, [(4, half), (half + 12, half + 36)])}


def owned_table(pieces):
    """DataParallel.owned_table, restated: [nr][2] int64 (first element, float4 groups before the range), and the element total"""
    rows, pre = [], 0
    for first, n in pieces:
        assert first % 4 == 0 and n % 4 == 0
        rows.append((first, pre))
        pre += n // 4
    return torch.tensor(rows, dtype=torch.int64), len(rows), 4 * pre


def adam_ranges_case(name, cus=MI355X_CUS):
    N, pieces = adam_range_tables(cus)[name]
    assert all(a + n <= b for (a, n), (b, _) in zip(pieces, pieces[1:])) and pieces[-1][0] + pieces[-1][1] <= N
    step = 7
    p, grad, m, v = adam_state(_gen(72, N, len(pieces)), N, step, "unit")
    inside = torch.zeros(N, dtype=torch.bool)
    for first, n in pieces:
        inside[first:first + n] = True

    def ref(dt):
        pn, mn, vn = adam_update(p[inside], grad[inside], m[inside], v[inside], step, dt)
        return dict(update=pn - p[inside].to(dt), m=mn, v=vn)
    return Case(f"adam ranges {name}", dict(N=N, pieces=pieces, step=step, inside=inside, p=p, g=grad, m=m, v=v), ref)


def run_adam_ranges(kern, c, existing=None):
    """the ranged launch against the plain one over the same elements, bit for bit (the kernel promises it: one update function, no FMA
    contraction); the elements outside the ranges bit-identical to their preload; and the packed plain launch against fp64"""
    r64, r32 = c.refs()
    tab, nr, tot = owned_table(c.pieces)
    at = guarded.Arena(kern.dev, dtype=torch.int64, fill=0)        # a table row read past the end would name element 0: a wrong update
    tb = at.inp(tab, "table", ld=2)
    a = guarded.Arena(kern.dev)
    p, g, m, v = a.inout(c.p, "p"), a.inp(c.g, "g"), a.inout(c.m, "m"), a.inout(c.v, "v")
    kern.adam_step_ranges(p.op, g.op, m.op, v.op, tb.tensor(), nr, tot, *_adam_args(c.step))
    at.check()
    a.check()
    ins = c.inside
    b = guarded.Arena(kern.dev)                                   # the plain launch over the packed elements of the ranges
    pp, pg, pm, pv = b.inout(c.p[ins], "p"), b.inp(c.g[ins], "g"), b.inout(c.m[ins], "m"), b.inout(c.v[ins], "v")
    kern.adam_step(pp.op, pg.op, pm.op, pv.op, tot, *_adam_args(c.step))
    b.check()
    for what, ranged, plain, pre in (("p", p, pp, c.p), ("m", m, pm, c.m), ("v", v, pv, c.v)):
        got = ranged.get()
        exact(f"{c.name} {what} inside the ranges against rpb_adam_step", got[ins], plain.get())
        exact(f"{c.name} {what} outside the ranges", got[~ins], pre[~ins])
    packed = Case(c.name, dict(p=c.p[ins]), None)
    _judge_adam(f"{c.name} (plain launch, packed)", packed, pp, pm, pv, r64, r32, existing)


# ================================================================================================ normaliser affines
AFFINE_STATS = [(True, True), (True, False), (False, True), (False, False)]           # (target pair, input pair) non-null


def rollout_shapes(cus=MI355X_CUS):
    """(ncell, Cp, Cx); the last: 7 cells past one trip of the grid at 5 channels per cell"""
    return [(1, 1, 0), (999, 3, 2), (ceil_div(8 * cus * THREADS, 5) + 7, 3, 2)]


def rollout_affine(pred, para, st_t, st_i, dt, divide_by_std_t=False):
    t = pred.to(dt)
    if st_t is not None:
        t = (t / st_t[1].to(dt) if divide_by_std_t else t * st_t[1].to(dt)) + st_t[0].to(dt)
    if para is not None:
        t = torch.cat((t, para.to(dt)), -1)
    return t if st_i is None else (t - st_i[0].to(dt)) / st_i[1].to(dt)


def rollout_case(ncell, Cp, Cx, with_t, with_i):
    g = _gen(73, ncell, Cp, Cx, with_t, with_i)
    pred, para = _rn(g, ncell, Cp), (_rn(g, ncell, Cx) if Cx else None)
    st_t = (_rn(g, Cp), torch.rand(Cp, generator=g) + 0.5) if with_t else None
    st_i = (_rn(g, Cp + Cx), torch.rand(Cp + Cx, generator=g) + 0.5) if with_i else None
    return Case(f"rollout_affine ncell={ncell} Cp={Cp} Cx={Cx} target stats={int(with_t)} input stats={int(with_i)}",
                dict(dims=(ncell, Cp, Cx), pred=pred, para=para, st_t=st_t, st_i=st_i),
                lambda dt: dict(out=rollout_affine(pred, para, st_t, st_i, dt)))


def run_rollout_affine(kern, c, existing=None):
    ncell, Cp, Cx = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    pred, para = a.inp(c.pred, "pred"), (a.inp(c.para, "para") if Cx else None)
    st_t = None if c.st_t is None else _ops_of(a, c.st_t, ("mean_t", "std_t"))
    st_i = None if c.st_i is None else _ops_of(a, c.st_i, ("mean_i", "std_i"))
    out = a.out(ncell, Cp + Cx, name="out")
    kern.rollout_affine(pred.op, _op(para), out.op, ncell, Cp, Cx, *(_opd(st_t) or (None, None)), *(_opd(st_i) or (None, None)))
    a.check()
    if st_t is None and st_i is None:
        exact(c.name, out.get(), r32["out"])                      # nothing to compute: a copy and a concatenation
    else:
        judge(c.name, out.get(), r64["out"], r32["out"], _ex(existing, "rollout_affine"))


def channel_affine_cases(cus=MI355X_CUS):
    """(n, C, inverse); the last two: 5 elements past one trip of the grid"""
    return [(350 * C, C, inv) for C in (1, 3, 16) for inv in (False, True)] + [(8 * cus * THREADS + 5, 3, inv) for inv in (False, True)]


def channel_affine(x, C, mean, std, inverse, dt):
    n = x.numel()
    ch = torch.arange(n) % C
    m, s = mean.to(dt)[ch], std.to(dt)[ch]
    return x.to(dt) * s + m if inverse else (x.to(dt) - m) / s


def channel_affine_case(n, C, inverse):
    g = _gen(74, n, C, inverse)
    x, mean, std = _rn(g, n), _rn(g, C), torch.rand(C, generator=g) + 0.5
    return Case(f"channel_affine n={n} C={C} inverse={int(inverse)}", dict(dims=(n, C), inverse=inverse, x=x, mean=mean, std=std),
                lambda dt: dict(out=channel_affine(x, C, mean, std, inverse, dt)))


def run_channel_affine(kern, c, existing=None):
    n, C = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    x, mean, std = a.inp(c.x, "in"), a.inp(c.mean, "mean"), a.inp(c.std, "std")
    out = a.out(n, name="out")
    kern.channel_affine(x.op, out.op, n, C, mean.op, std.op, c.inverse)
    a.check()
    judge(c.name, out.get(), r64["out"], r32["out"], _ex(existing, "channel_affine"))


# ================================================================================================ small movers
MUL_SIZES = [4, 77 * 64]


def mul_case(n):
    g = _gen(75, n)
    x, y = _rn(g, n), _rn(g, n)
    return Case(f"mul n={n}", dict(n=n, x=x, y=y), lambda dt: dict(out=x.to(dt) * y.to(dt)))


def run_mul(kern, c, existing=None):
    a = guarded.Arena(kern.dev)
    x, y, out = a.inp(c.x, "a"), a.inp(c.y, "b"), a.out(c.n, name="out")
    kern.mul(x.op, y.op, out.op, c.n)
    a.check()
    exact(c.name, out.get(), c.refs()[1]["out"])                  # one correctly rounded fp32 product per element


PAIR_PACK_CASES = [(2, 37, 15, 2), (2, 37, 15, 0), (1, 5, 1, 0), (3, 300, 4, 2)]                # (B, ntok, Cl, n_para)


def pair_pack(num, real, para, st, dt, para_offset=0):
    mean_in, mean_tgt, std_in, std_tgt = (t.to(dt) for t in st)
    B, ntok, Cl = num.shape
    x = num.to(dt)
    if para is not None:
        x = torch.cat((x, para.to(dt).roll(para_offset, 1)[:, None, :].expand(B, ntok, para.shape[1])), -1)
    return dict(inp=(x - mean_in) / std_in, tgt=((real.to(dt) - mean_tgt) / std_tgt)[..., None])


def pair_pack_case(B, ntok, Cl, n_para):
    g = _gen(76, B, ntok, Cl, n_para)
    num, real, para = _rn(g, B, ntok, Cl), _rn(g, B, ntok), (_rn(g, B, n_para) if n_para else None)
    st = (_rn(g, Cl + n_para), _rn(g, 1), torch.rand(Cl + n_para, generator=g) + 0.5, torch.rand(1, generator=g) + 0.5)
    return Case(f"pair_pack B={B} ntok={ntok} Cl={Cl} n_para={n_para}", dict(dims=(B, ntok, Cl, n_para), num=num, real=real, para=para, st=st),
                lambda dt: pair_pack(num, real, para, st, dt))


PACK_STATS = ("mean_in", "mean_tgt", "std_in", "std_tgt")


def run_pair_pack(kern, c, existing=None):
    B, ntok, Cl, n_para = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    num, real, para = a.inp(c.num, "num"), a.inp(c.real, "real"), (a.inp(c.para, "para") if n_para else None)
    st = _ops_of(a, c.st, PACK_STATS)
    inp, tgt = a.out(B, ntok, Cl + n_para, name="inp"), a.out(B, ntok, 1, name="tgt")
    kern.pair_pack(num.op, real.op, _op(para), inp.op, tgt.op, B, ntok, Cl, n_para, *_opd(st))
    a.check()
    judge(f"{c.name} inp", inp.get(), r64["inp"], r32["inp"], _ex(existing, "pair_pack"))
    judge(f"{c.name} tgt", tgt.get(), r64["tgt"], r32["tgt"], _ex(existing, "pair_pack"))


# (name, B, horizon, in_step, Hf, Wf, sub_s, rows_subsampled, n_para, Cp, Cl, cleared flags [(sample, flag)], unit statistics)
# Hf = the rows PRESENT in the staged slab (with rows_subsampled the host kept every sub_s-th row already)
WINDOW_PACK_CASES = [("planar only", 2, 4, 2, 5, 7, 1, False, 0, 3, 0, [], False),
                     ("channels-last block, sub_s = 3", 2, 3, 1, 7, 8, 3, False, 3, 1, 15, [], False),
                     ("rows subsampled by the host", 2, 3, 1, 3, 8, 3, True, 3, 1, 15, [], False),
                     ("a planar flag cleared", 2, 3, 2, 7, 8, 3, False, 1, 3, 0, [(1, 2), (0, 0)], True),
                     ("flags[3] cleared", 2, 3, 1, 5, 4, 1, False, 0, 1, 15, [(0, 3)], True)]


def window_pack(planar, cl, flags, st, spec, dt, para_offset=0):
    name, B, horizon, in_step, Hf, Wf, sub_s, rows_sub, n_para, Cp, Cl, cleared, unit = spec
    mean_in, mean_tgt, std_in, std_tgt = (t.to(dt) for t in st)
    sub_h = 1 if rows_sub else sub_s
    on = flags[:, :Cp] != 0
    cells = torch.where(on[:, :, None, None, None], planar.to(dt)[:, :, :, ::sub_h, ::sub_s], torch.zeros((), dtype=dt))
    full = cells.permute(0, 2, 3, 4, 1)                           # [B][horizon][H][W][Cp]
    if Cl:
        block = torch.where((flags[:, 3] != 0)[:, None, None, None, None], cl.to(dt)[:, :, ::sub_h, ::sub_s], torch.zeros((), dtype=dt))
        full = torch.cat((full, block), -1)
    H, W = full.shape[2], full.shape[3]
    inp = full[:, :in_step]
    if n_para:
        par = flags[:, 4 + para_offset:4 + para_offset + n_para].to(dt)
        inp = torch.cat((inp, par[:, None, None, None, :].expand(B, in_step, H, W, n_para)), -1)
    return dict(inp=(inp - mean_in) / std_in, tgt=(full[:, in_step:] - mean_tgt) / std_tgt)


def window_pack_case(spec):
    name, B, horizon, in_step, Hf, Wf, sub_s, rows_sub, n_para, Cp, Cl, cleared, unit = spec
    g = _gen(77, B, horizon, in_step, Hf, Wf, sub_s, rows_sub, n_para, Cp, Cl, len(cleared))
    planar, cl = _rn(g, B, Cp, horizon, Hf, Wf), (_rn(g, B, horizon, Hf, Wf, Cl) if Cl else None)
    flags = torch.ones(B, 4 + max(n_para, 1))
    flags[:, 4:] = _rn(g, B, max(n_para, 1))
    for b, f in cleared:                                          # what a cleared flag switches off holds NaN: it may be loaded, not used
        flags[b, f] = 0.0
        if f < 3:
            planar[b, f] = NAN
        else:
            cl[b] = NAN
    Ci, Ct = Cp + Cl + n_para, Cp + Cl
    if unit:                                                      # mean 0, std 1: the zero fill comes out as exact zeros
        st = (torch.zeros(Ci), torch.zeros(Ct), torch.ones(Ci), torch.ones(Ct))
    else:
        st = (_rn(g, Ci), _rn(g, Ct), torch.rand(Ci, generator=g) + 0.5, torch.rand(Ct, generator=g) + 0.5)
    return Case(f"window_pack {name}", dict(spec=spec, planar=planar, cl=cl, flags=flags, st=st),
                lambda dt: window_pack(planar, cl, flags, st, spec, dt))


def run_window_pack(kern, c, existing=None):
    name, B, horizon, in_step, Hf, Wf, sub_s, rows_sub, n_para, Cp, Cl, cleared, unit = c.spec
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    planar, cl, flags = a.inp(c.planar, "planar"), (a.inp(c.cl, "cl") if Cl else None), a.inp(c.flags, "flags")
    st = _ops_of(a, c.st, PACK_STATS)
    inp, tgt = a.out(*r64["inp"].shape, name="inp"), a.out(*r64["tgt"].shape, name="tgt")
    kern.window_pack(planar.op, _op(cl), flags.op, inp.op, tgt.op, B, horizon, in_step, Hf, Wf, sub_s, n_para, Cp, Cl, *_opd(st), rows_sub)
    a.check()
    for what, o in (("inp", inp), ("tgt", tgt)):
        got = o.get()
        for b, f in cleared:
            chans = slice(f, f + 1) if f < 3 else slice(Cp, Cp + Cl)
            zero = got[b][..., chans]
            exact(f"{c.name} {what}: the zero fill of sample {b}, flag {f}", zero, torch.zeros_like(zero))
        judge(f"{c.name} {what}", got, r64[what], r32[what], _ex(existing, "window_pack"))


# ================================================================================================ reducers
# (rows, L, row_stride, col0, scale, accumulate): rows = 255 / 256 is the wide / tall switch; row_stride > L leaves gaps (NaN)
REDUCE_CASES = [(255, 20, 20, 0, 1.0, False), (256, 20, 20, 0, 1.0, False), (255, 130, 150, 11, 0.5, False), (256, 130, 150, 11, 0.5, False),
                (255, 70, 70, 0, 1.0, True), (256, 70, 96, 5, 2.0, True), (37, 20, 50, 11, 1.0, False)]
REDUCE_BATCHED_CASES = [(3, 255, 70, 70), (2, 256, 70, 96), (5, 4, 130, 130)]       # (nbatch, rows, L, row_stride)
REDUCE_GROUPED_ITEMS = [(255, 70, 70), (256, 1030, 1030), (37, 20, 50)]              # (rows, L, row_stride); L = 1030: a second block


def _gapped(g, rows, L, stride, col0=0):
    """[rows][stride] with a random [rows][L] block from column ``col0`` on and NaN everywhere else"""
    buf = torch.full((rows, stride), NAN)
    buf[:, col0:col0 + L] = _rn(g, rows, L, shift=0.3)
    return buf


def _once(v, dt):
    """an fp64 result as the kernel stores it: rounded once (the fp64 reference keeps it)"""
    return v.float() if dt == F32 else v


def reduce_rows(part, L, col0, scale, oldf, oldd, dt):
    """fp64 accumulation; the fp32 output rounded once (after the fp64 add of an accumulating launch)"""
    v = part[:, col0:col0 + L].double().sum(0) * scale
    f = v if oldf is None else oldf.double() + v
    return dict(f32=f.float() if dt == F32 else f, f64=v if oldd is None else oldd + v)


def reduce_case(rows, L, stride, col0, scale, acc):
    g = _gen(78, rows, L, stride, col0, acc)
    part = _gapped(g, rows, L, stride, col0)
    oldf, oldd = (_rn(g, L), _rn(g, L).double()) if acc else (None, None)
    return Case(f"reduce_partials rows={rows} L={L} stride={stride} col0={col0} scale={scale} acc={int(acc)}",
                dict(dims=(rows, L, stride, col0), scale=scale, part=part, oldf=oldf, oldd=oldd),
                lambda dt: reduce_rows(part, L, col0, scale, oldf, oldd, dt))


def run_reduce_partials(kern, c, existing=None):
    rows, L, stride, col0 = c.dims
    r64, r32 = c.refs()
    for outs in ("f32", "f64", "both"):
        a, ad = guarded.Arena(kern.dev), guarded.Arena(kern.dev, dtype=F64)
        part = a.inp(c.part, "part", ld=stride)
        of = od = None
        if outs != "f64":
            of = a.out(L, name="out_f32") if c.oldf is None else a.inout(c.oldf, "out_f32")
        if outs != "f32":
            od = ad.out(L, name="out_f64") if c.oldd is None else ad.inout(c.oldd, "out_f64")
        kern.reduce_partials(part.at(col0), rows, L, stride, _op(of), od.tensor() if od else None, c.scale, c.oldf is not None)
        a.check()
        if od:
            ad.check()
            judge(f"{c.name} [{outs}] fp64 output", od.get(), r64["f64"], r32["f64"], _ex(existing, "reduce_partials"))
        if of:
            judge(f"{c.name} [{outs}] fp32 output", of.get(), r64["f32"], r32["f32"], _ex(existing, "reduce_partials"))


def reduce_batched_case(nbatch, rows, L, stride):
    part = _gapped(_gen(79, nbatch, rows, L, stride), nbatch * rows, L, stride).view(nbatch, rows, stride)
    return Case(f"reduce_partials_batched nbatch={nbatch} rows={rows} L={L} stride={stride}", dict(dims=(nbatch, rows, L, stride), part=part),
                lambda dt: dict(out=_once(part[:, :, :L].double().sum(1), dt)))


def run_reduce_batched(kern, c, existing=None):
    nbatch, rows, L, stride = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    part, out = a.inp(c.part, "part", ld=stride), a.out(nbatch, L, name="out")
    kern.reduce_partials_batched(part.op, nbatch, rows, L, stride, rows * stride, out.op)
    a.check()
    judge(c.name, out.get(), r64["out"], r32["out"], _ex(existing, "reduce_partials"))


def reduce_grouped_case():
    parts = [_gapped(_gen(80, *it), *it) for it in REDUCE_GROUPED_ITEMS]
    return Case("reduce_partials_grouped " + " ".join(f"{r}x{L}/{s}" for r, L, s in REDUCE_GROUPED_ITEMS), dict(parts=parts),
                lambda dt: {str(k): _once(p[:, :L].double().sum(0), dt) for k, (p, (r, L, s)) in enumerate(zip(parts, REDUCE_GROUPED_ITEMS))})


def run_reduce_grouped(kern, c, existing=None):
    """items [n][6] int64: { part address, out address, rows, L, row_stride, first block of this item }; a block owns ``cols`` columns"""
    r64, r32 = c.refs()
    cols = kern.reduce_grouped_cols()
    assert cols == GROUPED_COLS, cols
    a = guarded.Arena(kern.dev)
    parts = [a.inp(p, f"part{k}", ld=s) for k, (p, (r, L, s)) in enumerate(zip(c.parts, REDUCE_GROUPED_ITEMS))]
    outs = [a.out(L, name=f"out{k}") for k, (r, L, s) in enumerate(REDUCE_GROUPED_ITEMS)]
    table, chunk0 = [], 0
    for p, o, (r, L, s) in zip(parts, outs, REDUCE_GROUPED_ITEMS):
        table.append((kern.addr(p), kern.addr(o), r, L, s, chunk0))
        chunk0 += ceil_div(L, cols)
    at = guarded.Arena(kern.dev, dtype=torch.int64, fill=0)
    tb = at.inp(torch.tensor(table, dtype=torch.int64), "items", ld=6)
    kern.reduce_partials_grouped(tb.tensor(), len(table), chunk0)
    at.check()
    a.check()
    for k, o in enumerate(outs):
        judge(f"{c.name} item {k}", o.get(), r64[str(k)], r32[str(k)], _ex(existing, "reduce_partials"))


# ================================================================================================ spectrum bins (rpb_spectrum_bin)
SPECTRUM_CASES = [(1, 64), (2, 3), (5, 320), (23, 64)]            # (R, NB); NB = 320: a thread owns two columns
SPECTRUM_RMAX = 64                                                 # the entry point's limit


def radial_bins(R, rounded=False):
    """bin of every (i, j, k) of the R^3 corner: floor(sqrt(i^2 + j^2 + k^2)), in integers"""
    i = torch.arange(R)
    n2 = (i[:, None, None] ** 2 + i[None, :, None] ** 2 + i[None, None, :] ** 2).reshape(-1)
    if rounded:                                                   # the host test's wrong term
        return torch.tensor([int(round(math.sqrt(v))) for v in n2.tolist()])
    return torch.tensor([math.isqrt(v) for v in n2.tolist()])


def spectrum_bin(Y, R, NB, dt, rounded=False):
    """out[r][n] = sum over the corner bins q with rad(q) == r of re^2 + im^2; bins with rad >= R are dropped"""
    power = (Y.to(dt).view(R ** 3, 2, NB) ** 2).sum(1)
    rad = radial_bins(R, rounded)
    keep = rad < R
    return torch.zeros(R, NB, dtype=dt).index_add_(0, rad[keep], power[keep])


def spectrum_case(R, NB):
    Y = _rn(_gen(81, R, NB), R, R, R, 2, NB)
    return Case(f"spectrum_bin R={R} NB={NB}", dict(dims=(R, NB), Y=Y), lambda dt: dict(out=spectrum_bin(Y, R, NB, dt)))


def run_spectrum_bin(kern, c, existing=None):
    R, NB = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    Y, out = a.inp(c.Y, "Y", ld=NB), a.out(R, NB, name="out")
    kern.spectrum_bin(Y.op, out.op, R, NB)
    a.check()
    judge(c.name, out.get(), r64["out"], r32["out"], _ex(existing, "spectrum_bin"))
