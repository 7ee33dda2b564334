"""TEST INFRASTRUCTURE ONLY -- the shapes, inputs and drivers of the per-kernel Galerkin Transformer tests, shared by
tests/test_gpu_galerkin_kernels.py (which runs the HIP kernels) and tests/test_galerkin_kernels_host.py (which proves, without a GPU, that
every case is well conditioned and that a wrong kernel would be noticed).  ``Case``, the two measures, the bound and the conditioning cap
are those of tests/unet_kernel_cases.py; the verdict is tests/kernel_verdict.py.

A DRIVER (``run_*``) lays the operands of ONE launch out in a guard-banded arena (tests/guarded.py) in the layout the model uses, calls
``kern.<entry point>``, runs ``Arena.check()`` and judges every output against the fp64 restatement.  ``kern`` is the adapter of the GPU
test (realpdebench_amd.ops on a device) or a torch fake on a CPU arena (the host test: the correct fake passes every driver, a fake with
one wrong term fails at least one), so the code that judges the kernels is the code the host test proves can fail.

Block counts that depend on the number of compute units are restated here from the launchers for the host test (``MI355X_CUS``); the
GPU test takes them from the library's query functions and asserts that the two agree.

What the shapes are for.  headnorm: fewer rows than one block of 4 waves (idle waves must write zero partial rows), one block +- 1,
and rows0 + 5 rows (rows0 = the capped wave count: five waves take a second trip).  head_scores: one token, one short of / one past a
32-token tile and a pair of them, an odd token count, n = 513 and 1025 (two and three chunks whose last one ends in a tile of ONE token).
head_apply: the same edges with 1, 2 and 4 heads (``wave % nh``, ``wave / nh`` and the LDS offsets depend on the count).  Token GEMMs:
M = 1 / 129 / 300 (the exact-fp32 kernel: one row, one row past a 128-row tile, a ragged third tile), 4096 / 4129 (the 64-row-tile
split kernel, whole tiles and a ragged last one).  Weight gradients: one token, an odd count, one past 1000 / 1024 (a second split),
and 4095 / 4099 on either side of the row count from which N, K % 256 == 0 runs on the split-operand kernel."""
import torch

import galerkin_restatement as R
import guarded
from kernel_verdict import verdict
from unet_kernel_cases import (BADLY_CONDITIONED, F32, F64, MEASURES, MI355X_CUS, Case, _gen, _rn,      # noqa: F401
                               bound_of, measures)

TAG = "galerkin-kernels"
C, FH, REG = 256, 256, 128                   # n_hidden, dim_feedforward, regressor width (the Galerkin YAMLs)
EPS = 1e-7


def ceil_div(a, b):
    return (a + b - 1) // b


# ================================================================================================ block counts (restated launchers)
def headnorm_rows(M, cus=MI355X_CUS):
    """rpb_headnorm_bwd_rows: the waves of min(ceil(M / 4), 8 CUs) blocks of 4"""
    return 4 * max(1, min(ceil_div(M, 4), 8 * cus))


def head_scores_chunks(B, n, cus=MI355X_CUS):
    """rpb_head_scores_chunks: ceil(6 CUs / B), at least 512 tokens per chunk"""
    return max(1, min(ceil_div(6 * cus, B), ceil_div(n, 512)))


def chunk_ranges(n, nchunk, step=32):
    """the token range of every chunk / split: ceil(n / nchunk) rounded up to ``step`` tokens each"""
    per = ceil_div(ceil_div(n, nchunk), step) * step
    return [(min(i * per, n), min((i + 1) * per, n)) for i in range(nchunk)]


def stream_blocks(items, cus=MI355X_CUS):
    """the grid of the streaming kernels: ceil(items / 256), at most 16 per CU"""
    return max(1, min(ceil_div(items, 256), 16 * cus))


def _balanced_splits(tiles, per_cu, cap, hard_max, cus):
    smax = max(1, min(ceil_div(cus * per_cu, tiles), cap, hard_max))
    best, best_fill = 1, 0.0
    for sp in range(1, smax + 1):
        blocks = tiles * sp
        fill = blocks / (ceil_div(blocks, cus) * cus)
        if fill >= best_fill:
            best, best_fill = sp, fill
    return best


def tn_path(M, N, K):
    """the entry point ops.gemm_tn takes: the split-operand kernel from 4096 rows for N, K multiples of 256"""
    return "gemm3x_tn" if (M >= 4096 and N % 256 == 0 and K % 256 == 0) else "gemm_tn"


def tn_splits(M, N, K, cus=MI355X_CUS):
    """rpb_gemm3x_tn_splits / rpb_gemm_tn_splits for the three Galerkin weight shapes"""
    if tn_path(M, N, K) == "gemm3x_tn":
        return max(8, (cus * 2 // ((N // 128) * (K // 256))) // 8 * 8)
    if N in (64, 128, 256, 384) and K % 64 == 0 and K <= 384 and N * K <= 49152:          # tn_small_kernel
        return _balanced_splits(K // 64, 3, ceil_div(M, 1024), 1024, cus)
    wk2, bn = 64 * (4 if K % 128 == 0 else 2), 64 * (4 if N > 128 else 2 if N > 64 else 1)
    return _balanced_splits(ceil_div(N, bn) * ceil_div(K, wk2), 3, ceil_div(M, 512), 256, cus)


def tn_split_step(M, N, K):
    return 16 if tn_path(M, N, K) == "gemm3x_tn" else 32


# ================================================================================================ the verdict
def judge(name, got, ref64, ref32, existing=None):
    """``got`` against the fp64 restatement on both measures, bound max(8 * e32, 1e-6) (or ``existing``, a bound another test of the
    same kernel already asserts); e32 = the same measure of the fp32 restatement.  Prints every figure before it asserts."""
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    verdict(TAG, name, zip(MEASURES, measures(ref32, ref64), measures(got, ref64)), existing)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def view2d(flat, rows, cols, ld):
    """[rows][cols] with leading dimension ``ld`` from the first element of ``flat`` (the torch fakes' view of a pointer argument)"""
    return flat.as_strided((rows, cols), (ld, 1))


def _other_columns(M, ld, col0, width):
    unw = torch.ones(M, ld, dtype=torch.bool)
    unw[:, col0:col0 + width] = False
    return unw


def _ex(existing, kernel):
    return (existing or {}).get(kernel)


# ================================================================================================ per-head LayerNorm
HEADNORM_M = [1, 3, 4, 5, 777]


def headnorm_trip_M(rows0):
    """rows0 = rpb_headnorm_bwd_rows of a huge M (the capped wave count): five waves take a second trip"""
    return rows0 + 5


def headnorm_case(M, flat_head=0):
    """the model's layouts: x = columns [C, 2C) and [2C, 3C) of the Q|K|V tensor, out = a half of the 2C-wide K|V tensor, gy likewise,
    gx = the same column range of the 3C-wide gradient.  ``flat_head``: head 1 of the keys of rows 0 and M // 2 holds 64 equal inputs
    (0.75: the mean of 64 copies is exact in fp32 and fp64).  There the variance is 0, the normalised value is exactly 0, so the
    reference gives y = beta exactly, gx = (dy - mean_h dy) / sqrt(eps) -- the formula's limit, 3162 times the size of an ordinary row --
    and no contribution to dgamma.  The fp32 restatement holds that (the host test measures it), so the case stays."""
    g = _gen(31, M, flat_head)
    i = dict(M=M, flat_head=flat_head, QKV=_rn(g, M, 3 * C, scale=1.5, shift=0.3), gamma=_rn(g, 2, C), beta=_rn(g, 2, C), gKVn=_rn(g, M, 2 * C))
    if flat_head:
        for r in {0, M // 2}:
            i["QKV"][r, C + 64:C + 128] = 0.75

    def ref(dt):
        out = {}
        for which in (0, 1):
            x, gy = i["QKV"][:, (1 + which) * C:(2 + which) * C], i["gKVn"][:, which * C:(1 + which) * C]
            gx, dg, db = R.headnorm_bwd(x, i["gamma"][which], gy, EPS, dt)
            out.update({f"y{which}": R.headnorm_fwd(x, i["gamma"][which], i["beta"][which], EPS, dt), f"gx{which}": gx,
                        f"dgb{which}": torch.cat((dg, db))})
        return out
    return Case(f"headnorm M={M}" + (" flat-head" if flat_head else ""), i, ref)


def run_headnorm(kern, c, existing=None):
    """both normalisations (keys, values), forward and backward; returns the partial-row count of the backward"""
    M = c.M
    r64, r32 = c.refs()
    rows = kern.headnorm_bwd_rows(M)
    for which in (0, 1):
        col, ocol = (1 + which) * C, which * C
        a = guarded.Arena(kern.dev)
        x, gam, bet = a.inp(c.QKV, "QKV"), a.inp(c.gamma[which], "gamma"), a.inp(c.beta[which], "beta")
        out = a.out(M, 2 * C, name="KVn", unwritten=_other_columns(M, 2 * C, ocol, C))
        kern.headnorm_fwd(x.at(col), 3 * C, gam.op, bet.op, out.at(ocol), 2 * C, M, C, EPS)
        a.check()
        judge(f"{c.name} fwd which={which}", out.get()[:, ocol:ocol + C], r64[f"y{which}"], r32[f"y{which}"], _ex(existing, "headnorm_fwd"))
        if c.flat_head and which == 0:                            # 64 equal inputs: 0 * gamma + beta, whatever 1 / sqrt(eps) is
            for r in {0, M // 2}:
                assert same_bits(out.get()[r, 64:128], c.beta[0][64:128]), f"{c.name}: row {r}, head 1 is not beta exactly"
        a = guarded.Arena(kern.dev)
        x, gam, gy = a.inp(c.QKV, "QKV"), a.inp(c.gamma[which], "gamma"), a.inp(c.gKVn, "gKVn")
        gx, part = a.out(M, 3 * C, name="gQKV", unwritten=_other_columns(M, 3 * C, col, C)), a.out(rows, 2 * C, name="part")
        kern.headnorm_bwd(x.at(col), 3 * C, gam.op, gy.at(ocol), 2 * C, gx.at(col), 3 * C, part.op, M, C, EPS)
        a.check()                                                 # every row of part is written: idle waves write zeros
        tag = f"{c.name} bwd which={which} rows={rows}"
        judge(tag + " gx", gx.get()[:, col:col + C], r64[f"gx{which}"], r32[f"gx{which}"], _ex(existing, "headnorm_bwd"))
        p = part.get()
        assert not p[M:].any(), f"{tag}: {int((p[M:] != 0).sum())} non-zero element(s) in the partial rows of waves without a row"
        judge(tag + " dgamma|dbeta", p.double().sum(0), r64[f"dgb{which}"], r32[f"dgb{which}"], _ex(existing, "headnorm_bwd"))
    return rows


# ================================================================================================ tokens <-> padded cells
PAD_SHAPES = [(2, 3, 5, 7, 6, 32), (1, 1, 1, 1, 2, 4), (3, 2, 4, 1, 0, 256), (1, 4, 3, 9, 3, 8)]


def pad_case(B, T, H, W, pad, Cc):
    """three distinct, non-symmetric grids (none is another one reversed, shifted or scaled), so that a swapped axis shows"""
    g = _gen(32, B, T, H, W, pad, Cc)
    ncrop, ncell = B * T * H * W, B * (T + pad) * (H + pad) * (W + pad)
    grids = [0.1 + 0.37 * torch.arange(T, dtype=F32), -0.5 + 0.05 * torch.arange(H, dtype=F32) ** 2, 2.0 - 0.21 * torch.arange(W, dtype=F32) ** 1.5]
    i = dict(dims=(B, T, H, W, Cc, pad), U=_rn(g, ncrop, Cc), Wg=_rn(g, Cc, 3), bias=_rn(g, Cc), grids=grids, g=_rn(g, ncell, Cc))
    mesh = (B, T, H, W)
    return Case(f"pad_grid B={B} mesh={T}x{H}x{W} pad={pad} C={Cc}", i,
                lambda dt: dict(out=R.pad_grid(i["U"], grids, i["Wg"], i["bias"], mesh, pad, dt), crop=R.crop_gather(i["g"], mesh, pad)),
                exact=("crop",))


def run_pad_grid(kern, c, existing=None):
    B, T, H, W, Cc, pad = c.dims
    r64, r32 = c.refs()
    a = guarded.Arena(kern.dev)
    U, gt, gh, gw = a.inp(c.U, "U"), a.inp(c.grids[0], "gt"), a.inp(c.grids[1], "gh"), a.inp(c.grids[2], "gw")
    Wg, bias, out = a.inp(c.Wg, "Wg"), a.inp(c.bias, "bias"), a.out(*r64["out"].shape, name="cells", ld=Cc)
    kern.pad_grid_fwd(U.op, gt.op, gh.op, gw.op, Wg.op, bias.op, out.op, c.dims)
    a.check()                                                     # the pad is WRITTEN (never-written check) ...
    got = out.get()
    inside = torch.zeros(got.shape[:-1], dtype=torch.bool)
    inside[:, :T, :H, :W] = True
    padv = got[~inside]
    assert not padv.view(torch.int32).any(), f"{c.name}: {int((padv.view(torch.int32) != 0).sum())} pad element(s) are not +0.0"      # ... with exact zeros
    judge(c.name, got, r64["out"], r32["out"], _ex(existing, "pad_grid"))
    a = guarded.Arena(kern.dev)
    g, back = a.inp(c.g, "g"), a.out(B * T * H * W, Cc, name="tokens")
    kern.crop_gather(g.op, back.op, c.dims)
    a.check()
    assert same_bits(back.get(), r64["crop"].float()), f"{c.name}: crop_gather is not the gather of the mesh's cells"


# ================================================================================================ head_scores
HS_HEADS = [1, 2, 3, 4]
HS_SHAPES = [(1, 1), (1, 15), (2, 17), (1, 31), (3, 33), (2, 64), (1, 65), (2, 513), (1, 1025), (3, 1000)]


def scores_case(nh, B, n):
    """nh = 4, the model's two call forms in turn: K^T V (G and A the two halves of the 2C-wide K|V tensor) and dP = Q^T g (G = the
    first C columns of the 3C-wide Q|K|V tensor, A dense).  nh < 4 (the U-Net's use): widths 64 nh, G the last 64 nh columns of a tensor 8 columns wider, A dense."""
    g = _gen(33, nh, B, n)
    M, w = B * n, 64 * nh
    if nh == 4 and HS_SHAPES.index((B, n)) % 2 == 0:
        t = _rn(g, M, 2 * C)
        i = dict(form="KtV", Gt=t, gcol=0, At=t, acol=C)
    elif nh == 4:
        i = dict(form="dP", Gt=_rn(g, M, 3 * C), gcol=0, At=_rn(g, M, C), acol=0)
    else:
        i = dict(form="padded-ld", Gt=_rn(g, M, w + 8), gcol=8, At=_rn(g, M, w), acol=0)
    i.update(nh=nh, B=B, n=n)
    G, A = i["Gt"][:, i["gcol"]:i["gcol"] + w], i["At"][:, i["acol"]:i["acol"] + w]
    return Case(f"head_scores nh={nh} B={B} n={n} {i['form']}", i, lambda dt: dict(S=R.head_scores(G, A, B, n, nh, dt)))


def run_head_scores(kern, c, existing=None):
    """returns the chunk count"""
    nh, B, n = c.nh, c.B, c.n
    r64, r32 = c.refs()
    chunks = kern.head_scores_chunks(B, n)
    ldg, lda = c.Gt.shape[1], c.At.shape[1]
    a = guarded.Arena(kern.dev)
    G = a.inp(c.Gt, "G", guard=32 * ldg + 1024)                   # a 32-token tile of rows is how far the kernel can overreach
    A = G if c.At is c.Gt else a.inp(c.At, "A", guard=32 * lda + 1024)
    part = a.out(chunks, B * nh * 4096, name="part")
    kern.head_scores(G.at(c.gcol), ldg, A.at(c.acol), lda, part.op, B, n, nh)
    a.check()                                                     # every element of every chunk row is written
    S = part.get().double().sum(0).view(B, nh, 64, 64)            # rpb_reduce_partials has its own tests: the sum is formed here
    judge(f"{c.name} chunks={chunks}", S, r64["S"], r32["S"], _ex(existing, "head_scores"))
    return chunks


# ================================================================================================ head_apply
HA_HEADS = [1, 2, 4]
HA_SHAPES = [(1, 1), (2, 31), (1, 32), (3, 33), (1, 65), (2, 97), (2, 1000)]
HA_EPILOGUES = ["none", "mask", "residual", "mask+residual", "drop", "drop+residual"]
HA_DROP = (987654321, 0.9)


def apply_case(nh, B, n):
    """X = the middle third of a 3 w-wide tensor, out = the second half of a 2 w-wide one (w = 64 nh); mask and residual dense.
    In-kernel dropout is keyed on row * w + channel (csrc/rpb_galerkin.hip)."""
    g = _gen(34, nh, B, n)
    M, w = B * n, 64 * nh
    i = dict(nh=nh, B=B, n=n, Xt=_rn(g, M, 3 * w), Wm=_rn(g, B, nh, 64, 64, scale=0.125), res=_rn(g, M, w),
             mask=(torch.rand(M, w, generator=g) < 0.8).float() / 0.8, hmask=R.dropout_mask_2d(M, w, w, *HA_DROP))
    if nh == 4:                                                   # the three call forms of the model's backward
        i.update(ga=_rn(g, M, C), KVn=_rn(g, M, 2 * C), P=_rn(g, B, 4, 64, 64, scale=0.125), dS=_rn(g, B, 4, 64, 64, scale=0.125))
    X = i["Xt"][:, w:2 * w]

    def ref(dt):
        out = {}
        for ep in HA_EPILOGUES:
            mask = i["mask"] if "mask" in ep else i["hmask"] if "drop" in ep else None
            out[ep] = R.head_apply(X, i["Wm"], B, n, nh, dt, mask, i["res"] if "residual" in ep else None)
        if nh == 4:
            tr = lambda m: m.transpose(-1, -2)
            out.update(dQ=R.head_apply(i["ga"], tr(i["P"]), B, n, 4, dt), dKn=R.head_apply(i["KVn"][:, C:], tr(i["dS"]), B, n, 4, dt),
                       dVn=R.head_apply(i["KVn"][:, :C], i["dS"], B, n, 4, dt))
        return out
    return Case(f"head_apply nh={nh} B={B} n={n}", i, ref)


def run_head_apply(kern, c, existing=None):
    nh, B, n = c.nh, c.B, c.n
    M, w = B * n, 64 * nh
    r64, r32 = c.refs()
    got = {}
    for ep in HA_EPILOGUES:
        a = guarded.Arena(kern.dev)
        X, Wm = a.inp(c.Xt, "X", guard=32 * 3 * w + 1024), a.inp(c.Wm, "Wm")
        res = a.inp(c.res, "residual", guard=32 * w + 1024) if "residual" in ep else None
        mask = a.inp(c.mask, "mask", guard=32 * w + 1024) if "mask" in ep else None
        out = a.out(M, 2 * w, name="out", guard=32 * 2 * w + 1024, unwritten=_other_columns(M, 2 * w, w, w))
        kern.head_apply(X.at(w), 3 * w, Wm.op, out.at(w), 2 * w, B, n, nh, res.op if res else None, w if res else 0,
                        mask.op if mask else None, w if mask else 0, HA_DROP if "drop" in ep else None)
        a.check()
        got[ep] = out.get()[:, w:]
        judge(f"{c.name} {ep}", got[ep], r64[ep], r32[ep], _ex(existing, "head_apply"))
    # one independent generator: without a residual the dropped-out result IS the plain result times the host's Philox mask
    assert same_bits(got["drop"], got["none"] * c.hmask), (
        f"{c.name}: drop={HA_DROP} is not the plain result times the host mask keyed on row * {w} + channel: "
        f"{int((got['drop'] != got['none'] * c.hmask).sum())} element(s) differ")
    if nh == 4:
        tr = lambda m: m.transpose(-1, -2).contiguous()
        forms = (("dQ", c.ga, 0, C, tr(c.P), 3 * C, 0), ("dKn", c.KVn, C, 2 * C, tr(c.dS), 2 * C, 0), ("dVn", c.KVn, 0, 2 * C, c.dS, 2 * C, C))
        for key, Xt, xcol, ldx, Wmat, ldo, ocol in forms:
            a = guarded.Arena(kern.dev)
            X, Wm = a.inp(Xt, "X", guard=32 * ldx + 1024), a.inp(Wmat, "Wm")
            out = a.out(M, ldo, name="out", guard=32 * ldo + 1024, unwritten=_other_columns(M, ldo, ocol, C))
            kern.head_apply(X.at(xcol), ldx, Wm.op, out.at(ocol), ldo, B, n, 4, None, 0, None, 0, None)
            a.check()
            judge(f"{c.name} backward form {key}", out.get()[:, ocol:ocol + C], r64[key], r32[key], _ex(existing, "head_apply"))


# ================================================================================================ dropout_mul
DROP_KEEPS = [0.05, 0.5, 0.95]
DROP_SEEDS = [55, 987654321, 123456789012345]                    # the last one above 2^32: both key words count


def dropout_sizes(blocks):
    """``blocks`` = the streaming grid of a huge tensor: the last size is one float4 past a full grid of 256-thread blocks"""
    return [4, 1028, 4 * (blocks * 256) + 4]


def run_dropout_mul(kern, n, seed, keep):
    x = _rn(_gen(35, n), n)
    a = guarded.Arena(kern.dev)
    g, out = a.inp(x, "g"), a.out(n, name="out")
    kern.dropout_mul(g.op, out.op, n, seed, keep)
    a.check()
    hm = R.dropout_mask(torch.arange(n).numpy(), seed, keep)
    kept = float((hm != 0).float().mean())
    print(f"[{TAG}] dropout_mul n={n} seed={seed} keep={keep}: host mask keeps {kept:.4f}")
    got = out.get()
    assert same_bits(got, x * hm), (f"dropout_mul n={n} seed={seed} keep={keep}: {int((got != x * hm).sum())} element(s) differ from "
                                    f"g * the host's Philox4x32-10 mask")


# ================================================================================================ token GEMMs through ops.gemm_nt
#        name     N     K    bias  act  residual  dropout site
SITES = {"qkv":  (3 * C, C,  True,  0,  False, None),
         "lr1":  (FH,    C,  True,  3,  False, (987654321, 0.9)),
         "lr2":  (C,     FH, True,  0,  True,  (55, 0.8)),
         "gH":   (FH,    C,  False, 4,  False, (987654321, 0.9)),
         "gX1":  (C,     FH, False, 0,  True,  None),
         "gX0":  (C, 3 * C,  False, 0,  True,  None),
         "lift": (REG,   C,  False, 0,  False, None),
         "gLift": (C,  REG,  False, 0,  False, None)}
LDO_SEED = 123456789012345
# (site, mode, ldo - N): every dropout site with no dropout, a mask tensor and drop=(seed, keep); two of them once more with ldo != N,
# where m * ldo + n and m * N + n disagree
GEMM_VARIANTS = ([(s, "none", 0) for s in SITES] + [(s, m, 0) for s in ("lr1", "lr2", "gH") for m in ("mask", "drop")]
                 + [("lr1", "drop", 8), ("lr2", "drop", 8)])
GEMM_M_FP32 = [1, 129, 300]
GEMM_M_SPLIT64 = [4096, 4129]
GEMM_BIG = ("lr2", "mask", 0, 65536 + 77)                         # the one large case: the mask-tensor route above GEMM_SPLIT_MIN_ROWS
# run once more at the GEMM_M_FP32 row counts with ops.GEMM_SPLIT_MIN_ROWS lowered to 0 (the same cases, so the same references)
GEMM_LOWERED = [("qkv", "none", 0), ("lr1", "drop", 0), ("lr2", "drop", 8), ("gH", "drop", 0), ("gX0", "none", 0), ("lift", "none", 0),
                ("lr1", "mask", 0), ("lr2", "mask", 0), ("gH", "mask", 0)]
GEMM_DIRECT_128 =[(s, "mask", 0, M) for s in ("lr1", "lr2", "gH") for M in (129, 300)]


def split64_rule(N, K, mask, drop):
    """which split kernel the ``rpb_gemm3x`` entry point runs (rpb_gemm3x2_supported of csrc/rpb_gemm3x2.hip, which the C ABI does not
    export: restated): the 64-row-tile kernel without a mask tensor for N % 256 == 0, and for N % 128 == 0 without dropout"""
    return (not mask) and K % 64 == 0 and (N % 256 == 0 or (N % 128 == 0 and not drop))


def expected_gemm_kernel(site, mode, M):
    """what ops.gemm_nt must choose, written from its docstring and DESIGN.md section 9, not from its code: the 64-row-tile split
    kernel from 4096 rows without a mask tensor; with a mask tensor the Galerkin products (K, N <= 256 and a second [M][N] operand)
    stay on the exact-fp32 kernel at any row count.  So no Galerkin site reaches the 128-row split kernel through ops.gemm_nt, however
    ops.GEMM_SPLIT_MIN_ROWS is set; ``GEMM_DIRECT_128`` runs it on the three mask-tensor epilogues through its entry point."""
    N, K = SITES[site][:2]
    return "split64" if (M >= 4096 and mode != "mask" and split64_rule(N, K, False, mode == "drop")) else "fp32"


def kernel_of(label, N, K, mask, drop):
    if label.startswith("gemm_nt["):
        return "fp32"
    assert label.startswith("gemm3x["), label
    return "split64" if split64_rule(N, K, mask, drop) else "split128"


def gemm_case(site, mode, pad, M):
    N, K, has_bias, act, has_res, dsite = SITES[site]
    g = _gen(36, sorted(SITES).index(site), ("none", "mask", "drop").index(mode), pad, M)
    ldo = N + pad
    seed, keep = (LDO_SEED, dsite[1]) if (pad and dsite) else (dsite or (0, 0.0))
    i = dict(site=site, mode=mode, M=M, N=N, K=K, ldo=ldo, act=act, drop=(seed, keep) if mode == "drop" else None,
             A=_rn(g, M, K), W=_rn(g, N, K, scale=K ** -0.5), bias=_rn(g, N) if has_bias else None,
             res=_rn(g, M, N) if has_res else None, mask=None, hmask=None,
             # a real ReLU output: exact zeros on about half of the elements, and the incoming gradient A W^T is not zero there
             aux=torch.relu(_rn(g, M, N)) if act == 4 else None)
    if mode == "mask":
        i["mask"] = (torch.rand(M, N, generator=g) < keep).float() / keep
    if mode == "drop":
        i["hmask"] = R.dropout_mask_2d(M, N, ldo, seed, keep)       # the documented index m * ldo + n, from the pointer of the call

    def ref(dt):
        m = i["mask"] if mode == "mask" else i["hmask"]
        out = dict(y=R.gemm_epilogue(i["A"], i["W"], dt, i["bias"], act, i["aux"], m, i["res"]))
        if mode == "drop":
            out["pre"] = R.gemm_epilogue(i["A"], i["W"], dt, i["bias"], act, i["aux"])      # before mask and residual
        return out
    return Case(f"gemm_nt {site} M={M} N={N} K={K} {mode}" + (f" ldo={ldo}" if pad else ""), i, ref)


def _padded(t, ldo):
    """[M][N] as the first N columns of [M][ldo]; the other columns hold NaN (a read of them would reach the result)"""
    if t is None or t.shape[1] == ldo:
        return t
    out = torch.full((t.shape[0], ldo), float("nan"))
    out[:, :t.shape[1]] = t
    return out


def run_gemm(kern, c, existing=None, expect=None, entry="gemm_nt"):
    """one call site on one kernel; ``expect`` = the kernel the dispatch must choose.  Returns (label, kernel)."""
    M, N, K, ldo = c.M, c.N, c.K, c.ldo
    r64, r32 = c.refs()

    def launch(with_res):
        a = guarded.Arena(kern.dev)
        A, W = a.inp(c.A, "A", guard=128 * K + 1024), a.inp(c.W, "W")         # a 128-row tile is how far a token GEMM can overreach
        bias = a.inp(c.bias, "bias") if c.bias is not None else None
        ops_ = {k: (a.inp(_padded(t, ldo), k, ld=ldo, guard=128 * ldo + 1024) if t is not None else None)
                for k, t in (("res", c.res if with_res else None), ("aux", c.aux), ("mask", c.mask))}
        out = a.out(M, ldo, name="out", guard=128 * ldo + 1024, unwritten=_other_columns(M, ldo, 0, N) if ldo != N else None)
        op = lambda o: None if o is None else o.op
        label = getattr(kern, entry)(A.op, W.op, out.op, M, N, K, op(bias), op(ops_["res"]), c.act, op(ops_["aux"]), op(ops_["mask"]),
                                     c.drop, K, ldo)
        a.check()
        return label, out.get()[:, :N]

    label, y = launch(True)
    kernel = kernel_of(label, N, K, c.mask is not None, c.drop is not None)
    tag = f"{c.name} [{label} -> {kernel}]"
    if expect is not None:
        assert kernel == expect, f"{tag}: expected the {expect} kernel"
    judge(tag, y, r64["y"], r32["y"], _ex(existing, kernel))
    if c.mode == "drop":
        y0 = launch(False)[1] if c.res is not None else y         # the same call without the residual: zeros stay visible
        dropped = c.hmask == 0
        pre = r64["pre"]
        # the kernel is within 3e-6 max|ref| of the reference, so a value above 1e-4 max|ref| cannot have been computed as zero
        sure = ~dropped & (pre.abs() > 1e-4 * pre.abs().max())
        print(f"[{TAG}] {tag}: host mask drops {int(dropped.sum())} of {dropped.numel()}, {int(sure.sum())} kept elements are clearly non-zero")
        assert not (y0[dropped] != 0).any(), (f"{tag}: {int((y0[dropped] != 0).sum())} element(s) the host mask (index m * {ldo} + n, "
                                              f"seed {c.drop[0]}) drops are not exactly 0.0")
        assert not (y0[sure] == 0).any(), f"{tag}: {int((y0[sure] == 0).sum())} element(s) the host mask keeps are 0.0"
    return label, kernel


# ================================================================================================ weight gradients through ops.gemm_tn
TN_SHAPES = [(C, FH), (3 * C, C), (REG, C)]
TN_M = [1, 65, 1000, 1025, 4095, 4099]


def tn_case(N, K, M):
    """G dense, as the model's three wgrad calls have it (g2, gH, gQKV are whole tensors); the regressor-width one is ALSO given a
    leading dimension larger than N (a column range of a 256-wide tensor), which the model does not do but the entry point admits"""
    g = _gen(37, N, K, M)
    ldg = 2 * N if N == REG else N
    i = dict(M=M, N=N, K=K, ldg=ldg, Gt=_rn(g, M, ldg), A=_rn(g, M, K), gcol=ldg - N)
    G = i["Gt"][:, i["gcol"]:]

    def ref(dt):
        dW, db = R.wgrad(G, i["A"], dt)
        return dict(dW=dW, db=db)
    return Case(f"gemm_tn M={M} N={N} K={K} ldg={ldg}", i, ref)


def run_gemm_tn(kern, c, existing=None):
    """returns (path, splits)"""
    M, N, K, ldg = c.M, c.N, c.K, c.ldg
    r64, r32 = c.refs()
    splits = kern.gemm_tn_splits(M, N, K, ldg, K)
    a = guarded.Arena(kern.dev)
    G, A = a.inp(c.Gt, "G", guard=32 * ldg + 1024), a.inp(c.A, "A", guard=32 * K + 1024)
    part = a.out(splits, N * K + N, name="part")
    label = kern.gemm_tn(G.at(c.gcol), A.op, part.op, M, N, K, ldg, K)
    a.check()                                                     # every partial row is written, the rows of empty splits too
    path = label.split("[")[0]
    tag = f"{c.name} [{label}] splits={splits}"
    assert path == tn_path(M, N, K), f"{tag}: expected {tn_path(M, N, K)}"
    tot = part.get().double().sum(0)
    judge(tag + " dW", tot[:N * K].view(N, K), r64["dW"], r32["dW"], _ex(existing, path))
    judge(tag + " db", tot[N * K:], r64["db"], r32["db"], _ex(existing, path))
    return path, splits


# ================================================================================================ every GPU case
def gemm_cases():
    out = [(s, m, p, M) for (s, m, p) in GEMM_VARIANTS for M in GEMM_M_FP32 + GEMM_M_SPLIT64]
    return out + GEMM_DIRECT_128                                  # (GEMM_BIG is one more: too large to probe twice; see the host test)


def all_cases(cus=MI355X_CUS):
    """(case constructor, arguments) of every GPU case, for the host tests"""
    out = [(headnorm_case, (M,)) for M in HEADNORM_M + [headnorm_trip_M(headnorm_rows(10 ** 9, cus))]] + [(headnorm_case, (5, 1))]
    out += [(pad_case, s) for s in PAD_SHAPES]
    out += [(scores_case, (nh, *s)) for nh in HS_HEADS for s in HS_SHAPES]
    out += [(apply_case, (nh, *s)) for nh in HA_HEADS for s in HA_SHAPES]
    out += [(gemm_case, s) for s in gemm_cases()] + [(gemm_case, GEMM_BIG)]
    out += [(tn_case, (N, K, M)) for (N, K) in TN_SHAPES for M in TN_M]
    return out
