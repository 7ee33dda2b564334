"""Host side (no GPU) of the per-kernel Galerkin Transformer tests:
* every restatement of tests/galerkin_restatement.py, in fp64, against an independent statement of the same mathematics (torch autograd,
  F.layer_norm, F.pad), and the Philox4x32-10 round function against its published known-answer vectors;
* every case of tests/test_gpu_galerkin_kernels.py is well conditioned: 8 * e32 <= 1e-5 on every output and measure;
* the cases whose point depends on the number of compute units reach the paths they claim at the MI355X's 256;
* the drivers would notice: ``TorchKernels`` is a torch stand-in for the library on a CPU ``Arena`` (it partitions the work as the
  launchers do: chunks, splits, grid-stride trips).  Unmutated it passes every driver; with ONE wrong term it trips ``Arena.check()``,
  the verdict or the dropout assertions at at least one case -- the same driver code the GPU test runs."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_l2

sys.path.insert(0, os.path.join(ROOT, "tests"))
import galerkin_kernel_cases as K           # noqa: E402
import galerkin_restatement as R            # noqa: E402

F32, F64 = torch.float32, torch.float64
TOL = 1e-12                                   # fp64 against fp64
C = K.C
ROWS0 = K.headnorm_rows(10 ** 9)
TRIP_M = K.headnorm_trip_M(ROWS0)


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)                        # the references of a case are computed once for all the tests of this file


# ================================================================================================ the torch stand-in for the library
class TorchKernels:
    """the entry points the drivers call, in fp32 torch on the views of a CPU arena; ``mut`` = one wrong term"""
    dev = "cpu"

    def __init__(self, mut=None, cus=K.MI355X_CUS):
        self.mut, self.cus = mut, cus

    # ---- headnorm
    def headnorm_bwd_rows(self, M):
        return K.headnorm_rows(M, self.cus)

    def _hn_mut(self):
        return self.mut if self.mut in ("one_mean_for_all_heads", "variance_over_63") else None

    def headnorm_fwd(self, x, ldx, gamma, beta, out, ldo, M, Cc, eps):
        K.view2d(out, M, Cc, ldo)[:] = R.headnorm_fwd(K.view2d(x, M, Cc, ldx), gamma[:Cc], beta[:Cc], eps, F32, self._hn_mut())

    def headnorm_bwd(self, x, ldx, gamma, gy, ldg, gx, ldgx, part, M, Cc, eps):
        rows = self.headnorm_bwd_rows(M)
        xv, gv, p = K.view2d(x, M, Cc, ldx), K.view2d(gy, M, Cc, ldg), K.view2d(part, rows, 2 * Cc, 2 * Cc)
        g, _, _ = R.headnorm_bwd(xv, gamma[:Cc], gv, eps, F32, self._hn_mut())
        K.view2d(gx, M, Cc, ldgx)[:] = g
        p[:] = 0.0                                                # wave w adds up the rows w, w + rows, ...: idle waves write zeros
        for trip in range(0, M, rows):
            if trip and self.mut == "partials_lose_the_second_trip":
                break
            m = min(rows, M - trip)
            xh, _ = R._normalised(xv[trip:trip + m], eps, F32, self._hn_mut())
            gh = gv[trip:trip + m].reshape(m, -1, 64)
            p[:m, :Cc] += (gh * xh).reshape(m, Cc)
            p[:m, Cc:] += gv[trip:trip + m]

    # ---- tokens <-> cells
    def pad_grid_fwd(self, U, gt, gh, gw, Wg, bias, out, dims):
        B, T, H, W, Cc, pad = dims
        mut = self.mut if self.mut == "h_and_w_grid_swapped" else None
        ref = R.pad_grid(U[:B * T * H * W * Cc].view(-1, Cc), (gt[:T], gh[:H], gw[:W]), Wg[:3 * Cc].view(Cc, 3), bias[:Cc], (B, T, H, W), pad, F32, mut)
        o = out[:ref.numel()].view(ref.shape)
        if self.mut == "pad_left_unwritten":
            o[:, :T, :H, :W] = ref[:, :T, :H, :W]
        else:
            o[:] = ref

    def crop_gather(self, g, out, dims):
        B, T, H, W, Cc, pad = dims
        ncell = B * (T + pad) * (H + pad) * (W + pad)
        out[:B * T * H * W * Cc] = R.crop_gather(g[:ncell * Cc].view(ncell, Cc), (B, T, H, W), pad).reshape(-1)

    # ---- per-head products
    def head_scores_chunks(self, B, n):
        return K.head_scores_chunks(B, n, self.cus)

    def head_scores(self, G, ldg, A, lda, part, B, n, nh):
        chunks, w = self.head_scores_chunks(B, n), 64 * nh
        Gv, Av = K.view2d(G, B * n, w, ldg).reshape(B, n, w), K.view2d(A, B * n, w, lda).reshape(B, n, w)
        p = part[:chunks * B * nh * 4096].view(chunks, B, nh, 64, 64)
        for ch, (lo, hi) in enumerate(K.chunk_ranges(n, chunks)):
            if self.mut == "last_partial_tile_left_out":
                hi = lo + (hi - lo) // 32 * 32
            if self.mut == "odd_token_of_a_pair_left_out":
                hi = lo + (hi - lo) // 2 * 2
            p[ch] = R.head_scores(Gv[:, lo:hi].reshape(-1, w), Av[:, lo:hi].reshape(-1, w), B, hi - lo, nh, F32)

    def head_apply(self, X, ldx, Wm, out, ldo, B, n, nh, residual, ldr, mask, ldm, drop):
        M, w = B * n, 64 * nh
        m = K.view2d(mask, M, w, ldm) if mask is not None else None
        if drop is not None:
            m = R.dropout_mask_2d(M, w, w, *drop, _mut="seed_halves_swapped" if self.mut == "seed_halves_swapped" else None)
        mut = self.mut if self.mut in ("matrix_of_the_next_head", "matrix_transposed") else None
        K.view2d(out, M, w, ldo)[:] = R.head_apply(K.view2d(X, M, w, ldx), Wm[:B * nh * 4096], B, n, nh, F32, m,
                                                  K.view2d(residual, M, w, ldr) if residual is not None else None, mut)

    def dropout_mul(self, g, out, n, seed, keep):
        out[:n] = g[:n] * R.dropout_mask(np.arange(n), seed, keep, _mut="seed_halves_swapped" if self.mut == "seed_halves_swapped" else None)

    # ---- token GEMMs
    def _gemm(self, A, W, out, M, N, Kk, bias, residual, act, aux, mask, drop, lda, ldo):
        v = lambda t: None if t is None else K.view2d(t, M, N, ldo)
        m = v(mask)
        if drop is not None:
            mut = {"dropout_indexed_by_m_times_N": "indexed_by_m_times_N", "seed_halves_swapped": "seed_halves_swapped"}.get(self.mut)
            m = R.dropout_mask_2d(M, N, ldo, *drop, _mut=mut)
        mut = "relu_grad_where_aux_ge_0" if self.mut == "relu_grad_where_aux_ge_0" else None
        v(out)[:] = R.gemm_epilogue(K.view2d(A, M, Kk, lda), W[:N * Kk].view(N, Kk), F32, None if bias is None else bias[:N], act, v(aux), m,
                                    v(residual), mut)

    def gemm_nt(self, A, W, out, M, N, Kk, bias, residual, act, aux, mask, drop, lda, ldo):
        self._gemm(A, W, out, M, N, Kk, bias, residual, act, aux, mask, drop, lda, ldo)
        split = M >= 4096 and mask is None
        return f"gemm3x[N{N},K{Kk}]" if split else f"gemm_nt[N{N},K{Kk},conv=0]"

    def gemm3x_direct(self, A, W, out, M, N, Kk, bias, residual, act, aux, mask, drop, lda, ldo):
        self._gemm(A, W, out, M, N, Kk, bias, residual, act, aux, mask, drop, lda, ldo)
        return f"gemm3x[N{N},K{Kk}]"

    # ---- weight gradients
    def gemm_tn_splits(self, M, N, Kk, ldg, lda):
        return K.tn_splits(M, N, Kk, self.cus)

    def gemm_tn(self, G, A, part, M, N, Kk, ldg, lda):
        splits = self.gemm_tn_splits(M, N, Kk, ldg, lda)
        Gv, Av, p = K.view2d(G, M, N, ldg), K.view2d(A, M, Kk, lda), K.view2d(part, splits, N * Kk + N, N * Kk + N)
        ranges = K.chunk_ranges(M, splits, K.tn_split_step(M, N, Kk))
        last = max(s for s, (lo, hi) in enumerate(ranges) if hi > lo)
        for s, (lo, hi) in enumerate(ranges):
            dW, db = R.wgrad(Gv[lo:hi], Av[lo:hi], F32)
            if self.mut == "dW_misses_one_split" and s == last and last > 0:
                dW = torch.zeros_like(dW)
            if self.mut == "db_from_A":
                db = Av[lo:hi].sum(0)[torch.arange(N) % Kk]
            p[s, :N * Kk], p[s, N * Kk:] = dW.reshape(-1), db
        return f"{K.tn_path(M, N, Kk)}[N{N},K{Kk}]"


GOOD = TorchKernels()


def rejected(driver, mut, *args):
    """the driver fails on the mutated stand-in: an assertion of Arena.check(), of the verdict or of the dropout comparisons"""
    with pytest.raises(AssertionError, match="kernel error|never written|differ|are not exactly 0.0|is not the plain result"):
        driver(TorchKernels(mut), *args)


# ================================================================================================ restatements against independent statements
def test_philox_known_answer_vectors():
    """the published vectors of Philox4x32-10 (Random123's kat_vectors), the bare ten rounds"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = R.philox4x32_10([np.array([c]) for c in ctr], [np.array([k]) for k in key])
        assert tuple(int(g[0]) for g in got) == want, (ctr, key, [hex(int(g[0])) for g in got])


def test_dropout_mask_threshold_multiplier_and_indexing():
    for keep in K.DROP_KEEPS + [0.8, 0.9]:
        thr = R.dropout_threshold(keep)
        assert thr == int(np.float64(np.float32(keep)) * 2.0 ** 32) and 0 < thr < 2 ** 32
        assert R.dropout_multiplier(keep).dtype == np.float32 and R.dropout_multiplier(keep) == np.float32(1) / np.float32(keep)
    seed = 123456789012345
    assert seed >> 32 and R.dropout_mask(np.arange(64), seed, 0.5).tolist() != R.dropout_mask(np.arange(64), seed & 0xFFFFFFFF, 0.5).tolist()
    # element e is word e & 3 of block e >> 2, wherever it is asked from
    whole = R.dropout_mask(np.arange(4096), 55, 0.8)
    pick = np.array([4095, 0, 7, 7, 1234])
    assert torch.equal(R.dropout_mask(pick, 55, 0.8), whole[torch.from_numpy(pick)])
    assert torch.equal(R.dropout_mask_2d(16, 256, 256, 55, 0.8).reshape(-1), whole)
    strided = R.dropout_mask_2d(15, 256, 264, 55, 0.8)
    assert torch.equal(strided[3], R.dropout_mask(3 * 264 + np.arange(256), 55, 0.8)) and not torch.equal(strided, R.dropout_mask_2d(15, 256, 256, 55, 0.8))
    m = R.dropout_mask(np.arange(1 << 18), 987654321, 0.9)
    assert set(m.unique().tolist()) == {0.0, float(np.float32(1) / np.float32(0.9))}
    assert abs(float((m != 0).float().mean()) - 0.9) < 4 * (0.09 / (1 << 18)) ** 0.5          # four standard deviations of the kept fraction


def test_headnorm_against_layer_norm_autograd():
    c = K.headnorm_case(5)
    for which in (0, 1):
        x = c.QKV[:, (1 + which) * C:(2 + which) * C].double().requires_grad_(True)
        gam, bet = c.gamma[which].double().requires_grad_(True), c.beta[which].double().requires_grad_(True)
        y = F.layer_norm(x.reshape(5, 4, 64), (64,), None, None, R.eps32(K.EPS)).reshape(5, C) * gam + bet
        y.backward(c.gKVn[:, which * C:(1 + which) * C].double())
        r = c.refs()[0]
        assert rel_l2(r[f"y{which}"], y.detach()) < TOL and rel_l2(r[f"gx{which}"], x.grad) < TOL
        assert rel_l2(r[f"dgb{which}"], torch.cat((gam.grad, bet.grad))) < TOL


def test_headnorm_flat_head_is_the_formulas_limit():
    c = K.headnorm_case(5, 1)
    r64, r32 = c.refs()
    sl = slice(64, 128)
    for r in (r64, r32):
        assert torch.equal(r["y0"][0, sl], c.beta[0][sl].to(r["y0"].dtype)) and torch.equal(r["y0"][2, sl], c.beta[0][sl].to(r["y0"].dtype))
    dy = c.gKVn[0, sl].double() * c.gamma[0][sl].double()
    assert rel_l2(r64["gx0"][0, sl], (dy - dy.mean()) / R.eps32(K.EPS) ** 0.5) < TOL
    assert float(r64["gx0"][0, sl].abs().max()) > 100 * float(r64["gx0"][1].abs().max())


def test_pad_grid_against_pad_and_autograd():
    c = K.pad_case(*K.PAD_SHAPES[0])
    B, T, H, W, Cc, pad = c.dims
    U = c.U.double().requires_grad_(True)
    grid = torch.stack(torch.meshgrid(*(g.double() for g in c.grids), indexing="ij"), -1)
    cells = F.pad((U.view(B, T, H, W, Cc) + grid @ c.Wg.double().t() + c.bias.double()), (0, 0, 0, pad, 0, pad, 0, pad))
    assert rel_l2(c.refs()[0]["out"], cells.detach()) < TOL and cells.shape == c.refs()[0]["out"].shape
    cells.backward(c.g.double().view(cells.shape))
    assert torch.equal(c.refs()[0]["crop"].double(), U.grad)      # the adjoint of the scatter
    assert len({tuple(g.tolist()) for g in c.grids} | {tuple(g.flip(0).tolist()) for g in c.grids}) == 6


def test_head_products_against_matmul_and_autograd():
    c = K.apply_case(2, 2, 31)
    B, n, nh, w = 2, 31, 2, 128
    X = c.Xt[:, w:2 * w].double().requires_grad_(True)
    Wm = c.Wm.double().requires_grad_(True)
    out = torch.stack([torch.cat([X[b * n:(b + 1) * n, 64 * h:64 * h + 64] @ Wm[b, h] for h in range(nh)], 1) for b in range(B)]).reshape(B * n, w)
    full = out * c.mask.double() + c.res.double()
    assert rel_l2(c.refs()[0]["none"], out.detach()) < TOL and rel_l2(c.refs()[0]["mask+residual"], full.detach()) < TOL
    go = torch.randn(B * n, w, dtype=F64, generator=K._gen(1))
    out.backward(go)
    assert rel_l2(R.head_scores(X.detach(), go, B, n, nh, F64), Wm.grad) < TOL                        # dP = X^T g
    assert rel_l2(R.head_apply(go, Wm.detach().transpose(-1, -2), B, n, nh, F64), X.grad) < TOL       # dX = g P^T


def test_gemm_epilogue_and_wgrad_against_autograd():
    torch.manual_seed(0)
    M, N, Kk = 37, 24, 16
    A, W, b = (torch.randn(*s, dtype=F64, requires_grad=True) for s in ((M, Kk), (N, Kk), (N,)))
    mask, res, go = (torch.rand(M, N) < 0.7).double() / 0.7, torch.randn(M, N, dtype=F64), torch.randn(M, N, dtype=F64)
    h = torch.relu(F.linear(A, W, b))
    y = h * mask + res
    assert rel_l2(R.gemm_epilogue(A.detach(), W.detach(), F64, b.detach(), 3, None, mask, res), y.detach()) < TOL
    y.backward(go)
    gpre = R.gemm_epilogue(go * mask, torch.eye(N, dtype=F64), F64, None, 4, h.detach())             # the gradient at the pre-activation
    assert rel_l2(R.gemm_epilogue(gpre, W.detach().t().contiguous(), F64), A.grad) < TOL                # the data gradient is a token GEMM too
    dW, db = R.wgrad(gpre, A.detach(), F64)
    assert rel_l2(dW, W.grad) < TOL and rel_l2(db, b.grad) < TOL
    assert bool((h.detach() == 0).any())


# ================================================================================================ conditioning of the GPU cases
def _ids(v):
    return getattr(v, "__name__", None) or "-".join(str(a) for a in v)


def _is_big(args):
    return args == K.GEMM_BIG


@pytest.mark.parametrize("make,args", K.all_cases(), ids=_ids)
def test_gpu_cases_are_well_conditioned(make, args):
    case = make(*args) if _is_big(args) else case_of(make, args)
    r64, r32 = case.refs()
    assert set(r64) == set(r32)
    for key in r64:
        if key in case.exact:
            assert torch.equal(r64[key].float(), r32[key]), f"{case.name} {key} is not exact"
            continue
        for kind, e32 in zip(K.MEASURES, K.measures(r32[key], r64[key])):
            print(f"[galerkin-cases] {case.name} {key} {kind}: e32 {e32:.3e}")
            assert 8 * e32 <= K.BADLY_CONDITIONED, f"{case.name} {key}: the fp32 restatement itself is off by {e32:.3e} ({kind})"
    if make is K.gemm_case and case.aux is not None:               # ReLU' is asked about aux == 0 with a non-zero incoming gradient
        zero = case.aux == 0
        assert 0.3 < float(zero.float().mean()) < 0.7 and bool(((case.A @ case.W.t())[zero] != 0).all())


def test_cases_reach_the_paths_they_claim():
    """at the MI355X's 256 compute units"""
    assert ROWS0 == 8192 and TRIP_M == 8197 and K.headnorm_rows(TRIP_M) == ROWS0
    assert [len(range(wv, TRIP_M, ROWS0)) for wv in (0, 4, 5, ROWS0 - 1)] == [2, 2, 1, 1]            # five waves take a second trip
    assert [K.headnorm_rows(M) for M in K.HEADNORM_M] == [4, 4, 4, 8, 780]                             # idle waves at 1, 3, 5, 777
    # head_scores: n = 513 / 1025 split into 2 / 3 chunks; the last one is short and ends in a tile of ONE token.  (No chunk holds a
    # single token unless n = 1: a chunk is ceil(n / chunks) rounded up to 32 tokens, so only the last tile can be that short.)
    for (B, n), chunks in (((2, 513), 2), ((1, 1025), 3)):
        assert K.head_scores_chunks(B, n) == chunks
        ranges = K.chunk_ranges(n, chunks)
        lo, hi = ranges[-1]
        assert 0 < hi - lo < ranges[0][1] - ranges[0][0] and (hi - lo) % 32 == 1
    assert K.head_scores_chunks(1, 1) == 1 and K.head_scores_chunks(3, 1000) == 2
    # dropout_mul: one float4 past a full grid
    blocks = K.stream_blocks(10 ** 12)
    assert blocks == 4096 and K.dropout_sizes(blocks)[-1] // 4 == blocks * 256 + 1
    # weight gradients: a second split from 1000 / 1025 tokens on, empty splits on the split-operand kernel, both paths
    assert [K.tn_path(M, 256, 256) for M in K.TN_M] == ["gemm_tn"] * 5 + ["gemm3x_tn"]
    assert [K.tn_path(M, 128, 256) for M in K.TN_M] == ["gemm_tn"] * 6
    assert [K.tn_splits(M, 256, 256) for M in (1, 65, 1000, 1025, 4095)] == [1, 1, 2, 3, 8]
    assert [K.tn_splits(M, 128, 256) for M in (1000, 1025)] == [1, 2]
    sp = K.tn_splits(4099, 768, 256)
    assert sp == 80 and sum(hi > lo for lo, hi in K.chunk_ranges(4099, sp, 16)) < sp
    # token GEMMs: every kernel a site can reach through ops.gemm_nt is asked for
    kernels = {K.expected_gemm_kernel(s, m, M) for (s, m, p, M) in K.gemm_cases()[:-len(K.GEMM_DIRECT_128)]}
    assert kernels == {"fp32", "split64"} and K.expected_gemm_kernel(*K.GEMM_BIG[:2], K.GEMM_BIG[3]) == "fp32"
    assert all(K.kernel_of("gemm3x[..]", *K.SITES[s][:2], True, False) == "split128" for s, *_ in K.GEMM_DIRECT_128)
    assert any(p for (_, m, p, _) in K.gemm_cases() if m == "drop")                                     # a dropout site with ldo != N


# ================================================================================================ the stand-in passes, its mutations fail
@pytest.mark.parametrize("M,flat", [(1, 0), (5, 0), (777, 0), (5, 1), (TRIP_M, 0)])
def test_standin_headnorm(M, flat):
    c = case_of(K.headnorm_case, (M, flat))
    K.run_headnorm(GOOD, c)
    rejected(K.run_headnorm, "one_mean_for_all_heads", c)
    rejected(K.run_headnorm, "variance_over_63", c)
    if M == TRIP_M:
        rejected(K.run_headnorm, "partials_lose_the_second_trip", c)


@pytest.mark.parametrize("shape", K.PAD_SHAPES, ids=_ids)
def test_standin_pad_grid(shape):
    c = case_of(K.pad_case, shape)
    K.run_pad_grid(GOOD, c)
    if shape[2] > 1 or shape[3] > 1:                              # (a 1 x 1 mesh has one grid value per axis: the swap shows elsewhere)
        rejected(K.run_pad_grid, "h_and_w_grid_swapped", c)
    if shape[4]:
        rejected(K.run_pad_grid, "pad_left_unwritten", c)


@pytest.mark.parametrize("nh", K.HS_HEADS)
@pytest.mark.parametrize("B,n", K.HS_SHAPES)
def test_standin_head_scores(nh, B, n):
    c = case_of(K.scores_case, (nh, B, n))
    K.run_head_scores(GOOD, c)
    if any((hi - lo) % 32 for lo, hi in K.chunk_ranges(n, K.head_scores_chunks(B, n))):
        rejected(K.run_head_scores, "last_partial_tile_left_out", c)
    if any((hi - lo) % 2 for lo, hi in K.chunk_ranges(n, K.head_scores_chunks(B, n))):
        rejected(K.run_head_scores, "odd_token_of_a_pair_left_out", c)


@pytest.mark.parametrize("nh", K.HA_HEADS)
@pytest.mark.parametrize("B,n", K.HA_SHAPES)
def test_standin_head_apply(nh, B, n):
    c = case_of(K.apply_case, (nh, B, n))
    K.run_head_apply(GOOD, c)
    if nh > 1:
        rejected(K.run_head_apply, "matrix_of_the_next_head", c)
    rejected(K.run_head_apply, "matrix_transposed", c)
    rejected(K.run_head_apply, "seed_halves_swapped", c)


@pytest.mark.parametrize("seed", K.DROP_SEEDS)
def test_standin_dropout_mul(seed):
    for n in K.dropout_sizes(2)[:3]:
        for keep in K.DROP_KEEPS:
            K.run_dropout_mul(GOOD, n, seed, keep)
    rejected(K.run_dropout_mul, "seed_halves_swapped", 1028, seed, 0.5)      # (a seed below 2^32 becomes another seed: it shows as well)


GEMM_STANDIN = [(s, m, p, M) for (s, m, p, M) in K.gemm_cases() if M in (129, 4129)]


@pytest.mark.parametrize("site,mode,pad,M", GEMM_STANDIN, ids=lambda v: str(v))
def test_standin_token_gemm(site, mode, pad, M):
    c = case_of(K.gemm_case, (site, mode, pad, M))
    K.run_gemm(GOOD, c, expect=K.expected_gemm_kernel(site, mode, M))
    if c.act == 4:
        rejected(K.run_gemm, "relu_grad_where_aux_ge_0", c)
    if mode == "drop":
        rejected(K.run_gemm, "seed_halves_swapped", c)
        if pad:
            rejected(K.run_gemm, "dropout_indexed_by_m_times_N", c)
        else:
            K.run_gemm(TorchKernels("dropout_indexed_by_m_times_N"), c)      # where ldo == N the two indices agree: this is why ldo != N is run


def test_standin_direct_128_row_entry():
    c = case_of(K.gemm_case, K.GEMM_DIRECT_128[0])
    assert K.run_gemm(GOOD, c, expect="split128", entry="gemm3x_direct")[1] == "split128"


@pytest.mark.parametrize("N,Kk", K.TN_SHAPES)
@pytest.mark.parametrize("M", K.TN_M)
def test_standin_gemm_tn(N, Kk, M):
    c = case_of(K.tn_case, (N, Kk, M))
    path, splits = K.run_gemm_tn(GOOD, c)
    rejected(K.run_gemm_tn, "db_from_A", c)
    if sum(hi > lo for lo, hi in K.chunk_ranges(M, splits, K.tn_split_step(M, N, Kk))) > 1:
        rejected(K.run_gemm_tn, "dW_misses_one_split", c)
    else:
        assert M < 1000 or (N, M) == (K.REG, 1000)
