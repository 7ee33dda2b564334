"""TEST INFRASTRUCTURE ONLY -- plain torch restatements of the Galerkin Transformer kernels (csrc/rpb_galerkin.hip) and of the token-GEMM
epilogues the Galerkin step issues, written from the formulas in the kernel comments and include/rpb.h, not from the kernels' code order.
Every function takes a dtype: fp64 is the reference, fp32 the conditioning probe (tests/galerkin_kernel_cases.py).  The dropout mask is a
host restatement of Philox4x32-10 (Salmon et al., SC'11) in numpy integer arithmetic; nothing here touches a GPU.

``_mut`` names ONE deliberately wrong term; tests/test_galerkin_kernels_host.py uses it to prove that the cases would notice."""
import numpy as np
import torch

DK = 64                                       # channels per head


def eps32(eps):
    """the kernels take eps as a float: the reference adds the same number"""
    return float(np.float32(eps))


# ================================================================================================ per-head LayerNorm
def _heads(t, dt):
    return t.to(dt).reshape(t.shape[0], -1, DK)


def headnorm_fwd(x, gamma, beta, eps, dt, _mut=None):
    """y[m][64h + j] = (x - mean_h) / sqrt(var_h + eps) * gamma + beta: mean and BIASED variance over the 64 channels of head h"""
    xh, _ = _normalised(x, eps, dt, _mut)
    return xh.reshape(x.shape) * gamma.to(dt) + beta.to(dt)


def _normalised(x, eps, dt, _mut=None):
    v = _heads(x, dt)
    mean = v.mean(-1, keepdim=True)
    if _mut == "one_mean_for_all_heads":
        mean = v.mean((-1, -2), keepdim=True).expand_as(mean)
    d = v - mean
    var = (d * d).sum(-1, keepdim=True) / (DK - 1 if _mut == "variance_over_63" else DK)
    inv = 1.0 / torch.sqrt(var + eps32(eps))
    return d * inv, inv


def headnorm_bwd(x, gamma, gy, eps, dt, _mut=None):
    """(gx, dgamma, dbeta) of the above given gy = dLoss/dy: with dy = gy gamma and the normalised xh,
    gx = (dy - mean_h(dy) - xh mean_h(dy xh)) / sqrt(var_h + eps), dgamma = sum_m gy xh, dbeta = sum_m gy"""
    xh, inv = _normalised(x, eps, dt, _mut)
    g = _heads(gy, dt)
    dy = g * gamma.to(dt).reshape(1, -1, DK)
    gx = (dy - dy.mean(-1, keepdim=True) - xh * (dy * xh).mean(-1, keepdim=True)) * inv
    return gx.reshape(x.shape), (g * xh).sum(0).reshape(-1), g.sum(0).reshape(-1)


# ================================================================================================ tokens <-> padded cells
def pad_grid(U, grids, Wg, bias, mesh, pad, dt, _mut=None):
    """out[b,t,h,w,:] = U[token(b,t,h,w)] + Wg (gt[t], gh[h], gw[w]) + bias inside the mesh, exact zeros in the pad;
    U [B T H W][C], Wg [C][3] -> [B][T+pad][H+pad][W+pad][C]"""
    B, T, H, W = mesh
    C = U.shape[-1]
    gt, gh, gw = (g.to(dt) for g in grids)
    wg = Wg.to(dt)
    if _mut == "h_and_w_grid_swapped":
        wg = wg[:, [0, 2, 1]]
    term = (gt.view(T, 1, 1, 1) * wg[:, 0] + gh.view(1, H, 1, 1) * wg[:, 1] + gw.view(1, 1, W, 1) * wg[:, 2])
    out = torch.zeros(B, T + pad, H + pad, W + pad, C, dtype=dt)
    out[:, :T, :H, :W] = U.to(dt).view(B, T, H, W, C) + term + bias.to(dt)
    return out


def crop_gather(g, mesh, pad):
    """out[token] = g[padded cell of token]: a pure gather, exact in any dtype"""
    B, T, H, W = mesh
    C = g.shape[-1]
    return g.view(B, T + pad, H + pad, W + pad, C)[:, :T, :H, :W].reshape(B * T * H * W, C).clone()


# ================================================================================================ per-head products
def head_scores(G, A, B, n, nh, dt):
    """S[b][h][i][j] = sum_m G[b,m][64h + i] A[b,m][64h + j] (before the 1 / n); G, A [B n][64 nh]"""
    return torch.einsum("bnhi,bnhj->bhij", G.to(dt).reshape(B, n, nh, DK), A.to(dt).reshape(B, n, nh, DK))


def head_apply(X, Wm, B, n, nh, dt, mask=None, residual=None, _mut=None):
    """out[b,m][64h + j] = (sum_i X[b,m][64h + i] Wm[b][h][i][j]) * mask + residual"""
    w = Wm.to(dt).reshape(B, nh, DK, DK)
    if _mut == "matrix_of_the_next_head":
        w = w.roll(-1, 1)
    if _mut == "matrix_transposed":
        w = w.transpose(-1, -2)
    o = torch.einsum("bnhi,bhij->bnhj", X.to(dt).reshape(B, n, nh, DK), w).reshape(B * n, nh * DK)
    if mask is not None:
        o = o * mask.to(dt)
    if residual is not None:
        o = o + residual.to(dt)
    return o


# ================================================================================================ token GEMM + epilogue
def gemm_epilogue(A, W, dt, bias=None, act=0, aux=None, mask=None, residual=None, _mut=None):
    """out = epilogue(A W^T), in the order of include/rpb.h: bias; act 0 none, 3 ReLU, 4 zero where aux <= 0 (the backward through a
    ReLU whose OUTPUT aux was saved); mask (the inverted-dropout multiplier); residual"""
    v = A.to(dt) @ W.to(dt).t()
    if bias is not None:
        v = v + bias.to(dt)
    if act == 3:
        v = torch.relu(v)
    elif act == 4:
        keep = (aux >= 0) if _mut == "relu_grad_where_aux_ge_0" else (aux > 0)
        v = torch.where(keep, v, torch.zeros_like(v))
    else:
        assert act == 0
    if mask is not None:
        v = v * mask.to(dt)
    if residual is not None:
        v = v + residual.to(dt)
    return v


def wgrad(G, A, dt):
    """(dW [N][K], db [N]) = (G^T A, colsum G)"""
    g, a = G.to(dt), A.to(dt)
    return g.t() @ a, g.sum(0)


# ================================================================================================ Philox4x32-10 and the dropout mask
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """ten rounds of Philox4x32 on uint64 arrays holding 32-bit words: ``counter`` = 4 arrays, ``key`` = 2 -> 4 arrays.
    A round: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2; c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped after it."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK32) for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & np.uint64(MASK32) for k in key)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2              # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return c0, c1, c2, c3


def dropout_threshold(keep):
    """keep iff word < floor(float64(float32(keep)) * 2^32)"""
    return int(np.floor(np.float64(np.float32(keep)) * 4294967296.0))


def dropout_multiplier(keep):
    return np.float32(1.0) / np.float32(keep)


def dropout_mask(elem, seed, keep, _mut=None):
    """the inverted-dropout multiplier (fp32 tensor, 0 or 1 / keep) of the elements with linear index ``elem`` (any integer array):
    element e is word e & 3 of the Philox block with counter (q & 0xFFFFFFFF, q >> 32, 0x243F6A88, 0x85A308D3), q = e >> 2, and key
    (seed & 0xFFFFFFFF, seed >> 32)"""
    e = np.asarray(elem, dtype=np.uint64)
    q, lane = e >> np.uint64(2), (e & np.uint64(3)).astype(np.int64)
    uq, inv = np.unique(q, return_inverse=True)
    lo, hi = int(seed) & MASK32, (int(seed) >> 32) & MASK32
    if _mut == "seed_halves_swapped":
        lo, hi = hi, lo
    words = np.stack(philox4x32_10((uq & np.uint64(MASK32), uq >> np.uint64(32), np.full_like(uq, 0x243F6A88), np.full_like(uq, 0x85A308D3)),
                                   (np.full_like(uq, lo), np.full_like(uq, hi))), -1)
    w = words[inv.reshape(-1), lane.reshape(-1)].reshape(e.shape)
    m = np.where(w < np.uint64(dropout_threshold(keep)), dropout_multiplier(keep), np.float32(0.0)).astype(np.float32)
    return torch.from_numpy(m)


def dropout_mask_2d(M, N, ld, seed, keep, col0=0, _mut=None):
    """the mask of an [M][N] tensor whose element (m, n) has the linear index m * ld + col0 + n (the GEMM epilogues: ld = ldo, the
    index counts from the pointer the call was given, so col0 = 0; head_apply: ld = 64 nheads; a dense tensor: ld = N)"""
    if _mut == "indexed_by_m_times_N":
        ld = N
    e = np.arange(M, dtype=np.uint64)[:, None] * np.uint64(ld) + np.uint64(col0) + np.arange(N, dtype=np.uint64)[None, :]
    return dropout_mask(e, seed, keep, _mut)
