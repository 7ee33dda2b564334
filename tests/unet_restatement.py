"""TEST INFRASTRUCTURE ONLY -- plain-torch restatements of the U-Net kernel family, one function per kernel, written from the kernels'
documented contracts (the header comments of csrc/rpb_unet.hip, rpb_unet_glue.hip, rpb_galerkin.hip, rpb_transolver.hip, rpb_gemm.hip,
rpb_pointwise.hip, the argument lists of include/rpb.h) and from how model/unet.py composes them; never from a kernel's output.

Every function takes the working ``dtype`` last: the floating-point arguments are cast to it, everything is computed in it (fp64 = the
reference, fp32 = "what plain fp32 arithmetic loses on these inputs", tests/test_gpu_unet_kernels.py).  Token tensors are channels-last,
as the kernels see them.  tests/test_unet_kernels_host.py checks each restatement in fp64 against an independent statement (torch's own
group_norm / layer_norm / conv3d autograd, oracle/unet_oracle.py)."""
import torch
import torch.nn.functional as F

HEADS, DH, HID = 4, 32, 128
SCALE = DH ** -0.5


def _c(dtype, *ts):
    out = tuple(None if t is None else t.to(dtype) for t in ts)
    return out if len(out) > 1 else out[0]


# ================================================================================================ GroupNorm + SiLU channel passes
def chan_stats(x, dtype):
    """x [B][n][C] -> [B][2][C]: (sum_n x, sum_n x^2)"""
    x = _c(dtype, x)
    return torch.stack((x.sum(1), (x * x).sum(1)), 1)


def _silu_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def affine_silu_fwd(x, A, Bc, res, dtype):
    """y = silu(x * A[b][c] + Bc[b][c]) (+ res); x [B][n][C], A / Bc [B][C]"""
    x, A, Bc, res = _c(dtype, x, A, Bc, res)
    y = F.silu(x * A[:, None] + Bc[:, None])
    return y if res is None else y + res


def affine_silu_bwd_reduce(x, gy, A, Bc, dtype):
    """[B][2][C]: (sum_n dz * x, sum_n dz), dz = gy * silu'(x A + Bc)"""
    x, gy, A, Bc = _c(dtype, x, gy, A, Bc)
    dz = gy * _silu_grad(x * A[:, None] + Bc[:, None])
    return torch.stack(((dz * x).sum(1), dz.sum(1)), 1)


def affine_silu_bwd_apply(x, gy, A, Bc, P, Q, dtype):
    """gx = dz * A + P + Q * x"""
    x, gy, A, Bc, P, Q = _c(dtype, x, gy, A, Bc, P, Q)
    dz = gy * _silu_grad(x * A[:, None] + Bc[:, None])
    return dz * A[:, None] + P[:, None] + Q[:, None] * x


# ================================================================================================ channel LayerNorm (beta = 0)
def layernorm_fwd(x, gamma, eps, dtype):
    """x [M][C]: (x - mean) / sqrt(biased var + eps) * gamma"""
    x, gamma = _c(dtype, x, gamma)
    mu = x.mean(1, keepdim=True)
    d = x - mu
    return d / ((d * d).mean(1, keepdim=True) + eps).sqrt() * gamma


def layernorm_bwd(x, gamma, gy, eps, dtype):
    """(gx [M][C], dgamma [C] = sum_m gy * xhat, dbeta [C] = sum_m gy):
    gx = rstd * (gy gamma - mean_c(gy gamma) - xhat * mean_c(gy gamma xhat))"""
    x, gamma, gy = _c(dtype, x, gamma, gy)
    mu = x.mean(1, keepdim=True)
    d = x - mu
    rstd = 1 / ((d * d).mean(1, keepdim=True) + eps).sqrt()
    xh = d * rstd
    gg = gy * gamma
    gx = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    return gx, (gy * xh).sum(0), gy.sum(0)


# ================================================================================================ init_conv as im2col
def im2col(x, KS, ldc, dtype):
    """x [B][T][H][W][Cin] -> col [B*T*H*W][ldc]: column tap * Cin + ci with tap = (kt * KS + kh) * KS + kw, the value
    x[b][t + kt - R][h + kh - R][w + kw - R][ci] (zero outside the mesh), columns >= KS^3 * Cin zero."""
    x = _c(dtype, x)
    B, T, H, W, Cin = x.shape
    R = KS // 2
    xp = F.pad(x, (0, 0, R, R, R, R, R, R))                                # pads W, H, T (last dimension first)
    k = torch.arange(KS)
    it = (torch.arange(T)[:, None] + k[None, :])                           # [T][KS] index into the padded axis
    ih = (torch.arange(H)[:, None] + k[None, :])
    iw = (torch.arange(W)[:, None] + k[None, :])
    g = xp[:, it[:, None, None, :, None, None], ih[None, :, None, None, :, None], iw[None, None, :, None, None, :]]
    col = torch.zeros(B * T * H * W, ldc, dtype=dtype)                     # g: [B][T][H][W][kt][kh][kw][Cin]
    col[:, :KS ** 3 * Cin] = g.reshape(B * T * H * W, KS ** 3 * Cin)
    return col


# ================================================================================================ column reductions
def col_reduce(x, mode, dtype):
    """x [F][n][C] -> [F][C]: mode 0 = the column maximum over the frame's tokens (kmax of the k softmax, unet.py:_linear_attn),
    mode 1 = the column sum (Z = sum_n exp(k - kmax))"""
    x = _c(dtype, x)
    return x.amax(1) if mode == 0 else x.sum(1)


def colsum(x, dtype):
    """x [M][N] -> [N]"""
    return _c(dtype, x).sum(0)


def copy_cols(src, dst, C, soff, doff, dtype):
    """dst[m][doff : doff + C] = src[m][soff : soff + C]; every other element of dst is kept"""
    out = _c(dtype, dst).clone()
    out[:, doff:doff + C] = _c(dtype, src)[:, soff:soff + C]
    return out


def add(a, b, dtype):
    a, b = _c(dtype, a, b)
    return a + b


# ================================================================================================ spatial linear attention, stage by stage
def linattn_prep_fwd(qkv, kmax, dtype):
    """qkv [F][n][384], kmax [F][128] -> qe [F][n][256] = [ q' | E ]:  q' = softmax over the 32 channels of a head (q) * 32^-1/2,
    E = exp(k - kmax[f][c])   (ksoft = E / Z is never formed; unet.py:_linear_attn divides the 32 x 32 context by Z)"""
    qkv, kmax = _c(dtype, qkv, kmax)
    Fr, n, _ = qkv.shape
    q = qkv[..., :HID].reshape(Fr, n, HEADS, DH).softmax(-1).reshape(Fr, n, HID) * SCALE
    E = (qkv[..., HID:2 * HID] - kmax[:, None]).exp()
    return torch.cat((q, E), -1)


def linattn_prep_bwd(qe, dqe, dz, dtype):
    """qe, dqe [F][n][256] = [q' | E], [d q' | d E'], dz [F][128] -> columns 0..255 of gqkv:
    d q = q' * (d q' - <q', d q'>_head / 32^-1/2),  d k = (d E' + d Z[f][c]) * E"""
    qe, dqe, dz = _c(dtype, qe, dqe, dz)
    Fr, n, _ = qe.shape
    q, g = qe[..., :HID].reshape(Fr, n, HEADS, DH), dqe[..., :HID].reshape(Fr, n, HEADS, DH)
    dq = q * (g - (q * g).sum(-1, keepdim=True) / SCALE)
    dk = (dqe[..., HID:] + dz[:, None]) * qe[..., HID:]
    return torch.cat((dq.reshape(Fr, n, HID), dk), -1)


def head_scores(G, A, dtype, nheads=2):
    """G, A [F][n][64 * nheads] -> [F][nheads][64][64]: S[f][h][i][j] = sum_m G[f][m][64h + i] * A[f][m][64h + j]"""
    G, A = _c(dtype, G, A)
    Fr, n, _ = G.shape
    return torch.einsum("fmhi,fmhj->fhij", G.reshape(Fr, n, nheads, 64), A.reshape(Fr, n, nheads, 64))


def head_apply(X, Wm, dtype, nheads=2):
    """X [F][n][64 * nheads], Wm [F][nheads][64][64] -> out[f][m][64h + j] = sum_i X[f][m][64h + i] * Wm[f][h][i][j]"""
    X, Wm = _c(dtype, X, Wm)
    Fr, n, _ = X.shape
    return torch.einsum("fmhi,fhij->fmhj", X.reshape(Fr, n, nheads, 64), Wm).reshape(Fr, n, 64 * nheads)


# ================================================================================================ temporal attention
def _rot(t, rc, rs):
    """t [..., T, 32], tables [T][32] (angle[t][d] = t * freq[d // 2]): interleaved-pair rotation t * cos + (-t1, t0) * sin"""
    x = t.reshape(*t.shape[:-1], -1, 2)
    r = torch.stack((-x[..., 1], x[..., 0]), -1).reshape(t.shape)
    return t * rc + r * rs


def tattn_fwd(qkv, rc, rs, bias, dtype):
    """qkv [B][T][HW][384], rotary tables rc / rs [T][32], bias [4][T][T] -> out [B][T][HW][128]: per location and head,
    softmax_j(rot(q / sqrt 32)_i . rot(k)_j + bias[h][i][j]) v_j over the T frames"""
    qkv, rc, rs, bias = _c(dtype, qkv, rc, rs, bias)
    B, T, HW, _ = qkv.shape
    q, k, v = (t.reshape(B, T, HW, HEADS, DH).permute(0, 2, 3, 1, 4) for t in qkv.split(HID, -1))     # b hw h t d
    s = _rot(q * SCALE, rc, rs) @ _rot(k, rc, rs).transpose(-1, -2) + bias
    return (s.softmax(-1) @ v).permute(0, 3, 1, 2, 4).reshape(B, T, HW, HID)


def tattn_bwd(qkv, rc, rs, bias, go, dtype):
    """(d qkv, d bias) of tattn_fwd for the output gradient go, by autograd of the restatement in ``dtype``"""
    qkv, bias = _c(dtype, qkv).clone().requires_grad_(True), _c(dtype, bias).clone().requires_grad_(True)
    tattn_fwd(qkv, rc, rs, bias, dtype).backward(_c(dtype, go))
    return qkv.grad, bias.grad


# ================================================================================================ bottleneck attention
def sattn_fwd(qkv, dtype):
    """qkv [F][n][384] -> (out [F][n][128], lse [F][4][n]): softmax attention over the n tokens of a frame, q scaled by 32^-1/2, no
    rotary, no bias; lse = natural log-sum-exp of the scaled logits of a query row"""
    qkv = _c(dtype, qkv)
    Fr, n, _ = qkv.shape
    q, k, v = (t.reshape(Fr, n, HEADS, DH).transpose(1, 2) for t in qkv.split(HID, -1))              # f h n d
    s = (q * SCALE) @ k.transpose(-1, -2)
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(Fr, n, HID), torch.logsumexp(s, -1)


def sattn_bwd(qkv, go, dtype):
    qkv = _c(dtype, qkv).clone().requires_grad_(True)
    sattn_fwd(qkv, dtype)[0].backward(_c(dtype, go))
    return qkv.grad


# ================================================================================================ GEMMs and the (1,4,4) convolutions
def gemm_nt(A, W, bias, residual, dtype):
    """A [M][K] W[N][K]^T + bias[N] + residual[M][N]"""
    A, W, bias, residual = _c(dtype, A, W, bias, residual)
    y = A @ W.t()
    if bias is not None:
        y = y + bias
    return y if residual is None else y + residual


def gemm_tn(G, A, dtype):
    """(dW [N][K] = G^T A, db [N] = column sums of G) for G [M][N], A [M][K]"""
    G, A = _c(dtype, G, A)
    return G.t() @ A, G.sum(0)


def _tok(t):                                                               # [B][C][T][H][W] -> tokens [B*T*H*W][C]
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


def _vol(x, B, mesh):                                                      # tokens -> [B][C][T][H][W]
    return x.reshape(B, *mesh, x.shape[-1]).permute(0, 4, 1, 2, 3)


def strided_conv(x, w, bias, B, mesh, dtype):
    """nn.Conv3d(Ci, Co, (1,4,4), stride (1,2,2), padding (0,1,1)): tokens x [B*T*H*W][Ci], w [Co][Ci][1][4][4] -> [B*T*H/2*W/2][Co]"""
    x, w, bias = _c(dtype, x, w, bias)
    return _tok(F.conv3d(_vol(x, B, mesh), w, bias, stride=(1, 2, 2), padding=(0, 1, 1)))


def strided_conv_wgrad(gy, x, Co, B, mesh, dtype):
    """(dW [Co][Ci][1][4][4], db [Co]) of strided_conv for the output-token gradient gy, by torch's conv3d autograd"""
    gy, x = _c(dtype, gy, x)
    Ci = x.shape[-1]
    w = torch.zeros(Co, Ci, 1, 4, 4, dtype=dtype, requires_grad=True)
    b = torch.zeros(Co, dtype=dtype, requires_grad=True)
    y = F.conv3d(_vol(x, B, mesh), w, b, stride=(1, 2, 2), padding=(0, 1, 1))
    y.backward(_vol(gy, B, (mesh[0], mesh[1] // 2, mesh[2] // 2)))
    return w.grad, b.grad


def transposed_conv(x, w, bias, B, mesh, dtype):
    """nn.ConvTranspose3d(Ci, Co, (1,4,4), (1,2,2), (0,1,1)): tokens x [B*T*H*W][Ci], w [Ci][Co][1][4][4] -> [B*T*2H*2W][Co]"""
    x, w, bias = _c(dtype, x, w, bias)
    return _tok(F.conv_transpose3d(_vol(x, B, mesh), w, bias, stride=(1, 2, 2), padding=(0, 1, 1)))


# ================================================================================================ relative-position bias
def relpos_fwd(table, idx, dtype):
    """table [nbuckets][heads], idx [n2] -> bias [heads][n2] = table[idx[p]][h]"""
    return _c(dtype, table)[idx.long()].t().contiguous()


def relpos_bwd(g, idx, nbuckets, dtype):
    """g [heads][n2] -> d table [nbuckets][heads]: the scatter-add that transposes relpos_fwd"""
    g = _c(dtype, g)
    return torch.zeros(nbuckets, g.shape[0], dtype=dtype).index_add_(0, idx.long(), g.t())
