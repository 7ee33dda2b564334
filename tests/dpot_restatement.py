"""Plain-torch restatements of the DPOT kernel family (csrc/rpb_dpot.hip) on the layouts documented in include/rpb.h ("DPOT: AFNO patch
transformer"), written from that header and oracle/dpot_oracle.py.  Dtype-generic, CPU only: the GPU tests (test_gpu_dpot_kernels.py)
compare every kernel against the matching function here in fp64 and take their tolerance from the same function in fp32;
tests/test_dpot_restatement_host.py pins this file against torch's own operators and the CPU oracle without a GPU."""
import math

import torch


# ------------------------------------------------------------------------------------------------ gathers
def patch_tokens(u, gx, gy, gt, Cm, ps):
    """u [B][T][H][W][Cd], grids gx [H], gy [W], gt [T] -> P [((b*nx + px)*ny + py)*T + t][(c*ps + i)*ps + j], c over the Cm + 3 channels
    (data | ones up to Cm | grid x | grid y | grid t)."""
    B, T, H, W, Cd = u.shape
    nx, ny = H // ps, W // ps
    full = torch.ones(B, T, H, W, Cm + 3, dtype=u.dtype)
    full[..., :Cd] = u
    full[..., Cm] = gx.to(u.dtype).view(1, 1, H, 1)
    full[..., Cm + 1] = gy.to(u.dtype).view(1, 1, 1, W)
    full[..., Cm + 2] = gt.to(u.dtype).view(1, T, 1, 1)
    v = full.view(B, T, nx, ps, ny, ps, Cm + 3).permute(0, 2, 4, 1, 6, 3, 5)              # b px py t c i j
    return v.reshape(B * nx * ny * T, (Cm + 3) * ps * ps)


def patch_tokens_bwd(gP, B, T, H, W, Cd, Cm, ps):
    """gP [B*nx*ny*T][(Cm+3)*ps*ps] -> gu [B][T][H][W][Cd]: the adjoint of patch_tokens w.r.t. u (patches do not overlap)."""
    nx, ny = H // ps, W // ps
    g = gP.view(B, nx, ny, T, Cm + 3, ps, ps)[:, :, :, :, :Cd]                            # b px py t c i j
    return g.permute(0, 3, 1, 5, 2, 6, 4).reshape(B, T, H, W, Cd)


def unpatch(O, B, T, H, W, Cd, Co, ps):
    """O [(((b*nx + px)*ny + py)*ps + i)*ps + j][ldo], column t*Co + c -> pred [B][T][H][W][Cd] (c < Cd)."""
    nx, ny = H // ps, W // ps
    ldo = O.shape[1]
    o = O.view(B, nx, ny, ps, ps, ldo)[..., :T * Co].reshape(B, nx, ny, ps, ps, T, Co)[..., :Cd]     # b px py i j t c
    return o.permute(0, 5, 1, 3, 2, 4, 6).reshape(B, T, H, W, Cd)


def unpatch_bwd(gpred, Co, ps, ldo):
    """gpred [B][T][H][W][Cd] -> gO [B*H*W][ldo]: the adjoint of unpatch, zero on the columns it does not read."""
    B, T, H, W, Cd = gpred.shape
    nx, ny = H // ps, W // ps
    g = gpred.view(B, T, nx, ps, ny, ps, Cd).permute(0, 2, 4, 3, 5, 1, 6)                 # b px py i j t c
    tc = torch.zeros(B, nx, ny, ps, ps, T, Co, dtype=gpred.dtype)
    tc[..., :Cd] = g
    gO = torch.zeros(B, nx, ny, ps, ps, ldo, dtype=gpred.dtype)
    gO[..., :T * Co] = tc.reshape(B, nx, ny, ps, ps, T * Co)
    return gO.reshape(B * H * W, ldo)


def rowtable_add(x, table, rows_per_entry):
    """x [M][C] + table[(r / rows_per_entry) % nent][:]"""
    idx = (torch.arange(x.shape[0]) // rows_per_entry) % table.shape[0]
    return x + table[idx]


def rowtable_grad(g, B, rows_per_entry, nent):
    """g [(b*nent + e)*rows_per_entry + t][C] -> dtable [nent][C]"""
    return g.view(B, nent, rows_per_entry, g.shape[1]).sum((0, 2))


# ------------------------------------------------------------------------------------------------ TimeAggregator
def _tagg_arg(gamma, tt, dt):
    """tt[t] * gamma[i] rounded to fp32 -- the argument the reference's fp32 module and the kernel both hand to the cosine -- in the
    working precision.  Differentiable w.r.t. gamma with the exact factor tt (the rounding is carried as a constant)."""
    a = tt.to(dt)[:, None] * gamma.to(dt)[None, :]
    a32 = (tt.detach().float()[:, None] * gamma.detach().float()[None, :]).to(dt)
    return a + (a32 - a.detach())


def tagg_prep(w, gamma, tt):
    """w [T][C][C], gamma [C], tt [T] -> (Wf [C][T*C], Wb [T*C][C], e [T][C]); e = cos(tt gamma), Wb[(t,i)][j] = e[t][i] w[t][i][j]."""
    T, C, _ = w.shape
    e = torch.cos(_tagg_arg(gamma, tt, w.dtype))
    Wb = (e[:, :, None] * w).reshape(T * C, C)
    return Wb.t().contiguous(), Wb, e


def tagg_finish(dWb, w, gamma, tt, dWsum=None):
    """dWb [T*C][C] (+ dWsum [C][C] added to every frame's block) -> (dw [T][C][C], dgamma [C])."""
    T, C, _ = w.shape
    arg = _tagg_arg(gamma, tt, w.dtype)
    d = dWb.view(T, C, C)
    if dWsum is not None:
        d = d + dWsum[None]
    dw = torch.cos(arg)[:, :, None] * d
    dgamma = (-torch.sin(arg) * tt.to(w.dtype)[:, None] * (d * w).sum(-1)).sum(0)
    return dw, dgamma


# ------------------------------------------------------------------------------------------------ GroupNorm on token rows
def gn_tokens_fwd(x, x2, gamma, beta, G, eps=1e-5):
    """x (+ x2) [B][P][C], groups of C / G consecutive channels -> (y [B][P][C], stat [B*G][2] = (mean, rstd)); two-pass variance."""
    B, P, C = x.shape
    v = (x if x2 is None else x + x2).view(B, P, G, C // G)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = ((v - mean) * rstd).reshape(B, P, C) * gamma + beta
    return y, torch.stack((mean.reshape(B * G), rstd.reshape(B * G)), -1)


def gn_tokens_bwd(x, x2, gamma, stat, gy, gadd, G):
    """-> (gx [B][P][C] (+ gadd), pg [B][C], pb [B][C]): the data gradient and the per-sample partials of d weight / d bias."""
    B, P, C = x.shape
    cg = C // G
    v = (x if x2 is None else x + x2).view(B, P, G, cg)
    mu, rstd = stat.view(B, 1, G, 1, 2).unbind(-1)
    xh = (v - mu) * rstd
    gh = (gy * gamma).view(B, P, G, cg)
    m1 = gh.mean((1, 3), keepdim=True)
    m2 = (gh * xh).mean((1, 3), keepdim=True)
    gx = (rstd * (gh - m1 - xh * m2)).reshape(B, P, C)
    if gadd is not None:
        gx = gx + gadd
    return gx, (gy * xh.reshape(B, P, C)).sum(1), gy.sum(1)


# ------------------------------------------------------------------------------------------------ AFNO block MLP
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def afno_wprep(w, transpose):
    """w [2 (re, im)][nb][bs_in][bs_out] (einsum '...bi,bio->...bo') -> real composite [nb][2 bs_in][2 bs_out] acting on (re | im) rows:
    (re,i)->(re,o) = wr, (im,i)->(re,o) = -wi, (re,i)->(im,o) = wi, (im,i)->(im,o) = wr; ``transpose``: each block transposed."""
    wr, wi = w[0], w[1]
    Wc = torch.cat((torch.cat((wr, wi), -1), torch.cat((-wi, wr), -1)), -2)
    return Wc.transpose(1, 2).contiguous() if transpose else Wc


def _blocks(X, nb, bs):
    """[ntok][2][nb*bs] -> [nb][ntok][2*bs]"""
    n = X.shape[0]
    return X.view(n, 2, nb, bs).permute(2, 0, 1, 3).reshape(nb, n, 2 * bs)


def _rows(Xb, nb, bs):
    """[nb][ntok][2*bs] -> [ntok][2][nb*bs]"""
    n = Xb.shape[1]
    return Xb.view(nb, n, 2, bs).permute(1, 2, 0, 3).reshape(n, 2, nb * bs)


def afno_mlp(X, Wa, ba, Wb, bb, aux, nb, bs, mode):
    """X, aux, mid, out: [ntok][2][C = nb*bs]; Wa, Wb: composites [nb][2bs][2bs]; ba, bb: [2][C] or None.
    mode 0: mid = X Wa + ba, out = gelu(mid) Wb + bb.   mode 1: mid = (X Wa) * gelu'(aux), out = mid Wb.   -> (mid, out)"""
    C = nb * bs
    h = _rows(torch.bmm(_blocks(X, nb, bs), Wa), nb, bs)
    if mode == 0:
        if ba is not None:
            h = h + ba.reshape(2, C)
        out = _rows(torch.bmm(_blocks(gelu(h), nb, bs), Wb), nb, bs)
        if bb is not None:
            out = out + bb.reshape(2, C)
        return h, out
    h = h * gelu_grad(aux)
    return h, _rows(torch.bmm(_blocks(h, nb, bs), Wb), nb, bs)


def afno_wgrad(A, G, nb, bs, a_gelu):
    """A, G [ntok][2][C] -> dw [2][nb][bs][bs], the gradient of the complex block weights of out = A w when G = d out (A through GELU
    when ``a_gelu``): d wr = Ar^T Gr + Ai^T Gi, d wi = Ar^T Gi - Ai^T Gr."""
    n = A.shape[0]
    if a_gelu:
        A = gelu(A)
    Ar, Ai = A.view(n, 2, nb, bs).unbind(1)
    Gr, Gi = G.view(n, 2, nb, bs).unbind(1)
    mm = lambda a, g: torch.einsum("nbi,nbo->bio", a, g)
    return torch.stack((mm(Ar, Gr) + mm(Ai, Gi), mm(Ar, Gi) - mm(Ai, Gr)))
