"""tests/dpot_restatement.py without a GPU: every restatement in fp64 on the CPU against torch's own operators, torch autograd and
oracle/dpot_oracle.py.  Agreement below 1e-12 Rel-L2 everywhere (two fp64 evaluations of one formula in different orders); the pure
index maps are compared exactly.  The GPU tests (test_gpu_dpot_kernels.py) then use these functions as the kernels' reference."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_l2

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dpot_restatement as R                 # noqa: E402
from oracle import dpot_oracle as O          # noqa: E402

F64 = torch.float64
TOL = 1e-12


def rnd(*shape):
    return torch.randn(*shape, dtype=F64)


def spectral_rows(xp, kx, ky):
    """channels-last field [B][H][W][C] -> the kept modes of rfft2 as rows [B*kx*ky][2][C]"""
    X = torch.fft.rfft2(xp, dim=(1, 2), norm="ortho")[:, :kx, :ky]
    return torch.stack((X.real, X.imag), -2).reshape(-1, 2, xp.shape[-1])


@pytest.mark.parametrize("B,C,H,W,nb,modes", [(2, 32, 8, 8, 2, 3), (1, 48, 6, 6, 3, 6), (2, 16, 8, 6, 1, 32)])
def test_afno_forward_matches_oracle(B, C, H, W, nb, modes):
    """rfft2 rows -> afno_mlp mode 0 on the wprep composites -> zero padding, irfft2, + skip  ==  oracle.dpot_oracle.afno2d, with fewer
    modes than the latent grid, with modes == H (clipped to W/2 + 1 along y) and with all modes kept."""
    torch.manual_seed(B * 100 + C)
    bs = C // nb
    x = rnd(B, C, H, W)
    sd = {"w1": rnd(2, nb, bs, bs) / bs ** 0.5, "b1": rnd(2, nb, bs), "w2": rnd(2, nb, bs, bs) / bs ** 0.5, "b2": rnd(2, nb, bs)}
    ref = O.afno2d(sd, "", x, nb, modes)
    kx, ky = min(modes, H), min(modes, W // 2 + 1)
    xp = x.permute(0, 2, 3, 1)
    rows = spectral_rows(xp, kx, ky)
    mid, out = R.afno_mlp(rows, R.afno_wprep(sd["w1"], False), sd["b1"].reshape(2, C), R.afno_wprep(sd["w2"], False),
                          sd["b2"].reshape(2, C), None, nb, bs, 0)
    o = out.view(B, kx, ky, 2, C)
    Z = F.pad(torch.complex(o[..., 0, :], o[..., 1, :]), (0, 0, 0, W // 2 + 1 - ky, 0, H - kx))
    y = torch.fft.irfft2(Z, s=(H, W), dim=(1, 2), norm="ortho") + xp
    assert rel_l2(y.permute(0, 3, 1, 2), ref) < TOL
    # the saved pre-activation is the first layer's output before GELU
    Xc = torch.complex(rows[:, 0], rows[:, 1]).view(-1, nb, bs)
    h = torch.einsum("nbi,bio->nbo", Xc, torch.complex(sd["w1"][0], sd["w1"][1])).reshape(-1, C)
    assert rel_l2(mid, torch.stack((h.real, h.imag), 1) + sd["b1"].reshape(2, C)) < TOL


@pytest.mark.parametrize("ntok,nb,bs", [(7, 2, 16), (33, 1, 48)])
def test_afno_backward_matches_autograd(ntok, nb, bs):
    """mode 1 on the transposed composites and afno_wgrad == autograd through mode 0 (data gradient, d w1, d w2)."""
    torch.manual_seed(ntok)
    C = nb * bs
    X = rnd(ntok, 2, C).requires_grad_(True)
    w1 = (rnd(2, nb, bs, bs) / (2 * bs) ** 0.5).requires_grad_(True)
    w2 = (rnd(2, nb, bs, bs) / (2 * bs) ** 0.5).requires_grad_(True)
    b1, b2 = rnd(2, C), rnd(2, C)
    mid, out = R.afno_mlp(X, R.afno_wprep(w1, False), b1, R.afno_wprep(w2, False), b2, None, nb, bs, 0)
    gout = rnd(ntok, 2, C)
    gX, gw1, gw2 = torch.autograd.grad((out * gout).sum(), (X, w1, w2))
    with torch.no_grad():
        gmid, gin = R.afno_mlp(gout, R.afno_wprep(w2, True), None, R.afno_wprep(w1, True), None, mid, nb, bs, 1)
        dw2 = R.afno_wgrad(mid, gout, nb, bs, True)
        dw1 = R.afno_wgrad(X, gmid, nb, bs, False)
    assert rel_l2(gin, gX) < TOL
    assert rel_l2(dw1, gw1) < TOL and rel_l2(dw2, gw2) < TOL
    assert torch.equal(R.afno_wprep(w1, True), R.afno_wprep(w1, False).transpose(1, 2))


@pytest.mark.parametrize("B,P,C,G", [(2, 5, 24, 8), (1, 9, 40, 1), (3, 4, 16, 16)])
@pytest.mark.parametrize("with_x2", [False, True])
@pytest.mark.parametrize("with_gadd", [False, True])
def test_groupnorm_matches_torch(B, P, C, G, with_x2, with_gadd):
    torch.manual_seed(P)
    x = (rnd(B, P, C) + 8).requires_grad_(True)
    x2 = rnd(B, P, C) if with_x2 else None
    gadd = rnd(B, P, C) if with_gadd else None
    w, b = rnd(C).requires_grad_(True), rnd(C).requires_grad_(True)
    gy = rnd(B, P, C)
    v = x if x2 is None else x + x2
    ref = F.group_norm(v.permute(0, 2, 1), G, w, b, 1e-5).permute(0, 2, 1)
    gx, gw, gb = torch.autograd.grad((ref * gy).sum(), (x, w, b))
    with torch.no_grad():
        y, stat = R.gn_tokens_fwd(x, x2, w, b, G, 1e-5)
        dx, pg, pb = R.gn_tokens_bwd(x, x2, w, stat, gy, gadd, G)
        vg = v.detach().view(B, P, G, C // G)
    assert rel_l2(y, ref.detach()) < TOL
    assert rel_l2(stat[:, 0], vg.mean((1, 3)).reshape(-1)) < TOL
    assert rel_l2(stat[:, 1], 1 / torch.sqrt(vg.var((1, 3), unbiased=False) + 1e-5).reshape(-1)) < TOL
    assert rel_l2(dx, gx if gadd is None else gx + gadd) < TOL
    assert pg.shape == (B, C) and pb.shape == (B, C)
    assert rel_l2(pg.sum(0), gw) < TOL and rel_l2(pb.sum(0), gb) < TOL


@pytest.mark.parametrize("B,T,H,W,Cd,Cm,ps", [(2, 3, 8, 16, 2, 4, 4), (1, 1, 6, 3, 3, 3, 3)])
def test_patch_embedding_matches_conv2d(B, T, H, W, Cd, Cm, ps):
    """patch_tokens(...) @ conv_w.reshape(E, -1).T == F.conv2d(stride = ps) on [data | ones | grid x | grid y | grid t]: pins the column
    order (c*ps + i)*ps + j and the token order (b, px, py, t)."""
    torch.manual_seed(H)
    E = 5
    u = rnd(B, T, H, W, Cd)
    lin = lambda m: torch.tensor(np.linspace(0, 1, m), dtype=F64)
    gx, gy, gt = lin(H), lin(W), lin(T)
    conv_w = rnd(E, Cm + 3, ps, ps)
    xx = torch.ones(B, T, H, W, Cm, dtype=F64)
    xx[..., :Cd] = u
    xx = torch.cat((xx, gx.view(1, 1, H, 1, 1).expand(B, T, H, W, 1), gy.view(1, 1, 1, W, 1).expand(B, T, H, W, 1),
                    gt.view(1, T, 1, 1, 1).expand(B, T, H, W, 1)), -1)
    ref = F.conv2d(xx.permute(0, 1, 4, 2, 3).reshape(B * T, Cm + 3, H, W), conv_w, stride=ps)      # (b t) e px py
    nx, ny = H // ps, W // ps
    ref = ref.view(B, T, E, nx, ny).permute(0, 3, 4, 1, 2).reshape(B * nx * ny * T, E)
    P = R.patch_tokens(u, gx, gy, gt, Cm, ps)
    assert P.shape == (B * nx * ny * T, (Cm + 3) * ps * ps)
    assert rel_l2(P @ conv_w.reshape(E, -1).t(), ref) < TOL
    # the _bwd restatement is the autograd adjoint of the gather
    ur = u.clone().requires_grad_(True)
    gP = rnd(*P.shape)
    (gu,) = torch.autograd.grad((R.patch_tokens(ur, gx, gy, gt, Cm, ps) * gP).sum(), ur)
    assert torch.equal(R.patch_tokens_bwd(gP, B, T, H, W, Cd, Cm, ps), gu)


@pytest.mark.parametrize("T,C", [(1, 32), (4, 96)])
@pytest.mark.parametrize("with_sum", [False, True])
def test_time_aggregator_matches_autograd(T, C, with_sum):
    """tagg_finish == autograd through tagg_prep's Wb (and through sum_t Wb_t when dWsum is given); Wf is Wb transposed; the forward
    weights equal the oracle's h * cos(t gamma) followed by the einsum with w."""
    torch.manual_seed(C)
    w = (rnd(T, C, C) / (T * C ** 0.5)).requires_grad_(True)
    gamma = (2 ** torch.linspace(-10, 10, C)).double().requires_grad_(True)
    tt = torch.linspace(0, 1, T).double()
    dWb = rnd(T * C, C)
    dWsum = rnd(C, C) if with_sum else None
    Wf, Wb, e = R.tagg_prep(w, gamma, tt)
    loss = (Wb * dWb).sum()
    if with_sum:
        loss = loss + (Wb.view(T, C, C).sum(0) * dWsum).sum()
    gw, gg = torch.autograd.grad(loss, (w, gamma))
    with torch.no_grad():
        dw, dgamma = R.tagg_finish(dWb, w, gamma, tt, dWsum)
        assert torch.equal(Wf, Wb.t()) and Wf.shape == (C, T * C) and e.shape == (T, C)
        # the argument is the fp32 product (what the reference's fp32 module evaluates), the cosine is taken in fp64
        assert torch.equal(e, torch.cos((tt.float()[:, None] * gamma.float()[None, :]).double()))
        h = rnd(3, T, C)
        ref = torch.einsum("tij,nti->nj", w, h * e)
        assert rel_l2(h.reshape(3, T * C) @ Wb, ref) < TOL
    assert rel_l2(dw, gw) < TOL
    if T == 1:                                       # tt = [0]: the cosine does not depend on gamma
        assert float(dgamma.abs().max()) == 0.0 and float(gg.abs().max()) == 0.0
    else:
        assert rel_l2(dgamma, gg) < TOL


@pytest.mark.parametrize("B,T,H,W,Cd,Co,ps,ldo", [(2, 2, 8, 16, 3, 4, 4, 8), (1, 3, 6, 3, 2, 4, 3, 32), (1, 1, 8, 8, 4, 4, 8, 4)])
def test_unpatch_round_trips(B, T, H, W, Cd, Co, ps, ldo):
    torch.manual_seed(ldo)
    rows = B * H * W
    O_ = rnd(rows, ldo)
    pred = R.unpatch(O_, B, T, H, W, Cd, Co, ps)
    assert pred.shape == (B, T, H, W, Cd)
    gO = R.unpatch_bwd(pred, Co, ps, ldo)
    keep = torch.zeros(ldo, dtype=torch.bool)
    for t in range(T):
        keep[t * Co:t * Co + Cd] = True
    # unpatch followed by the re-gather is the identity on the c < Cd columns; the adjoint is zero on columns >= T*Co and on Cd <= c < Co
    assert torch.equal(gO[:, keep], O_[:, keep])
    assert float(gO[:, ~keep].abs().max() if (~keep).any() else 0.0) == 0.0
    # ... and unpatch_bwd is the autograd adjoint of unpatch
    Or = O_.clone().requires_grad_(True)
    g = rnd(B, T, H, W, Cd)
    (ga,) = torch.autograd.grad((R.unpatch(Or, B, T, H, W, Cd, Co, ps) * g).sum(), Or)
    assert torch.equal(R.unpatch_bwd(g, Co, ps, ldo), ga)
    # pixel (x, y) of frame t comes from row (((b*nx + x/ps)*ny + y/ps)*ps + x%ps)*ps + y%ps, column t*Co + c
    b, t, x, y, c = B - 1, T - 1, H - 2, W - 1, Cd - 1
    row = (((b * (H // ps) + x // ps) * (W // ps) + y // ps) * ps + x % ps) * ps + y % ps
    assert pred[b, t, x, y, c] == O_[row, t * Co + c]


def test_rowtable_matches_autograd():
    torch.manual_seed(3)
    B, nent, rpe, C = 3, 5, 4, 8
    x, table = rnd(B * nent * rpe, C), rnd(nent, C).requires_grad_(True)
    y = R.rowtable_add(x, table, rpe)
    assert torch.equal(y.detach().view(B, nent, rpe, C), x.view(B, nent, rpe, C) + table.detach().view(1, nent, 1, C))
    g = rnd(B * nent * rpe, C)
    (gt,) = torch.autograd.grad((y * g).sum(), table)
    assert rel_l2(R.rowtable_grad(g, B, rpe, nent), gt) < TOL


def test_gelu_matches_torch():
    x = (torch.linspace(-6, 6, 241, dtype=F64)).requires_grad_(True)
    ref = F.gelu(x)
    (g,) = torch.autograd.grad(ref.sum(), x)
    assert rel_l2(R.gelu(x.detach()), ref.detach()) < TOL and rel_l2(R.gelu_grad(x.detach()), g) < TOL
