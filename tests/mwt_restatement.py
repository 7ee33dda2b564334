"""Plain-torch restatement of the MWT3d evaluation forward (reference realpdebench/model/MWT_libs/models.py:498-790) on the layout and
the host-side pieces of realpdebench_amd.model.mwt: its filter bank, its corner-block table and its truncated-DFT stage matrices --
no ``torch.fft`` on the full grid.  Runs on the CPU in fp32 or fp64; the GPU tests compare every kernel family against the matching
function here, and tests/test_mwt_host.py compares this file against the reference's vectors."""
import math

import torch
import torch.nn.functional as F

from realpdebench_amd.model.mwt import LevelPlan, cz_buffers


def lift(x, w, b):
    """[B,T,H,W,Cin] -> [B,H,W,T,36]"""
    return F.linear(x.permute(0, 2, 3, 1, 4), w, b)


def decompose(x, ec_d, ec_s):
    B, Nx, Ny, T, _ = x.shape
    x = x.reshape(B, Nx, Ny, T, 4, 9)
    xa = torch.cat([x[:, ::2, ::2], x[:, ::2, 1::2], x[:, 1::2, ::2], x[:, 1::2, 1::2]], -1)
    return (xa @ ec_d).reshape(B, Nx // 2, Ny // 2, T, 36), (xa @ ec_s).reshape(B, Nx // 2, Ny // 2, T, 36)


def reconstruct(x, us, ud, rc, relu):
    """rc [4][18][9] in the order ee, eo, oe, oo; x broadcasts along Ny when it has one column."""
    B, Nx, Ny, T, _ = us.shape
    v = torch.cat(((x + us).reshape(B, Nx, Ny, T, 4, 9), ud.reshape(B, Nx, Ny, T, 4, 9)), -1)
    out = torch.zeros(B, 2 * Nx, 2 * Ny, T, 4, 9, dtype=us.dtype)
    out[:, ::2, ::2], out[:, ::2, 1::2] = v @ rc[0], v @ rc[1]
    out[:, 1::2, ::2], out[:, 1::2, 1::2] = v @ rc[2], v @ rc[3]
    out = out.reshape(B, 2 * Nx, 2 * Ny, T, 36)
    return F.relu(out) if relu else out


def coarse(x, w, b):
    """x [B][1][mult][T][36], read as (B, 1, 1, T, 36 * mult) in row-major order"""
    B, T = x.shape[0], x.shape[3]
    return F.linear(x.reshape(B, 1, 1, T, -1), w, b)


def conv3(x, cw, cb, low, lob):
    h = F.relu(F.conv3d(x.permute(0, 4, 1, 2, 3), cw, cb, padding=1)).permute(0, 2, 3, 4, 1)
    return F.linear(h, low, lob)


def spectral(d, weights, low, lob, plan):
    """sparseKernelFT3d: ``weights`` = (weights1..4) complex [36,36,m,m,m]; ``plan`` a LevelPlan of d's grid."""
    B, Nx, Ny, T, C = d.shape
    m, KX, KY = plan.modes, plan.KX, plan.KY
    dt = d.dtype
    M = lambda t: t.to(dt)
    y = torch.einsum("ot,bxytc->bxyoc", M(plan.FT), d).reshape(B, Nx, Ny, 2, m, C)
    y = torch.einsum("pkyr,bxyrmc->bxpkmc", M(plan.FY).reshape(2, KY, Ny, 2), y)
    X = torch.einsum("pkxr,bxrjmc->bpkjmc", M(plan.FX).reshape(2, KX, Nx, 2), y)
    Xc = torch.complex(X[:, 0], X[:, 1]).reshape(B, KX * KY * m, C)
    cdt = torch.complex128 if dt == torch.float64 else torch.complex64
    W = torch.stack([w.to(cdt) for w in weights]).permute(0, 3, 4, 5, 1, 2).reshape(4 * m ** 3, C, C)
    Yc = torch.einsum("bni,nio->bno", Xc, W[plan.tab.long()]).reshape(B, KX, KY, m, C)
    Y = torch.stack([Yc.real, Yc.imag], 1)
    z = torch.einsum("xprk,brkjmc->bxpjmc", M(plan.GX).reshape(Nx, 2, 2, KX), Y)
    z = torch.einsum("yprj,bxrjmc->bxypmc", M(plan.GY).reshape(Ny, 2, 2, KY), z)
    v = torch.einsum("to,bxyoc->bxytc", M(plan.GT), z.reshape(B, Nx, Ny, 2 * m, C))
    return F.linear(F.relu(v), low, lob)


# ---- ``spectral`` once more, one function per launch of MWT3d.k_spectral (rpb_mwt_axis x 3, rpb_mwt_modes, rpb_mwt_axis x 2,
#      rpb_mwt_spec_out) on the flat buffers the kernels exchange; tests/test_mwt_kernels_host.py asserts that they compose to it
def axis(inp, M, outer, inner):
    """out[outer][o][inner] = sum_k M[o][k] in[outer][k][inner]"""
    O, K = M.shape
    return torch.einsum("ok,ukn->uon", M.to(inp.dtype), inp.reshape(outer, K, inner)).reshape(-1)


def modes(X, Wt, tab, B, NB):
    """X [B][2 (re|im)][NB][36] planar, Wt [weight bins][36 in][36 out][2], tab [NB] -> Y like X"""
    X = X.reshape(B, 2, NB, 36)
    W = Wt.to(X.dtype)[tab.long()]                                # [NB][in][out][2]
    a, b, wr, wi = X[:, 0], X[:, 1], W[..., 0], W[..., 1]
    yr = torch.einsum("bni,nio->bno", a, wr) - torch.einsum("bni,nio->bno", b, wi)
    yi = torch.einsum("bni,nio->bno", a, wi) + torch.einsum("bni,nio->bno", b, wr)
    return torch.stack([yr, yi], 1).reshape(-1)


def spec_out(S, GT, loT, lb, lines, T):
    """S [lines][K2][36], GT [T][K2], loT [36 in][36 out] -> [lines * T][36]"""
    dt = S.dtype
    v = torch.einsum("tk,lkc->ltc", GT.to(dt), S.reshape(lines, GT.shape[1], 36))
    return (F.relu(v) @ loT.to(dt) + lb.to(dt)).reshape(lines * T, 36)


def spectral_stage_calls(B, plan):
    """(matrix name, outer, inner) of the five rpb_mwt_axis launches of MWT3d.k_spectral, in order (rpb_mwt_modes runs after the third)"""
    Nx, Ny, m, KY, C = plan.Nx, plan.Ny, plan.modes, plan.KY, 36
    return [("FT", B * Nx * Ny, C), ("FY", B * Nx, m * C), ("FX", B, KY * m * C), ("GX", B, KY * m * C), ("GY", B * Nx, m * C)]


def spectral_by_stages(d, Wt, loT, lb, plan, keep=None):
    """``spectral`` as the composition of the stage functions; ``keep`` (a list) receives every stage's output"""
    B, Nx, Ny, T, _ = d.shape
    calls = spectral_stage_calls(B, plan)
    y = d.reshape(-1)
    for i, (name, outer, inner) in enumerate(calls):
        if i == 3:
            y = modes(y, Wt, plan.tab, B, plan.KX * plan.KY * plan.modes)
            if keep is not None:
                keep.append(y)
        y = axis(y, getattr(plan, name), outer, inner)
        if keep is not None:
            keep.append(y)
    out = spec_out(y, plan.GT, loT, lb, B * Nx * Ny, T).reshape(B, Nx, Ny, T, 36)
    if keep is not None:
        keep.append(out)
    return out


def head(x, w0, b0, w1, b1, shape_in, shape_out):
    B, Nx, Ny, T, _ = x.shape
    y = F.linear(F.relu(F.linear(x, w0, b0)), w1, b1)
    r = shape_out[0] // shape_in[0]
    y = y.reshape(B, Nx, Ny, T, shape_out[-1], r)
    return y.permute(0, 3, 5, 1, 2, 4).reshape(B, *shape_out)


def cz_block(x, sd, pre, relu, alpha=5, keep=None):
    """One MWT_CZ3d on x [B][Nx][Ny][T][36]; ``sd``: reference-named weights, ``pre`` = 'MWT_CZ.i.'.  The filter buffers are the
    project's own (cz_buffers), not entries of ``sd``."""
    dt = x.dtype
    buf = {k_: v.to(dt) for k_, v in cz_buffers(3).items()}
    rc = torch.stack([buf["rc_ee"], buf["rc_eo"], buf["rc_oe"], buf["rc_oo"]])
    g = lambda n: sd[pre + n].to(dt)
    ns = int(math.log2(x.shape[1]))
    T = x.shape[3]
    Ud, Us = [], []
    for i in range(ns):
        d, x = decompose(x, buf["ec_d"], buf["ec_s"])
        plan = LevelPlan(d.shape[1], d.shape[2], T, alpha)
        a = spectral(d, [sd[pre + f"A.weights{j}"] for j in range(1, 5)], g("A.Lo.weight"), g("A.Lo.bias"), plan)
        b = conv3(x, g("B.conv.0.weight"), g("B.conv.0.bias"), g("B.Lo.weight"), g("B.Lo.bias"))
        c = conv3(d, g("C.conv.0.weight"), g("C.conv.0.bias"), g("C.Lo.weight"), g("C.Lo.bias"))
        Ud.append(a + b)
        Us.append(c)
        if keep is not None:
            for name, t in (("d", d), ("s", x), ("A", a), ("B", b), ("C", c)):
                keep[f"{name}{i}"] = t
    x = coarse(x, g("T0.weight"), g("T0.bias"))
    for i in range(ns - 1, -1, -1):
        x = reconstruct(x, Us[i], Ud[i], rc, False)
        if keep is not None:
            keep[f"eo{i}"] = x                   # evenOdd's own output, before the ReLU between two blocks
    return F.relu(x) if relu else x


def forward(sd, x, shape_in, shape_out, nCZ, alpha=5, keep=None):
    """Whole model; ``keep`` (a dict) receives the per-level tensors of CZ block 0."""
    dt = x.dtype
    h = lift(x, sd["Lk.weight"].to(dt), sd["Lk.bias"].to(dt))
    for i in range(nCZ):
        h = cz_block(h, sd, f"MWT_CZ.{i}.", i < nCZ - 1, alpha, keep if i == 0 else None)
    return head(h, sd["Lc0.weight"].to(dt), sd["Lc0.bias"].to(dt), sd["Lc1.weight"].to(dt), sd["Lc1.bias"].to(dt), shape_in, shape_out)
