"""TEST INFRASTRUCTURE ONLY -- the shapes, inputs and references of the per-kernel tests of the MWT3d training step
(tests/test_gpu_mwt_train_kernels.py runs the entry points of csrc/rpb_mwt_train.hip on them; tests/test_mwt_train_host.py checks without a
GPU that every case is well conditioned).  Every reference is torch autograd of the matching function of tests/mwt_restatement.py, in
fp64 and in fp32; the ReLU gates of lo_bwd come from the supplied ``z`` (a ReLU output: zeros and positive values), so no gate is
ambiguous there.  The head recomputes its hidden layer: its inputs are checked (``head_margin``) to keep every hidden unit away from zero.
Inputs are uniform in (-1, 1) from seeded generators; weights are those of tests/mwt_kernel_cases.py."""
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mwt_kernel_cases as K                 # noqa: E402
import mwt_restatement as R                  # noqa: E402
from mwt_kernel_cases import C, MODES, Case, _u          # noqa: E402
from realpdebench_amd.model.mwt import LevelPlan          # noqa: E402

# (B, Nx, Ny, T): the last one is ragged -- 135 cells: a partly valid 16-cell column tile, a K step of the weight gradient with one
# valid cell, Nx and Ny no powers of two
SHAPES = [(2, 8, 16, 8), (3, 4, 8, 10), (3, 1, 2, 8), (1, 3, 5, 9)]
ZERO_SHAPE = (3, 1, 2, 8)                    # where every kernel also runs on an all-zero g_out
WG_L = C * C * 27 + C


def _grads(out, g, *leaves):
    return torch.autograd.grad(out, leaves, g)


def _leaf(t, dt):
    return t.detach().to(dt).clone().requires_grad_()


def flipped_taps(cw):
    """w'[i][o][26 - tap] = w[o][i][tap]: a plain convolution with it is the data gradient (F.conv_transpose3d)"""
    return cw.transpose(0, 1).flip(2, 3, 4).contiguous()


def lo_case(B, Nx, Ny, T):
    i = dict(g=_u(40, B, Nx, Ny, T, C), z=F.relu(_u(41, B, Nx, Ny, T, C)), lo=K.conv_weights("B")[2])

    def ref(dt):
        z, lo = i["z"].to(dt), _leaf(i["lo"], dt)
        a, lb = _leaf(z, dt), torch.zeros(C, dtype=dt, requires_grad=True)
        gz, dlo, dlb = _grads(F.linear(a * (z > 0), lo, lb), i["g"].to(dt), a, lo, lb)
        return dict(gz=gz, part=torch.cat([dlo.reshape(-1), dlb]))
    return Case(f"lo_bwd ({B},{Nx},{Ny},{T})", i, ref)


def conv_bwd_case(B, Nx, Ny, T):
    cw = K.conv_weights("B")[0]
    i = dict(g=_u(42, B, Nx, Ny, T, C), x=_u(3, B, Nx, Ny, T, C), base=_u(4, B, Nx, Ny, T, C), cw=cw, wd=flipped_taps(cw))

    def ref(dt):
        x, w, b = _leaf(i["x"], dt), _leaf(cw, dt), torch.zeros(C, dtype=dt, requires_grad=True)
        with torch.backends.mkldnn.flags(enabled=False):      # oneDNN's fp32 convolution backward is off by 1e-6 and more: e32 would be its error
            y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, b, padding=1).permute(0, 2, 3, 4, 1)
            gx, dw, db = _grads(y, i["g"].to(dt), x, w, b)
        return dict(dgrad=gx, dgrad_acc=gx + i["base"].to(dt), wgrad=torch.cat([dw.reshape(-1), db]))
    return Case(f"conv3 backward ({B},{Nx},{Ny},{T})", i, ref)


def keep_case(B, Nx, Ny, T):
    cw, cb, lw, lb = K.conv_weights("C")
    wp, lop = K.conv3_layouts(cw, lw)
    i = dict(v=_u(3, B, Nx, Ny, T, C), base=_u(4, B, Nx, Ny, T, C), wp=wp, lop=lop, cb48=K.cb48(cb), lb=lb)

    def ref(dt):
        z = F.relu(F.conv3d(i["v"].to(dt).permute(0, 4, 1, 2, 3), cw.to(dt), cb.to(dt), padding=1)).permute(0, 2, 3, 4, 1)
        return dict(z=z.contiguous())
    return Case(f"conv3_keep ({B},{Nx},{Ny},{T})", i, ref)


def modes_bwd_case(B, Nx, Ny, T):
    plan = LevelPlan(Nx, Ny, T, MODES)
    NB = plan.KX * plan.KY * MODES
    Wt = K.spectral_weights()[0]
    i = dict(X=_u(43, B, 2, NB, C), gY=_u(44, B, 2, NB, C), Wt=Wt, base=_u(45, 4 * MODES ** 3, C, C, 2), plan=plan, NB=NB)

    def ref(dt):
        X, W = _leaf(i["X"], dt), _leaf(Wt, dt)
        gX, dW = _grads(R.modes(X.reshape(-1), W, plan.tab, B, NB), i["gY"].to(dt).reshape(-1), X, W)
        return dict(gX=gX, dWt=dW + i["base"].to(dt))
    return Case(f"modes_bwd ({B},{Nx},{Ny},{T})", i, ref)


# The head kernel recomputes its hidden layer in fp32, so its gate is the kernel's own: a hidden pre-activation (37 terms, sum |w x| <= 4)
# is reached with a rounding error of at most 37 * 2^-24 * 4 = 9e-6, and every one of a case must lie further than HEAD_MARGIN from
# zero.  HEAD_SEED is the first input seed from 50 upwards for which all four shapes do (seed 3 of the forward cases: 5e-7 at 262 k units).
HEAD_SEED, HEAD_MARGIN = 55, 1e-5
HEAD_DOUT = {(2, 8, 16, 8): (3, 1), (3, 4, 8, 10): (2, 2), (3, 1, 2, 8): (16, 1), (1, 3, 5, 9): (3, 2)}      # (Cout, r) per shape


def head_bwd_case(B, Nx, Ny, T):
    Cout, r = HEAD_DOUT[(B, Nx, Ny, T)]
    h = K.head_case(B, Nx, Ny, T, Cout, r)
    i = dict(h.inp, g=_u(46, B, T * r, Nx, Ny, Cout), Cout=Cout, r=r)
    i["v"] = _u(HEAD_SEED, B, Nx, Ny, T, C)

    def ref(dt):
        x, w0, b0, w1, b1 = (_leaf(i[k], dt) for k in ("v", "w0", "b0", "w1", "b1"))
        out = R.head(x, w0, b0, w1, b1, (T, Nx, Ny, 3), (T * r, Nx, Ny, Cout))
        gx, d0, db0, d1, db1 = _grads(out, i["g"].to(dt), x, w0, b0, w1, b1)
        return dict(gx=gx, part=torch.cat([d1.reshape(-1), db1, d0.reshape(-1), db0]))
    return Case(f"head_bwd ({B},{Nx},{Ny},{T}) Cout={Cout} r={r}", i, ref)


def head_margin(c):
    """smallest |hidden pre-activation| of a head case, fp64: a gate the fp32 kernel could take the other way would sit at ~1e-7"""
    return float(F.linear(c.v.double(), c.w0.double(), c.b0.double()).abs().min())


LIFT_CIN = {(2, 8, 16, 8): 3, (3, 4, 8, 10): 5, (3, 1, 2, 8): 64, (1, 3, 5, 9): 1}


def lift_wgrad_case(B, Nx, Ny, T):
    Cin = LIFT_CIN[(B, Nx, Ny, T)]
    i = dict(x=_u(1, B, T, Nx, Ny, Cin), g=_u(47, B, Nx, Ny, T, C), Cin=Cin)

    def ref(dt):
        w, b = torch.zeros(C, Cin, dtype=dt, requires_grad=True), torch.zeros(C, dtype=dt, requires_grad=True)
        dw, db = _grads(R.lift(i["x"].to(dt), w, b), i["g"].to(dt), w, b)
        return dict(part=torch.cat([dw.reshape(-1), db]))
    return Case(f"lift_wgrad ({B},{Nx},{Ny},{T}) Cin={Cin}", i, ref)


def spec_keep_case(B, Nx, Ny, T):
    c = K.spec_out_case(B * Nx * Ny, T)
    _, loT, lb = K.spectral_weights()
    i = dict(c.inp, loT=loT, lb=lb, lines=B * Nx * Ny, T=T)

    def ref(dt):
        v = torch.einsum("tk,lkc->ltc", i["GT"].to(dt), i["S"].to(dt))
        return dict(rv=F.relu(v).reshape(-1, C))
    return Case(f"spec_out_keep ({B},{Nx},{Ny},{T})", i, ref)


def all_cases():
    return [(make, s) for make in (lo_case, conv_bwd_case, keep_case, modes_bwd_case, head_bwd_case, lift_wgrad_case, spec_keep_case)
            for s in SHAPES]
