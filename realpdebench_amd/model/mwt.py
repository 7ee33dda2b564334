"""MWT3d (multiwavelet operator) on MI355X -- drop-in for ``realpdebench.model.MWT_libs.models.MWT3d`` (reference
realpdebench/model/MWT_libs/models.py:498-790, built by ``load_model`` like model/load_model.py:93-107) for the configuration family of
the reference's ``configs/*/mwt.yaml``: ``k: 3, alpha: 5, c: 4, nCZ: 4, L: 0, base: legendre``.

Evaluation forward, ``train_loss`` as a value, the autoregressive rollout and checkpoint I/O.  By default every attempt to
backpropagate raises ``NotImplementedError`` (``_common.EvalByDefault``) instead of returning tensors without a graph.
``enable_training()`` (``hip_training: true`` through ``load_model``) opts an instance in: in ``train()`` mode ``forward`` /
``train_loss`` then run through ``_common.HipFunction``; the adjoints of the wavelet maps and of the DFT stages are the forward's own
launches on transposed tables, the rest is ``csrc/rpb_mwt_train.hip``.

Pipeline (activations channels-last fp32 ``[B][Nx][Ny][T][36]``, 36 = (c, k^2) = (4, 9); every product runs in a HIP kernel of
``csrc/rpb_mwt.hip``; no reference permute survives):
  rpb_mwt_lift (the [B,T,H,W,C] permute + Lk) -> nCZ x MWT_CZ3d -> rpb_mwt_head (Lc0, ReLU, Lc1, the output permute).
  MWT_CZ3d (models.py:651-680), Nx = H halves ``ns = log2 H`` times:
    level i:  rpb_mwt_decompose: x -> d_i, s_i (2 x 2 gather, ec_d / ec_s)
              Ud_i = A(d_i) + B(s_i):  A = truncated DFT (rpb_mwt_axis: T, Ny, Nx) -> rpb_mwt_modes (36 x 36 complex per retained bin,
                       through the corner table below) -> rpb_mwt_axis (Nx, Ny) -> rpb_mwt_spec_out (c2r along T, ReLU, Lo);
                       B = rpb_mwt_conv3 (3x3x3 convolution, ReLU, Lo) accumulating into Ud_i
              Us_i = C(d_i):  rpb_mwt_conv3
    coarsest: rpb_mwt_coarse (T0 on the row-major (B, 1, 1, T, 36 * W/H) view)
    level i, upwards: rpb_mwt_reconstruct (x + Us_i, cat Ud_i, rc_*, scatter to the 2 x 2 children; the ReLU between two CZ blocks
              rides in the top level's launch)
``set_arith("bf16x3" | "f16x2")`` moves the rpb_mwt_conv3 launches (and nothing else) to rpb_mwt_conv3x of ``csrc/rpb_mwt3x.hip``: the
same operator with its operands as 16-bit planes on the bf16 / fp16 matrix pipe; the default ``"f32"`` is the parity path.
``BN`` (one BatchNorm3d per CZ block) exists for ``state_dict`` compatibility and is never computed, as in the reference.

Parameters carry the reference's names, shapes and dtypes (``nn`` modules of the same tree), so ``state_dict`` / ``load_state_dict``
are the reference's; the kernel layouts (lane-ordered convolution weights, mode-major spectral weights, transposed linears) are
derived tensors rebuilt when a parameter changed (``_prep``, through the model's ``LayoutCache``).
"""
import math

import numpy as np
import torch
import torch.nn as nn
from numpy.polynomial import Polynomial
from numpy.polynomial import legendre as npleg

from .. import _lib, ops
from ..dft import _fwd_complex, _fwd_real, _inv_complex, _inv_real
from ..ops import _p, _stream
from ._common import EvalByDefault
from .model import Model

I16, I32 = torch.int16, torch.int32

_PLANES = {"bf16x3": 3, "f16x2": 2}      # 16-bit planes per operand of rpb_mwt_conv3x


# ----------------------------------------------------------------------------------------------------------- filter bank (numpy only)
def _int01(p, a, b):
    q = p.integ()
    return q(b) - q(a)


def _clean(a):
    a[np.abs(a) < 1e-8] = 0
    return a


def legendre_filter(k):
    """``get_filter('legendre', k)`` of the reference (MWT_libs/utils_MWT.py:22-72,131-190) without sympy / scipy: the orthonormal
    Legendre scaling functions phi_i(x) = sqrt(2i+1) P_i(2x-1) on [0, 1], the multiwavelets psi_i by Gram-Schmidt of sqrt(2) phi_i(2x)
    (piecewise polynomials psi1 on [0, 1/2], psi2 on [1/2, 1]) and the two-scale matrices by k-point Gauss-Legendre quadrature.
    Returns (H0, H1, G0, G1, PHI0, PHI1), float64."""
    k = int(k)
    lin = lambda a, b: Polynomial([a, b])
    P = [Polynomial(npleg.leg2poly([0.0] * i + [1.0])) for i in range(k)]
    phi = [math.sqrt(2 * i + 1) * P[i](lin(-1.0, 2.0)) for i in range(k)]
    phi2 = [math.sqrt(2.0) * math.sqrt(2 * i + 1) * P[i](lin(-1.0, 4.0)) for i in range(k)]
    psi1, psi2 = [], []
    for i in range(k):
        p1, p2 = phi2[i], Polynomial([0.0])
        for j in range(k):
            proj = _int01(phi2[i] * phi[j], 0.0, 0.5)
            p1, p2 = p1 - proj * phi[j], p2 - proj * phi[j]
        for j in range(i):
            proj = _int01(phi2[i] * psi1[j], 0.0, 0.5)
            p1, p2 = p1 - proj * psi1[j], p2 - proj * psi2[j]
        norm = math.sqrt(_int01(p1 * p1, 0.0, 0.5) + _int01(p2 * p2, 0.5, 1.0))
        pad = lambda p: np.concatenate([p.coef, np.zeros(k)])[:k]
        psi1.append(Polynomial(_clean(pad(p1) / norm)))
        psi2.append(Polynomial(_clean(pad(p2) / norm)))
    xg, wg = npleg.leggauss(k)
    xm, wm = (xg + 1.0) / 2.0, wg / 2.0
    psi = lambda i, x: np.where(x <= 0.5, psi1[i](x), psi2[i](x))
    H0, H1, G0, G1 = (np.zeros((k, k)) for _ in range(4))
    for a in range(k):
        for b in range(k):
            H0[a, b] = (wm * phi[a](xm / 2) * phi[b](xm)).sum() / math.sqrt(2.0)
            G0[a, b] = (wm * psi(a, xm / 2) * phi[b](xm)).sum() / math.sqrt(2.0)
            H1[a, b] = (wm * phi[a]((xm + 1) / 2) * phi[b](xm)).sum() / math.sqrt(2.0)
            G1[a, b] = (wm * psi(a, (xm + 1) / 2) * phi[b](xm)).sum() / math.sqrt(2.0)
    return _clean(H0), _clean(H1), _clean(G0), _clean(G1), np.eye(k), np.eye(k)


def cz_buffers(k, base="legendre"):
    """The six constant maps of MWT_CZ3d (models.py:599-648), float32: ec_s, ec_d [4 k^2, k^2]; rc_ee, rc_eo, rc_oe, rc_oo [2 k^2, k^2]."""
    if base != "legendre":
        raise NotImplementedError(f"MI355X MWT3d: base={base!r} is not built (no reference YAML uses it); only base='legendre'")
    H0, H1, G0, G1, PHI0, PHI1 = legendre_filter(k)
    H0r, G0r, H1r, G1r = _clean(H0 @ PHI0), _clean(G0 @ PHI0), _clean(H1 @ PHI1), _clean(G1 @ PHI1)
    kr, cat = np.kron, lambda *a: torch.tensor(np.concatenate(a, axis=0), dtype=torch.float32)
    return {
        "ec_s": cat(kr(H0, H0).T, kr(H0, H1).T, kr(H1, H0).T, kr(H1, H1).T),
        "ec_d": cat(kr(G0, G0).T, kr(G0, G1).T, kr(G1, G0).T, kr(G1, G1).T),
        "rc_ee": cat(kr(H0r, H0r), kr(G0r, G0r)),
        "rc_eo": cat(kr(H0r, H1r), kr(G0r, G1r)),
        "rc_oe": cat(kr(H1r, H0r), kr(G1r, G0r)),
        "rc_oo": cat(kr(H1r, H1r), kr(G1r, G1r)),
    }


def adjoint_tables(ec_d, ec_s, rc):
    """The tables on which ``reconstruct`` / ``decompose`` are each other's adjoints (the wavelet maps are constant; k^2 = 9).
    ``rc_adj`` [4][18][9]: ``reconstruct(0, g_s, g_d, rc_adj)`` is the adjoint of ``decompose`` (child j reads ec_s / ec_d rows 9j..9j+8,
    transposed).  ``ec_d_adj``, ``ec_s_adj`` [36][9]: ``decompose(g, ec_d_adj, ec_s_adj)`` gives (g_ud, g_(x + us)) of ``reconstruct``
    (rows 9..17 / 0..8 of every ``rc[j]``, transposed).  ``rc``: the four maps in the order ee, eo, oe, oo."""
    rc_adj = torch.stack([torch.cat([ec_s[9 * j:9 * j + 9].t(), ec_d[9 * j:9 * j + 9].t()]) for j in range(4)]).contiguous()
    ec_d_adj = torch.cat([r[9:18].t() for r in rc]).contiguous()
    ec_s_adj = torch.cat([r[0:9].t() for r in rc]).contiguous()
    return rc_adj, ec_d_adj, ec_s_adj


# ----------------------------------------------------------------------------------------------------------- corner-block table
def _axis_rows(n, modes):
    """Retained frequency rows of a two-sided axis of length ``n`` and, per row, (high, weight index): ``[:l]`` reads weight rows
    0..l-1, ``[-l:]`` reads them again on rows n-l..n-1; where the two overlap the later (high) assignment wins (models.py:569-576)."""
    l = min(modes, n // 2 + 1)
    rows = sorted(set(range(l)) | set(range(n - l, n)))
    return rows, [(1, r - (n - l)) if r >= n - l else (0, r) for r in rows]


def corner_table(Nx, Ny, modes):
    """(kx rows, ky rows, tab): ``tab[(a * KY + b) * modes + kt]`` = block * modes^3 + (ix * modes + iy) * modes + kt, block 0..3 =
    weights1..4, for the retained output bin (kx[a], ky[b], kt) of sparseKernelFT3d at an ``Nx x Ny`` level."""
    kx, mx = _axis_rows(Nx, modes)
    ky, my = _axis_rows(Ny, modes)
    tab = np.empty((len(kx), len(ky), modes), dtype=np.int32)
    for a, (hx, ix) in enumerate(mx):
        for b, (hy, iy) in enumerate(my):
            tab[a, b] = (hx + 2 * hy) * modes ** 3 + (ix * modes + iy) * modes + np.arange(modes)
    return kx, ky, tab.reshape(-1)


class LevelPlan:
    """Truncated-DFT stage matrices (dft.py conventions) and the corner table of one ``Nx x Ny x T`` level."""

    def __init__(self, Nx, Ny, T, modes, device="cpu"):
        self.Nx, self.Ny, self.T, self.modes = Nx, Ny, T, modes
        self.kx, self.ky, tab = corner_table(Nx, Ny, modes)
        self.KX, self.KY = len(self.kx), len(self.ky)
        kt = list(range(modes))
        f = lambda m: torch.from_numpy(np.ascontiguousarray(m)).to(torch.float32).to(device)
        self.FT = f(_fwd_real(T, kt))                       # [2 m, T]
        self.FY = f(_fwd_complex(Ny, self.ky))              # [2 KY, 2 Ny]
        self.FX = f(_fwd_complex(Nx, self.kx))              # [2 KX, 2 Nx]
        self.GX = f(_inv_complex(Nx, self.kx))              # [2 Nx, 2 KX]
        self.GY = f(_inv_complex(Ny, self.ky))              # [2 Ny, 2 KY]
        self.GT = f(_inv_real(T, kt, float(Nx) * Ny * T))   # [T, 2 m]: c2r of irfftn incl. 1 / (Nx Ny T)
        self.tab = torch.from_numpy(tab).to(device)
        self._adj = {}

    def adj(self, name):
        """The transposed stage matrix ``name``: the stages are constant linear maps, so the adjoint of an ``rpb_mwt_axis`` launch is
        the same launch on this table (the training step; built once per plan)."""
        if name not in self._adj:
            self._adj[name] = getattr(self, name).t().contiguous()
        return self._adj[name]


# ----------------------------------------------------------------------------------------------------------- parameter tree
class _SparseKernelFT3d(nn.Module):
    def __init__(self, k, alpha, c):
        super().__init__()
        w = c * k ** 2
        for i in range(1, 5):
            p = nn.Parameter(torch.zeros(w, w, alpha, alpha, alpha, dtype=torch.cfloat))
            nn.init.xavier_normal_(p)
            setattr(self, f"weights{i}", p)
        self.Lo = nn.Linear(w, w)


class _SparseKernel3d(nn.Module):
    def __init__(self, k, c):
        super().__init__()
        w = c * k ** 2
        self.conv = nn.Sequential(nn.Conv3d(w, w, 3, 1, 1), nn.ReLU(inplace=True))
        self.Lo = nn.Linear(w, w)


class _CZ(nn.Module):
    def __init__(self, k, alpha, c, mult, base, initializer):
        super().__init__()
        self.A = _SparseKernelFT3d(k, alpha, c)
        self.B = _SparseKernel3d(k, c)
        self.C = _SparseKernel3d(k, c)
        self.T0 = nn.Linear(c * k ** 2 * mult, c * k ** 2)
        if initializer is not None:
            initializer(self.T0.weight)
        for name, t in cz_buffers(k, base).items():
            self.register_buffer(name, t)


class MWT3d(EvalByDefault, Model):
    """``set_arith`` selects the arithmetic of the ``sparseKernel3d`` convolutions (kernels B and C of every CZ block and level) in the
    evaluation / rollout forward: ``"f32"`` (default, the parity path: ``rpb_mwt_conv3`` on the fp32 MFMA), ``"bf16x3"`` (opt-in:
    operands as three bf16 planes, ``hi + mid + lo`` exact, six products per fp32 product, fp32 accumulation) or ``"f16x2"`` (opt-in:
    operands as two fp16 planes of the tensor scaled by a power of two, three products, dropped term <= 2^-22; csrc/rpb_mwt3x.hip).
    Everything else in the forward is unchanged; training stays refused under every mode, and the opt-in training step
    (``enable_training()``) runs the ``"f32"`` kernels whatever is selected here."""
    batch_independent = True     # no batch statistics are ever computed (BN is never called): an enabled instance keeps declaring it
    training_unavailable = EvalByDefault.TRAIN_MSG.format("MWT", "MWT3d")
    # An enabled instance (``enable_training()``) runs the ``"f32"`` kernels whatever ``set_arith`` says;
    # ``micro_batch`` works, more than one rank is refused.
    DP_MSG = "MWT3d training has only been verified on one rank: data-parallel training is not built, run it on one rank"
    ARITHS = ("f32", "bf16x3", "f16x2")

    def __init__(self, k=3, alpha=2, c=1, nCZ=3, L=0, base="legendre", initializer=None, shape_in=None, shape_out=None, **kwargs):
        super().__init__()
        self.shape_in, self.shape_out = tuple(int(v) for v in shape_in), tuple(int(v) for v in shape_out)
        T, H, W, Cin = self.shape_in
        unsupported = []
        if base != "legendre":
            raise NotImplementedError(f"MI355X MWT3d: base={base!r} is not built (no reference YAML uses it); only base='legendre'")
        if L != 0:
            unsupported.append(f"L={L} (only L=0)")
        if c * k ** 2 != 36:
            unsupported.append(f"c*k^2={c * k ** 2} (the kernels are built for 36 = 4 * 3^2)")
        if H < 2 or H & (H - 1):
            unsupported.append(f"H={H} is not a power of two")
        elif W % H or (W // H) & (W // H - 1):
            unsupported.append(f"W={W} is not H * 2^j")
        if T // 2 + 1 < alpha:
            unsupported.append(f"T={T} keeps {T // 2 + 1} rfft bins < alpha={alpha}")
        if self.shape_out[0] % T or tuple(self.shape_out[1:3]) != (H, W):
            unsupported.append(f"shape_out={self.shape_out} (T_out must be a multiple of T_in on the same grid)")
        if unsupported:
            raise NotImplementedError("MI355X MWT3d covers the configuration family of the reference's configs/*/mwt.yaml; "
                                      "unsupported: " + "; ".join(unsupported))
        self.k, self.c, self.L, self.nCZ, self.alpha = int(k), int(c), int(L), int(nCZ), int(alpha)
        self.dim_in = Cin
        self.dim_out = self.shape_out[-1] * self.shape_out[0] // T
        self.mult = W // H
        self.ns = int(math.log2(H))
        w = c * k ** 2
        self.Lk = nn.Linear(Cin, w)
        self.MWT_CZ = nn.ModuleList([_CZ(k, alpha, c, self.mult, base, initializer) for _ in range(nCZ)])
        self.BN = nn.ModuleList([nn.BatchNorm3d(w) for _ in range(nCZ)])
        self.Lc0 = nn.Linear(w, 128)
        self.Lc1 = nn.Linear(128, self.dim_out)
        if initializer is not None:
            initializer(self.Lc0.weight)
            initializer(self.Lc1.weight)
        self._plans = {}

    # ------------------------------------------------------------------ checkpoints (models.py:791-844)
    def state_dict(self, *args, **kwargs):
        """The reference's names, shapes and dtypes.  Inside ``ArenaTrainer`` the complex64 weights view the one fp32 allocation every
        other parameter views, and ``torch.save`` refuses two dtypes on one storage: such entries are handed out as copies."""
        sd = super().state_dict(*args, **kwargs)
        if not kwargs.get("keep_vars", False):
            for k, v in sd.items():
                if torch.is_tensor(v) and v.is_complex() and v.untyped_storage().nbytes() > v.numel() * v.element_size():
                    sd[k] = v.clone()
        return sd

    def load_checkpoint(self, checkpoint_path, device="cpu"):
        """Key and shape matching as in the reference: entries whose name and shape agree are loaded, the rest are reported and left.
        Returns the bookkeeping entries like the other models; a bare weights file (which the reference's method accepts too) gives
        the entries of an untrained run (iteration 0, no losses)."""
        import logging
        ck = torch.load(checkpoint_path, map_location="cpu")
        sd = ck.get("model", ck.get("model_state_dict", ck))
        own = self.state_dict()
        ok = {key: v for key, v in sd.items() if key in own and tuple(v.shape) == tuple(own[key].shape)}
        skipped = [key for key in sd if key not in ok]
        logging.info(f"MWT3d.load_checkpoint: {len(ok)}/{len(sd)} entries match" + (f"; skipped {skipped[:5]}" if skipped else ""))
        self.load_state_dict(ok, strict=False)
        self.to(device)
        return self._bookkeeping(ck if sd is not ck else {})

    # ------------------------------------------------------------------ kernel-side layouts
    def _plan(self, Nx, Ny, device):
        key = (Nx, Ny, str(device))
        if key not in self._plans:
            self._plans[key] = LevelPlan(Nx, Ny, self.shape_in[0], self.alpha, device)
        return self._plans[key]

    def _prep(self, device):
        """The kernel-side layouts; the 16-bit planes of the convolution weights only for the selected arithmetic."""
        return self._layouts.get("prep", list(self.parameters()) + list(self.buffers()), lambda: self._build_prep(device, self.arith),
                                 extra=self.arith)

    def _prep_train(self, device):
        """The layouts of the training step: the ``"f32"`` ones plus the transposed wavelet tables, the flipped and transposed
        convolution taps and the ``Lo`` weights as they are."""
        return self._layouts.get("prep_train", list(self.parameters()) + list(self.buffers()),
                                 lambda: self._build_prep(device, "f32", train=True))

    def _build_prep(self, device, arith, train=False):
        f = dict(device=device, dtype=torch.float32)
        czs = []
        for cz in self.MWT_CZ:
            d = {}
            for name in ("B", "C"):
                m = getattr(cz, name)
                wp, lop = torch.empty(27 * 9 * 3 * 64, **f), torch.empty(3 * 4 * 3 * 64, **f)
                _lib.call("rpb_mwt_conv3_wprep", _p(m.conv[0].weight.detach().contiguous()), _p(m.Lo.weight.detach().contiguous()),
                          _p(wp), _p(lop), _stream())
                cb = torch.zeros(48, **f)
                cb[:36] = m.conv[0].bias.detach()
                d[name] = (wp, cb, lop, m.Lo.bias.detach().contiguous())
                if arith != "f32":                # the A operand as 16-bit planes, only for the selected mode
                    d[name] += self.k_conv3_wprep(m.conv[0].weight.detach().contiguous(), arith)
                if train:                         # the data gradient: the same main loop on w'[i][o][26 - tap] = w[o][i][tap]
                    d[name + "d"] = self.k_conv3_dgrad_wprep(m.conv[0].weight.detach())
            if train:
                d["lo"] = {name: getattr(cz, name).Lo.weight.detach().contiguous() for name in ("A", "B", "C")}
                d["rc_adj"], d["ec_d_adj"], d["ec_s_adj"] = adjoint_tables(cz.ec_d, cz.ec_s, [cz.rc_ee, cz.rc_eo, cz.rc_oe, cz.rc_oo])
            A = cz.A
            ws = torch.stack([getattr(A, f"weights{i}").detach() for i in range(1, 5)])          # [4][i][o][x][y][t]
            d["Wt"] = torch.view_as_real(ws.permute(0, 3, 4, 5, 1, 2).contiguous()).contiguous()  # [4][x][y][t][i][o][2]
            d["loT"], d["lb"] = A.Lo.weight.detach().t().contiguous(), A.Lo.bias.detach().contiguous()
            d["T0w"], d["T0b"] = cz.T0.weight.detach().contiguous(), cz.T0.bias.detach().contiguous()
            d["rc"] = torch.stack([cz.rc_ee, cz.rc_eo, cz.rc_oe, cz.rc_oo]).contiguous()
            d["ec_d"], d["ec_s"] = cz.ec_d.contiguous(), cz.ec_s.contiguous()
            czs.append(d)
        return dict(cz=czs, Lkw=self.Lk.weight.detach().contiguous(), Lkb=self.Lk.bias.detach().contiguous(),
                    w0t=self.Lc0.weight.detach().t().contiguous(), b0=self.Lc0.bias.detach().contiguous(),
                    w1=self.Lc1.weight.detach().contiguous(), b1=self.Lc1.bias.detach().contiguous())

    # ------------------------------------------------------------------ the kernels, one method per family (tests call these)
    @staticmethod
    def k_lift(x, w, b):
        B, T, H, W, Cin = x.shape
        out = torch.empty(B, H, W, T, 36, device=x.device, dtype=torch.float32)
        _lib.call("rpb_mwt_lift", _p(x), _p(w), _p(b), _p(out), B, T, H, W, Cin, _stream(), label="mwt_lift",
                  nbytes=4 * B * T * H * W * (Cin + 36))
        return out

    @staticmethod
    def k_decompose(x, ec_d, ec_s):
        B, Nx, Ny, T, _ = x.shape
        d = torch.empty(B, Nx // 2, Ny // 2, T, 36, device=x.device, dtype=torch.float32)
        s = torch.empty_like(d)
        _lib.call("rpb_mwt_decompose", _p(x), _p(ec_d), _p(ec_s), _p(d), _p(s), B, Nx // 2, Ny // 2, T, _stream(), label="mwt_decompose",
                  nbytes=4 * x.numel() + 8 * d.numel(), flops=2 * 2 * 36 * d.numel())
        return d, s

    @staticmethod
    def k_reconstruct(x, us, ud, rc, relu):
        B, Nx, Ny, T, _ = us.shape
        out = torch.empty(B, 2 * Nx, 2 * Ny, T, 36, device=us.device, dtype=torch.float32)
        _lib.call("rpb_mwt_reconstruct", _p(x), _p(us), _p(ud), _p(rc), _p(out), B, Nx, Ny, T, x.shape[2], int(relu), _stream(),
                  label="mwt_reconstruct", nbytes=4 * (x.numel() + 2 * us.numel() + out.numel()), flops=2 * 4 * 18 * us.numel())
        return out

    @staticmethod
    def k_coarse(x, w, b):
        B, T = x.shape[0], x.shape[3]
        K = w.shape[1]
        out = torch.empty(B, 1, 1, T, 36, device=x.device, dtype=torch.float32)
        _lib.call("rpb_mwt_coarse", _p(x), _p(w), _p(b), _p(out), B * T, K, _stream(), label="mwt_coarse")
        return out

    @staticmethod
    def k_conv3_wprep(w, arith):
        """Conv3d weight [36][36][3][3][3] -> (wpx, ew): the planes of ``rpb_mwt_conv3x`` for ``arith`` and, for ``"f16x2"``, the
        weight's power-of-two exponent (int32 on the device; None for ``"bf16x3"``)."""
        planes = _PLANES[arith]
        wpx = torch.empty(31 * 3 * planes * 64 * 8, device=w.device, dtype=torch.int16)
        ew = None
        if planes == 2:
            ew = torch.empty(1, device=w.device, dtype=torch.int32)
            _lib.call("rpb_amax_exp", _p(w), 36, 972, 972, _p(ew, I32), _stream(), label="amax_exp", nbytes=4 * w.numel())
        _lib.call("rpb_mwt_conv3x_wprep", _p(w), _p(wpx, I16), planes, _p(ew, I32), _stream())
        return wpx, ew

    @staticmethod
    def k_conv3(x, pack, out=None, arith="f32"):
        """sparseKernel3d; ``out`` given = accumulate into it.  ``arith`` other than ``"f32"`` needs the pack extended by
        ``k_conv3_wprep`` for that mode."""
        wp, cb, lop, lb = pack[:4]
        B, Nx, Ny, T, _ = x.shape
        acc = out is not None
        if out is None:
            out = torch.empty_like(x)
        nbytes, flops = 4 * x.numel() * (3 if acc else 2), 2 * x.numel() * (27 * 36 + 36)
        if arith != "f32":
            if len(pack) != 6 or pack[4].numel() != 31 * 3 * _PLANES[arith] * 64 * 8:
                raise _lib.RpbError(f"k_conv3: the weight pack was not prepared for arith={arith!r}")
            wpx, ew = pack[4:]
            planes, ea = _PLANES[arith], None
            if planes == 2:                       # per-tensor exponent of the activations, kept on the device
                ea = torch.empty(1, device=x.device, dtype=torch.int32)
                _lib.call("rpb_amax_exp", _p(x), x.numel() // 36, 36, 36, _p(ea, I32), _stream(), label="mwt_amax_exp", nbytes=4 * x.numel())
            _lib.call("rpb_mwt_conv3x", _p(x), _p(wpx, I16), _p(cb), _p(lop), _p(lb), _p(out), B, Nx, Ny, T, int(acc), planes,
                      _p(ea, I32), _p(ew, I32), _stream(),
                      label=f"mwt_conv3[{arith}]", nbytes=nbytes, flops=flops)
            return out
        _lib.call("rpb_mwt_conv3", _p(x), _p(wp), _p(cb), _p(lop), _p(lb), _p(out), B, Nx, Ny, T, int(acc), _stream(), label="mwt_conv3",
                  nbytes=nbytes, flops=flops)
        return out

    @staticmethod
    def k_axis(inp, M, outer, inner):
        O, K = M.shape
        out = torch.empty(outer * O * inner, device=inp.device, dtype=torch.float32)
        _lib.call("rpb_mwt_axis", _p(inp), _p(M), _p(out), outer, O, K, inner, _stream(), label="mwt_axis",
                  nbytes=4 * outer * inner * (O + K), flops=2 * outer * inner * O * K)
        return out

    @staticmethod
    def k_spectral(d, plan, Wt, loT, lb, out=None, keep=None):
        """sparseKernelFT3d on ``d`` [B][Nx][Ny][T][36]; ``out`` given = accumulate into it.  ``keep`` (a dict; the training step)
        receives the spectrum ``X`` and ``rv`` = the ReLU output in front of Lo (rpb_mwt_spec_out_keep: the same kernel text)."""
        B, Nx, Ny, T, C = d.shape
        m, KX, KY = plan.modes, plan.KX, plan.KY
        y = MWT3d.k_axis(d, plan.FT, B * Nx * Ny, C)                        # [B][Nx][Ny][(ri, kt)][36]
        y = MWT3d.k_axis(y, plan.FY, B * Nx, m * C)                         # [B][Nx][(ri, ky)][kt][36]
        X = MWT3d.k_axis(y, plan.FX, B, KY * m * C)                         # [B][(ri, kx)][ky][kt][36]
        NB = KX * KY * m
        Y = torch.empty_like(X)
        _lib.call("rpb_mwt_modes", _p(X), _p(Wt), _p(plan.tab, I32), _p(Y), B, NB, _stream(), label="mwt_modes",
                  nbytes=16 * B * NB * C + 8 * NB * C * C, flops=8 * B * NB * C * C)
        z = MWT3d.k_axis(Y, plan.GX, B, KY * m * C)                         # [B][(x, ri)][ky][kt][36]
        z = MWT3d.k_axis(z, plan.GY, B * Nx, m * C)                         # [B][Nx][(y, ri)][kt][36]
        acc = out is not None
        if out is None:
            out = torch.empty_like(d)
        nbytes, flops = 4 * d.numel() * (2 if acc else 1) + 4 * z.numel(), 2 * d.numel() * (2 * m + C)
        if keep is not None:
            keep["X"], keep["rv"] = X, torch.empty_like(d)
            _lib.call("rpb_mwt_spec_out_keep", _p(z), _p(plan.GT), _p(loT), _p(lb), _p(out), _p(keep["rv"]), B * Nx * Ny, T, 2 * m, int(acc),
                      _stream(), label="mwt_spec_out[keep]", nbytes=nbytes + 4 * d.numel(), flops=flops)
            return out
        _lib.call("rpb_mwt_spec_out", _p(z), _p(plan.GT), _p(loT), _p(lb), _p(out), B * Nx * Ny, T, 2 * m, int(acc), _stream(),
                  label="mwt_spec_out", nbytes=nbytes, flops=flops)
        return out

    # ------------------------------------------------------------------ the kernels of the training step (csrc/rpb_mwt_train.hip)
    @staticmethod
    def k_conv3_keep(x, pack, out=None):
        """``k_conv3`` on the fp32 MFMA that also returns z = ReLU(conv(x) + b) [B][Nx][Ny][T][36]: (out, z)."""
        wp, cb, lop, lb = pack[:4]
        B, Nx, Ny, T, _ = x.shape
        acc = out is not None
        if out is None:
            out = torch.empty_like(x)
        z = torch.empty_like(x)
        _lib.call("rpb_mwt_conv3_keep", _p(x), _p(wp), _p(cb), _p(lop), _p(lb), _p(out), _p(z), B, Nx, Ny, T, int(acc), _stream(),
                  label="mwt_conv3[keep]", nbytes=4 * x.numel() * (4 if acc else 3), flops=2 * x.numel() * (27 * 36 + 36))
        return out, z

    @staticmethod
    def k_conv3_dgrad_wprep(w):
        """Conv3d weight [36][36][3][3][3] -> the lane-ordered A operand of the data gradient: the taps flipped, the channels swapped."""
        wd = w.transpose(0, 1).flip(2, 3, 4).contiguous()
        wpd = torch.empty(27 * 9 * 3 * 64, device=w.device, dtype=torch.float32)
        unused = torch.empty(3 * 4 * 3 * 64, device=w.device, dtype=torch.float32)       # (the Lo half of the prep kernel's output)
        _lib.call("rpb_mwt_conv3_wprep", _p(wd), _p(wd), _p(wpd), _p(unused), _stream())
        return wpd

    @staticmethod
    def k_conv3_dgrad(g, wpd, out=None):
        """Conv3d(36, 36, 3, padding=1) of ``g`` on the taps of ``k_conv3_dgrad_wprep``; ``out`` given = accumulate into it."""
        B, Nx, Ny, T, _ = g.shape
        acc = out is not None
        if out is None:
            out = torch.empty_like(g)
        _lib.call("rpb_mwt_conv3_dgrad", _p(g), _p(wpd), _p(out), B, Nx, Ny, T, int(acc), _stream(), label="mwt_conv3_dgrad",
                  nbytes=4 * g.numel() * (3 if acc else 2), flops=2 * g.numel() * 27 * 36)
        return out

    @staticmethod
    def k_conv3_wgrad(g, x):
        """(dW [36][36][3][3][3], db [36]) of the convolution from g_z and its input, both [B][Nx][Ny][T][36]."""
        B, Nx, Ny, T, _ = x.shape
        L = 36 * 36 * 27 + 36
        splits = _lib.query("rpb_mwt_conv3_wgrad_splits", B * Nx * Ny * T)
        part = torch.empty(splits, L, device=x.device, dtype=torch.float32)
        _lib.call("rpb_mwt_conv3_wgrad", _p(g), _p(x), _p(part), B, Nx, Ny, T, _stream(), label="mwt_conv3_wgrad",
                  nbytes=4 * 27 * 2 * x.numel(), flops=2 * x.numel() * 27 * 36)
        tot = torch.empty(L, device=x.device, dtype=torch.float32)
        ops.reduce_partials(part, splits, L, out_f32=tot)
        return tot[:36 * 36 * 27].view(36, 36, 3, 3, 3), tot[36 * 36 * 27:]

    @staticmethod
    def k_lo_bwd(gout, z, lo):
        """(g_z, dLo [36][36], dlb [36]): g_z = (g_out Lo) [z > 0] on cells [..][36]; ``lo`` = Linear.weight."""
        ncell = z.numel() // 36
        rows = _lib.query("rpb_mwt_lo_bwd_rows", ncell)
        L = 36 * 36 + 36
        gz = torch.empty_like(z)
        part = torch.empty(rows, L, device=z.device, dtype=torch.float32)
        _lib.call("rpb_mwt_lo_bwd", _p(gout), _p(z), _p(lo), _p(gz), _p(part), ncell, _stream(), label="mwt_lo_bwd",
                  nbytes=12 * z.numel(), flops=2 * z.numel() * 72)
        tot = torch.empty(L, device=z.device, dtype=torch.float32)
        ops.reduce_partials(part, rows, L, out_f32=tot)
        return gz, tot[:36 * 36].view(36, 36), tot[36 * 36:]

    @staticmethod
    def k_modes_bwd(X, gY, Wt, tab, dWt, B, NB):
        """g_X (like X) of rpb_mwt_modes; ``dWt`` (the gradient in the Wt layout, zeroed by the caller) += this level's share."""
        gX = torch.empty_like(X)
        _lib.call("rpb_mwt_modes_bwd", _p(X), _p(gY), _p(Wt), _p(tab, I32), _p(gX), _p(dWt), B, NB, _stream(), label="mwt_modes_bwd",
                  nbytes=24 * B * NB * 36 + 24 * NB * 36 * 36, flops=16 * B * NB * 36 * 36)
        return gX

    @staticmethod
    def k_spectral_bwd(gv, X, plan, Wt, dWt):
        """Backward of ``k_spectral`` behind its ReLU: g_v [B][Nx][Ny][T][36] (from ``k_lo_bwd``) -> g_d; the seven linear stages are
        rpb_mwt_axis on the transposed matrices (``LevelPlan.adj``) around rpb_mwt_modes_bwd."""
        B, Nx, Ny, T, C = gv.shape
        m, KX, KY = plan.modes, plan.KX, plan.KY
        g = MWT3d.k_axis(gv, plan.adj("GT"), B * Nx * Ny, C)
        g = MWT3d.k_axis(g, plan.adj("GY"), B * Nx, m * C)
        g = MWT3d.k_axis(g, plan.adj("GX"), B, KY * m * C)
        g = MWT3d.k_modes_bwd(X, g, Wt, plan.tab, dWt, B, KX * KY * m)
        g = MWT3d.k_axis(g, plan.adj("FX"), B, KY * m * C)
        g = MWT3d.k_axis(g, plan.adj("FY"), B * Nx, m * C)
        return MWT3d.k_axis(g, plan.adj("FT"), B * Nx * Ny, C).view(B, Nx, Ny, T, C)

    @staticmethod
    def k_head_bwd(x, gout, w0t, b0, w1, Cout, r):
        """(g_x, dLc1 [dout][128], db1, dLc0 [128][36], db0) of ``k_head``; the hidden layer is recomputed."""
        B, Nx, Ny, T, _ = x.shape
        dout = Cout * r
        rows = _lib.query("rpb_mwt_head_bwd_rows", B * Nx * Ny * T)
        L = dout * 128 + dout + 128 * 36 + 128
        gx = torch.empty_like(x)
        part = torch.empty(rows, L, device=x.device, dtype=torch.float32)
        _lib.call("rpb_mwt_head_bwd", _p(x), _p(gout), _p(w0t), _p(b0), _p(w1), _p(gx), _p(part), B, Nx, Ny, T, Cout, r, _stream(),
                  label="mwt_head_bwd", nbytes=4 * (2 * x.numel() + gout.numel()), flops=2 * B * Nx * Ny * T * 128 * (3 * 36 + 2 * dout))
        tot = torch.empty(L, device=x.device, dtype=torch.float32)
        ops.reduce_partials(part, rows, L, out_f32=tot)
        o1, o2 = dout * 128, dout * 128 + dout
        return gx, tot[:o1].view(dout, 128), tot[o1:o2], tot[o2:o2 + 128 * 36].view(128, 36), tot[o2 + 128 * 36:]

    @staticmethod
    def k_lift_wgrad(g, x):
        """(dLk [36][Cin], db [36]) from g [B][H][W][T][36] and the model input x [B][T][H][W][Cin]."""
        B, T, H, W, Cin = x.shape
        rows = _lib.query("rpb_mwt_lift_wgrad_rows", B * T * H * W)
        L = 36 * Cin + 36
        part = torch.empty(rows, L, device=x.device, dtype=torch.float32)
        _lib.call("rpb_mwt_lift_wgrad", _p(g), _p(x), _p(part), B, T, H, W, Cin, _stream(), label="mwt_lift_wgrad",
                  nbytes=4 * (g.numel() + x.numel()), flops=2 * g.numel() * (Cin + 1))
        tot = torch.empty(L, device=x.device, dtype=torch.float32)
        ops.reduce_partials(part, rows, L, out_f32=tot)
        return tot[:36 * Cin].view(36, Cin), tot[36 * Cin:]

    @staticmethod
    def k_head(x, w0t, b0, w1, b1, Cout, r):
        B, Nx, Ny, T, _ = x.shape
        out = torch.empty(B, T * r, Nx, Ny, Cout, device=x.device, dtype=torch.float32)
        _lib.call("rpb_mwt_head", _p(x), _p(w0t), _p(b0), _p(w1), _p(b1), _p(out), B, Nx, Ny, T, Cout, r, _stream(), label="mwt_head",
                  nbytes=4 * (x.numel() + out.numel()), flops=2 * B * Nx * Ny * T * 128 * (36 + Cout * r))
        return out

    # ------------------------------------------------------------------ forward
    def _cz_forward(self, x, p, relu, keep=None):
        """One MWT_CZ3d block.  ``keep`` (a dict) receives the per-level tensors d, s, A(d) + B(s) and C(d) (tests; the follow-up's
        backward needs exactly these)."""
        Ud, Us = [], []
        for i in range(self.ns):
            d, x = self.k_decompose(x, p["ec_d"], p["ec_s"])
            plan = self._plan(d.shape[1], d.shape[2], d.device)
            ud = self.k_spectral(d, plan, p["Wt"], p["loT"], p["lb"])
            self.k_conv3(x, p["B"], out=ud, arith=self.arith)
            Ud.append(ud)
            Us.append(self.k_conv3(d, p["C"], arith=self.arith))
            if keep is not None:
                keep.setdefault("d", []).append(d)
                keep.setdefault("s", []).append(x)
        x = self.k_coarse(x, p["T0w"], p["T0b"])
        for i in range(self.ns - 1, -1, -1):
            x = self.k_reconstruct(x, Us[i], Ud[i], p["rc"], relu and i == 0)
        if keep is not None:
            keep["Ud"], keep["Us"] = Ud, Us
        return x

    # ------------------------------------------------------------------ the training step (through _common.HipFunction)
    def _cz_forward_train(self, x, p, relu, rec):
        """``_cz_forward`` on the ``"f32"`` kernels; ``rec`` (a dict, or None under no_grad) receives per level d, s, the spectrum X and
        the three ReLU outputs rv (A), zB, zC.  The keep-variants are the same kernel texts: the output is bit-equal to the eval forward's."""
        if rec is None:
            saved, self.arith = self.arith, "f32"
            try:
                return self._cz_forward(x, p, relu)
            finally:
                self.arith = saved
        Ud, Us, levels = [], [], []
        for i in range(self.ns):
            d, x = self.k_decompose(x, p["ec_d"], p["ec_s"])
            lv = {"d": d, "s": x}
            ud = self.k_spectral(d, self._plan(d.shape[1], d.shape[2], d.device), p["Wt"], p["loT"], p["lb"], keep=lv)
            _, lv["zB"] = self.k_conv3_keep(x, p["B"], out=ud)
            us, lv["zC"] = self.k_conv3_keep(d, p["C"])
            Ud.append(ud)
            Us.append(us)
            levels.append(lv)
        x = self.k_coarse(x, p["T0w"], p["T0b"])
        for i in range(self.ns - 1, -1, -1):
            x = self.k_reconstruct(x, Us[i], Ud[i], p["rc"], relu and i == 0)
        rec["levels"], rec["out"] = levels, x          # out: the next block's input; it holds the gate of the ReLU between two blocks
        return x

    @torch.no_grad()
    def _forward_hip(self, x, state):
        x = x.contiguous().float()
        p = self._prep_train(x.device)
        h = self.k_lift(x, p["Lkw"], p["Lkb"])
        blocks = []
        for i, cz in enumerate(p["cz"]):
            rec = None if state is None else {}
            h = self._cz_forward_train(h, cz, i < self.nCZ - 1, rec)
            blocks.append(rec)
        if state is not None:
            state.update(x=x, blocks=blocks)
        return self.k_head(h, p["w0t"], p["b0"], p["w1"], p["b1"], self.shape_out[-1], self.shape_out[0] // self.shape_in[0])

    def _cz_backward(self, g, p, cz, rec, grads):
        """g = dLoss/d(output of evenOdd at the finest level) -> dLoss/d(block input); the block's parameter gradients go into ``grads``.
        A, B and C are shared by all levels: their gradients sum over levels (fixed order, coarsest first)."""
        levels = rec["levels"]

        def add(param, t):
            grads[param] = grads[param] + t if param in grads else t

        g_ud, g_us = [], []
        for i in range(self.ns):                     # adjoint of reconstruct = decompose on the transposed rc; g_us = g_x = g_(x + us)
            gud, g = self.k_decompose(g, p["ec_d_adj"], p["ec_s_adj"])
            g_ud.append(gud)
            g_us.append(g)
        B, _, mult, T, _ = g.shape
        g2 = (g.sum(2) if mult > 1 else g).reshape(B * T, 36)        # the coarsest x was broadcast along Ny; tiny: plain torch, as T0 is
        s_last = levels[-1]["s"].reshape(B * T, 36 * mult)           # the row-major view rpb_mwt_coarse reads
        add(cz.T0.weight, g2.t() @ s_last)
        add(cz.T0.bias, g2.sum(0))
        gs = (g2 @ p["T0w"]).reshape(B, 1, mult, T, 36)
        dWt = torch.zeros_like(p["Wt"])
        for i in range(self.ns - 1, -1, -1):
            lv = levels[i]
            d, s = lv["d"], lv["s"]
            gv, dlo, dlb = self.k_lo_bwd(g_ud[i], lv["rv"], p["lo"]["A"])
            add(cz.A.Lo.weight, dlo)
            add(cz.A.Lo.bias, dlb)
            gd = self.k_spectral_bwd(gv, lv["X"], self._plan(d.shape[1], d.shape[2], d.device), p["Wt"], dWt)
            for name, gout, z, src in (("C", g_us[i], lv["zC"], d), ("B", g_ud[i], lv["zB"], s)):
                m = getattr(cz, name)
                gz, dlo, dlb = self.k_lo_bwd(gout, z, p["lo"][name])
                dW, db = self.k_conv3_wgrad(gz, src)
                for param, t in ((m.Lo.weight, dlo), (m.Lo.bias, dlb), (m.conv[0].weight, dW), (m.conv[0].bias, db)):
                    add(param, t)
                self.k_conv3_dgrad(gz, p[name + "d"], out=gd if name == "C" else gs)      # d collects A and C; s collects B and the coarser level
            zero = torch.zeros(B, d.shape[1], 1, T, 36, device=d.device, dtype=torch.float32)
            gs = self.k_reconstruct(zero, gs, gd, p["rc_adj"], False)                       # adjoint of decompose
        gw = torch.view_as_complex(dWt).permute(0, 4, 5, 1, 2, 3)    # [4][x][y][t][i][o] -> [4][i][o][x][y][t], once per block
        for j in range(4):
            grads[getattr(cz.A, f"weights{j + 1}")] = gw[j].contiguous()
        return gs

    @torch.no_grad()
    def _backward_hip(self, state, g_out, need_gx=False):
        """{parameter: gradient} from dLoss/d(out).  ``state`` is only read: a second call gives bit-equal gradients (no kernel uses
        atomics and every sum has a fixed order).  BN.* has no gradient: it is never called."""
        if need_gx:
            raise NotImplementedError("MWT3d training computes no input gradient (no trainer asks for one)")
        x, blocks = state["x"], state["blocks"]
        p = self._prep_train(x.device)
        grads = {}
        g, grads[self.Lc1.weight], grads[self.Lc1.bias], grads[self.Lc0.weight], grads[self.Lc0.bias] = self.k_head_bwd(
            blocks[-1]["out"], g_out, p["w0t"], p["b0"], p["w1"], self.shape_out[-1], self.shape_out[0] // self.shape_in[0])
        for i in range(self.nCZ - 1, -1, -1):
            if i < self.nCZ - 1:
                g = g * (blocks[i]["out"] > 0)       # the ReLU between two blocks, gated by the saved (ReLU'd) block output
            g = self._cz_backward(g, p["cz"][i], self.MWT_CZ[i], blocks[i], grads)
        grads[self.Lk.weight], grads[self.Lk.bias] = self.k_lift_wgrad(g, x)
        return grads

    def check_input(self, shape):
        if tuple(shape[1:]) != self.shape_in:
            raise ValueError(f"MWT3d was built for inputs [B, {', '.join(map(str, self.shape_in))}], got {tuple(shape)}")

    def _forward_eval(self, x):
        p = self._prep(x.device)
        h = self.k_lift(x, p["Lkw"], p["Lkb"])
        for i, cz in enumerate(p["cz"]):
            h = self._cz_forward(h, cz, relu=i < self.nCZ - 1)
        return self.k_head(h, p["w0t"], p["b0"], p["w1"], p["b1"], self.shape_out[-1], self.shape_out[0] // self.shape_in[0])
