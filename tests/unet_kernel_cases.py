"""TEST INFRASTRUCTURE ONLY -- the shapes and inputs of the per-kernel U-Net tests, shared by tests/test_gpu_unet_kernels.py (which runs
the HIP kernels on them) and tests/test_unet_kernels_host.py (which checks, without a GPU, that every case is well conditioned: the
fp32 restatement stays within 1e-5 / 8 of its fp64 run).  A ``Case`` holds fp32 CPU inputs and ``ref(dtype)``, a dict of restatement
results; ``refs()`` caches the (fp64, fp32) pair so that a reference is computed once however many tests look at it."""
import math

import torch

import unet_restatement as R

F32, F64 = torch.float32, torch.float64
HID = R.HID
MI355X_CUS = 256          # the host conditioning run has no library to ask; the GPU tests take the count from the library


class Case:
    def __init__(self, name, inp, ref, exact=()):
        self.name, self.inp, self._ref, self.exact, self._pair = name, inp, ref, set(exact), None

    def refs(self):
        if self._pair is None:
            self._pair = (self._ref(F64), self._ref(F32))
        return self._pair

    def __getattr__(self, k):                                   # case.x == case.inp["x"]
        try:
            return self.__dict__["inp"][k]
        except KeyError:
            raise AttributeError(k)


def _gen(*key):
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def _rn(g, *shape, scale=1.0, shift=0.0):
    return torch.randn(*shape, generator=g) * scale + shift


# ================================================================================================ GroupNorm + SiLU channel passes
CHAN_SHAPES = [(3, 50, 64), (1, 4097, 128), (2, 333, 256), (1, 70, 1024)]


def chan_case(B, n, C):
    g = _gen(1, B, n, C)
    i = dict(x=_rn(g, B, n, C, scale=1.5, shift=0.3), gy=_rn(g, B, n, C), res=_rn(g, B, n, C),
             A=torch.rand(B, C, generator=g) + 0.5, Bc=_rn(g, B, C, scale=0.3), P=_rn(g, B, C, scale=0.1), Q=_rn(g, B, C, scale=0.1))

    def ref(dt):
        return dict(stats=R.chan_stats(i["x"], dt), y=R.affine_silu_fwd(i["x"], i["A"], i["Bc"], None, dt),
                    y_res=R.affine_silu_fwd(i["x"], i["A"], i["Bc"], i["res"], dt),
                    red=R.affine_silu_bwd_reduce(i["x"], i["gy"], i["A"], i["Bc"], dt),
                    gx=R.affine_silu_bwd_apply(i["x"], i["gy"], i["A"], i["Bc"], i["P"], i["Q"], dt))
    return Case(f"chan B={B} n={n} C={C}", i, ref)


LN_SHAPES = [(1, 64), (77, 128), (4099, 256)]
LN_EPS = 1e-5


def ln_case(M, C):
    g = _gen(2, M, C)
    i = dict(x=_rn(g, M, C, scale=1.5, shift=0.3), gamma=torch.rand(C, generator=g) + 0.5, gy=_rn(g, M, C))

    def ref(dt):
        gx, dg, db = R.layernorm_bwd(i["x"], i["gamma"], i["gy"], LN_EPS, dt)
        return dict(y=R.layernorm_fwd(i["x"], i["gamma"], LN_EPS, dt), gx=gx, dgb=torch.cat((dg, db)))
    return Case(f"layernorm M={M} C={C}", i, ref)


# ================================================================================================ init_conv: im2col + token GEMMs
IM2COL_MESHES = [(2, 2, 5, 9), (1, 3, 8, 4)]
IM2COL_CIN = [3, 5, 16]
KS = 7


def init_ldc(Cin):
    return (KS ** 3 * Cin + 127) // 128 * 128                  # model/unet.py: _w("init", ...)


def im2col_case(B, T, H, W, Cin):
    g = _gen(3, B, T, H, W, Cin)
    cols, ldc, M = KS ** 3 * Cin, init_ldc(Cin), B * T * H * W
    Wi = torch.zeros(64, ldc)
    Wi[:, :cols] = _rn(g, 64, cols, scale=cols ** -0.5)
    i = dict(x=_rn(g, B, T, H, W, Cin), W=Wi, bias=_rn(g, 64), gy=_rn(g, M, 64))
    col32 = R.im2col(i["x"], KS, ldc, F32)                      # a pure gather: exact in fp32, and the GEMMs' input in both runs

    def ref(dt):
        dW, db = R.gemm_tn(i["gy"], col32, dt)
        return dict(col=col32, y=R.gemm_nt(col32, i["W"], i["bias"], None, dt), dW=dW, db=db)
    return Case(f"init_conv mesh={B}x{T}x{H}x{W} Cin={Cin} ldc={ldc}", i, ref, exact=("col",))


FINAL_CASES = [(M, N) for M in (180, 4100) for N in (3, 16)]


def _grid64(t):
    return torch.round(t * 64) / 64


def final_case(M, N):
    """x and gy sit on a grid of 1/64 (normal values, 7 to 9 significant bits): their products are multiples of 2^-12 and the sum of the
    absolute values of the 4100 terms of a column stays below 2^12 (about 4100 * 0.64), so every partial sum in any order is exact in
    fp32 and the M-long weight-gradient sums are well conditioned on every host.  On plain normal inputs an fp32 BLAS that adds the
    4100 terms of the 3-row product one after the other lost 1.7e-6 (max-abs; 1.1e-6 Rel-L2) on the GPU host: badly conditioned by the
    rule, though the kernel held 4.6e-7 (profiles/unet_kernels_pytest_first.txt).  y and gx multiply by an off-grid W and stay inexact."""
    g = _gen(4, M, N)
    i = dict(x=_grid64(_rn(g, M, 64)), W=_rn(g, N, 64, scale=0.125), bias=_rn(g, N), gy=_grid64(_rn(g, M, N)))

    def ref(dt):
        dW, db = R.gemm_tn(i["gy"], i["x"], dt)
        return dict(y=R.gemm_nt(i["x"], i["W"], i["bias"], None, dt), dW=dW, db=db,
                    gx=R.gemm_nt(i["gy"], i["W"].t().contiguous(), None, None, dt))
    return Case(f"final_conv M={M} N={N}", i, ref)


# ================================================================================================ (1,4,4) gather modes
GATHER_CASES = [(C, mesh) for C in (64, 128) for mesh in ((2, 3, 4, 6), (1, 1, 2, 2), (1, 2, 8, 8))]


def gather_case(C, mesh4):
    B, T, H, W = mesh4
    g = _gen(5, C, *mesh4)
    M, Mo = B * T * H * W, B * T * (H // 2) * (W // 2)
    i = dict(x=_rn(g, M, C), wd=_rn(g, C, C, 1, 4, 4, scale=(16 * C) ** -0.5), wu=_rn(g, C, C, 1, 4, 4, scale=(4 * C) ** -0.5),
             bias=_rn(g, C), gy=_rn(g, Mo, C))

    def ref(dt):
        dW, db = R.strided_conv_wgrad(i["gy"], i["x"], C, B, (T, H, W), dt)
        return dict(down=R.strided_conv(i["x"], i["wd"], i["bias"], B, (T, H, W), dt), dW=dW, db=db,
                    up=R.transposed_conv(i["x"], i["wu"], i["bias"], B, (T, H, W), dt))
    return Case(f"gather C={C} mesh={B}x{T}x{H}x{W}", i, ref)


def down_layout(wd):
    """Conv3d weight [Co][Ci][1][4][4] -> the gather GEMM's [Co][16 Ci], column (kh * 4 + kw) * Ci + ci (rpb_gemm.hip, conv = 2)"""
    return wd[:, :, 0].permute(0, 2, 3, 1).reshape(wd.shape[0], -1).contiguous()


def down_unlayout(dW, C):
    return dW.reshape(C, 4, 4, C).permute(0, 3, 1, 2).unsqueeze(2)


def up_layout(wu):
    """ConvTranspose3d weight [Ci][Co][1][4][4] -> [4 classes][Co][4 Ci]: class (ph, pw) takes kernel rows kh = ph ? (0, 2) : (1, 3)
    (the same for kw), column (jh * 2 + jw) * Ci + ci (rpb_gemm.hip, conv = 3)"""
    cls = []
    for ph in (0, 1):
        for pw in (0, 1):
            kh, kw = ((0, 2) if ph else (1, 3)), ((0, 2) if pw else (1, 3))
            sub = wu[:, :, 0][:, :, list(kh)][:, :, :, list(kw)]
            cls.append(sub.permute(1, 2, 3, 0).reshape(wu.shape[1], -1))
    return torch.stack(cls).contiguous()


def up_class_rows(cls, B, T, H, W):
    """rows of the (T, 2H, 2W) output mesh that parity class ``cls`` writes, in the order of the input tokens"""
    ph, pw = cls >> 1, cls & 1
    bt = torch.arange(B * T)[:, None, None]
    return ((bt * 2 * H + 2 * torch.arange(H)[None, :, None] + ph) * 2 * W + 2 * torch.arange(W)[None, None, :] + pw).reshape(-1)


# ================================================================================================ temporal attention
def tattn_shapes(cus):
    return [(2, 10, 9), (2, 11, 9), (1, 20, 33), (1, 21, 5), (1, 32, 5), (2, 20, (6 * cus + 5 + 1) // 2)]


def rotary_tables(T):
    freqs = 1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))
    ang = torch.repeat_interleave(torch.arange(T, dtype=F32)[:, None] * freqs[None, :], 2, dim=-1)
    return ang.cos().contiguous(), ang.sin().contiguous()


def tattn_case(B, T, HW):
    g = _gen(6, B, T, HW)
    rc, rs = rotary_tables(T)
    i = dict(qkv=_rn(g, B, T, HW, 3 * HID), bias=_rn(g, 4, T, T), go=_rn(g, B, T, HW, HID), rc=rc, rs=rs)

    def ref(dt):
        gq, gb = R.tattn_bwd(i["qkv"], rc, rs, i["bias"], i["go"], dt)
        return dict(out=R.tattn_fwd(i["qkv"], rc, rs, i["bias"], dt), gqkv=gq, dbias=gb)
    return Case(f"tattn B={B} T={T} HW={HW}", i, ref)


# ================================================================================================ bottleneck attention
SATTN_SHAPES = [(2, 256), (1, 64), (3, 33), (1, 129), (20, 16)]


def sattn_case(Fr, n):
    g = _gen(7, Fr, n)
    i = dict(qkv=_rn(g, Fr, n, 3 * HID), go=_rn(g, Fr, n, HID))

    def ref(dt):
        out, lse = R.sattn_fwd(i["qkv"], dt)
        return dict(out=out, lse=lse, gqkv=R.sattn_bwd(i["qkv"], i["go"], dt))
    return Case(f"sattn F={Fr} n={n}", i, ref)


# ================================================================================================ spatial linear attention
LINATTN_SHAPES = [(3, 50), (1, 4100), (20, 16)]


def linattn_case(Fr, n):
    """every stage of model/unet.py:_linear_attn on its own inputs: a later stage takes the fp64 result of the earlier one rounded to
    fp32 (``qe``), or independent random operands (the 64 x 64 matrices are dense, so that the cross-head blocks count)"""
    g = _gen(8, Fr, n)
    qkv = _rn(g, Fr, n, 3 * HID)
    kmax = R.col_reduce(qkv[..., HID:2 * HID], 0, F32)                            # a maximum: exact
    qe = R.linattn_prep_fwd(qkv, kmax, F64).float()
    i = dict(qkv=qkv, kmax=kmax, qe=qe, go=_rn(g, Fr, n, HID), dqe=_rn(g, Fr, n, 2 * HID), dz=_rn(g, Fr, HID, scale=0.1),
             Wm=_rn(g, 3, Fr, 2, 64, 64, scale=0.125))

    def ref(dt):
        return dict(kmax=kmax, qe=R.linattn_prep_fwd(qkv, kmax, dt), Z=R.col_reduce(qe[..., HID:], 1, dt),
                    S=R.head_scores(qe[..., HID:], qkv[..., 2 * HID:], dt), dctx=R.head_scores(qe[..., :HID], i["go"], dt),
                    o=R.head_apply(qe[..., :HID], i["Wm"][0], dt), dE=R.head_apply(qkv[..., 2 * HID:], i["Wm"][1], dt),
                    dv=R.head_apply(qe[..., HID:], i["Wm"][2], dt), gqk=R.linattn_prep_bwd(qe, i["dqe"], i["dz"], dt))
    return Case(f"linattn F={Fr} n={n}", i, ref, exact=("kmax",))


# ================================================================================================ copies, sums
COPY_SHAPES = [(64, 64), (256, 256), (64, 128)]
COPY_M = 77
COLSUM_SHAPES = [(77, 64), (4100, 384)]
ADD_SIZES = [4, 77 * 64, 1000004]


def colsum_case(M, N):
    i = dict(x=_rn(_gen(9, M, N), M, N))
    return Case(f"colsum M={M} N={N}", i, lambda dt: dict(s=R.colsum(i["x"], dt)))


# ================================================================================================ token-GEMM dispatch
GEMM_CASES = ([(M, N, K) for (N, K) in ((384, 64), (384, 128), (128, 128), (64, 128)) for M in (4095, 4133)]
              + [(65573, 384, 256), (65573, 256, 128)])


def gemm_case(M, N, K):
    g = _gen(10, M, N, K)
    i = dict(A=_rn(g, M, K), W=_rn(g, N, K, scale=K ** -0.5), bias=_rn(g, N), res=_rn(g, M, N))

    def ref(dt):
        y = R.gemm_nt(i["A"], i["W"], None, None, dt)
        return dict(plain=y, full=y + i["bias"].to(dt) + i["res"].to(dt))
    return Case(f"gemm_nt M={M} N={N} K={K}", i, ref)


# ================================================================================================ relative-position bias
RELPOS_T = [3, 20]


def relpos_case(T):
    from realpdebench_amd.model.unet import _rel_pos_index
    g = _gen(11, T)
    i = dict(table=_rn(g, 32, 4), idx=_rel_pos_index(T, "cpu"), g=_rn(g, 4, T * T))
    return Case(f"relpos T={T}", i, lambda dt: dict(bias=R.relpos_fwd(i["table"], i["idx"], dt), gt=R.relpos_bwd(i["g"], i["idx"], 32, dt)),
                exact=("bias",))


def all_cases(cus=MI355X_CUS):
    """(case constructor, arguments) of every GPU case, for the host conditioning test"""
    out = [(chan_case, s) for s in CHAN_SHAPES] + [(ln_case, s) for s in LN_SHAPES]
    out += [(im2col_case, (*m, c)) for m in IM2COL_MESHES for c in IM2COL_CIN]
    out += [(final_case, s) for s in FINAL_CASES] + [(gather_case, s) for s in GATHER_CASES]
    out += [(tattn_case, s) for s in tattn_shapes(cus)] + [(sattn_case, s) for s in SATTN_SHAPES]
    out += [(linattn_case, s) for s in LINATTN_SHAPES] + [(colsum_case, s) for s in COLSUM_SHAPES]
    out += [(gemm_case, s) for s in GEMM_CASES] + [(relpos_case, (t,)) for t in RELPOS_T]
    return out


def measures(a, ref):
    """(Rel-L2, max |error| / max |reference|) of ``a`` against ``ref``, in fp64"""
    a, ref = a.double().flatten(), ref.double().flatten()
    d = a - ref
    return (float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300)))


MEASURES = ("rel-l2", "max-abs")
BADLY_CONDITIONED = 1e-5


def bound_of(e32):
    return max(8 * e32, 1e-6)
