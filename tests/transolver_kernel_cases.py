"""TEST INFRASTRUCTURE ONLY -- the shapes and inputs of the per-kernel Transolver tests, shared by tests/test_gpu_transolver_kernels.py
(which runs the HIP kernels of csrc/rpb_transolver.hip on them) and tests/test_transolver_kernels_host.py (which checks, without a GPU,
that every case is well conditioned and that a wrong formula would be noticed).  ``Case``, the two measures, the bound and the
conditioning cap are those of tests/unet_kernel_cases.py.

Input scales (chosen, and re-measured by the host test).  The slice family has Ws ~ N(0,1)/16 and bs ~ 0.3 N(0,1): with the Ws ~ N(0,1)/4
of tests/test_gpu_transolver.py the head whose temperature is clamped to 0.1 saturates its softmax and the fp32 restatement of w is off by
2.7e-6 (max-abs), past the cap.  The attention cases have tokS = norm * N(0,1), so that t = tokS / (norm + 1e-5) is O(1): independent
tokS ~ 3 N(0,1) saturates the softmax among the slice tokens (fp32 gT and dWk off by 2.3e-6).

The temperatures put one head below the clamp (0.05), one above it (7.0) and the others inside."""
import torch

import transolver_restatement as R
from kernel_verdict import verdict
from unet_kernel_cases import (BADLY_CONDITIONED, F32, F64, MEASURES, MI355X_CUS, Case, _gen, _rn,      # noqa: F401
                               bound_of, measures)

LN_EPS = 1e-5
TEMPS = (0.5, 0.05, 1.3, 7.0, 0.9, 0.4, 2.0, 0.3)


# ================================================================================================ block counts
def slice_bps(B, cus=MI355X_CUS):
    """rpb_slice_blocks_per_sample: ceil(2 CUs / B)"""
    return max(1, (2 * cus + B - 1) // B)


def ln_bwd_rows(M, cus=MI355X_CUS):
    """rpb_layernorm_bwd_rows: the waves of min(ceil(M / 4), 8 CUs) blocks of 4"""
    return 4 * min((M + 3) // 4, 8 * cus)


# ================================================================================================ slice family
SLICE_SMALL = [(1, 1, 1, 4), (1, 31, 1, 4), (2, 33, 2, 16), (1, 64, 4, 8), (3, 70, 8, 32), (2, 45, 3, 12)]
SLICE_IDS = ["one-token", "tile-minus-1", "tile-plus-1", "exact-tiles", "eight-waves-G32", "odd-heads-G12", "two-full-tiles+5",
             "config-width-ragged-second-tile"]


def slice_shapes(bps16):
    """(B, ntok, heads, G); ``bps16`` = blocks per sample at B = 16.  In the last two every block of slice_fwd_kernel / slice_bwd_kernel
    walks more than one 32-token tile: two full ones and block 0 a third of 5 tokens; one full one and block 0 a second of 7 tokens (at
    the config's width, 8 heads: there deslice_kernel's 4 bps blocks of 4 tokens loop as well)."""
    big = [(16, 64 * bps16 + 5, 2, 16), (16, 32 * bps16 + 7, 8, 16)]
    assert all(ntok > 32 * bps16 for _, ntok, _, _ in big)
    return SLICE_SMALL + big


def slice_case(B, ntok, heads, G):
    g = _gen(21, B, ntok, heads, G)
    C, M = heads * 32, B * ntok
    i = dict(xf=_rn(g, M, 2 * C), gox=_rn(g, M, C), tok2=_rn(g, B, heads, G, 32), gT=_rn(g, B, heads, G, 32), gN=_rn(g, B, heads, G),
             Ws=_rn(g, G, 32, scale=1 / 16), bs=_rn(g, G, scale=0.3), temp=torch.tensor(TEMPS[:heads]))
    # the kernels after slice_fwd take the SAVED weights: the fp64 ones rounded to fp32, in the fp64 and in the fp32 run alike
    i["w"] = R.slice_fwd(i["xf"], i["Ws"], i["bs"], i["temp"], B, ntok, heads, G, F64)[0].float()
    dims = (B, ntok, heads, G)

    def ref(dt):
        w, tokS, norm = R.slice_fwd(i["xf"], i["Ws"], i["bs"], i["temp"], *dims, dt)
        gxf, dWs, dbs, dtau, dtau_abs = R.slice_bwd(i["xf"], i["w"], i["gox"], i["tok2"], i["gT"], i["gN"], i["Ws"], i["temp"], *dims, dt)
        return dict(w=w, tokS=tokS, norm=norm, gtok2=R.slice_tokens_given_w(i["gox"], i["w"], *dims, dt),
                    ox=R.deslice(i["w"], i["tok2"], *dims, dt), gxf=gxf, dWs=dWs, dbs=dbs, dtau=dtau, dtau_abs=dtau_abs)
    return Case(f"slice B={B} ntok={ntok} heads={heads} G={G}", i, ref)


def dtau_measure(dtau, r64):
    """max over the heads of |dtau - dtau64| / A64[h], A64[h] = (1/tau_h) sum |gl log w| of the fp64 restatement.
    dtau is a signed sum over every token and slice of gl * log w that cancels: on the well-conditioned inputs above fp32 autograd was
    off by up to 3.9e-5 RELATIVE TO dtau on single heads, which says nothing about the arithmetic.  A64 is the size of what was added
    up, and it comes from the reference alone."""
    return float(((dtau.double() - r64["dtau"]).abs() / r64["dtau_abs"]).max())


SLICE_KEYS = ("w", "tokS", "norm", "gtok2", "ox", "gxf", "dWs", "dbs")           # judged on the two usual measures; dtau on its own


# ================================================================================================ attention among the slice tokens
ATTN_SHAPES = [(1, 4), (3, 5), (6, 12), (16, 16), (24, 32)]


def attn_case(BH, G):
    g = _gen(22, BH, G)
    norm = torch.rand(BH, G, generator=g) * 4 + 0.5
    i = dict(norm=norm, tokS=norm[..., None] * _rn(g, BH, G, 32), Wq=_rn(g, 32, 32, scale=0.2), Wk=_rn(g, 32, 32, scale=0.2),
             Wv=_rn(g, 32, 32, scale=0.2), go=_rn(g, BH, G, 32), amask=(torch.rand(BH, G, G, generator=g) < 0.9).float() / 0.9)
    five = (i["tokS"], i["norm"], i["Wq"], i["Wk"], i["Wv"])

    def ref(dt):
        out = dict(out=R.slice_attn(*five, None, dt), out_m=R.slice_attn(*five, i["amask"], dt))
        for tag, mask in (("", None), ("_m", i["amask"])):
            gT, gN, gW = R.slice_attn_bwd(*five, mask, i["go"], dt)
            out.update({"gT" + tag: gT, "gN" + tag: gN, "gW" + tag: gW.reshape(BH, 3, 1024), "dW" + tag: gW.sum(0).reshape(3 * 1024)})
        return out
    return Case(f"slice_attn BH={BH} G={G}", i, ref)


# ================================================================================================ LayerNorm
LN_SHAPES = [(5, 64), (9, 192), (9, 320), (9, 384), (9, 448), (9, 768), (9, 1024), (777, 256)]


def ln_rows_shape(rows0):
    """the backward case whose waves walk more than one row: every wave accumulates two rows and 37 of them a third
    (``rows0`` = rpb_layernorm_bwd_rows of a huge M, the capped wave count)"""
    return (2 * rows0 + 37, 64)


def ln_case(M, C):
    g = _gen(23, M, C)
    i = dict(x=_rn(g, M, C, scale=1.5, shift=0.3), gamma=torch.rand(C, generator=g) + 0.5, beta=_rn(g, C, scale=0.3), gy=_rn(g, M, C),
             gadd=_rn(g, M, C))

    def ref(dt):
        gx, dg, db = R.layernorm_bwd(i["x"], i["gamma"], i["gy"], None, LN_EPS, dt)
        return dict(y=R.layernorm_fwd(i["x"], i["gamma"], i["beta"], LN_EPS, dt), gx=gx,
                    gx_add=R.layernorm_bwd(i["x"], i["gamma"], i["gy"], i["gadd"], LN_EPS, dt)[0], dgb=torch.cat((dg, db)))
    return Case(f"layernorm M={M} C={C}", i, ref)


# ================================================================================================ tokens_lift
LIFT_CASES = [(1000, 3, 512, 1), (1000, 3, 256, 0), (7, 1, 4, 1), (300, 8, 64, 0), (50, 32, 512, 1)]
LIFT_REFUSED = (32, 2048)             # (K, N): (K + 1) N 4 bytes = 270 336 > the 160 KiB of LDS


def lift_case(M, K, N, act):
    """act = 0 is the backward use (g @ W2 with a zero bias), act = 1 the forward one (bias + GELU)"""
    g = _gen(24, M, K, N, act)
    i = dict(x=_rn(g, M, K), W=_rn(g, N, K, scale=K ** -0.5), b=_rn(g, N) if act else torch.zeros(N))
    return Case(f"tokens_lift M={M} K={K} N={N} act={act}", i, lambda dt: dict(y=R.tokens_lift(i["x"], i["W"], i["b"], act, dt)))


def all_cases(cus=MI355X_CUS):
    """(case constructor, arguments) of every GPU case, for the host tests"""
    out = [(slice_case, s) for s in slice_shapes(slice_bps(16, cus))] + [(attn_case, s) for s in ATTN_SHAPES]
    out += [(ln_case, s) for s in LN_SHAPES + [ln_rows_shape(ln_bwd_rows(10 ** 9, cus))]] + [(lift_case, s) for s in LIFT_CASES]
    return out


# ================================================================================================ the verdict, shared by both tests
def judge(name, got, ref64, ref32, existing=None):
    """``got`` against the fp64 restatement on both measures, bound max(8 * e32, 1e-6) (or ``existing``, a bound another test of the
    same kernel already asserts); e32 = the same measure of the fp32 restatement.  Prints every figure before it asserts."""
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    _verdict(name, zip(MEASURES, measures(ref32, ref64), measures(got, ref64)), existing)


def judge_dtau(name, got, r64, r32, existing=None):
    """the same for the temperature gradient, on ``dtau_measure``"""
    assert tuple(got.shape) == tuple(r64["dtau"].shape), (name, got.shape, r64["dtau"].shape)
    _verdict(name, [("dtau/sum|terms|", dtau_measure(r32["dtau"], r64), dtau_measure(got, r64))], existing)


def _verdict(name, figures, existing):
    verdict("transolver-kernels", name, figures, existing)          # tests/kernel_verdict.py, shared with the MWT kernel tests
