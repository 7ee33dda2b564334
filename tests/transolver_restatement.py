"""TEST INFRASTRUCTURE ONLY -- plain-torch restatements of the Transolver kernel family (csrc/rpb_transolver.hip), one function per
kernel contract, written from the comment blocks of that file and from Physics_Attention.py:148-176; never from a kernel's output and
without autograd: the backward formulas are written out.  tests/test_transolver_kernels_host.py checks each of them in fp64 against
torch autograd of the composed forward and against oracle/transolver_oracle.py.

Every function takes the working ``dtype`` last: the floating-point arguments are cast to it and everything is computed in it (fp64 = the
reference, fp32 = "what plain fp32 arithmetic loses on these inputs").  Tokens are channels-last rows; a head is a contiguous group of
32 channels of a row.  Shapes: xf [B*ntok][2C] = [fx_mid | x_mid], w [B*ntok][heads][G], slice tokens [B][heads][G][32],
norm [B][heads][G].

Contractions over the 32 channels of a head or over the G <= 32 slices are matrix products.  Sums over TOKENS are written as an
element-wise product and ``Tensor.sum``, which adds pairwise, and not as a matrix product: what the fp32 run loses then does not depend
on the order in which the host's BLAS adds (tests/unet_kernel_cases.py:final_case met one that adds 4100 terms one after the other and
loses 1.7e-6 by it).

``_mut`` is for tests/test_transolver_kernels_host.py alone: it switches ONE term of a formula to a wrong one, to prove that the cases
of tests/transolver_kernel_cases.py would notice."""
import torch

import unet_restatement as U

DH = 32
SCALE = DH ** -0.5
NORM_EPS = 1e-5             # Physics_Attention.py:162: slice_token / (slice_norm + 1e-5)
TEMP_MIN, TEMP_MAX = 0.1, 5.0

_c = U._c


# ================================================================================================ per-token kernels
def tokens_lift(x, W, b, act, dtype):
    """out[m][n] = act(sum_k x[m][k] W[n][k] + b[n]); act: exact (erf) GELU or none"""
    x, W, b = _c(dtype, x, W, b)
    y = x @ W.t() + b
    return torch.nn.functional.gelu(y) if act else y


def layernorm_fwd(x, gamma, beta, eps, dtype):
    """x [M][C]: (x - mean) / sqrt(biased var + eps) * gamma + beta"""
    return U.layernorm_fwd(x, gamma, eps, dtype) + _c(dtype, beta)


def layernorm_bwd(x, gamma, gy, gadd, eps, dtype):
    """(gx [M][C], dgamma [C], dbeta [C]) of tests/unet_restatement.py:layernorm_bwd, with gx += gadd when it is given (the gradient
    that reaches x past the LayerNorm, through the residual connection)"""
    gx, dg, db = U.layernorm_bwd(x, gamma, gy, eps, dtype)
    return (gx if gadd is None else gx + _c(dtype, gadd)), dg, db


# ================================================================================================ slice / deslice
def _heads(t, B, ntok, heads):
    """[B*ntok][heads*32] -> [B][ntok][heads][32]"""
    return t.reshape(B, ntok, heads, DH)


def _token_sum(a, v):
    """a [B][ntok][heads][G], v [B][ntok][heads][32] -> [B][heads][G][32]: sum over the tokens of a sample of a[..g] * v[..c]"""
    return torch.stack([(a[b][..., :, None] * v[b][..., None, :]).sum(0) for b in range(a.shape[0])])


def clamp_temp(temp, dtype):
    return _c(dtype, temp).clamp(TEMP_MIN, TEMP_MAX)


def slice_weights(xm, Ws, bs, tau):
    """xm [B][ntok][heads][32], tau [heads] (already clamped) -> w [B][ntok][heads][G] = softmax_g((xm . Ws[g] + bs[g]) / tau[h])"""
    s = ((xm @ Ws.t()) + bs) / tau[:, None]
    e = (s - s.amax(-1, keepdim=True)).exp()
    return e / e.sum(-1, keepdim=True)


def slice_fwd(xf, Ws, bs, temp, B, ntok, heads, G, dtype):
    """rpb_slice_fwd without w_in: (w [B*ntok][heads][G], tokS [B][heads][G][32], norm [B][heads][G]),
    tokS = sum over a sample's tokens of w * fx_mid, norm = the same sum of w alone"""
    xf, Ws, bs = _c(dtype, xf, Ws, bs)
    C = heads * DH
    w = slice_weights(_heads(xf[:, C:], B, ntok, heads), Ws, bs, clamp_temp(temp, dtype))
    return w.reshape(B * ntok, heads, G), _token_sum(w, _heads(xf[:, :C], B, ntok, heads)), w.sum(1)


def slice_tokens_given_w(x, w, B, ntok, heads, G, dtype):
    """rpb_slice_fwd with w_in (the backward of deslice with respect to the attended slice tokens): x [B*ntok][C], w given ->
    [B][heads][G][32] = sum over a sample's tokens of w * x"""
    x, w = _c(dtype, x, w)
    return _token_sum(w.reshape(B, ntok, heads, G), _heads(x, B, ntok, heads))


def deslice(w, tok2, B, ntok, heads, G, dtype):
    """out[m][h*32 + c] = sum_g w[m][h][g] tok2[b][h][g][c]  -> [B*ntok][C]"""
    w, tok2 = _c(dtype, w, tok2)
    out = torch.einsum("bnhg,bhgc->bnhc", w.reshape(B, ntok, heads, G), tok2)
    return out.reshape(B * ntok, heads * DH)


def slice_bwd(xf, w, gox, tok2, gT, gN, Ws, temp, B, ntok, heads, G, dtype, _mut=None):
    """rpb_slice_bwd, from the SAVED weights w.  With gox = dL/d(deslice output), gT = dL/d(tokS), gN = dL/d(norm):
        gw[g]  = sum_c gox[c] tok2[g][c] + sum_c fx[c] gT[g][c] + gN[g]
        gl[g]  = w[g] (gw[g] - sum_g' w[g'] gw[g'])
        g_xmid = (1/tau) sum_g gl[g] Ws[g],   g_fxmid = sum_g w[g] gT[g]
        dWs[g][c] = (1/tau) sum gl[g] xmid[c],  dbs[g] = (1/tau) sum gl[g],  dtau[h] = -(1/tau) sum gl[g] log w[g]
    -> (gxf [B*ntok][2C] = [g_fxmid | g_xmid], dWs [G][32], dbs [G], dtau [heads], dtau_abs [heads]).

    CONVENTION: dtau is the derivative with respect to the CLAMPED temperature tau = clamp(temp, 0.1, 5) -- a head outside the clamp
    gets the value it would have at the clamp's edge, not zero.  The ``inside`` mask that zeroes it is applied by model/transolver.py,
    not by the kernel.
    dtau_abs[h] = (1/tau) sum |gl[g] log w[g]|, the sum of the absolute values of dtau's terms: the scale dtau's error is measured on
    (tests/transolver_kernel_cases.py:dtau_measure)."""
    xf, w, gox, tok2, gT, gN, Ws = _c(dtype, xf, w, gox, tok2, gT, gN, Ws)
    C = heads * DH
    tau = clamp_temp(temp, dtype)
    w = w.reshape(B, ntok, heads, G)
    fx, xm, go = (_heads(t, B, ntok, heads) for t in (xf[:, :C], xf[:, C:], gox))
    gw = torch.einsum("bnhc,bhgc->bnhg", go, tok2) + torch.einsum("bnhc,bhgc->bnhg", fx, gT)
    if _mut != "gw_without_gN":
        gw = gw + gN[:, None]
    gl = w * (gw - (w * gw).sum(-1, keepdim=True))
    glr = gl / tau[:, None]
    g_xm = glr @ Ws
    g_fx = torch.einsum("bnhg,bhgc->bnhc", w, gT)
    gxf = torch.cat((g_fx.reshape(B * ntok, C), g_xm.reshape(B * ntok, C)), 1)
    dWs = _token_sum(glr, xm).sum((0, 1))
    dbs = glr.sum((0, 1, 2))
    terms = gl * w.clamp_min(torch.finfo(dtype).tiny).log()          # w = 0 (a weight that underflowed): the term is 0, as in the kernel
    dtau, dtau_abs = -terms.sum((0, 1, 3)), terms.abs().sum((0, 1, 3))
    if _mut != "dtau_without_inv_tau":
        dtau = dtau / tau
    return gxf, dWs, dbs, dtau, dtau_abs / tau


# ================================================================================================ attention among the slice tokens
def _attn_parts(tokS, norm, Wq, Wk, Wv, amask):
    t = tokS / (norm + NORM_EPS)[..., None]
    q, k, v = t @ Wq.t(), t @ Wk.t(), t @ Wv.t()
    s = q @ k.transpose(-1, -2) * SCALE
    e = (s - s.amax(-1, keepdim=True)).exp()
    P = e / e.sum(-1, keepdim=True)
    return t, q, k, v, P, (P if amask is None else P * amask)


def slice_attn(tokS, norm, Wq, Wk, Wv, amask, dtype):
    """rpb_slice_attn (amask None) and the forward of rpb_slice_attn_train: tokS [BH][G][32], norm [BH][G], amask [BH][G][G] or None
        t = tokS / (norm + 1e-5);  q, k, v = t Wq^T, t Wk^T, t Wv^T;  P = softmax(q k^T / sqrt(32));  A = P * amask;  out = A v
    CONVENTION: the division is by norm + 1e-5, as Physics_Attention.py:162 has it, and so is every derivative below."""
    tokS, norm, Wq, Wk, Wv, amask = _c(dtype, tokS, norm, Wq, Wk, Wv, amask)
    *_, v, _, A = _attn_parts(tokS, norm, Wq, Wk, Wv, amask)
    return A @ v


def slice_attn_bwd(tokS, norm, Wq, Wk, Wv, amask, go, dtype, _mut=None):
    """the backward of rpb_slice_attn_train for go = dL/d(out) [BH][G][32] ->
    (gT [BH][G][32] = dL/d(tokS), gN [BH][G] = dL/d(norm), gW [BH][3][32][32] = PER-(b,h) dWq, dWk, dWv; the caller adds them up):
        gv = A^T go;  dP = (go v^T) * amask;  dS = P (dP - sum_j dP P) / sqrt(32);  gq = dS k;  gk = dS^T q
        dW*[c][j] = sum_g g*[g][c] t[g][j];  gt = gq Wq + gk Wk + gv Wv;  gT = gt / (norm + 1e-5);  gN = -sum_j gt t / (norm + 1e-5)"""
    tokS, norm, Wq, Wk, Wv, amask, go = _c(dtype, tokS, norm, Wq, Wk, Wv, amask, go)
    t, q, k, v, P, A = _attn_parts(tokS, norm, Wq, Wk, Wv, amask)
    gv = A.transpose(-1, -2) @ go
    dP = go @ v.transpose(-1, -2)
    if amask is not None and _mut != "dP_without_mask":
        dP = dP * amask
    dS = SCALE * P * (dP - (dP * P).sum(-1, keepdim=True))
    gq, gk = dS @ k, dS.transpose(-1, -2) @ q
    gW = torch.stack([g.transpose(-1, -2) @ t for g in (gq, gk, gv)], 1)
    gt = gq @ Wq + gk @ Wk + gv @ Wv
    den = (norm + NORM_EPS)[..., None]
    return gt / den, -((gt * t).sum(-1, keepdim=True) / den)[..., 0], gW
