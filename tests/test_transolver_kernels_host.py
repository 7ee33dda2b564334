"""Host side (no GPU) of the per-kernel Transolver tests:
* every restatement of tests/transolver_restatement.py, in fp64, against an independent statement of the same mathematics: torch
  autograd of the composed forward, F.layer_norm, and the Physics-Attention piece of oracle/transolver_oracle.py (pinned to the reference
  by tests/golden);
* every case of tests/test_gpu_transolver_kernels.py is well conditioned: 8 * e32 <= 1e-5 on every output and measure (the temperature
  gradient on its own measure, tests/transolver_kernel_cases.py:dtau_measure);
* the cases would notice: the fp32 restatement with ONE wrong term, judged exactly as a kernel's output is, fails the bound."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_l2

sys.path.insert(0, os.path.join(ROOT, "tests"))
import transolver_kernel_cases as K         # noqa: E402
import transolver_restatement as R          # noqa: E402

F32, F64 = torch.float32, torch.float64
TOL = 1e-12                                   # fp64 against fp64

BPS16 = K.slice_bps(16)
SLICE_SHAPES = K.slice_shapes(BPS16)
LN_ROWS0 = K.ln_bwd_rows(10 ** 9)
LN_ROWS_SHAPE = K.ln_rows_shape(LN_ROWS0)


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)                        # the references of a case are computed once for all the tests of this file


# ================================================================================================ restatements against independent statements
def test_slice_bwd_against_autograd():
    """L = sum gox * deslice(w, tok2) + sum gT * tokS + sum gN * norm, differentiated with respect to xf, Ws, bs and the CLAMPED tau"""
    B, ntok, heads, G = 2, 45, 3, 12
    c = K.slice_case(B, ntok, heads, G)
    C = heads * 32
    xf, Ws, bs = (c.inp[k].double().requires_grad_(True) for k in ("xf", "Ws", "bs"))
    tau = c.temp.double().clamp(0.1, 5.0).requires_grad_(True)
    assert float(tau.detach()[1]) == 0.1 and float(c.temp[1]) < 0.1                       # a clamped head is among them
    gox, tok2, gT, gN = (c.inp[k].double() for k in ("gox", "tok2", "gT", "gN"))
    fx, xm = (xf[:, s].reshape(B, ntok, heads, 32).permute(0, 2, 1, 3) for s in (slice(0, C), slice(C, 2 * C)))     # B h N c
    w = torch.softmax((xm @ Ws.t() + bs) / tau.view(1, heads, 1, 1), -1)                                               # B h N G
    tokS, norm = torch.einsum("bhnc,bhng->bhgc", fx, w), w.sum(2)
    ox = torch.einsum("bhgc,bhng->bhnc", tok2, w).permute(0, 2, 1, 3).reshape(B * ntok, C)
    w64, tokS64, norm64 = R.slice_fwd(c.xf, c.Ws, c.bs, c.temp, B, ntok, heads, G, F64)
    assert rel_l2(w64, w.detach().permute(0, 2, 1, 3).reshape(B * ntok, heads, G)) < TOL
    assert rel_l2(tokS64, tokS.detach()) < TOL and rel_l2(norm64, norm.detach()) < TOL
    assert rel_l2(R.deslice(w64, tok2, B, ntok, heads, G, F64), ox.detach()) < TOL
    assert rel_l2(R.slice_tokens_given_w(gox, w64, B, ntok, heads, G, F64),
                  torch.einsum("bhnc,bhng->bhgc", gox.reshape(B, ntok, heads, 32).permute(0, 2, 1, 3), w.detach())) < TOL
    ((gox * ox).sum() + (gT * tokS).sum() + (gN * norm).sum()).backward()
    gxf, dWs, dbs, dtau, dtau_abs = R.slice_bwd(c.xf, w64, gox, tok2, gT, gN, c.Ws, c.temp, B, ntok, heads, G, F64)
    assert rel_l2(gxf, xf.grad) < TOL and rel_l2(dWs, Ws.grad) < TOL and rel_l2(dbs, bs.grad) < TOL
    assert rel_l2(dtau, tau.grad) < TOL and float(dtau[1].abs()) > 0             # the clamped head has its value at the clamp's edge
    assert bool((dtau_abs >= dtau.abs()).all())


@pytest.mark.parametrize("masked", [False, True])
def test_slice_attn_against_autograd(masked):
    """sum go * o, differentiated with respect to tokS, norm and per-(b,h) copies of the three weights"""
    BH, G = 6, 12
    c = K.attn_case(BH, G)
    tokS, norm = (c.inp[k].double().requires_grad_(True) for k in ("tokS", "norm"))
    Wq, Wk, Wv = (c.inp[k].double().expand(BH, 32, 32).clone().requires_grad_(True) for k in ("Wq", "Wk", "Wv"))
    amask, go = (c.amask.double() if masked else None), c.go.double()
    t = tokS / (norm + 1e-5)[..., None]
    q, k, v = (t @ W.transpose(-1, -2) for W in (Wq, Wk, Wv))
    attn = torch.softmax(q @ k.transpose(-1, -2) * 32 ** -0.5, -1)
    o = (attn * amask if masked else attn) @ v
    five = (c.tokS, c.norm, c.Wq, c.Wk, c.Wv)
    assert rel_l2(R.slice_attn(*five, c.amask if masked else None, F64), o.detach()) < TOL
    (go * o).sum().backward()
    gT, gN, gW = R.slice_attn_bwd(*five, c.amask if masked else None, c.go, F64)
    assert rel_l2(gT, tokS.grad) < TOL and rel_l2(gN, norm.grad) < TOL
    assert rel_l2(gW, torch.stack((Wq.grad, Wk.grad, Wv.grad), 1)) < TOL


def test_layernorm_against_torch_autograd():
    M, C = 9, 192
    c = K.ln_case(M, C)
    x, gamma, beta = (c.inp[k].double().requires_grad_(True) for k in ("x", "gamma", "beta"))
    y = F.layer_norm(x, (C,), gamma, beta, K.LN_EPS)
    y.backward(c.gy.double())
    assert rel_l2(R.layernorm_fwd(c.x, c.gamma, c.beta, K.LN_EPS, F64), y.detach()) < TOL
    gx, dg, db = R.layernorm_bwd(c.x, c.gamma, c.gy, c.gadd, K.LN_EPS, F64)
    assert rel_l2(gx, x.grad + c.gadd.double()) < TOL and rel_l2(dg, gamma.grad) < TOL and rel_l2(db, beta.grad) < TOL
    assert rel_l2(R.layernorm_bwd(c.x, c.gamma, c.gy, None, K.LN_EPS, F64)[0], x.grad) < TOL


def test_tokens_lift_against_torch():
    c = K.lift_case(300, 8, 64, 0)
    assert rel_l2(R.tokens_lift(c.x, c.W, c.b, 0, F64), F.linear(c.x.double(), c.W.double())) < TOL
    c = K.lift_case(7, 1, 4, 1)
    assert rel_l2(R.tokens_lift(c.x, c.W, c.b, 1, F64), F.gelu(F.linear(c.x.double(), c.W.double(), c.b.double()))) < TOL


def test_forward_chain_against_the_oracle():
    """slice_fwd -> slice_attn -> deslice between the oracle's own convolutions and output projection"""
    from oracle import transolver_oracle as TO
    torch.manual_seed(3)
    B, H, W, D, heads, G = 2, 3, 4, 5, 2, 8
    C, N = heads * 32, H * W * D
    pre = "a."
    sd = {"in_project_fx.weight": torch.randn(C, C, 3, 3, 3) / 40, "in_project_fx.bias": torch.randn(C) * 0.1,
          "in_project_x.weight": torch.randn(C, C, 3, 3, 3) / 40, "in_project_x.bias": torch.randn(C) * 0.1,
          "temperature": torch.tensor(K.TEMPS[:heads]).view(1, heads, 1, 1), "in_project_slice.weight": torch.randn(G, 32) / 4,
          "in_project_slice.bias": torch.randn(G) * 0.3, "to_q.weight": torch.randn(32, 32) / 5, "to_k.weight": torch.randn(32, 32) / 5,
          "to_v.weight": torch.randn(32, 32) / 5, "to_out.0.weight": torch.randn(C, C) / 8, "to_out.0.bias": torch.randn(C) * 0.1}
    sd = {pre + k: v.double() for k, v in sd.items()}
    x = torch.randn(B, N, C, dtype=F64)
    ref = TO.physics_attention(sd, pre, x, heads, H, W, D)
    xc = x.reshape(B, H, W, D, C).permute(0, 4, 1, 2, 3)
    rows = [F.conv3d(xc, sd[pre + n + ".weight"], sd[pre + n + ".bias"], padding=1).permute(0, 2, 3, 4, 1).reshape(B * N, C)
            for n in ("in_project_fx", "in_project_x")]
    w, tokS, norm = R.slice_fwd(torch.cat(rows, 1), sd[pre + "in_project_slice.weight"], sd[pre + "in_project_slice.bias"],
                                sd[pre + "temperature"].reshape(-1), B, N, heads, G, F64)
    tok2 = R.slice_attn(tokS.reshape(B * heads, G, 32), norm.reshape(B * heads, G), sd[pre + "to_q.weight"], sd[pre + "to_k.weight"],
                        sd[pre + "to_v.weight"], None, F64)
    ox = R.deslice(w, tok2.reshape(B, heads, G, 32), B, N, heads, G, F64)
    out = ox @ sd[pre + "to_out.0.weight"].t() + sd[pre + "to_out.0.bias"]
    assert rel_l2(out.reshape(B, N, C), ref) < 1e-11


# ================================================================================================ conditioning of the GPU cases
def _ids(v):
    return getattr(v, "__name__", None) or "-".join(str(a) for a in v)


@pytest.mark.parametrize("make,args", K.all_cases(), ids=_ids)
def test_gpu_cases_are_well_conditioned(make, args):
    case = case_of(make, args)
    r64, r32 = case.refs()
    assert set(r64) == set(r32)
    for key in r64:
        if key in ("dtau", "dtau_abs"):
            continue
        for kind, e32 in zip(K.MEASURES, K.measures(r32[key], r64[key])):
            print(f"[transolver-cases] {case.name} {key} {kind}: e32 {e32:.3e}")
            assert 8 * e32 <= K.BADLY_CONDITIONED, f"{case.name} {key}: the fp32 restatement itself is off by {e32:.3e} ({kind})"
    if "dtau" in r64:
        e32 = K.dtau_measure(r32["dtau"], r64)
        rel = float(((r32["dtau"].double() - r64["dtau"]).abs() / r64["dtau"].abs()).max())
        print(f"[transolver-cases] {case.name} dtau dtau/sum|terms|: e32 {e32:.3e} (relative to dtau itself: {rel:.3e})")
        assert 8 * e32 <= K.BADLY_CONDITIONED, f"{case.name} dtau: the fp32 restatement itself is off by {e32:.3e}"


def test_block_counts_of_the_large_cases():
    """the properties the two B = 16 slice cases and the long LayerNorm case exist for, at the MI355X's 256 compute units"""
    assert BPS16 == 32 and LN_ROWS0 == 8192 and LN_ROWS_SHAPE == (16421, 64)
    (B1, n1, _, _), (B2, n2, h2, _) = SLICE_SHAPES[-2:]
    assert B1 == B2 == 16 and n1 == 64 * BPS16 + 5 and n2 == 32 * BPS16 + 7 and h2 == 8
    tiles = lambda n, blk: len(range(blk * 32, n, BPS16 * 32))                   # the tile loop of slice_fwd_kernel / slice_bwd_kernel
    assert [tiles(n1, b) for b in range(BPS16)] == [3] + [2] * (BPS16 - 1)
    assert [tiles(n2, b) for b in range(BPS16)] == [2] + [1] * (BPS16 - 1)
    assert n2 > 4 * BPS16 * (256 // (h2 * 8))                                    # deslice_kernel: 4 bps blocks of 256 / (C / 4) tokens loop
    M = LN_ROWS_SHAPE[0]
    assert [len(range(wv, M, LN_ROWS0)) for wv in (0, 36, 37, LN_ROWS0 - 1)] == [3, 3, 2, 2]
    K_, N_ = K.LIFT_CASES[-1][1:3]
    assert (K_ + 1) * N_ * 4 == 67584 > 64 * 1024 and (K.LIFT_REFUSED[0] + 1) * K.LIFT_REFUSED[1] * 4 > 160 * 1024


# ================================================================================================ the cases would notice
def rejected(judge, *args):
    with pytest.raises(AssertionError, match="kernel error"):
        judge(*args)


def _first_tiles(t, B, ntok, keep):
    """the rows of the first ``keep`` tokens of every sample"""
    return t.reshape(B, ntok, -1)[:, :keep].reshape(B * keep, -1)


@pytest.mark.parametrize("shape", SLICE_SHAPES[-2:], ids=K.SLICE_IDS[-2:])
def test_mutation_a_second_tile_left_out(shape):
    """token sums and dWs without the tokens of a block's second and later tiles (tokens >= 32 bps of a sample)"""
    B, ntok, heads, G = shape
    c = case_of(K.slice_case, shape)
    r64, r32 = c.refs()
    keep = 32 * BPS16
    cut = {k: _first_tiles(c.inp[k], B, ntok, keep) for k in ("xf", "gox", "w")}
    _, tokS, norm = R.slice_fwd(cut["xf"], c.Ws, c.bs, c.temp, B, keep, heads, G, F32)
    gtok2 = R.slice_tokens_given_w(cut["gox"], cut["w"], B, keep, heads, G, F32)
    _, dWs, dbs, dtau, _ = R.slice_bwd(cut["xf"], cut["w"], cut["gox"], c.tok2, c.gT, c.gN, c.Ws, c.temp, B, keep, heads, G, F32)
    for key, got in (("tokS", tokS), ("norm", norm), ("gtok2", gtok2), ("dWs", dWs), ("dbs", dbs)):
        rejected(K.judge, f"(a) {c.name} {key}", got, r64[key], r32[key])
    rejected(K.judge_dtau, f"(a) {c.name} dtau", dtau, r64, r32)


@pytest.mark.parametrize("shape", SLICE_SHAPES, ids=K.SLICE_IDS)
def test_mutations_b_c_f_of_the_slice_family(shape):
    B, ntok, heads, G = shape
    c = case_of(K.slice_case, shape)
    r64, r32 = c.refs()
    args = (c.xf, c.w, c.gox, c.tok2, c.gT, c.gN, c.Ws, c.temp, B, ntok, heads, G, F32)
    # (b) dtau without the 1 / tau factor
    rejected(K.judge_dtau, f"(b) {c.name} dtau", R.slice_bwd(*args, _mut="dtau_without_inv_tau")[3], r64, r32)
    # (c) gN left out of gw: it reaches g_xmid, dWs, dbs and dtau (g_fxmid does not depend on it)
    gxf, dWs, dbs, dtau, _ = R.slice_bwd(*args, _mut="gw_without_gN")
    for key, got in (("gxf", gxf), ("dWs", dWs), ("dbs", dbs)):
        rejected(K.judge, f"(c) {c.name} {key}", got, r64[key], r32[key])
    rejected(K.judge_dtau, f"(c) {c.name} dtau", dtau, r64, r32)
    # (f) the padded slice rows g >= G of the 32-row MFMA tile leak one unit of weight into norm (no such rows at G = 32)
    if G < 32:
        leak = r32["norm"].clone()
        leak[..., G - 1] += 1.0
        rejected(K.judge, f"(f) {c.name} norm", leak, r64["norm"], r32["norm"])


def test_mutation_d_layernorm_partials_keep_the_first_row_only():
    c = case_of(K.ln_case, LN_ROWS_SHAPE)
    r64, r32 = c.refs()
    _, dg, db = R.layernorm_bwd(c.x[:LN_ROWS0], c.gamma, c.gy[:LN_ROWS0], None, K.LN_EPS, F32)       # row m belongs to wave m % rows0
    rejected(K.judge, f"(d) {c.name} dgamma|dbeta", torch.cat((dg, db)), r64["dgb"], r32["dgb"])


@pytest.mark.parametrize("BH,G", K.ATTN_SHAPES)
def test_mutation_e_attention_backward_without_the_mask(BH, G):
    c = case_of(K.attn_case, (BH, G))
    r64, r32 = c.refs()
    assert bool((c.amask == 0).any()) or BH == 1                                 # some attention weights are dropped
    gT, gN, gW = R.slice_attn_bwd(c.tokS, c.norm, c.Wq, c.Wk, c.Wv, c.amask, c.go, F32, _mut="dP_without_mask")
    for key, got in (("gT_m", gT), ("gN_m", gN), ("gW_m", gW.reshape(BH, 3, 1024)), ("dW_m", gW.sum(0).reshape(-1))):
        rejected(K.judge, f"(e) {c.name} {key}", got, r64[key], r32[key])
