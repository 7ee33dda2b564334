"""Host side (no GPU) of the per-kernel U-Net tests:
* tests/guarded.py must trip on each kind of stray access -- proven with fake "kernels" written in torch on a CPU arena;
* every restatement of tests/unet_restatement.py, in fp64, against an independent statement of the same mathematics (torch's own
  group_norm / layer_norm / conv3d and their autograd, and oracle/unet_oracle.py, which is pinned to the reference by tests/golden);
* every case of tests/test_gpu_unet_kernels.py is well conditioned: 8 * e32 <= 1e-5 on both measures."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_l2

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                              # noqa: E402
import unet_kernel_cases as K               # noqa: E402
import unet_restatement as R                # noqa: E402

F32, F64 = torch.float32, torch.float64
TOL = 1e-12                                   # fp64 against fp64


# ================================================================================================ the arena trips
def _past(view, n):
    """the view's storage from its first element on, ``n`` elements long -- how a kernel with a wrong bound sees its pointer"""
    return torch.as_strided(view, (n,), (1,), view.storage_offset())


def _before(view, n):
    return torch.as_strided(view, (n,), (1,), view.storage_offset() - n)


def _arena():
    a = guarded.Arena("cpu")
    x, y = a.inp(torch.arange(12.0).view(3, 4), name="x"), a.out(3, 4, name="y")
    return a, x, y


def test_arena_passes_a_correct_kernel_and_keeps_alignment():
    a, x, y = _arena()
    y.op[:] = 2 * x.op
    a.check()
    assert torch.equal(y.get(), 2 * torch.arange(12.0).view(3, 4))
    assert x.off % 4 == 0 and y.off % 4 == 0 and x.guard >= 4096 and y.guard >= 4096
    b = guarded.Arena("cpu")
    w = b.inp(torch.zeros(2, 5504))
    assert w.guard >= 2 * 5504                                   # two rows of the widest operand


def test_arena_sees_a_write_past_the_end():
    a, x, y = _arena()
    _past(y.op, 13)[:] = 1.0
    with pytest.raises(AssertionError, match="guard after operand 'y'.*the first 1 element"):
        a.check()


def test_arena_sees_a_write_before_the_start():
    a, x, y = _arena()
    y.op[:] = 1.0
    _before(y.op, 1)[:] = 1.0
    with pytest.raises(AssertionError, match="guard before operand 'y'.*the first 1 element"):
        a.check()


def test_arena_sees_an_unwritten_element():
    a, x, y = _arena()
    y.op[:11] = 1.0
    with pytest.raises(AssertionError, match="1 element.s. were never written, the first at flat index 11"):
        a.check()


def test_arena_sees_a_result_computed_from_a_guard_element():
    a, x, y = _arena()
    y.op[:] = _past(x.op, 13)[1:]                                # reads one element past the input
    with pytest.raises(AssertionError, match="NaN"):
        a.check()
    a, x, y = _arena()
    y.op[:] = _before(x.op, 1).sum() + x.op                      # ... and one before it
    with pytest.raises(AssertionError, match="NaN"):
        a.check()


def test_arena_sees_a_write_to_an_input_and_to_a_named_unwritten_element():
    a, x, y = _arena()
    y.op[:] = 1.0
    x.op[3] = 7.0
    with pytest.raises(AssertionError, match="input operand 'x'"):
        a.check()
    for stray in (False, True):
        a = guarded.Arena("cpu")
        keep = torch.zeros(3, 4, dtype=torch.bool)
        keep[:, 2:] = True                                       # a column-range output: the kernel owns columns 0..1
        y = a.out(3, 4, unwritten=keep)
        y.op.view(3, 4)[:, :3 if stray else 2] = 1.0
        if stray:
            with pytest.raises(AssertionError, match="documented not to write"):
                a.check()
        else:
            a.check()


def test_integer_arena_guards_with_the_given_value():
    a = guarded.Arena("cpu", torch.int32, fill=40)
    i = a.inp(torch.tensor([1, 2, 3], dtype=torch.int32))
    assert int(_past(i.op, 5)[4]) == 40 and int(_before(i.op, 1)[0]) == 40
    a.check()


def test_fp64_arena_trips_too():
    a = guarded.Arena("cpu", F64)
    y = a.out(5)
    y.op[:] = 1.0
    a.check()
    a = guarded.Arena("cpu", F64)
    y = a.out(5)
    _past(y.op, 6)[:] = 1.0
    with pytest.raises(AssertionError, match="guard after"):
        a.check()
    a = guarded.Arena("cpu", F64)
    y = a.out(5)
    y.op[:4] = 1.0
    with pytest.raises(AssertionError, match="never written"):
        a.check()


# ================================================================================================ restatements against independent statements
def test_chan_algebra_against_group_norm_silu_autograd():
    torch.manual_seed(0)
    B, n, C, G = 2, 30, 64, 8
    cg, cnt = C // G, float(n * (C // G))
    x = (torch.randn(B, n, C, dtype=F64) * 1.5 + 0.3).requires_grad_(True)
    gamma, beta, gy = torch.rand(C, dtype=F64) + 0.5, torch.randn(C, dtype=F64), torch.randn(B, n, C, dtype=F64)
    y_ref = F.silu(F.group_norm(x.transpose(1, 2), G, gamma, beta, 1e-5)).transpose(1, 2)
    gx_ref, = torch.autograd.grad(y_ref, x, gy)
    S = R.chan_stats(x.detach(), F64).requires_grad_(True)
    assert rel_l2(S.detach()[:, 0], x.detach().sum(1)) < TOL and rel_l2(S.detach()[:, 1], (x.detach() ** 2).sum(1)) < TOL
    Sg = S.view(B, 2, G, cg).sum(-1)
    mean = Sg[:, 0] / cnt
    inv = (Sg[:, 1] / cnt - mean * mean + 1e-5).rsqrt()
    A = inv.repeat_interleave(cg, 1) * gamma
    Bc = beta - mean.repeat_interleave(cg, 1) * A
    assert rel_l2(R.affine_silu_fwd(x.detach(), A.detach(), Bc.detach(), None, F64), y_ref.detach()) < TOL
    res = torch.randn(B, n, C, dtype=F64)
    assert rel_l2(R.affine_silu_fwd(x.detach(), A.detach(), Bc.detach(), res, F64), y_ref.detach() + res) < TOL
    red = R.affine_silu_bwd_reduce(x.detach(), gy, A.detach(), Bc.detach(), F64)        # (dL/dA, dL/dBc)
    dS, = torch.autograd.grad([A, Bc], S, [red[:, 0], red[:, 1]])
    gx = R.affine_silu_bwd_apply(x.detach(), gy, A.detach(), Bc.detach(), dS[:, 0], 2 * dS[:, 1], F64)
    assert rel_l2(gx, gx_ref) < 1e-10


def test_layernorm_against_torch_autograd():
    torch.manual_seed(1)
    M, C = 9, 128
    x = (torch.randn(M, C, dtype=F64) * 1.5 + 0.3).requires_grad_(True)
    gamma, beta = (torch.rand(C, dtype=F64) + 0.5).requires_grad_(True), torch.zeros(C, dtype=F64, requires_grad=True)
    gy = torch.randn(M, C, dtype=F64)
    y = F.layer_norm(x, (C,), gamma, beta, 1e-5)
    y.backward(gy)
    assert rel_l2(R.layernorm_fwd(x.detach(), gamma.detach(), 1e-5, F64), y.detach()) < TOL
    gx, dg, db = R.layernorm_bwd(x.detach(), gamma.detach(), gy, 1e-5, F64)
    assert rel_l2(gx, x.grad) < TOL and rel_l2(dg, gamma.grad) < TOL and rel_l2(db, beta.grad) < TOL


@pytest.mark.parametrize("Cin", [3, 5])
def test_im2col_times_init_weight_against_conv3d(Cin):
    torch.manual_seed(2)
    B, T, H, W, dim = 2, 2, 5, 9, 8
    x = torch.randn(B, T, H, W, Cin, dtype=F64)
    w, b = torch.randn(dim, Cin, 7, 7, 7, dtype=F64), torch.randn(dim, dtype=F64)
    cols, ldc = 343 * Cin, K.init_ldc(Cin)
    Wi = torch.zeros(dim, ldc, dtype=F64)
    Wi[:, :cols] = w.permute(0, 2, 3, 4, 1).reshape(dim, cols)                     # model/unet.py: _w("init", ...)
    col = R.im2col(x, 7, ldc, F64)
    assert not col[:, cols:].any()
    ref = F.conv3d(x.permute(0, 4, 1, 2, 3), w, b, padding=3).permute(0, 2, 3, 4, 1).reshape(-1, dim)
    assert rel_l2(R.gemm_nt(col, Wi, b, None, F64), ref) < TOL


def test_strided_and_transposed_layouts_against_conv3d():
    """the gather layouts the GPU test hands to the kernels, multiplied out by hand, against the restatements (= torch's convolutions)"""
    torch.manual_seed(3)
    B, T, H, W, C = 1, 2, 4, 6, 4
    x = torch.randn(B * T * H * W, C, dtype=F64)
    wd, wu, bias = torch.randn(C, C, 1, 4, 4, dtype=F64), torch.randn(C, C, 1, 4, 4, dtype=F64), torch.randn(C, dtype=F64)
    xv = F.pad(x.view(B, T, H, W, C), (0, 0, 1, 1, 1, 1))
    Wd, down = K.down_layout(wd), R.strided_conv(x, wd, bias, B, (T, H, W), F64).view(B, T, H // 2, W // 2, C)
    for h in range(H // 2):
        for w in range(W // 2):
            patch = xv[:, :, 2 * h:2 * h + 4, 2 * w:2 * w + 4].reshape(B, T, 16 * C)
            assert rel_l2(patch @ Wd.t() + bias, down[:, :, h, w]) < TOL
    Wc, up = K.up_layout(wu), R.transposed_conv(x, wu, bias, B, (T, H, W), F64)
    for cls in range(4):
        ph, pw = cls >> 1, cls & 1
        offs = [(dh, dw) for dh in ((1, 0) if ph else (0, -1)) for dw in ((1, 0) if pw else (0, -1))]       # jh, jw = 0, 1
        gathered = torch.cat([xv[:, :, 1 + dh:1 + dh + H, 1 + dw:1 + dw + W] for dh, dw in offs], -1).reshape(-1, 4 * C)
        assert rel_l2(gathered @ Wc[cls].t() + bias, up[K.up_class_rows(cls, B, T, H, W)]) < TOL
    gy = torch.randn(B * T * (H // 2) * (W // 2), C, dtype=F64)
    dW, db = R.strided_conv_wgrad(gy, x, C, B, (T, H, W), F64)
    patches = torch.stack([xv[:, :, 2 * h:2 * h + 4, 2 * w:2 * w + 4].reshape(B, T, 16 * C) for h in range(H // 2) for w in range(W // 2)], 2)
    assert rel_l2(K.down_unlayout(gy.t() @ patches.reshape(-1, 16 * C), C), dW) < TOL and rel_l2(gy.sum(0), db) < TOL


def _tok(t):
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


def _prenorm(x5, gamma, Wqkv):
    x = _tok(x5)
    y = R.layernorm_fwd(x, gamma.reshape(-1), 1e-5, F64)
    return x, y, R.gemm_nt(y, Wqkv, None, None, F64)


def _prenorm_bwd(x, y, gamma, Wqkv, gqkv, G):
    """(d x with the residual branch, d gamma, d W_qkv)"""
    gx, dg, _ = R.layernorm_bwd(x, gamma.reshape(-1), R.gemm_nt(gqkv, Wqkv.t(), None, None, F64), 1e-5, F64)
    return gx + G, dg, R.gemm_tn(gqkv, y, F64)[0]


def _diag32(S):
    """[F][2][64][64] products of the 2 x 64 channel pairs -> the four 32 x 32 per-head blocks (model/unet.py:_diag32, any dtype)"""
    S = S.view(S.shape[0], 2, 2, 32, 2, 32)
    return torch.stack([S[:, 0, 0, :, 0], S[:, 0, 1, :, 1], S[:, 1, 0, :, 0], S[:, 1, 1, :, 1]], dim=1)


def _embed32(Wh):
    """[F][4][32][32] -> block-diagonal [F][2][64][64] (model/unet.py:_embed32, which is fp32 only)"""
    out = torch.zeros(Wh.shape[0], 2, 2, 32, 2, 32, dtype=Wh.dtype)
    out[:, 0, 0, :, 0], out[:, 0, 1, :, 1], out[:, 1, 0, :, 0], out[:, 1, 1, :, 1] = Wh[:, 0], Wh[:, 1], Wh[:, 2], Wh[:, 3]
    return out.view(Wh.shape[0], 2, 64, 64)


def _leaves(sd):
    return {k: v.clone().requires_grad_(True) for k, v in sd.items()}


def test_linear_attention_stages_against_the_oracle():
    from oracle import unet_oracle as UO
    torch.manual_seed(4)
    b, c, f, h, w = 2, 64, 2, 3, 5
    Fr, n = b * f, h * w
    sd = {"norm.gamma": torch.rand(1, c, 1, 1, 1, dtype=F64) + 0.5, "fn.to_qkv.weight": torch.randn(384, c, 1, 1, dtype=F64) / 4,
          "fn.to_out.weight": torch.randn(c, 128, 1, 1, dtype=F64) / 8, "fn.to_out.bias": torch.randn(c, dtype=F64)}
    x5 = torch.randn(b, c, f, h, w, dtype=F64, requires_grad=True)
    lv = _leaves(sd)
    out_ref = UO.spatial_linear_attn(lv, "", x5)
    G5 = torch.randn_like(out_ref)
    out_ref.backward(G5)
    Wqkv, Wout = sd["fn.to_qkv.weight"].view(384, c), sd["fn.to_out.weight"].view(c, 128)
    x, y, qkv = _prenorm(x5.detach(), sd["norm.gamma"], Wqkv)
    qkv = qkv.view(Fr, n, 384)
    kmax = R.col_reduce(qkv[..., 128:256], 0, F64)
    qe = R.linattn_prep_fwd(qkv, kmax, F64)
    q1, E, v = qe[..., :128], qe[..., 128:], qkv[..., 256:]
    Z = R.col_reduce(E, 1, F64).view(Fr, 4, 32)
    S = _diag32(R.head_scores(E, v, F64))                                    # E^T v, the four 32 x 32 head blocks
    ctx = S / Z[..., None]
    o = R.head_apply(q1, _embed32(ctx), F64)
    out = R.gemm_nt(o.reshape(-1, 128), Wout, sd["fn.to_out.bias"], x, F64)
    assert rel_l2(out, _tok(out_ref.detach())) < 1e-11
    # ---- backward, composed as model/unet.py:_linear_attn composes the kernels
    G = _tok(G5)
    go = R.gemm_nt(G, Wout.t(), None, None, F64).view(Fr, n, 128)
    dq1 = R.head_apply(go, _embed32(ctx.transpose(-1, -2)), F64)
    dctx = _diag32(R.head_scores(q1, go, F64))
    dS, dZ = dctx / Z[..., None], -(dctx * S).sum(-1) / (Z * Z)
    dE = R.head_apply(v, _embed32(dS.transpose(-1, -2)), F64)
    dv = R.head_apply(E, _embed32(dS), F64)
    gqk = R.linattn_prep_bwd(qe, torch.cat((dq1, dE), -1), dZ.reshape(Fr, 128), F64)
    gqkv = torch.cat((gqk, dv), -1).reshape(-1, 384)
    gx, dg, dWq = _prenorm_bwd(x, y, sd["norm.gamma"], Wqkv, gqkv, G)
    assert rel_l2(gx, _tok(x5.grad)) < 1e-10
    assert rel_l2(dg, lv["norm.gamma"].grad.reshape(-1)) < 1e-10 and rel_l2(dWq, lv["fn.to_qkv.weight"].grad.view(384, c)) < 1e-10
    assert rel_l2(R.gemm_tn(G, o.reshape(-1, 128), F64)[0], lv["fn.to_out.weight"].grad.view(c, 128)) < 1e-10


def test_temporal_attention_against_the_oracle():
    from oracle import unet_oracle as UO
    torch.manual_seed(5)
    b, c, f, h, w = 2, 64, 7, 2, 3
    freqs = (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))).double()
    sd = {"norm.gamma": torch.rand(1, c, 1, 1, 1, dtype=F64) + 0.5, "fn.fn.to_qkv.weight": torch.randn(384, c, dtype=F64) / 4,
          "fn.fn.to_out.weight": torch.randn(c, 128, dtype=F64) / 8}
    lv = _leaves(sd)
    lv["fn.fn.rotary_emb.freqs"] = freqs
    bias = torch.randn(4, f, f, dtype=F64, requires_grad=True)
    x5 = torch.randn(b, c, f, h, w, dtype=F64, requires_grad=True)
    out_ref = UO.temporal_attn(lv, "", x5, bias)
    G5 = torch.randn_like(out_ref)
    out_ref.backward(G5)
    ang = torch.repeat_interleave(torch.arange(f, dtype=F64)[:, None] * freqs[None, :], 2, dim=-1)
    rc, rs = ang.cos(), ang.sin()
    x, y, qkv = _prenorm(x5.detach(), sd["norm.gamma"], sd["fn.fn.to_qkv.weight"])
    qkv = qkv.view(b, f, h * w, 384)
    o = R.tattn_fwd(qkv, rc, rs, bias.detach(), F64)
    out = R.gemm_nt(o.reshape(-1, 128), sd["fn.fn.to_out.weight"], None, x, F64)
    assert rel_l2(out, _tok(out_ref.detach())) < 1e-11
    G = _tok(G5)
    go = R.gemm_nt(G, sd["fn.fn.to_out.weight"].t(), None, None, F64).view(b, f, h * w, 128)
    gqkv, dbias = R.tattn_bwd(qkv, rc, rs, bias.detach(), go, F64)
    gx, dg, dWq = _prenorm_bwd(x, y, sd["norm.gamma"], sd["fn.fn.to_qkv.weight"], gqkv.reshape(-1, 384), G)
    assert rel_l2(gx, _tok(x5.grad)) < 1e-10 and rel_l2(dbias, bias.grad) < 1e-10
    assert rel_l2(dg, lv["norm.gamma"].grad.reshape(-1)) < 1e-10 and rel_l2(dWq, lv["fn.fn.to_qkv.weight"].grad) < 1e-10


def test_bottleneck_attention_against_the_oracle():
    from oracle import unet_oracle as UO
    torch.manual_seed(6)
    b, c, f, h, w = 1, 64, 3, 5, 7
    sd = {"norm.gamma": torch.rand(1, c, 1, 1, 1, dtype=F64) + 0.5, "fn.fn.to_qkv.weight": torch.randn(384, c, dtype=F64) / 4,
          "fn.fn.to_out.weight": torch.randn(c, 128, dtype=F64) / 8}
    lv = _leaves(sd)
    x5 = torch.randn(b, c, f, h, w, dtype=F64, requires_grad=True)
    out_ref = UO.mid_spatial_attn(lv, "", x5)
    G5 = torch.randn_like(out_ref)
    out_ref.backward(G5)
    x, y, qkv = _prenorm(x5.detach(), sd["norm.gamma"], sd["fn.fn.to_qkv.weight"])
    qkv = qkv.view(b * f, h * w, 384)
    o, lse = R.sattn_fwd(qkv, F64)
    q, k = (t.reshape(b * f, h * w, 4, 32).transpose(1, 2) for t in (qkv[..., :128], qkv[..., 128:256]))
    assert rel_l2(lse.exp(), ((q * 32 ** -0.5) @ k.transpose(-1, -2)).exp().sum(-1)) < 1e-11
    out = R.gemm_nt(o.reshape(-1, 128), sd["fn.fn.to_out.weight"], None, x, F64)
    assert rel_l2(out, _tok(out_ref.detach())) < 1e-11
    G = _tok(G5)
    go = R.gemm_nt(G, sd["fn.fn.to_out.weight"].t(), None, None, F64).view(b * f, h * w, 128)
    gx, dg, dWq = _prenorm_bwd(x, y, sd["norm.gamma"], sd["fn.fn.to_qkv.weight"], R.sattn_bwd(qkv, go, F64).reshape(-1, 384), G)
    assert rel_l2(gx, _tok(x5.grad)) < 1e-10
    assert rel_l2(dg, lv["norm.gamma"].grad.reshape(-1)) < 1e-10 and rel_l2(dWq, lv["fn.fn.to_qkv.weight"].grad) < 1e-10


def test_small_restatements_against_plain_torch():
    torch.manual_seed(7)
    from oracle import unet_oracle as UO
    from realpdebench_amd.model.unet import _rel_pos_index
    x = torch.randn(5, 12, dtype=F64)
    assert torch.equal(R.colsum(x, F64), x.sum(0))
    dst = torch.randn(5, 20, dtype=F64)
    got = R.copy_cols(x, dst, 8, 4, 12, F64)
    assert torch.equal(got[:, 12:], x[:, 4:12]) and torch.equal(got[:, :12], dst[:, :12])
    assert torch.equal(R.copy_cols(x, torch.zeros(5, 24, dtype=F64), 12, 0, 12, F64), torch.cat((torch.zeros(5, 12, dtype=F64), x), 1))
    table = torch.randn(32, 4, dtype=F64, requires_grad=True)
    ref = UO.rel_pos_bias(table, 20)
    idx = _rel_pos_index(20, "cpu")
    assert torch.equal(R.relpos_fwd(table.detach(), idx, F64).view(4, 20, 20), ref.detach())
    g = torch.randn(4, 20, 20, dtype=F64)
    ref.backward(g)
    assert rel_l2(R.relpos_bwd(g.view(4, 400), idx, 32, F64), table.grad) < TOL
    G, A = torch.randn(9, 3, dtype=F64), torch.randn(9, 6, dtype=F64)
    dW, db = R.gemm_tn(G, A, F64)
    assert rel_l2(dW, torch.einsum("mn,mk->nk", G, A)) < TOL and rel_l2(db, G.sum(0)) < TOL


# ================================================================================================ conditioning of the GPU cases
@pytest.mark.parametrize("make,args", K.all_cases(), ids=lambda v: getattr(v, "__name__", None) or "-".join(str(a) for a in v))
def test_gpu_cases_are_well_conditioned(make, args):
    case = make(*args)
    r64, r32 = case.refs()
    assert set(r64) == set(r32)
    for key in r64:
        if key in case.exact:
            continue
        for kind, e32 in zip(K.MEASURES, K.measures(r32[key], r64[key])):
            print(f"[unet-cases] {case.name} {key} {kind}: e32 {e32:.3e}")
            assert 8 * e32 <= K.BADLY_CONDITIONED, f"{case.name} {key}: the fp32 restatement itself is off by {e32:.3e} ({kind})"
