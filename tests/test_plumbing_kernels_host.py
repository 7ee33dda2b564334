"""Host side (no GPU) of the per-kernel tests of the step plumbing kernels (tests/plumbing_kernel_cases.py):
* every restatement, in fp64, against an independent statement of the same mathematics: torch autograd for the lift, the BatchNorm
  passes, the loss and the layer-0 weight gradient, ``torch.optim.Adam`` for Adam (from a preloaded state and chained), a direct triple
  loop with ``math.isqrt`` for the radial bins, plain Python loops for the packers, small_gemm and the reducers;
* ``floor(sqrt(float32(n))) == isqrt(n)`` for every n <= 3 * 63^2: the spectrum kernel's "exact for these small integers", up to its
  R <= 64 limit;
* every case of tests/test_gpu_plumbing_kernels.py is well conditioned: the drivers run here on ``TorchKernels``, a torch stand-in for
  the library on a CPU ``Arena`` that computes the fp32 restatement, and the verdict rejects a case whose 8 * e32 exceeds 1e-5 -- on
  exactly the quantities the GPU test judges (row sums of partial rows, Adam's update);
* the second-trip cases take the second trip at the MI355X's 256 compute units;
* the drivers would notice: with ONE wrong term or ONE out-of-range access the stand-in trips ``Arena.check()``, a bit comparison or
  the verdict in at least one case of its kernel family -- the same driver code the GPU test runs."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_l2

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                               # noqa: E402
import plumbing_kernel_cases as K            # noqa: E402

F32, F64 = torch.float32, torch.float64
TOL = 1e-12                                   # fp64 against fp64
CUS = K.MI355X_CUS
NAN = float("nan")


def _v(t, *shape):
    n = 1
    for s in shape:
        n *= s
    return t[:n].view(shape)


def _past_the_end(t, n):
    """element ``n`` of a flat operand view of ``n`` elements: the first element of the guard behind it"""
    return t.as_strided((n + 1,), (1,))[n:]


# ================================================================================================ the torch stand-in for the library
class TorchKernels:
    """the entry points the drivers call, in fp32 torch on the views of a CPU arena; ``mut`` = one wrong term or out-of-range access"""
    dev = "cpu"

    def __init__(self, mut=None, cus=CUS):
        self.mut, self.cus, self.views = mut, cus, {}

    def _write_rows(self, dst, rows, busy):
        """rows of blocks that walked no item: zeros, or left alone by the wrong kernel"""
        if self.mut == "idle_block_leaves_its_row_unwritten":
            n = min(busy, rows.shape[0])
            dst[:n] = rows[:n]
        else:
            dst[:] = rows

    # ---- lift
    def _lift_in(self, x, grids, dims):
        B, T, H, W, Cin = dims[:5]
        g3 = (grids[0][:T], grids[1][:H], grids[2][:W])
        if self.mut == "grid_t_and_grid_h_swapped":
            g3 = (g3[1][torch.arange(T) % H], g3[0][torch.arange(H) % T], g3[2])
        return (x[:B * T * H * W * Cin] if Cin else x), g3

    def lift_pad_fwd(self, x, grids, w0, b0, out, dims):
        B, T, H, W, Cin, C, pad = dims
        ncell = B * (T + pad) * (H + pad) * (W + pad)
        xv, g3 = self._lift_in(x, grids, dims)
        ref = K.lift_fwd(xv, g3, _v(w0, C, Cin + 3), b0[:C], dims, F32)
        ov = _v(out, ncell, C)
        if self.mut == "margin_left_unwritten":
            ov.view(B, T + pad, H + pad, W + pad, C)[:, :T, :H, :W] = ref.view(B, T + pad, H + pad, W + pad, C)[:, :T, :H, :W]
        else:
            ov[:] = ref
        if self.mut == "x_read_although_there_are_no_inputs" and Cin == 0:
            ov[0, 0] += 0.0 * x[0]
        if self.mut == "row_written_one_cell_too_far":
            _past_the_end(out, ncell * C)[:] = 0.0

    def lift_bwd_rows(self):
        return K.lift_bwd_rows(self.cus)

    def lift_bwd(self, g, x, grids, part, dims):
        B, T, H, W, Cin, C, pad = dims
        F_ = Cin + 3
        xv, g3 = self._lift_in(x, grids, dims)
        gv = _v(g, B * (T + pad) * (H + pad) * (W + pad), C)
        if self.mut == "margin_of_the_gradient_is_read":
            gv = gv.clone().view(B, T + pad, H + pad, W + pad, C)
            gv[:, :T, :H, :W] += 0.0 * gv.roll(1, 3)[:, :T, :H, :W]
        rows = self.lift_bwd_rows()
        self._write_rows(_v(part, rows, C * F_ + C), K.lift_bwd(gv, xv, g3, dims, rows, F32), B * T * H)

    def lift_feat(self, x, grids, out, dims, FW):
        B, T, H, W, Cin, C, pad = dims
        fd = (B, T, H, W, Cin, pad, FW)
        xv, g3 = self._lift_in(x, grids, dims)
        n = B * (T + pad) * (H + pad) * (W + pad) * FW
        out[:n] = K.lift_feat(xv, g3, fd, F32, ones=0.0 if self.mut == "ones_field_missing" else 1.0).reshape(-1)
        if self.mut == "row_written_one_cell_too_far":
            _past_the_end(out, n)[:] = 0.0

    # ---- layer-0 feature algebra
    def feat_mix(self, Phi, w0, b0, Xh, B, M2, NB, Cin, C):
        P = _v(Phi, M2, NB)
        if self.mut == "padding_column_of_phi_is_read":
            P = P.clone()
            P[:, B * Cin + 3] += 0.0 * P[:, B * Cin + 4]
        bias = torch.zeros(C) if self.mut == "bias_field_dropped" else b0[:C]
        _v(Xh, B, M2, C)[:] = K.feat_mix(P, _v(w0, C, Cin + 3), bias, B, Cin, F32)

    def feat_mix_wgrad_rows(self):
        return K.feat_mix_wgrad_rows(self.cus)

    def feat_mix_wgrad(self, G, Phi, part, B, M2, NB, Cin, C):
        P = _v(Phi, M2, NB)
        if self.mut == "fields_of_sample_0_for_every_sample":
            P = P.clone()
            P[:, :B * Cin] = P[:, :Cin].repeat(1, B)
        rows = self.feat_mix_wgrad_rows()
        self._write_rows(_v(part, rows, C, Cin + 4), K.feat_mix_wgrad(_v(G, B * M2, C), P, B, Cin, C, rows, F32), K.ceil_div(B * M2, 256 // C))

    def small_gemm(self, A, Bm, out, M, N, K_, a_rs, a_cs, b_rs, b_cs, ldo, accumulate):
        ov = out.as_strided((M, N), (ldo, 1))
        old = ov.clone() if accumulate and self.mut != "accumulate_ignored" else None
        if self.mut == "a_read_transposed":
            a_rs, a_cs = a_cs, a_rs
        n = lambda rows, cols, rs, cs: (rows - 1) * abs(rs) + (cols - 1) * abs(cs) + 1
        ov[:] = K.small_gemm(A.as_strided((n(M, K_, a_rs, a_cs),), (1,)), Bm[:n(K_, N, b_rs, b_cs)], old, (M, N, K_, a_rs, a_cs, b_rs, b_cs), F32)
        if self.mut == "stride_gap_written" and ldo > N:
            out[N] = 0.0

    # ---- cell BatchNorm
    def bn_finalize(self, sums, count, eps, momentum, mean, invstd, rmean, rvar, C):
        assert (eps, momentum) == (K.BN_EPS, K.BN_MOMENTUM)
        sv = sums[:2 * C]
        if self.mut == "variance_not_clamped":                    # a negative variance taken as it is: add it back after the clamp
            m = sv[:C] / count
            neg = (sv[C:] / count - m * m).clamp_max(0.0)
            r = K.bn_finalize(sv, count, None if rmean is None else rmean[:C], None if rvar is None else rvar[:C], F32)
            r["invstd"] = (1.0 / torch.sqrt((sv[C:] / count - m * m).clamp_min(0.0) + neg + K.f32(eps))).float()
        else:
            r = K.bn_finalize(sv, count, None if rmean is None else rmean[:C], None if rvar is None else rvar[:C], F32,
                              normalise_unbiased=self.mut == "unbiased_variance_normalises")
        n = 64 if self.mut == "second_block_not_launched" else C
        mean[:min(n, C)], invstd[:min(n, C)] = r["mean"][:n], r["invstd"][:n]
        if rmean is not None:
            rmean[:C], rvar[:C] = r["rmean"], r["rvar"]

    def bn_eval_prep(self, rvar, eps, invstd, C):
        invstd[:C] = 1.0 / torch.sqrt(rvar[:C] + K.f32(0.0 if self.mut == "eps_dropped" else eps))

    def _stat(self, stat, C):
        st = tuple(t[:C] for t in stat)
        return st[:3] + (torch.zeros(C),) if self.mut == "beta_dropped" else st

    def bn_act_fwd(self, s, stat, y, ncell, C, gelu):
        _v(y, ncell, C)[:] = K.bn_act(_v(s, ncell, C), self._stat(stat, C), gelu, F32)

    def bn_bwd_rows(self):
        return K.bn_bwd_rows(self.cus)

    def bn_bwd_reduce(self, s, gy, stat, part, ncell, C, gelu):
        rows = self.bn_bwd_rows()
        r = K.bn_bwd_reduce(_v(s, ncell, C), _v(gy, ncell, C), self._stat(stat, C), gelu, rows, F32,
                            sums_of_s=self.mut == "sum_gz_s_instead_of_sum_gz_shat")
        self._write_rows(_v(part, rows, 2 * C), r, K.ceil_div(ncell, 1024 // C))

    def bn_bwd_apply(self, s, gy, stat, sums, count, gs, ncell, C, gelu):
        _v(gs, ncell, C)[:] = K.bn_bwd_apply(_v(s, ncell, C), _v(gy, ncell, C), self._stat(stat, C), sums[:2 * C], count, gelu, F32,
                                             no_shat_term=self.mut == "shat_term_dropped")

    # ---- loss, Adam
    def mse_rows(self):
        return K.mse_rows(self.cus)

    def mse(self, pred, tgt, elem, gout, part, n, gscale):
        rows = self.mse_rows()
        r = K.mse(pred[:n], tgt[:n], gscale, rows, F32, factor=1.0 if self.mut == "gout_without_the_factor_2" else 2.0)
        m = min(n, rows * 256) if self.mut == "second_trip_not_taken" else n
        if m < n:
            r["part"] = K.mse(pred[:m], tgt[:m], gscale, rows, F32)["part"]
        if elem is not None:
            elem[:m] = r["elem"][:m]
        if gout is not None:
            gout[:m] = r["gout"][:m]
        self._write_rows(part[:rows], r["part"], K.ceil_div(n, 256))

    def adam_step(self, p, g, m, v, n, lr, b1, b2, eps, step, gscale):
        assert (b1, b2, eps, gscale) == (K.ADAM["beta1"], K.ADAM["beta2"], K.ADAM["eps"], K.ADAM["gscale"])
        k = n - n % 4 if self.mut == "tail_not_updated" else n
        p[:k], m[:k], v[:k] = K.adam_update(p[:k], g[:k], m[:k], v[:k], step, F32, lr=lr, eps_inside_sqrt=self.mut == "eps_inside_the_root")

    def adam_step_ranges(self, p, g, m, v, tab, nr, total, lr, b1, b2, eps, step, gscale):
        t = tab[:2 * nr].view(nr, 2).tolist()
        for k, (first, pre) in enumerate(t):
            n = 4 * ((t[k + 1][1] if k + 1 < nr else total // 4) - pre)
            if self.mut == "one_group_past_the_last_range" and k == nr - 1:
                n += 4
            sl = slice(first, first + n)
            if n > p.numel() - first:                             # (past the operand: into its guard)
                p, g, m, v = (t_.as_strided((first + n,), (1,)) for t_ in (p, g, m, v))
            p[sl], m[sl], v[sl] = K.adam_update(p[sl], g[sl], m[sl], v[sl], step, F32, lr=lr)

    # ---- affines, movers
    def rollout_affine(self, pred, para, out, ncell, Cp, Cx, mean_t, std_t, mean_i, std_i):
        st_t = None if mean_t is None else (mean_t[:Cp], std_t[:Cp])
        st_i = None if mean_i is None else (mean_i[:Cp + Cx], std_i[:Cp + Cx])
        _v(out, ncell, Cp + Cx)[:] = K.rollout_affine(_v(pred, ncell, Cp), _v(para, ncell, Cx) if Cx else None, st_t, st_i, F32,
                                                      divide_by_std_t=self.mut == "target_std_divides")

    def channel_affine(self, x, out, n, C, mean, std, inverse):
        out[:n] = K.channel_affine(x[:n], C, mean[:C], std[:C], inverse != (self.mut == "directions_swapped"), F32)

    def mul(self, a, b, out, n):
        out[:n] = a[:n] * b[:n] * (1.0 + 2.0 ** -23 if self.mut == "one_ulp_off" else 1.0)

    def pair_pack(self, num, real, para, inp, tgt, B, ntok, Cl, n_para, mean_in, mean_tgt, std_in, std_tgt):
        st = (mean_in[:Cl + n_para], mean_tgt[:1], std_in[:Cl + n_para], std_tgt[:1])
        r = K.pair_pack(_v(num, B, ntok, Cl), _v(real, B, ntok), _v(para, B, n_para) if n_para else None, st, F32,
                        para_offset=1 if self.mut == "parameter_channels_shifted" else 0)
        _v(inp, B, ntok, Cl + n_para)[:], _v(tgt, B, ntok, 1)[:] = r["inp"], r["tgt"]

    def window_pack(self, planar, cl, flags, inp, tgt, B, horizon, in_step, Hf, Wf, sub_s, n_para, Cp, Cl, mean_in, mean_tgt, std_in,
                    std_tgt, rows_subsampled):
        spec = ("", B, horizon, in_step, Hf, Wf, sub_s, rows_subsampled, n_para, Cp, Cl, [], False)
        Ci, Ct = Cp + Cl + n_para, Cp + Cl
        fl = _v(flags, B, 4 + max(n_para, 1))
        if self.mut == "cleared_flag_ignored":
            fl = fl.clone()
            fl[:, :4] = 1.0
        if self.mut == "host_subsampled_rows_strided_again":
            spec = spec[:7] + (False,) + spec[8:]
        r = K.window_pack(_v(planar, B, Cp, horizon, Hf, Wf), _v(cl, B, horizon, Hf, Wf, Cl) if Cl else None, fl,
                          (mean_in[:Ci], mean_tgt[:Ct], std_in[:Ci], std_tgt[:Ct]), spec, F32)
        inp[:r["inp"].numel()], tgt[:r["tgt"].numel()] = r["inp"].reshape(-1), r["tgt"].reshape(-1)

    # ---- reducers
    def _reduce(self, part, rows, L, stride):
        if self.mut == "last_row_skipped":
            rows -= 1
        if self.mut == "stride_gaps_are_summed" and stride > L:
            return part.as_strided((rows, L), (stride, 1)) + 0.0 * part.as_strided((rows, L), (stride, 1), 1)
        return part.as_strided((rows, L), (stride, 1))

    def reduce_partials(self, part, rows, L, stride, outf, outd, scale, accumulate):
        acc = accumulate and self.mut != "accumulate_ignored"
        r = K.reduce_rows(self._reduce(part, rows, L, stride), L, 0, scale, outf[:L].clone() if acc and outf is not None else None,
                          outd[:L].clone() if acc and outd is not None else None, F32)
        if outf is not None:
            outf[:L] = r["f32"]
        if outd is not None:
            outd[:L] = r["f64"]

    def reduce_partials_batched(self, part, nbatch, rows, L, stride, batch_stride, out):
        for b in range(nbatch):
            out[b * L:(b + 1) * L] = self._reduce(part[b * batch_stride:], rows, L, stride).double().sum(0).float()

    def reduce_grouped_cols(self):
        return K.GROUPED_COLS

    def addr(self, operand):
        self.views[1000 + len(self.views)] = operand.op
        return 999 + len(self.views)

    def reduce_partials_grouped(self, tab, n, total_chunks):
        for pp, op, rows, L, stride, chunk0 in tab[:6 * n].view(n, 6).tolist():
            self.views[op][:L] = self._reduce(self.views[pp], rows, L, stride).double().sum(0).float()

    # ---- spectrum bins
    def spectrum_bin(self, Y, out, R, NB):
        _v(out, R, NB)[:] = K.spectrum_bin(_v(Y, R, R, R, 2, NB), R, NB, F32, rounded=self.mut == "rounds_instead_of_floor")


GOOD = TorchKernels()
CAUGHT = "kernel error|never written|were written|was written|NaN|differ in their bits|without a work item"


def rejected(driver, mut, *args, match=CAUGHT):
    """the driver fails on the mutated stand-in: an assertion of Arena.check(), of a bit comparison or of the verdict"""
    with pytest.raises(AssertionError, match=match):
        driver(TorchKernels(mut), *args)


def _ids(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


# ================================================================================================ restatements against independent statements
def test_lift_against_autograd():
    for dims in [K.LIFT_CASES[0], K.LIFT_CASES[3], K.LIFT_CASES[7]]:
        c = K.lift_case(*dims)
        B, T, H, W, Cin, C, pad = dims
        w0, b0 = c.w0.double().requires_grad_(True), c.b0.double().requires_grad_(True)
        gt, gh, gw = (t.double() for t in c.grids)
        grid = torch.stack(torch.meshgrid(gt, gh, gw, indexing="ij"), -1).expand(B, T, H, W, 3)
        feats = torch.cat((c.x.double().view(B, T, H, W, Cin), grid), -1) if Cin else grid
        inner = F.linear(feats, w0, b0)
        want = F.pad(inner.permute(0, 4, 1, 2, 3), (0, pad, 0, pad, 0, pad)).permute(0, 2, 3, 4, 1)        # fno.py: permute, F.pad
        r = c.refs()[0]
        assert rel_l2(r["fwd"].view_as(want), want.detach()) < TOL
        inner.backward(c.g.double()[:, :T, :H, :W])
        tot = K.total(r["bwd"])
        assert rel_l2(tot[:C * (Cin + 3)].view(C, Cin + 3), w0.grad) < TOL and rel_l2(tot[C * (Cin + 3):], b0.grad) < TOL
        # lift_feat: the same fields, a one and zeros per cell; the lifted tensor is [fc0.weight | fc0.bias] applied to them
        FW = 8 if Cin + 4 <= 8 else 32
        x = c.x if Cin else torch.zeros(0)
        phi = K.lift_feat(x, c.grids, (B, T, H, W, Cin, pad, FW), F64)
        w0ext = torch.cat((c.w0.double(), c.b0.double()[:, None], torch.zeros(C, FW - Cin - 4, dtype=F64)), 1)
        assert rel_l2(phi @ w0ext.t(), r["fwd"]) < TOL


def test_feat_mix_against_its_definition_and_wgrad_against_autograd():
    c = K.feat_case(64, 3, 3, 10)
    C, Cin, B, M2 = c.dims
    w0, b0 = c.w0.double().requires_grad_(True), c.b0.double().requires_grad_(True)
    Phi = c.Phi.double()
    X = torch.zeros(B, M2, C, dtype=F64)
    for b in range(B):                                            # csrc/rpb_feat.hip's formula, term by term
        for j in range(Cin):
            X[b] += Phi[:, b * Cin + j, None] * w0[:, j]
        for j in range(3):
            X[b] += Phi[:, B * Cin + j, None] * w0[:, Cin + j]
        X[b] += Phi[:, B * Cin + 3, None] * b0
    r = c.refs()[0]
    assert rel_l2(r["mix"], X.detach()) < TOL
    (X * c.G.double().view(B, M2, C)).sum().backward()
    tot = K.total(r["wgrad"])
    assert rel_l2(tot[:, :Cin + 3], w0.grad) < TOL and rel_l2(tot[:, Cin + 3], b0.grad) < TOL


def test_small_gemm_and_reducers_against_loops():
    c = K.small_gemm_case(*K.SMALL_GEMM_SHAPES[3], 3, True)
    M, N, K_, a_rs, a_cs, b_rs, b_cs = c.shape
    want = c.old.double().clone()
    for m in range(M):
        for n in range(N):
            want[m, n] += sum(float(c.A[m * a_rs + k * a_cs]) * float(c.Bm[k * b_rs + n * b_cs]) for k in range(K_))
    assert rel_l2(c.refs()[0]["out"], want) < TOL
    c = K.reduce_case(37, 20, 50, 11, 0.5, True)
    want = [float(c.oldd[j]) + 0.5 * math.fsum(float(c.part[r, 11 + j]) for r in range(37)) for j in range(20)]
    assert rel_l2(c.refs()[0]["f64"], torch.tensor(want, dtype=F64)) < TOL
    assert rel_l2(c.refs()[0]["f32"], torch.tensor(want, dtype=F64) - c.oldd + c.oldf.double()) < TOL


def _batch_stats(s):
    mean = s.mean(0)
    return mean, 1 / torch.sqrt(((s - mean) ** 2).mean(0) + K.f32(K.BN_EPS))


def test_batchnorm_against_autograd_and_torch_batch_norm():
    for gelu in (True, False):
        c = K.bn_case(64, 257, gelu)
        C, ncell = c.dims
        s = c.s.double().requires_grad_(True)
        gamma, beta = c.stat[2].double().requires_grad_(True), c.stat[3].double().requires_grad_(True)
        rm, rv = torch.zeros(C, dtype=F64), torch.ones(C, dtype=F64)
        z = F.batch_norm(s, rm, rv, gamma, beta, training=True, momentum=K.f32(K.BN_MOMENTUM), eps=K.f32(K.BN_EPS))
        y = F.gelu(z) if gelu else z
        y.backward(c.gy.double())
        mean, invstd = _batch_stats(s.detach())
        stat = (mean, invstd, gamma.detach(), beta.detach())
        assert rel_l2(K.bn_act(s.detach(), stat, gelu, F64), y.detach()) < TOL
        rows = K.total(K.bn_bwd_reduce(s.detach(), c.gy, stat, gelu, c.rows, F64))
        assert rel_l2(rows[:C], beta.grad) < TOL and rel_l2(rows[C:], gamma.grad) < TOL          # d beta = sum gz, d gamma = sum gz shat
        assert rel_l2(K.bn_bwd_apply(s.detach(), c.gy, stat, rows, ncell, gelu, F64), s.grad) < 1e-10
        # bn_finalize from the sums of the same tensor: batch statistics, and nn.BatchNorm's update of the running ones
        sums = torch.cat((s.detach().sum(0), (s.detach() ** 2).sum(0)))
        r = K.bn_finalize(sums, float(ncell), torch.zeros(C), torch.ones(C), F64)
        assert rel_l2(r["mean"], mean) < TOL and rel_l2(r["invstd"], invstd) < 1e-10
        assert rel_l2(r["rmean"], rm) < TOL and rel_l2(r["rvar"], rv) < 1e-10
    zz = torch.linspace(-6, 6, 1001, dtype=F64, requires_grad=True)
    F.gelu(zz).sum().backward()
    assert rel_l2(K.gelu_grad(zz.detach()), zz.grad) < TOL
    # count = 1: torch refuses a one-sample batch; the branch keeps the variance (0) as it is instead of dividing by count - 1 = 0
    r = K.bn_finalize(torch.tensor([3.0, 9.0], dtype=F64), 1.0, torch.zeros(1), torch.ones(1), F64)
    assert float(r["mean"]) == 3.0 and abs(float(r["invstd"]) - K.f32(K.BN_EPS) ** -0.5) < 1e-9 and abs(float(r["rvar"]) - (1 - K.f32(0.1))) < TOL
    # the constant channel: without the clamp the variance would be negative
    c = K.bn_finalize_case(64, 5000, "constant channel")
    assert abs(float(c.refs()[0]["invstd"][3]) - K.f32(K.BN_EPS) ** -0.5) < 1e-9
    c = K.bn_eval_prep_case(64)
    assert rel_l2(c.refs()[0]["invstd"], (c.rvar.double() + K.f32(K.BN_EPS)).rsqrt()) < TOL


def test_mse_against_autograd():
    c = K.mse_case(255)
    pred = c.pred.double().requires_grad_(True)
    loss = F.mse_loss(pred, c.tgt.double())
    loss.backward()
    r = c.refs()[0]
    assert rel_l2(r["gout"], pred.grad) < 1e-7                      # gscale = 1 / n travels as an fp32 number
    assert rel_l2(r["gout"] / K.f32(1 / 255) / 255, pred.grad) < TOL
    assert abs(float(K.total(r["part"])) / 255 - float(loss.detach())) < TOL and rel_l2(r["elem"], (pred.detach() - c.tgt.double()) ** 2) < TOL


def _torch_adam(p, g, m, v, step, lr):
    w = p.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([w], lr=K.f32(lr), betas=(K.f32(K.ADAM["beta1"]), K.f32(K.ADAM["beta2"])), eps=K.f32(K.ADAM["eps"]))
    opt.state[w] = dict(step=torch.tensor(float(step - 1)), exp_avg=m.double().clone(), exp_avg_sq=v.double().clone())
    w.grad = g.double() * K.f32(K.ADAM["gscale"])
    opt.step()
    return w.detach(), opt.state[w]["exp_avg"], opt.state[w]["exp_avg_sq"]


@pytest.mark.parametrize("step", K.ADAM_STEPS)
@pytest.mark.parametrize("regime", K.ADAM_REGIMES)
def test_adam_against_torch_optim_adam(step, regime):
    """from a preloaded state, with the hyperparameters the ABI receives (fp32 numbers)"""
    c = K.adam_case(1003, step, regime)
    w, m, v = _torch_adam(c.p, c.g, c.m, c.v, step, K.ADAM["lr"])
    r = c.refs()[0]
    assert rel_l2(r["update"], w - c.p.double()) < 1e-10 and rel_l2(r["m"], m) < TOL and rel_l2(r["v"], v) < TOL
    if regime == "tiny" and step >= 1000:                          # eps is about 10 % of the denominator
        share = K.f32(K.ADAM["eps"]) / (torch.sqrt(r["v"]) / math.sqrt(1 - K.f32(K.ADAM["beta2"]) ** step) + K.f32(K.ADAM["eps"]))
        assert 0.07 < float(share.median()) < 0.14
    assert float(c.p.abs().max()) <= K.ADAM["lr"]


def test_adam_chain_against_torch_optim_adam():
    c = K.adam_chain_case()
    w, m, v = c.p, torch.zeros(c.n), torch.zeros(c.n)
    for k, lr in enumerate(K.ADAM_CHAIN_LR):
        w, m, v = _torch_adam(w, c.grads[k], m, v, k + 1, lr)
    r = c.refs()[0]
    assert rel_l2(r["update"], w - c.p.double()) < 1e-10 and rel_l2(r["m"], m) < TOL and rel_l2(r["v"], v) < TOL


def test_owned_table_is_the_data_parallel_one():
    from realpdebench_amd.dp import DataParallel

    class Plan:
        def shard_plan(self):
            return K.adam_range_tables()["adjacent ranges"][1], None
    tab, nr, tot = DataParallel.owned_table(Plan(), "cpu")
    mine = K.owned_table(K.adam_range_tables()["adjacent ranges"][1])
    assert torch.equal(tab, mine[0]) and (nr, tot) == mine[1:]


def test_affines_and_packers_against_loops():
    c = K.rollout_case(999, 3, 2, True, True)
    r = c.refs()[0]["out"]
    for cell in (0, 500, 998):                                    # eval.py: denormalise the prediction, append the controls, normalise
        t = [float(c.pred[cell, k]) * float(c.st_t[1][k]) + float(c.st_t[0][k]) for k in range(3)] + [float(v) for v in c.para[cell]]
        want = [(t[k] - float(c.st_i[0][k])) / float(c.st_i[1][k]) for k in range(5)]
        assert rel_l2(r[cell], torch.tensor(want, dtype=F64)) < TOL
    c = K.channel_affine_case(350 * 3, 3, False)
    back = K.channel_affine(c.refs()[0]["out"], 3, c.mean, c.std, True, F64)
    assert rel_l2(back, c.x.double()) < TOL
    c = K.pair_pack_case(2, 37, 15, 2)
    r = c.refs()[0]
    for b, tok in ((0, 0), (1, 36)):
        row = [float(v) for v in c.num[b, tok]] + [float(v) for v in c.para[b]]
        want = [(row[k] - float(c.st[0][k])) / float(c.st[2][k]) for k in range(17)]
        assert rel_l2(r["inp"][b, tok], torch.tensor(want, dtype=F64)) < TOL
        assert abs(float(r["tgt"][b, tok, 0]) - (float(c.real[b, tok]) - float(c.st[1][0])) / float(c.st[3][0])) < TOL
    for spec in K.WINDOW_PACK_CASES:                              # numpy's [::sub_s, ::sub_s], channel by channel
        c = K.window_pack_case(spec)
        name, B, horizon, in_step, Hf, Wf, sub_s, rows_sub, n_para, Cp, Cl, cleared, unit = spec
        r = c.refs()[0]
        sub_h = 1 if rows_sub else sub_s
        H, W = len(range(0, Hf, sub_h)), len(range(0, Wf, sub_s))
        assert r["inp"].shape == (B, in_step, H, W, Cp + Cl + n_para) and r["tgt"].shape == (B, horizon - in_step, H, W, Cp + Cl)
        assert not torch.isnan(r["inp"]).any() and not torch.isnan(r["tgt"]).any()
        for b in range(B):
            for t in range(horizon):
                for h in (0, H - 1):
                    for w in (0, W - 1):
                        row = [float(c.planar[b, k, t, h * sub_h, w * sub_s]) if c.flags[b, k] != 0 else 0.0 for k in range(Cp)]
                        row += [float(c.cl[b, t, h * sub_h, w * sub_s, k]) if c.flags[b, 3] != 0 else 0.0 for k in range(Cl)]
                        if t < in_step:
                            row += [float(c.flags[b, 4 + k]) for k in range(n_para)]
                        mean, std = (c.st[0], c.st[2]) if t < in_step else (c.st[1], c.st[3])
                        want = torch.tensor([(v - float(mean[k])) / float(std[k]) for k, v in enumerate(row)], dtype=F64)
                        got = r["inp"][b, t, h, w] if t < in_step else r["tgt"][b, t - in_step, h, w]
                        assert float((got - want).abs().max()) < 1e-12


def test_radial_bins_against_the_triple_loop():
    """realpdebench/utils/metrics.py walks the corner in a triple loop and adds |F|^2 to bin floor(sqrt(i^2 + j^2 + k^2)) if that is < R"""
    for R, NB in ((5, 3), (2, 3), (1, 64)):
        c = K.spectrum_case(R, NB)
        Y = c.Y.double()
        want = torch.zeros(R, NB, dtype=F64)
        for i in range(R):
            for j in range(R):
                for k in range(R):
                    rad = math.isqrt(i * i + j * j + k * k)
                    if rad < R:
                        want[rad] += Y[i, j, k, 0] ** 2 + Y[i, j, k, 1] ** 2
        assert rel_l2(c.refs()[0]["out"], want) < TOL
    # the kernel bins with floorf(sqrtf((float)n)): exact for every n its R <= 64 limit can produce (correctly rounded sqrt)
    n = torch.arange(3 * (K.SPECTRUM_RMAX - 1) ** 2 + 1)
    assert torch.equal(torch.floor(torch.sqrt(n.to(F32))).long(), torch.tensor([math.isqrt(v) for v in n.tolist()]))


# ================================================================================================ the shapes reach what they claim
def test_cases_reach_the_paths_they_claim():
    """at the MI355X's 256 compute units"""
    assert [K.lift_instantiation(s[4], True) for s in K.LIFT_CASES] == K.LIFT_KERNELS
    assert [K.lift_instantiation(s[4], False) for s in K.LIFT_CASES] == K.LIFT_KERNELS[:7] + ["generic"]
    assert K.LIFT_CASES[4][3] * K.LIFT_CASES[4][4] == 2064 > 8 * 256 and K.LIFT_CASES[6][4] + 3 == 24
    dims = K.lift_fwd_trip_dims()
    B, T, H, W, Cin, C, pad = dims
    nrows = B * (T + pad) * (H + pad)
    print(f"[plumbing-cases] lift forward second trip: {dims}, {nrows} rows, hand-offs {sorted(K.lift_fwd_handoffs(dims))}")
    assert 8 * CUS + 3 <= nrows <= 8 * CUS + 64 and (W, C) == (3, 32) and {"live>live", "live>pad", "pad>live"} <= K.lift_fwd_handoffs(dims)
    B, T, H, W, Cin, C, pad = K.lift_bwd_trip_dims()
    assert B * T * H == 4 * CUS + 3 == 1027 and (W, C) == (3, 32) and K.trips(B * T * H, K.lift_bwd_rows()).count(2) == 3
    B, T, H, W, Cin, pad, FW = K.lift_feat_trip_dims()
    assert B * (T + pad) * (H + pad) == 32 * CUS + 5 and W + pad == 3 and K.trips(32 * CUS + 5, 32 * CUS).count(2) == 5
    assert [(s[3] + s[5]) for s in K.LIFT_FEAT_CASES[:2]] == [5, 40] and 40 * 2 > 64
    C, Cin, B, M2 = K.feat_mix_trip_case()
    assert B * M2 * C // 4 >= 8 * CUS * 256 + 5 and K.pw_grid(B * M2 * C // 4) == 8 * CUS and B * M2 * C * 4 < 20e6
    for C, Cin, B, M2 in K.feat_wgrad_trip_cases():
        assert B * M2 == 2 * CUS * (256 // C) + 3          # three pairs past one trip: 1, 2 or 3 blocks walk a second group of 256 / C
        assert K.trips(K.ceil_div(B * M2, 256 // C), K.feat_mix_wgrad_rows()).count(2) == K.ceil_div(3, 256 // C)
    assert max(s[1] for s in K.FEAT_WGRAD_CASES) + 4 == 24            # FM_FMAX
    for C in K.BN_C:
        n = K.bn_ncells(C)[-1]
        assert n * C // 4 == 8 * CUS * 256 + 5 * C // 4 and K.pw_grid(n * C // 4) == 8 * CUS and n * C * 4 < 9e6
        assert K.trips(K.ceil_div(n, 1024 // C), K.bn_bwd_rows()).count(2) >= 1
    n = K.mse_sizes()[-1]
    assert K.trips(K.ceil_div(n, 256), K.mse_rows()).count(3) == 2 and n == 524545
    n = K.adam_sizes()[-1]
    assert n // 4 > 8 * CUS * 256 and n % 4 == 3 and K.pw_grid((n + 3) // 4) == 8 * CUS
    N, pieces = K.adam_range_tables()["past a grid trip"]
    assert sum(c for _, c in pieces) // 4 == 8 * CUS * 256 + 9 and len(K.adam_range_tables()["nr = 257"][1]) == 257
    ncell, Cp, Cx = K.rollout_shapes()[-1]
    assert ncell * (Cp + Cx) > 8 * CUS * 256 and K.channel_affine_cases()[-1][0] > 8 * CUS * 256
    assert sum(1 for s in K.SMALL_GEMM_SHAPES if s[1] * s[2] < 256) >= 1 and sum(1 for s in K.SMALL_GEMM_SHAPES if s[1] * s[2] > 256) >= 1


# ================================================================================================ the stand-in passes, its mutations fail
LIFT_ALL = K.LIFT_CASES + [K.lift_fwd_trip_dims(), K.lift_bwd_trip_dims()]


@pytest.mark.parametrize("dims", LIFT_ALL, ids=_ids)
def test_standin_lift(dims):
    c = K.lift_case(*dims)
    K.run_lift_fwd(GOOD, c)
    K.run_lift_bwd(GOOD, c)
    B, T, H, W, Cin, C, pad = dims
    if T > 1 or H > 1:
        rejected(K.run_lift_fwd, "grid_t_and_grid_h_swapped", c)
        rejected(K.run_lift_bwd, "grid_t_and_grid_h_swapped", c)
    rejected(K.run_lift_fwd, "margin_left_unwritten", c)
    rejected(K.run_lift_fwd, "row_written_one_cell_too_far", c)
    rejected(K.run_lift_bwd, "margin_of_the_gradient_is_read", c)
    if B * T * H < c.rows:
        rejected(K.run_lift_bwd, "idle_block_leaves_its_row_unwritten", c)
    if Cin == 0:
        rejected(K.run_lift_fwd, "x_read_although_there_are_no_inputs", c)


@pytest.mark.parametrize("dims", K.LIFT_FEAT_CASES + [K.lift_feat_trip_dims()], ids=_ids)
def test_standin_lift_feat(dims):
    c = K.lift_feat_case(*dims)
    K.run_lift_feat(GOOD, c)
    rejected(K.run_lift_feat, "ones_field_missing", c)
    rejected(K.run_lift_feat, "row_written_one_cell_too_far", c)


@pytest.mark.parametrize("shape", K.FEAT_MIX_CASES + [K.feat_mix_trip_case()], ids=_ids)
def test_standin_feat_mix(shape):
    c = K.feat_case(*shape)
    K.run_feat_mix(GOOD, c)
    rejected(K.run_feat_mix, "padding_column_of_phi_is_read", c)
    rejected(K.run_feat_mix, "bias_field_dropped", c)


@pytest.mark.parametrize("shape", K.FEAT_WGRAD_CASES + K.feat_wgrad_trip_cases(), ids=_ids)
def test_standin_feat_mix_wgrad(shape):
    c = K.feat_case(*shape)
    K.run_feat_mix_wgrad(GOOD, c)
    C, Cin, B, M2 = shape
    if K.ceil_div(B * M2, 256 // C) < c.rows:
        rejected(K.run_feat_mix_wgrad, "idle_block_leaves_its_row_unwritten", c)
    if B > 1:
        rejected(K.run_feat_mix_wgrad, "fields_of_sample_0_for_every_sample", c)


@pytest.mark.parametrize("shape", K.SMALL_GEMM_CASES, ids=_ids)
def test_standin_small_gemm(shape):
    c = K.small_gemm_case(*shape)
    K.run_small_gemm(GOOD, c)
    if shape[-1]:
        rejected(K.run_small_gemm, "accumulate_ignored", c)
    if shape[-2]:
        rejected(K.run_small_gemm, "stride_gap_written", c)
    if shape[4] != shape[5] and shape[1] > 1:
        rejected(K.run_small_gemm, "a_read_transposed", c)


@pytest.mark.parametrize("gelu", [True, False])
@pytest.mark.parametrize("C", K.BN_C)
def test_standin_batchnorm(C, gelu):
    for ncell in K.bn_ncells(C):
        c = K.bn_case(C, ncell, gelu)
        K.run_bn_act_fwd(GOOD, c)
        K.run_bn_bwd_reduce(GOOD, c)
        K.run_bn_bwd_apply(GOOD, c)
        rejected(K.run_bn_act_fwd, "beta_dropped", c)
        rejected(K.run_bn_bwd_apply, "shat_term_dropped", c)
        rejected(K.run_bn_bwd_reduce, "sum_gz_s_instead_of_sum_gz_shat", c)
        if K.ceil_div(ncell, 1024 // C) < c.rows:
            rejected(K.run_bn_bwd_reduce, "idle_block_leaves_its_row_unwritten", c)


@pytest.mark.parametrize("shape", K.BN_FINALIZE_CASES, ids=_ids)
def test_standin_bn_finalize(shape):
    c = K.bn_finalize_case(*shape)
    K.run_bn_finalize(GOOD, c)
    C, count, variant = shape
    if count > 1:
        rejected(K.run_bn_finalize, "unbiased_variance_normalises", c)
    if C > 64:
        rejected(K.run_bn_finalize, "second_block_not_launched", c)
    if variant == "constant channel":
        rejected(K.run_bn_finalize, "variance_not_clamped", c)
    e = K.bn_eval_prep_case(C)
    K.run_bn_eval_prep(GOOD, e)
    rejected(K.run_bn_eval_prep, "eps_dropped", e)


@pytest.mark.parametrize("n", K.mse_sizes())
def test_standin_mse(n):
    c = K.mse_case(n)
    for with_elem, with_gout in K.MSE_OUTPUTS:
        K.run_mse(GOOD, c, with_elem, with_gout)
    rejected(K.run_mse, "gout_without_the_factor_2", c, True, True)
    if K.ceil_div(n, 256) < c.rows:
        rejected(K.run_mse, "idle_block_leaves_its_row_unwritten", c, False, False)
    if n > c.rows * 256:
        rejected(K.run_mse, "second_trip_not_taken", c, True, True)
        rejected(K.run_mse, "second_trip_not_taken", c, False, False)


@pytest.mark.parametrize("run", K.adam_runs(), ids=_ids)
def test_standin_adam(run):
    n, step, regime = run
    c = K.adam_case(n, step, regime)
    K.run_adam(GOOD, c)
    if n % 4:
        rejected(K.run_adam, "tail_not_updated", c)
    if regime == "tiny" and step >= 1000:                          # where eps is 10 % of the denominator a misplaced eps shows ...
        rejected(K.run_adam, "eps_inside_the_root", c)
    elif regime == "unit":                                        # ... and at |g| ~ 1 it does not: that regime alone would not do
        K.run_adam(TorchKernels("eps_inside_the_root"), c)


def test_standin_adam_chain():
    c = K.adam_chain_case()
    K.run_adam_chain(GOOD, c)
    rejected(K.run_adam_chain, "tail_not_updated", c)


@pytest.mark.parametrize("name", list(K.adam_range_tables()))
def test_standin_adam_ranges(name):
    c = K.adam_ranges_case(name)
    K.run_adam_ranges(GOOD, c)
    rejected(K.run_adam_ranges, "one_group_past_the_last_range", c)


@pytest.mark.parametrize("stats", K.AFFINE_STATS, ids=_ids)
@pytest.mark.parametrize("shape", K.rollout_shapes(), ids=_ids)
def test_standin_rollout_affine(shape, stats):
    c = K.rollout_case(*shape, *stats)
    K.run_rollout_affine(GOOD, c)
    if stats[0]:
        rejected(K.run_rollout_affine, "target_std_divides", c)


@pytest.mark.parametrize("shape", K.channel_affine_cases(), ids=_ids)
def test_standin_channel_affine(shape):
    c = K.channel_affine_case(*shape)
    K.run_channel_affine(GOOD, c)
    rejected(K.run_channel_affine, "directions_swapped", c)


def test_standin_movers():
    for n in K.MUL_SIZES:
        K.run_mul(GOOD, K.mul_case(n))
        rejected(K.run_mul, "one_ulp_off", K.mul_case(n))
    for shape in K.PAIR_PACK_CASES:
        c = K.pair_pack_case(*shape)
        K.run_pair_pack(GOOD, c)
        if shape[3] > 1:
            rejected(K.run_pair_pack, "parameter_channels_shifted", c)
    for spec in K.WINDOW_PACK_CASES:
        c = K.window_pack_case(spec)
        K.run_window_pack(GOOD, c)
        if spec[11]:
            rejected(K.run_window_pack, "cleared_flag_ignored", c)
        if spec[7]:
            rejected(K.run_window_pack, "host_subsampled_rows_strided_again", c, match=CAUGHT + "|shape|size")


def test_standin_reducers():
    for shape in K.REDUCE_CASES:
        c = K.reduce_case(*shape)
        K.run_reduce_partials(GOOD, c)
        rejected(K.run_reduce_partials, "last_row_skipped", c)
        if shape[2] > shape[1]:
            rejected(K.run_reduce_partials, "stride_gaps_are_summed", c)
        if shape[5]:
            rejected(K.run_reduce_partials, "accumulate_ignored", c)
    for shape in K.REDUCE_BATCHED_CASES:
        c = K.reduce_batched_case(*shape)
        K.run_reduce_batched(GOOD, c)
        rejected(K.run_reduce_batched, "last_row_skipped", c)
        if shape[3] > shape[2]:
            rejected(K.run_reduce_batched, "stride_gaps_are_summed", c)
    c = K.reduce_grouped_case()
    K.run_reduce_grouped(TorchKernels(), c)
    rejected(K.run_reduce_grouped, "last_row_skipped", c)
    rejected(K.run_reduce_grouped, "stride_gaps_are_summed", c)


@pytest.mark.parametrize("shape", K.SPECTRUM_CASES, ids=_ids)
def test_standin_spectrum_bin(shape):
    c = K.spectrum_case(*shape)
    K.run_spectrum_bin(GOOD, c)
    if shape[0] > 1:
        rejected(K.run_spectrum_bin, "rounds_instead_of_floor", c)


# ================================================================================================ the arena's assertions on the dtypes used here
def test_arena_assertions_trip_on_fp64_and_int64_arenas():
    """the fp64 outputs of rpb_reduce_partials and the int64 tables sit in arenas of their own dtype"""
    a = guarded.Arena("cpu", dtype=F64)
    o = a.out(5, name="out")
    o.op[:4] = 1.0
    with pytest.raises(AssertionError, match="never written"):
        a.check()
    a = guarded.Arena("cpu", dtype=torch.int64, fill=0)
    t = a.inp(torch.arange(6), "table")
    _past_the_end(t.op, 6)[:] = 7
    with pytest.raises(AssertionError, match="guard after operand 'table'"):
        a.check()
    a = guarded.Arena("cpu", dtype=torch.int64, fill=0)
    t = a.inp(torch.arange(6), "table")
    t.op[2] = 9
    with pytest.raises(AssertionError, match="input operand 'table'"):
        a.check()
