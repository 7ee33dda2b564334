"""Host side (no GPU) of the per-kernel tests of the FNO3d step kernels:
* every restatement of tests/fno_kernel_cases.py, in fp64, against an independent statement of the same mathematics (torch autograd for
  the BatchNorm(+GELU) backward and the backward cell_mix, torch.fft for an axis_gemm stage matrix of realpdebench_amd/dft.py);
* every case of tests/test_gpu_fno_kernels.py is well conditioned: 8 * e32 <= 1e-5 on every output and measure, the bias column of the
  row kernel (measured against sum |gs|) and the sum gz * shat cases (made well conditioned by construction) included;
* the second-trip cases take the second trip at the MI355X's 256 compute units, and the ragged + 3 / + 5 leaves waves without one;
* the drivers would notice: ``TorchKernels`` is a torch stand-in for the library on a CPU ``Arena`` that partitions the work as the
  launchers do.  Unmutated it passes every driver; with ONE wrong term it trips ``Arena.check()`` or the verdict in at least one case --
  the same driver code the GPU test runs."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT, rel_l2

sys.path.insert(0, os.path.join(ROOT, "tests"))
import fno_kernel_cases as K                # noqa: E402

F32, F64 = torch.float32, torch.float64
TOL = 1e-12                                   # fp64 against fp64
CUS = K.MI355X_CUS


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)


def _v(t, *shape):
    n = 1
    for s in shape:
        n *= s
    return t[:n].view(shape)


def _xf(xf, C):
    return None if xf is None else tuple(t[:C] for t in xf[:4]) + (xf[4],)


# ================================================================================================ the torch stand-in for the library
class TorchKernels:
    """the entry points the drivers call, in fp32 torch on the views of a CPU arena; ``mut`` = one wrong term"""
    dev = "cpu"

    def __init__(self, mut=None, cus=CUS):
        self.mut, self.cus = mut, cus

    def _write_rows(self, dst, rows, items):
        """rows of waves that walked no item: zeros, or left alone by the wrong kernel"""
        if self.mut == "idle_wave_leaves_its_row_unwritten":
            n = min(items, rows.shape[0])
            dst[:n] = rows[:n]
        else:
            dst[:] = rows

    # ---- axis_gemm
    def axis_gemm(self, x, out, Mt, G, K_, O, N, in_g, in_k, out_g, out_o, kv, accumulate, xf):
        kv = K_ if kv is None else kv
        xv = x.as_strided((G, K_, N), (in_g, in_k, 1))
        if self.mut == "rows_past_k_valid_are_read":
            kv = K_
        ref = K.axis_gemm(xv, _v(Mt, K_, O), kv, _xf(xf, N), F32)
        ov = out.as_strided((G, O, N), (out_g, out_o, 1))
        items, slots = G * (N // 64), K.axg_slots(G, N, self.cus)
        if self.mut == "items_past_nslots_not_produced" and N % 64 == 0 and items > slots:
            for it in range(slots):                               # item = (g, 64-column strip)
                g, st = divmod(it, N // 64)
                ov[g, :, 64 * st:64 * st + 64] = ref[g, :, 64 * st:64 * st + 64]
            return
        ov[:] = ov + ref if accumulate else ref
        if self.mut == "tail_tile_writes_past_its_line" and out_o > N:
            out.as_strided((G, O, N + 1), (out_g, out_o, 1))[-1, -1, N] = 1.0

    # ---- mode_contract
    def _mode(self, X, W, GY, B, M, C):
        z = torch.zeros(B, 2, M, C)
        Wv = _v(W, M, C, C, 2) if W is not None else torch.zeros(M, C, C, 2)
        if self.mut == "weights_not_conjugated":
            Wv = Wv * torch.tensor([1.0, -1.0])
        if self.mut == "weights_transposed":
            Wv = Wv.transpose(1, 2)
        return K.mode_contract(z if X is None else _v(X, B, 2, M, C), Wv, z if GY is None else _v(GY, B, 2, M, C), F32)

    def mode_contract_fwd(self, X, W, Y, B, M, C):
        ref = self._mode(X, W, None, B, M, C)["Y"]
        if self.mut == "modes_past_the_grid_not_produced":
            _v(Y, B, 2, M, C)[:, :, :K.mode_grid(M, self.cus)] = ref[:, :, :K.mode_grid(M, self.cus)]
        else:
            _v(Y, B, 2, M, C)[:] = ref

    def mode_contract_dgrad(self, GY, W, GX, B, M, C):
        _v(GX, B, 2, M, C)[:] = self._mode(None, W, GY, B, M, C)["GX"]

    def mode_contract_wgrad(self, X, GY, GW, B, M, C, accumulate):
        ref = self._mode(X, None, GY, B, M, C)["GW"]
        gv = _v(GW, M, C, C, 2)
        gv[:] = gv + ref if accumulate else ref

    # ---- cell_mix
    def cell_mix_writes_gz(self, ncell, KC, CO, K2, Wp):
        return KC == CO and KC in (64, 128) and 0 < K2 <= 32 and Wp >= 32 and ncell % Wp == 0

    def _cmx_rows(self, ncell, C, K2, Wp, bwd):
        """(partial rows, cells per work item): lines on the bf16 pipe, 32-cell tiles on the fp32 kernel"""
        if self.cell_mix_writes_gz(ncell, C, C, K2, Wp):
            return K.cmx_rows(ncell // Wp, Wp, C, self.cus), Wp
        return K.cell_fp32_rows(ncell, C, C, K2, Wp, True, bwd, self.cus), 32

    def cell_mix_stat_rows(self, ncell, C, K2, Wp, bwd):
        return self._cmx_rows(ncell, C, K2, Wp, bwd)[0]

    def cell_mix(self, x, Wc, bias, z2, GW, out, part, ncell, C, K2, Wp, transpose_w, xf, bnb, oxf, write_gz):
        lines = ncell // Wp
        rows, item = self._cmx_rows(ncell, C, K2, Wp, bnb is not None and transpose_w)
        xv, Wv, zv, Gv = _v(x, ncell, C), _v(Wc, C, C), _v(z2, lines, K2, C), _v(GW, K2, Wp)
        if self.mut == "partials_by_lines_on_the_tile_kernel":
            item = Wp
        if transpose_w:
            b = None if bnb is None else (_v(bnb[0], ncell, C),) + _xf(bnb[1:], C)
            r = K.cell_mix_bwd(xv, Wv, zv, Gv, b, write_gz, rows, F32, sums_of_s=self.mut == "sum_gz_s_instead_of_sum_gz_shat", item=item)
        else:
            r = K.cell_mix_fwd(xv, Wv, bias[:C], zv, Gv, _xf(xf, C), _xf(oxf, C), rows if part is not None else 0, F32, item)
        ov = _v(out, ncell, C)
        if self.mut == "lines_past_nslots_not_produced":
            ov[:min(lines, rows) * Wp] = r["out"][:min(lines, rows) * Wp]
        else:
            ov[:] = r["out"]
        if self.mut == "one_wrong_cell":
            ov[ncell // 2, 17] += 2e-5 * float(r["out"].abs().max())
        if part is not None:
            self._write_rows(_v(part, rows, 2, C), r["part"], K.ceil_div(ncell, item))

    def cell_mix_gather_rows(self, ncell, KC, CO):
        return K.cell_fp32_rows(ncell, KC, CO, 0, 1, False, True, self.cus)

    def cell_mix_gather(self, gu, Wm, out, part, ncell, KC, CO, dims, bnb):
        B, T, H, W, pad = dims
        rows = self.cell_mix_gather_rows(ncell, KC, CO)
        r = K.cell_mix_gather(_v(gu, B * T * H * W, KC), _v(Wm, KC, CO), _v(bnb[0], ncell, CO), tuple(t[:CO] for t in bnb[1:5]), bnb[5], dims,
                              rows, F32)
        ov = _v(out, ncell, CO).view(B, T + pad, H + pad, W + pad, CO)
        if self.mut == "gather_leaves_the_margin_unwritten":
            ov[:, :T, :H, :W] = r["out"].view(ov.shape)[:, :T, :H, :W]
        else:
            ov[:] = r["out"].view(ov.shape)
        self._write_rows(_v(part, rows, 2, CO), r["part"], K.ceil_div(ncell, 32))

    def cell_mix_feat(self, phi, Wcomp, bias, z2, GW, out, part, ncell, FW, K2, Wp, oxf):
        C, lines = 64, ncell // Wp
        rows = K.cmx_stat_rows(lines, self.cus)
        pv = _v(phi, ncell, FW)
        if self.mut == "feature_fields_shifted_by_one":
            pv = torch.roll(pv, 1, 1)
        r = K.cell_mix_fwd(pv, _v(Wcomp, C, FW), bias[:C], _v(z2, lines, K2, C), _v(GW, K2, Wp), None, _xf(oxf, C), rows if part is not None else 0, F32)
        _v(out, ncell, C)[:] = r["out"]
        if part is not None:
            self._write_rows(_v(part, rows, 2, C), r["part"], lines)

    # ---- cell_mix_wgrad
    def cell_mix_wgrad_slots(self, ncell, Wp):
        return K.cmx_wg_slots(ncell // Wp, self.cus)

    def cell_mix_wgrad(self, gs, Wc, z2, GW, out, sp, wp, ncell, K2, Wp, bnb, write_gz):
        C, lines = 64, ncell // Wp
        slots = K.cmx_wg_slots(lines, self.cus)
        b = (_v(bnb[0], ncell, C),) + _xf(bnb[1:], C)
        r = K.cell_mix_wgrad(_v(gs, ncell, C), _v(Wc, C, C), _v(z2, lines, K2, C), _v(GW, K2, Wp), b, write_gz, slots, F32,
                             transposed=self.mut == "dWc_transposed", sums_of_s=self.mut == "sum_gz_s_instead_of_sum_gz_shat")
        _v(out, ncell, C)[:] = r["out"]
        self._write_rows(_v(sp, slots, 2, C), r["part"], lines)
        self._write_rows(_v(wp, slots, C, C), r["dW"], lines)

    # ---- bn_bwd_row
    def bn_bwd_row_slots(self, G):
        return K.bn_bwd_row_slots(G, self.cus)

    def bn_bwd_row(self, s, gy, x, gs, stat, sums, count, gelu, xf, GW, Y1, part, G, Wp, C, K2):
        ncell, rows = G * Wp, K.bn_bwd_row_slots(G, self.cus)
        slots = K.bwr_slots(G, self.cus) if C == 64 else rows     # C = 32: the fp32 kernel, one wave per promised row
        r = K.bn_bwd_row(_v(s, ncell, C), _v(gy, ncell, C).clone(), None if x is None else _v(x, ncell, C), tuple(t[:C] for t in stat),
                         sums[:2 * C], gelu, _xf(xf, C), _v(GW, Wp, K2).t(), slots, rows, F32)
        if self.mut == "second_trip_lost_from_the_partials" and G > slots:
            g3 = r["gs"].view(G, Wp, C)[slots:]                   # the lines of the second trip: their sums never reach the rows
            r["bias"][:slots] -= K._rows(g3.sum(1), slots)
            if x is not None:
                act = K.xf_apply(_v(x, ncell, C), _xf(xf, C), F32).view(G, Wp, C)[slots:]
                r["dW"][:slots] -= K._rows(torch.einsum("lwo,lwi->loi", g3, act), slots)
        _v(gs, ncell, C)[:] = r["gs"]
        _v(Y1, G, K2, C)[:] = r["Y1"]
        pv = _v(part, rows, C * C + C)
        n = rows if self.mut != "idle_wave_leaves_its_row_unwritten" else min(G, rows)
        pv[:n, C * C:] = r["bias"][:n]
        if x is not None:
            pv[:n, :C * C] = r["dW"].reshape(rows, C * C)[:n]
        else:
            pv[slots:n, :C * C] = 0.0                             # the launcher's memset of the rows beyond its own

    def bn_bwd_row_feat(self, s, gy, phi, gs, stat, sums, count, gelu, GW, Y1, part, G, Wp, C, K2, FW):
        ncell, rows = G * Wp, K.bn_bwd_row_slots(G, self.cus)
        r = K.bn_bwd_row(_v(s, ncell, C), _v(gy, ncell, C).clone(), _v(phi, ncell, FW), tuple(t[:C] for t in stat), sums[:2 * C], gelu, None,
                         _v(GW, Wp, K2).t(), rows, rows, F32)
        if gs is not None:
            _v(gs, ncell, C)[:] = r["gs"]
        elif self.mut == "gs_stored_although_not_asked_for":
            _v(gy, ncell, C)[:] = r["gs"]
        _v(Y1, G, K2, C)[:] = r["Y1"]
        pv = _v(part, rows, C * C + C)
        n = rows if self.mut != "idle_wave_leaves_its_row_unwritten" else min(G, rows)
        pv[:n, C * C:] = r["bias"][:n]
        blk = pv[:, :C * C].view(rows, C, C)
        blk[:n, :, :32] = 0.0
        blk[:n, :, :FW] = r["dW"][:n]
        if self.mut == "moment_block_written_64_wide":
            blk[:n, :, 32:] = 0.0

    def bn_bwd_row_c128_supported(self, Wp, K2):
        return 1 <= K2 <= 48

    def bn_bwd_row_c128(self, s, gy, gs, stat, sums, count, gelu, GW, Y1, part, G, Wp, K2):
        C, ncell, L, slots, rows = 128, G * Wp, 64 * 64 + 64, K.bwr_slots(G, self.cus), K.bn_bwd_row_slots(G, self.cus)
        r = K.bn_bwd_row(_v(s, ncell, C), _v(gy, ncell, C).clone(), None, tuple(t[:C] for t in stat), sums[:2 * C], gelu, None,
                         _v(GW, Wp, K2).t(), slots, rows, F32)
        _v(gs, ncell, C)[:] = r["gs"]
        _v(Y1, G, K2, C)[:] = r["Y1"]
        pv = _v(part, 2, rows, L)
        n = rows if self.mut != "idle_wave_leaves_its_row_unwritten" else min(G, rows)
        for h in (0, 1):
            pv[h, :n, 64 * 64:] = r["bias"][:n, 64 * h:64 * h + 64]
            pv[h, slots:n, :64 * 64] = 0.0

    # ---- the head
    def head_bwd_slots(self, dims):
        return K.head_slots(dims[0] * dims[1] * dims[2], self.cus)

    def head_bwd_row(self, DO):
        return K.head_row(DO)

    def _head(self, s, w1, b1, w2, b2, gout, target, g, part, lpart, dims, DO, stat):
        B, T, H, W, pad, _ = dims
        C, L, ncell = 64, B * T * H, B * (T + pad) * (H + pad) * (W + pad)
        slots, row = self.head_bwd_slots(dims), K.head_row(DO)
        sv = torch.nan_to_num(_v(s, ncell, C))                     # (the margin is sliced away by the restatement; NaN * 0 must not arise)
        r = K.head(sv, tuple(t[:C] for t in stat), _v(w1, K.HID, C), b1[:K.HID], _v(w2, DO, K.HID), None if b2 is None else b2[:DO],
                   None if gout is None else _v(gout, L * W, DO), None if target is None else _v(target, L * W, DO), dims, slots, F32)
        gv = _v(g, ncell, C).view(B, T + pad, H + pad, W + pad, C)
        if self.mut == "head_leaves_the_w_margin_unwritten":
            gv[:, :, :, :W] = r["g"].view(gv.shape)[:, :, :, :W]
        else:
            gv[:] = r["g"].view(gv.shape)
        self._write_rows(_v(part, slots, row), r["part"], L)
        if lpart is not None:
            self._write_rows(_v(lpart, slots), r["loss"], L)

    def head_bwd(self, s, w1, b1, w2, gout, g, part, dims, DO, stat):
        self._head(s, w1, b1, w2, None, gout, None, g, part, None, dims, DO, stat)

    def head_fwd_bwd(self, s, w1, b1, w2, b2, target, gscale, g, part, lpart, dims, DO, stat):
        assert gscale == K.GSCALE
        self._head(s, w1, b1, w2, b2, None, target, g, part, lpart, dims, DO, stat)

    def reduce_partials(self, part, rows, L, out):
        out[:L] = _v(part, rows, L).double().sum(0).float()

    def head_bwd_finalize(self, tot, w1, gamma, beta, DO, dw1, dw2, db1, db2, bn_sums):
        r = K.head_finalize(tot[:K.head_row(DO)], _v(w1, K.HID, 64), gamma[:64], beta[:64], DO)
        if self.mut == "fc1_gradient_without_the_beta_term":
            r["dw1"] = gamma[:64] * tot[:K.HID * 64].view(K.HID, 64)
        for k, o in (("dw1", dw1), ("dw2", dw2), ("db1", db1), ("db2", db2), ("bn_sums", bn_sums)):
            o[:r[k].numel()] = r[k].reshape(-1)


GOOD = TorchKernels()


def rejected(driver, mut, *args, match="kernel error|never written|were written|NaN"):
    """the driver fails on the mutated stand-in: an assertion of Arena.check() or of the verdict"""
    with pytest.raises(AssertionError, match=match):
        driver(TorchKernels(mut), *args)


# ================================================================================================ restatements against independent statements
def test_gelu_grad_and_bn_backward_against_autograd():
    c = K.bwr_case(3, 33, 7, "x", "bn+gelu", True, True)
    G, Wp, K2 = c.dims
    s = c.s.double().requires_grad_(True)
    gamma, beta = c.stat[2].double(), c.stat[3].double()
    mean = s.mean(0)
    z = (s - mean) / torch.sqrt(((s - mean) ** 2).mean(0) + 1e-5) * gamma + beta
    F.gelu(z).backward(c.gy.double())
    r = c.refs()[0]
    # the case hands the kernel mean / invstd / sums rounded to fp32, autograd keeps them in fp64: they agree to fp32 rounding, and the
    # restatement agrees with autograd to 1e-12 when handed autograd's own statistics
    stat64 = (mean.detach(), 1 / torch.sqrt(((s.detach() - mean.detach()) ** 2).mean(0) + 1e-5), gamma, beta)
    sh = (s.detach() - stat64[0]) * stat64[1]
    gz = c.gy.double() * K.gelu_grad(sh * gamma + beta)
    sums = torch.cat((gz.sum(0), (gz * sh).sum(0)))
    r2 = K.bn_bwd_row(s.detach(), c.gy, c.x, stat64, sums, True, c.xf, c.GWt, c.slots, c.rows, F64)
    assert rel_l2(r2["gs"], s.grad) < TOL
    assert rel_l2(r["gs"], s.grad) < 1e-5
    zz = torch.linspace(-6, 6, 1001, dtype=F64, requires_grad=True)
    F.gelu(zz).sum().backward()
    assert rel_l2(K.gelu_grad(zz.detach()), zz.grad) < TOL
    # Y1 and the partial rows: the adjoint W stage and gs^T act(BN(x)), as plain matrix products
    assert rel_l2(r2["Y1"], torch.einsum("kw,gwc->gkc", c.GWt.double(), r2["gs"].view(G, Wp, 64))) < TOL
    act = F.gelu((c.x.double() - c.xf[0].double()) * c.xf[1].double() * c.xf[2].double() + c.xf[3].double())
    assert rel_l2(K.total(r2["dW"]), r2["gs"].t() @ act) < TOL
    # the column sums of gs are analytically 0 (that is what BatchNorm's backward does): absolute, against sum |gs|
    assert float(K.total(r2["bias"]).abs().max()) < TOL * float(r2["abs"].max()) and torch.equal(r2["abs"], r2["gs"].abs().sum(0))


def test_backward_cell_mix_against_autograd():
    """gx = d/dx of the forward cell_mix (the spectral term is its own input here), gz through BN's affine part + GELU, dWc"""
    c = K.wg_case(33, 3, 7, True, True)
    Wp, lines, K2 = c.dims
    Wc = c.Wc.double().requires_grad_(True)
    a_in = K.xf_apply(c.s.double(), c.stat + (True,), F64)         # the layer input act(BN(s_prev))
    y = a_in @ Wc.t()
    y.backward(c.gs.double())
    r = c.refs()[0]
    assert rel_l2(K.total(r["dW"]), Wc.grad) < TOL
    g = c.gs.double().requires_grad_(True)                         # gx: the adjoint of x -> x Wc^T is g -> g Wc
    x = torch.randn(lines * Wp, 64, dtype=F64, generator=K._gen(7))
    ((x @ Wc.detach().t()) * g).sum().backward()
    sh = (c.s.double() - c.stat[0].double()) * c.stat[1].double()
    zz = (sh * c.stat[2].double() + c.stat[3].double()).requires_grad_(True)
    spec = torch.einsum("kw,gkc->gwc", c.GWt.double(), c.z2.double()).reshape(-1, 64)
    gx = spec + c.gs.double() @ Wc.detach()
    F.gelu(zz).backward(gx)
    assert rel_l2(r["out"], zz.grad) < TOL
    assert rel_l2(K.total(r["part"])[0], zz.grad.sum(0)) < TOL and rel_l2(K.total(r["part"])[1], (zz.grad * sh).sum(0)) < TOL
    # the forward: F.linear + the spectral term, statistics as plain sums
    cm = K.cmx_case(33, 3, 7)
    f = cm.refs()[0]
    ref = torch.einsum("kw,gkc->gwc", cm.GWt.double(), cm.z2.double()).reshape(-1, 64) + F.linear(
        F.gelu((cm.x.double() - cm.stat[0].double()) * cm.stat[1].double() * cm.stat[2].double() + cm.stat[3].double()), cm.Wc.double(), cm.bias.double())
    assert rel_l2(f["fwd+bn+gelu:out"], ref) < TOL
    assert rel_l2(K.total(f["fwd+bn+gelu:part"])[0], ref.sum(0)) < TOL and rel_l2(K.total(f["fwd+bn+gelu:part"])[1], (ref ** 2).sum(0)) < TOL


def test_axis_gemm_against_fft_with_a_stage_matrix_of_the_model():
    from realpdebench_amd import dft
    n, m = 22, 6
    x = torch.randn(3, n, 64, dtype=F64, generator=K._gen(8))
    want = torch.fft.rfft(x, dim=1)[:, :m]
    M = torch.from_numpy(dft._fwd_real(n, dft.kept_modes(n, m, False)))          # the forward W stage: [Re rows | Im rows] x n
    got = K.axis_gemm(x, M.t().contiguous(), None, None, F64)
    assert rel_l2(got[:, :m], want.real) < TOL and rel_l2(got[:, m:], want.imag) < TOL
    # k_valid: the rows past it count as zeros (the zero pad of an axis is never read)
    xz = x.clone()
    xz[:, 15:] = 0
    assert rel_l2(K.axis_gemm(x, M.t().contiguous(), 15, None, F64)[:, :m], torch.fft.rfft(xz, dim=1)[:, :m].real) < TOL
    # ... and the inverse stage of the same axis undoes it for a band-limited signal
    band = torch.fft.irfft(torch.fft.rfft(x, dim=1)[:, :m], n=n, dim=1)
    Minv = torch.from_numpy(dft._inv_real(n, dft.kept_modes(n, m, False), float(n)))
    spec = K.axis_gemm(band, M.t().contiguous(), None, None, F64)
    assert rel_l2(K.axis_gemm(spec, Minv.t().contiguous(), None, None, F64), band) < TOL


def test_mode_contract_against_autograd():
    c = K.mode_case(64, 3, 10)
    r = c.refs()[0]
    x = torch.complex(c.X[:, 0].double(), c.X[:, 1].double()).requires_grad_(True)
    w = torch.view_as_complex(c.W.double()).requires_grad_(True)
    y = torch.einsum("bmi,mio->bmo", x, w)
    assert rel_l2(r["Y"][:, 0], y.real.detach()) < TOL and rel_l2(r["Y"][:, 1], y.imag.detach()) < TOL
    g = torch.complex(c.GY[:, 0].double(), c.GY[:, 1].double())
    (y.real * g.real + y.imag * g.imag).sum().backward()            # the real inner product: torch's gradient convention is conj-free
    assert rel_l2(r["GX"][:, 0], x.grad.real) < TOL and rel_l2(r["GX"][:, 1], x.grad.imag) < TOL
    assert rel_l2(r["GW"], torch.view_as_real(w.grad)) < TOL
    wc = torch.view_as_complex(c.W.double())
    assert rel_l2(torch.view_as_real(wc), torch.view_as_real(wc.transpose(1, 2).conj().resolve_conj())) > 1.0     # far from Hermitian


# ================================================================================================ conditioning of the GPU cases
def _ids(v):
    return getattr(v, "__name__", None) or "-".join(str(a) for a in v)


@pytest.mark.parametrize("make,args", K.all_cases(), ids=_ids)
def test_gpu_cases_are_well_conditioned(make, args):
    case = case_of(make, args)
    r64, r32 = case.refs()
    assert set(r64) == set(r32)
    for key in r64:
        a32, a64 = r32[key], r64[key]
        if key == "abs":
            continue
        if key.endswith(("part", "loss")) or key in ("dW", "bias"):           # partial rows are judged by their row sum
            a32, a64 = K.total(a32), K.total(a64)
        if key == "bias":                                           # analytically ~0: measured against sum |gs|
            e = float((a32 - a64).abs().max()) / float(r64["abs"].max())
            print(f"[fno-cases] {case.name} {key} max-abs/sum|gs|: e32 {e:.3e}")
            assert 8 * e <= K.BADLY_CONDITIONED
            continue
        two = key.endswith("part") and a64.dim() == 2                # cell_mix: [2][C], each sum judged on its own
        subs = [(f"{key}[{j}]", a32[j], a64[j]) for j in range(2)] if two else [(key, a32, a64)]
        for name, b32, b64 in subs:
            for kind, e32 in zip(K.MEASURES, K.measures(b32, b64)):
                print(f"[fno-cases] {case.name} {name} {kind}: e32 {e32:.3e}")
                assert 8 * e32 <= K.BADLY_CONDITIONED, f"{case.name} {name}: the fp32 restatement itself is off by {e32:.3e} ({kind})"


def test_cases_reach_the_paths_they_claim():
    """at the MI355X's 256 compute units"""
    assert [K.axg_case(*s).kernel for s in K.AXG_CASES] == K.AXG_KERNELS
    assert [K.axg_case(*s).kernel for s in K.axg_trip_cases()] == ["axg<1>", "axg_resident"]
    # the fp32 cell_mix: 12 waves forward, 8 with the BatchNorm-backward sums, 7 at KC = 128; fewer tiles than waves in each case
    assert [(c.rows, c.rows_bwd, c.fp32) for c in (K.cmx_case(*s[:3], CUS, s[3]) for s in K.CELL_FP32_SHAPES)] == [(12, 8, True), (12, 8, True)]
    assert K.gather_case(True).rows == 21 and K.cell_fp32_waves(128, 64, 0, 1, False, True) == 7
    assert not any(K.cmx_case(*s, CUS).fp32 for s in K.CMX_SHAPES) and len(K.BWR_VARIANTS) == 10
    assert [K.bwr_case(*K.BWR32_SHAPE, *v, CUS, 32).slots for v in K.BWR32_VARIANTS] == [16, 16]
    assert K.AXG_CASES[0][1] % 32 == 1                               # one row in the tail K-step, with O % 16 != 0
    for G, K_, O, N, kv, mode in K.axg_trip_cases():
        t = K.trips(G * (N // 64), K.axg_slots(G, N))
        assert G == 2051 and K.axg_slots(G, N) == 2048 and t.count(2) == 3 and t.count(1) == 2045
    C, B, M = K.mode_trip_case()
    assert (B, M) == (5, 517) and K.mode_grid(M) == 512 and K.trips(M, 512).count(2) == 5 and M * C * C * 2 * 4 < 20e6
    Wp, lines, K2 = K.cmx_trip_shape()
    assert lines == 2053 and K.cmx_stat_rows(lines) == 2048 and K.trips(lines, 2048).count(2) == 5
    assert [K.cmx_stat_rows(s[1]) for s in K.CMX_SHAPES] == [8, 8, 16, 8]                 # idle waves at 1, 3, 9 and 5 lines
    Wp, lines, K2 = K.cmx128_trip_shape()
    assert lines == 1029 and K.cmx128_waves(Wp) == 8 and K.cmx128_stat_rows(lines, Wp) == 1024 and K.trips(lines, 1024).count(2) == 5
    assert [K.cmx128_stat_rows(s[1], s[0]) for s in K.CMX128_SHAPES] == [8, 16] and K.cmx128_waves(134) == 6
    Wp, lines, K2 = K.wg_trip_shape()
    assert lines == 1027 and K.cmx_wg_slots(lines) == 1024 and K.trips(lines, 1024).count(2) == 3
    G, Wp, K2 = K.bwr_trip_shape()
    assert G == 1027 and K.bwr_slots(G) == 1024 and K.bn_bwd_row_slots(G) == 1032 and K.trips(G, 1024).count(2) == 3
    assert [(K.bwr_slots(s[0]), K.bn_bwd_row_slots(s[0])) for s in K.BWR_SHAPES] == [(4, 8), (16, 16), (4, 8), (8, 8)]
    assert max(G * Wp * 64 * 4 for G, Wp, K2 in [K.bwr_trip_shape()]) < 20e6
    for B, T, H, W, pad, DO in K.head_trip_shapes():
        assert (T * H, B * (T + pad) * (H + pad) * (W + pad)) == (1027, 8505) and K.head_slots(T * H) == 1024 and K.trips(T * H, 1024).count(2) == 3
    assert [K.head_slots(s[0] * s[1] * s[2]) for s in K.HEAD_SHAPES] == [4, 8, 32, 8, 8]


# ================================================================================================ the stand-in passes, its mutations fail
@pytest.mark.parametrize("shape", K.AXG_CASES + K.axg_trip_cases(), ids=_ids)
def test_standin_axis_gemm(shape):
    c = case_of(K.axg_case, shape)
    G, K_, O, N, kv = c.dims
    K.run_axis_gemm(GOOD, c)
    if kv is not None:
        rejected(K.run_axis_gemm, "rows_past_k_valid_are_read", c)
    if c.mode in ("", "xf", "xfg", "odd"):
        rejected(K.run_axis_gemm, "tail_tile_writes_past_its_line", c)
    if c.mode == "dense":
        rejected(K.run_axis_gemm, "items_past_nslots_not_produced", c)


@pytest.mark.parametrize("shape", K.MODE_CASES + [K.mode_trip_case()], ids=_ids)
def test_standin_mode_contract(shape):
    c = case_of(K.mode_case, shape)
    K.run_mode_contract(GOOD, c)
    rejected(K.run_mode_contract, "weights_not_conjugated", c)
    rejected(K.run_mode_contract, "weights_transposed", c)
    if shape == K.mode_trip_case():
        rejected(K.run_mode_contract, "modes_past_the_grid_not_produced", c)


@pytest.mark.parametrize("shape", K.CELL_FP32_SHAPES, ids=_ids)
def test_standin_cell_mix_fp32_kernel(shape):
    c = case_of(K.cmx_case, shape[:3] + (CUS, shape[3]))
    for mode in K.CELL_FP32_MODES:
        K.run_cell_mix(GOOD, c, mode)
    rejected(K.run_cell_mix, "sum_gz_s_instead_of_sum_gz_shat", c, "bwd+gelu")
    rejected(K.run_cell_mix, "idle_wave_leaves_its_row_unwritten", c, "fwd")
    rejected(K.run_cell_mix, "idle_wave_leaves_its_row_unwritten", c, "bwd")
    # the partition matters to what is asserted: rows of waves without a TILE are zero, which a walk by lines does not give
    rejected(K.run_cell_mix, "partials_by_lines_on_the_tile_kernel", c, "fwd", match="waves without a work item")


@pytest.mark.parametrize("gelu", [True, False])
def test_standin_cell_mix_gather(gelu):
    c = case_of(K.gather_case, (gelu, CUS))
    K.run_cell_mix_gather(GOOD, c)
    rejected(K.run_cell_mix_gather, "gather_leaves_the_margin_unwritten", c)
    rejected(K.run_cell_mix_gather, "idle_wave_leaves_its_row_unwritten", c)


@pytest.mark.parametrize("shape", K.FEAT_SHAPES, ids=_ids)
def test_standin_cell_mix_feat(shape):
    c = case_of(K.feat_case, shape + (CUS,))
    for mode in ("fwd", "oxf"):
        K.run_cell_mix_feat(GOOD, c, mode)
        rejected(K.run_cell_mix_feat, "feature_fields_shifted_by_one", c, mode)
    rejected(K.run_cell_mix_feat, "idle_wave_leaves_its_row_unwritten", c, "fwd")


@pytest.mark.parametrize("variant", K.BWR32_VARIANTS, ids=_ids)
def test_standin_bn_bwd_row_c32(variant):
    c = case_of(K.bwr_case, K.BWR32_SHAPE + variant + (CUS, 32))
    K.run_bn_bwd_row(GOOD, c)
    rejected(K.run_bn_bwd_row, "idle_wave_leaves_its_row_unwritten", c)


@pytest.mark.parametrize("FW,gelu,inplace", K.BWRF_VARIANTS)
def test_standin_bn_bwd_row_feat(FW, gelu, inplace):
    c = case_of(K.bwr_case, K.BWRF_SHAPE + ("x", None, gelu, inplace, CUS, 64, FW))
    K.run_bn_bwd_row(GOOD, c)
    rejected(K.run_bn_bwd_row, "idle_wave_leaves_its_row_unwritten", c)
    rejected(K.run_bn_bwd_row, "moment_block_written_64_wide", c)
    if not inplace:
        rejected(K.run_bn_bwd_row, "gs_stored_although_not_asked_for", c, match="input operand 'gy'")


@pytest.mark.parametrize("shape", [s + (64,) for s in K.CMX_SHAPES + [K.cmx_trip_shape()]]
                         + [s + (128,) for s in K.CMX128_SHAPES + [K.cmx128_trip_shape()]], ids=_ids)
def test_standin_cell_mix(shape):
    c = case_of(K.cmx_case, shape[:3] + (CUS, shape[3]))
    shape = shape[:3]
    Wp, lines, K2, C = c.dims
    for mode in K.CMX_MODES:
        K.run_cell_mix(GOOD, c, mode)
    K.run_cell_mix(GOOD, c, "fwd+bn+gelu", with_stats=False)
    rejected(K.run_cell_mix, "sum_gz_s_instead_of_sum_gz_shat", c, "bwd+gelu")
    if lines < c.rows:
        rejected(K.run_cell_mix, "idle_wave_leaves_its_row_unwritten", c, "fwd")
        rejected(K.run_cell_mix, "idle_wave_leaves_its_row_unwritten", c, "bwd+gelu+gz")
    if shape == K.cmx_trip_shape():
        rejected(K.run_cell_mix, "lines_past_nslots_not_produced", c, "fwd+bn")
        # one wrong cell among 4.2 million: Rel-L2 alone would pass it, the max measure does not
        r64, r32 = c.refs()
        bad = r32["plain:out"].clone()
        bad[bad.shape[0] // 2, 17] += 2e-5 * float(bad.abs().max())
        e_l2, e_max = K.measures(bad, r64["plain:out"])
        assert bad.numel() > 10 ** 5 and e_l2 < 1e-6 < e_max
        rejected(K.run_cell_mix, "one_wrong_cell", c, "plain", match="max-abs: kernel error")


@pytest.mark.parametrize("shape,mode", [(s, m) for s in K.WG_SHAPES for m in K.WG_MODES] + [(K.wg_trip_shape(), (True, True))], ids=_ids)
def test_standin_cell_mix_wgrad(shape, mode):
    c = case_of(K.wg_case, shape + mode + (CUS,))
    K.run_cell_mix_wgrad(GOOD, c)
    rejected(K.run_cell_mix_wgrad, "dWc_transposed", c)
    rejected(K.run_cell_mix_wgrad, "sum_gz_s_instead_of_sum_gz_shat", c)
    if shape[1] < c.slots:
        rejected(K.run_cell_mix_wgrad, "idle_wave_leaves_its_row_unwritten", c)


@pytest.mark.parametrize("shape,variant", [(s, v) for s in K.BWR_SHAPES for v in K.BWR_VARIANTS]
                         + [(K.bwr_trip_shape(), v) for v in K.BWR_TRIP_VARIANTS], ids=_ids)
def test_standin_bn_bwd_row(shape, variant):
    c = case_of(K.bwr_case, shape + variant + (CUS,))
    K.run_bn_bwd_row(GOOD, c)
    if shape[0] < K.bn_bwd_row_slots(shape[0]):
        rejected(K.run_bn_bwd_row, "idle_wave_leaves_its_row_unwritten", c)
    if shape == K.bwr_trip_shape() and variant[0] == "x":
        rejected(K.run_bn_bwd_row, "second_trip_lost_from_the_partials", c)


@pytest.mark.parametrize("shape,variant", [(s, v) for s in K.BWR128_SHAPES for v in K.BWR128_VARIANTS], ids=_ids)
def test_standin_bn_bwd_row_c128(shape, variant):
    c = case_of(K.bwr128_case, shape + variant + (CUS,))
    K.run_bn_bwd_row_c128(GOOD, c)
    rejected(K.run_bn_bwd_row_c128, "idle_wave_leaves_its_row_unwritten", c)


def test_head_against_autograd():
    """fno.py's head on the cropped cells: the gradient with respect to BN(s) (zeros in the margin), the four parameter gradients, the
    BatchNorm-backward sums and the loss"""
    c = K.head_case(1, 2, 3, 33, 2, 2)
    B, T, H, W, pad, DO = c.dims
    f8 = lambda t: t.double()
    s = f8(c.s)
    mean, invstd, gamma, beta = (f8(t) for t in c.stat)
    w1, b1, w2, b2 = (f8(t).requires_grad_(True) for t in (c.w1, c.b1, c.w2, c.b2))
    sh = (s - mean) * invstd
    a_full = (sh * gamma + beta).requires_grad_(True)
    a = a_full.view(B, T + pad, H + pad, W + pad, 64)[:, :T, :H, :W].reshape(-1, 64)
    out = F.gelu(a @ w1.t() + b1) @ w2.t() + b2
    loss = ((out - f8(c.target)) ** 2).sum()
    (0.5 * K.GSCALE * loss).backward()                             # d/d out = GSCALE (out - target)
    r = c.refs()[0]
    assert rel_l2(K.total(r["loss:loss"]).reshape(1), loss.detach().reshape(1)) < TOL
    assert rel_l2(r["loss:g"], a_full.grad) < TOL and not r["loss:g"].view(B, T + pad, H + pad, W + pad, 64)[:, :, :, W:].any()
    for k, t in (("dw1", w1), ("dw2", w2), ("db1", b1), ("db2", b2)):
        assert rel_l2(r[f"loss:{k}"], t.grad) < TOL, k
    assert rel_l2(r["loss:bn_sums"][0], a_full.grad.sum(0)) < TOL and rel_l2(r["loss:bn_sums"][1], (a_full.grad * sh).sum(0)) < TOL
    assert float(c.stat[2][3]) == 0.0 and float(c.stat[3][5]) == 0.0
    # the target is independent of the output: out - target cancels nothing
    assert float((out.detach() - f8(c.target)).abs().mean()) > 0.5 * float(out.detach().abs().mean())


@pytest.mark.parametrize("shape", K.HEAD_SHAPES + K.head_trip_shapes(), ids=_ids)
def test_standin_head(shape):
    c = case_of(K.head_case, shape + (CUS,))
    K.run_head(GOOD, c)
    if shape[4]:
        rejected(K.run_head, "head_leaves_the_w_margin_unwritten", c)
    rejected(K.run_head, "fc1_gradient_without_the_beta_term", c)
    if shape[0] * shape[1] * shape[2] < c.slots:
        rejected(K.run_head, "idle_wave_leaves_its_row_unwritten", c)
