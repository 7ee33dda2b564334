"""TEST INFRASTRUCTURE ONLY -- the shapes, inputs, restatements and drivers of the per-kernel tests of the FNO3d step kernels, shared by
tests/test_gpu_fno_kernels.py (which runs the HIP kernels) and tests/test_fno_kernels_host.py (which proves, without a GPU, that every
restatement agrees with an independent statement, that every case is well conditioned and that a wrong kernel would be noticed).
``Case``, the two measures and the conditioning cap are those of tests/unet_kernel_cases.py; the verdict is tests/kernel_verdict.py.

A RESTATEMENT (``axis_gemm``, ``mode_contract``, ``cell_mix_*``, ``bn_bwd_row``, ``head``) states one launch in plain torch at a given dtype.  The
ones with partial rows partition their sums AS THE LAUNCHER DOES: wave ``w`` of ``nslots`` adds up the lines w, w + nslots, ... into row
``w``; the rows are added up afterwards (in fp64, by the driver, for the kernel and for the fp32 restatement alike).  The fp32 run of
a restatement gives e32, the fp64 run the reference.

A DRIVER (``run_*``) lays the operands of ONE launch out in a guard-banded arena (tests/guarded.py), calls ``kern.<entry point>``, runs
``Arena.check()`` and judges every output on Rel-L2 and max |error| / max |reference| with the bound max(8 * e32, 1e-6).  ``kern`` is
the adapter of the GPU test (realpdebench_amd.ops on a device) or the torch stand-in of the host test on a CPU arena.

Slot counts depend on the number of compute units; they are restated here from the launchers (``*_slots``, ``*_rows``) and the GPU
test asserts that they equal the library's queries on its device.  The C ABI does not export ``rpb_axg_supported`` (which axis_gemm
launches run on the bf16-pipe kernels of csrc/rpb_axg.hip and which fall back to csrc/rpb_axis_gemm.hip), so its rule is restated
here as ``axg_supported`` / ``axg_kernel``; the host test asserts the kernel every case is meant for.

What the shapes are for.  axis_gemm: K % 32 == 1 (one row in the tail K-step), ragged 16-row tiles, gapped strides on both sides
(gaps of the input hold NaN, gaps of the output are named unwritten), rows k >= k_valid hold NaN, and G = 8 CUs + 3 items (three
waves take a second trip).  mode_contract: B on either side of the 32-sample pass, M = 2 CUs + 5 (the persistent kernel's second trip
with its next-mode prefetch).  cell_mix / cell_mix_wgrad / bn_bwd_row: one exact 32-cell tile with idle waves (every promised partial
row must be written), a one-cell tail tile, K2 % 8 != 0, and waves * CUs + 3 / + 5 lines.  The head: one cell, lines of 33 / 32 / 40 / 7
cells at fc2 widths 1 .. 4 (width 2 runs on rpb_pjg.hip), the pad margin of its input holding NaN and that of its output exact zeros,
a target drawn independently of the output, and T H = 4 CUs + 3 lines."""
import math

import torch

import guarded
from kernel_verdict import verdict
from unet_kernel_cases import (BADLY_CONDITIONED, F32, F64, MEASURES, MI355X_CUS, Case, _gen, _rn,      # noqa: F401
                               measures)

TAG = "fno-kernels"
NAN = float("nan")


def ceil_div(a, b):
    return (a + b - 1) // b


# ================================================================================================ slot counts (restated launchers)
def _persistent(items, waves, cus):
    return waves * max(1, min(cus, ceil_div(items, waves)))


def axg_slots(G, N, cus=MI355X_CUS):
    """rpb_axg_launch: items = G * N / 64, 8 waves (AXG_WAVES == AXG_WAVES_XF == 8)"""
    return _persistent(G * (N // 64), 8, cus)


def axg_supported(K, O, N, in_g, in_k, out_g, out_o, k_valid, accumulate, has_xf):
    """rpb_axg_supported (csrc/rpb_axg.hip), restated: the C ABI does not export it"""
    if accumulate or N % 64 or k_valid < 1 or ((in_g | in_k | out_g | out_o) & 3) or (has_xf and N > 128):
        return False
    if (k_valid + 32) * in_k * 4 + 256 >= 2 ** 31 or (O + 16) * out_o * 4 + 256 >= 2 ** 31:
        return False
    return ceil_div(k_valid, 32) * 3 * ceil_div(O, 16) * 64 * 16 <= 160 * 1024


def axg_kernel(K, O, N, in_g, in_k, out_g, out_o, k_valid, accumulate, has_xf):
    """the kernel rpb_axis_gemm launches: rpb_axg_launch's choice, or the fp32 kernel's NV"""
    if axg_supported(K, O, N, in_g, in_k, out_g, out_o, k_valid, accumulate, has_xf):
        mt = ceil_div(O, 16)
        if not has_xf and k_valid <= 64 and mt > 4:
            return "axg_resident"
        return f"axg<{min(mt, 4)}{',xf' if has_xf else ''}>" + ("+passes" if mt > 4 else "")
    ot = ceil_div(O, 32)
    OT = 3 if ot >= 3 else ot
    NV = 4 if N % 128 == 0 else 2 if N % 64 == 0 else 1
    if ot >= 3 and NV == 4:
        OT = 2
    while OT * NV > 8:
        NV >>= 1
    if NV == 4 and ((in_g | in_k | out_g | out_o) & 3):
        NV = 2
    if NV == 2 and ((in_g | in_k | out_g | out_o) & 1):
        NV = 1
    return f"fp32<NV{NV}>"


def mode_grid(M, cus=MI355X_CUS):
    """mode_bf16_kernel<., true> (B <= 32, C = 64): min(M, MB_PERSIST_WGS * CUs) workgroups, MB_PERSIST_WGS = 2"""
    return min(M, 2 * cus)


def cmx_stat_rows(lines, cus=MI355X_CUS):
    """rpb_cmx_stat_rows: 8 waves per workgroup in every statistics mode"""
    return _persistent(lines, 8, cus)


def cmx128_waves(Wp):
    """cmx_waves128: 8 waves where the workgroup's LDS (weight planes, the line's GW planes, 12 KB per wave) fits 160 KB, else 6"""
    lds = lambda waves: (48 * 64 + 3 * Wp * 4 + waves * 12 * 64) * 16 + 3 * 128 * 4 + 16
    return 8 if lds(8) <= 160 * 1024 else 6 if lds(6) <= 160 * 1024 else 0


def cmx128_stat_rows(lines, Wp, cus=MI355X_CUS):
    """rpb_cmx128_stat_rows: workgroup PAIRS (one 64-channel output half each) walk the lines, CUs / 2 pairs at most"""
    waves = cmx128_waves(Wp)
    return waves * max(1, min(cus // 2, ceil_div(lines, waves)))


def cmx_rows(lines, Wp, C, cus=MI355X_CUS):
    return cmx_stat_rows(lines, cus) if C == 64 else cmx128_stat_rows(lines, Wp, cus)


def cell_fp32_waves(KC, CO, K2, Wp, spec, bnb):
    """cell_mix_waves (csrc/rpb_cell.hip): the most waves whose LDS (GW, the weight tile, a transposing tile and a row map per wave) fits
    160 KB; 512 threads at KC = 128 or with BatchNorm-backward sums, else CM_MAX_THREADS = 768"""
    k2s = 0 if not spec else 8 if K2 <= 16 else 16 if K2 <= 32 else 20
    wmax = (512 if (KC >= 128 or bnb) else 768) // 64
    for w in (16, 14, 12, 10, 8, 7, 6, 4, 2, 1):
        if w <= wmax and ((2 * k2s * Wp if spec else 0) + KC * CO + w * 32 * (KC + 1) + w * 32) * 4 <= 160 * 1024:
            return w
    return 0


def cell_fp32_rows(ncell, KC, CO, K2, Wp, spec, bnb, cus=MI355X_CUS):
    """rpb_cell_mix_stat_rows on the fp32 kernel: the work items are 32-cell tiles of the flat cell list (they straddle lines)"""
    return _persistent(ceil_div(ncell, 32), cell_fp32_waves(KC, CO, K2, Wp, spec, bnb), cus)


def cmx_wg_slots(lines, cus=MI355X_CUS):
    """rpb_cmx_wg_slots: CMX_WG_PAIRS = 4 wave pairs per workgroup"""
    return _persistent(lines, 4, cus)


def bwr_slots(G, cus=MI355X_CUS):
    """rpb_bwr_slots: the waves of the bf16-pipe row kernel, BW_WAVES = 4"""
    return _persistent(G, 4, cus)


def bn_bwd_row_slots(G, cus=MI355X_CUS):
    """rpb_bn_bwd_row_slots: the rows the caller allocates (8-wave blocks of the fp32 kernel); the bf16-pipe launcher clears the rows
    beyond its own bwr_slots(G) with a memset"""
    return min(8 * cus, ceil_div(G, 8) * 8)


def trips(items, nslots):
    """how many items each slot walks"""
    return [len(range(w, items, nslots)) for w in range(nslots)]


# ================================================================================================ restatements
def gelu_grad(z):
    """d/dz of the erf GELU"""
    return 0.5 * (1 + torch.erf(z / math.sqrt(2.0))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


def xf_apply(x, p, dt):
    """the lazy input / eval output transform: ``p`` = None or (mean, invstd, gamma, beta, gelu)"""
    if p is None:
        return x
    mean, invstd, gamma, beta, gelu = p
    z = (x - mean.to(dt)) * invstd.to(dt) * gamma.to(dt) + beta.to(dt)
    return torch.nn.functional.gelu(z) if gelu else z


def axis_gemm(x, Mt, k_valid, xf, dt):
    """out[g, o, n] = sum_{k < k_valid} Mt[k, o] * xf(x)[g, k, n]; the transform's channels are n"""
    kv = x.shape[1] if k_valid is None else k_valid
    return torch.einsum("ko,gkn->gon", Mt[:kv].to(dt), xf_apply(x[:, :kv].to(dt), xf, dt))


def _cplx(t):
    return torch.complex(t[..., 0, :, :], t[..., 1, :, :])          # [B][2][M][C] -> [B][M][C]


def _planar(z):
    return torch.stack((z.real, z.imag), dim=-3)


def mode_contract(X, W, GY, dt):
    """y = x w, gx = gy conj(w)^T, gw = conj(x)^T gy per mode, planar [B][2][M][C] tensors and interleaved [M][i][o][2] weights"""
    x, g, w = _cplx(X.to(dt)), _cplx(GY.to(dt)), torch.view_as_complex(W.to(dt).contiguous())
    return dict(Y=_planar(torch.einsum("bmi,mio->bmo", x, w)), GX=_planar(torch.einsum("bmo,mio->bmi", g, w.conj())),
                GW=torch.view_as_real(torch.einsum("bmi,bmo->mio", x.conj(), g)))


def _rows(per_line, nslots):
    """[lines][...] -> [nslots][...]: wave w adds up the lines w, w + nslots, ...; waves without a line hold zeros"""
    lines = per_line.shape[0]
    out = torch.zeros((nslots,) + tuple(per_line.shape[1:]), dtype=per_line.dtype)
    return out.index_add_(0, torch.arange(lines) % nslots, per_line)


def _part(per_cell, item, nslots):
    """[ncell][...] -> [nslots][...]: the work items are runs of ``item`` cells (a line of Wp cells on the bf16 pipe, a 32-cell tile on the
    fp32 kernel; the last one may be short), dealt to the waves as ``_rows`` does"""
    n, items = per_cell.shape[0], ceil_div(per_cell.shape[0], item)
    padded = torch.zeros((items * item,) + tuple(per_cell.shape[1:]), dtype=per_cell.dtype)
    padded[:n] = per_cell
    return _rows(padded.view((items, item) + tuple(per_cell.shape[1:])).sum(1), nslots)


def _spec(z2, GWt, dt):
    return torch.einsum("kw,gkc->gwc", GWt.to(dt), z2.to(dt))       # [lines][Wp][C]


def cell_mix_fwd(x, Wc, bias, z2, GWt, xf, oxf, nslots, dt, item=None):
    """out = spectral term + xf(x) Wc^T + bias over lines of Wp cells (x: [ncell][KC], Wc: [C][KC] -- KC = FW, the feature fields, at
    layer 0); part[w] = (sum out, sum out^2) of wave w's items (``item`` cells each, default a line); with ``oxf`` the stored tensor is
    oxf(out)"""
    lines, Wp, C = z2.shape[0], GWt.shape[1], Wc.shape[0]
    out = (_spec(z2, GWt, dt) + (xf_apply(x.to(dt), xf, dt) @ Wc.to(dt).t() + bias.to(dt)).view(lines, Wp, C)).reshape(lines * Wp, C)
    r = dict(out=xf_apply(out, oxf, dt))
    if nslots:
        r["part"] = _part(torch.stack((out, out * out), 1), item or Wp, nslots)
    return r


def cell_mix_bwd(g, Wc, z2, GWt, bnb, write_gz, nslots, dt, sums_of_s=False, item=None):
    """gx = spectral term + g Wc; gz = gx gelu'(z) (z = BN of ``s``); part[w] = (sum gz, sum gz shat) of wave w's lines; the stored tensor
    is gz with ``write_gz``, else gx.  ``bnb`` = (s, mean, invstd, gamma, beta, gelu) or None (plain transposed-weight launch)"""
    lines, Wp, C = z2.shape[0], GWt.shape[1], Wc.shape[0]
    gx = _spec(z2, GWt, dt) + (g.to(dt) @ Wc.to(dt)).view(lines, Wp, C)
    if bnb is None:
        return dict(out=gx.reshape(-1, C))
    s, mean, invstd, gamma, beta, gelu = bnb
    sh = ((s.to(dt) - mean.to(dt)) * invstd.to(dt)).view(lines, Wp, C)
    gz = gx * gelu_grad(sh * gamma.to(dt) + beta.to(dt)) if gelu else gx
    second = gz * (s.to(dt).view(lines, Wp, C) if sums_of_s else sh)                 # sums_of_s: the host test's wrong term
    return dict(out=(gz if write_gz else gx).reshape(-1, C),
                part=_part(torch.stack((gz.reshape(-1, C), second.reshape(-1, C)), 1), item or Wp, nslots))


def cell_mix_gather(gu, Wm, s, stat, gelu, dims, nslots, dt):
    """the fc1 data gradient scattered into the padded layout (exact zeros in the margin) with the BatchNorm-backward sums of the last
    layer: gx[crop] = gu Wm, part[w] = (sum gz, sum gz shat) over wave w's 32-cell tiles of the padded cell list"""
    B, T, H, W, pad = dims
    CO = Wm.shape[1]
    gx = torch.zeros(B, T + pad, H + pad, W + pad, CO, dtype=dt)
    gx[:, :T, :H, :W] = (gu.to(dt) @ Wm.to(dt)).view(B, T, H, W, CO)
    gx = gx.view(-1, CO)
    mean, invstd, gamma, beta = (t.to(dt) for t in stat)
    sh = (s.to(dt) - mean) * invstd
    gz = gx * gelu_grad(sh * gamma + beta) if gelu else gx
    return dict(out=gx, part=_part(torch.stack((gz, gz * sh), 1), 32, nslots))


def cell_mix_wgrad(gs, Wc, z2, GWt, bnb, write_gz, nslots, dt, transposed=False, sums_of_s=False):
    """cell_mix_bwd with d Wc[o][i] = sum_cells gs[cell][o] act(BN(s))[cell][i] riding along, one [C][C] row per wave pair"""
    lines, Wp, C = z2.shape[0], GWt.shape[1], Wc.shape[0]
    r = cell_mix_bwd(gs, Wc, z2, GWt, bnb, write_gz, nslots, dt, sums_of_s)
    act = xf_apply(bnb[0].to(dt), bnb[1:], dt).view(lines, Wp, C)
    eq = "lwi,lwo->loi" if transposed else "lwo,lwi->loi"
    r["dW"] = _rows(torch.einsum(eq, gs.to(dt).view(lines, Wp, C), act), nslots)
    return r


def bn_bwd_row(s, gy, x, stat, sums, gelu, xf, GWt, nslots, rows, dt):
    """gs = gamma invstd (gz - sums0 / n - shat sums1 / n) with gz = gy gelu'(z); Y1[g] = GWt gs[g]; part[w] = (gs^T xf(x) | sum gs) of wave
    w's lines, ``rows`` >= nslots rows in all (the launcher clears the others)"""
    mean, invstd, gamma, beta = (t.to(dt) for t in stat)
    G, Wp, C = s.shape[0] // GWt.shape[1], GWt.shape[1], s.shape[1]
    n = s.shape[0]
    sh = (s.to(dt) - mean) * invstd
    gz = gy.to(dt) * gelu_grad(sh * gamma + beta) if gelu else gy.to(dt)
    gs = gamma * invstd * (gz - sums[:C].to(dt) / n - sh * sums[C:].to(dt) / n)
    g3 = gs.view(G, Wp, C)
    r = dict(gs=gs, Y1=torch.einsum("kw,gwc->gkc", GWt.to(dt), g3), abs=gs.abs().sum(0))
    bias = torch.zeros(rows, C, dtype=dt)
    bias[:nslots] = _rows(g3.sum(1), nslots)
    r["bias"] = bias
    if x is not None:
        KC = x.shape[1]                                           # C, or FW at layer 0: the field moments sum_cells gs (x) phi
        dW = torch.zeros(rows, C, KC, dtype=dt)
        dW[:nslots] = _rows(torch.einsum("lwo,lwi->loi", g3, xf_apply(x.to(dt), xf, dt).view(G, Wp, KC)), nslots)
        r["dW"] = dW
    return r


def bn_sums(s, gy, stat, gelu):
    """the BatchNorm-backward sums the row kernel is handed (fp64, rounded to fp32 as the trainer's reduction stores them)"""
    mean, invstd, gamma, beta = (t.double() for t in stat)
    sh = (s.double() - mean) * invstd
    gz = gy.double() * gelu_grad(sh * gamma + beta) if gelu else gy.double()
    return torch.cat((gz.sum(0), (gz * sh).sum(0))).float()


# ================================================================================================ the verdict
def judge(name, got, ref64, ref32, existing=None):
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    verdict(TAG, name, zip(MEASURES, measures(ref32, ref64), measures(got, ref64)), existing)


def judge_against(name, got, ref64, ref32, scale, existing=None):
    """an output that is analytically ~0 (the column sums of a BatchNorm-backward gs): max |error| against ``scale`` (sum |gs|)"""
    top = float(scale.double().abs().max())
    err = lambda t: float((t.double() - ref64.double()).abs().max()) / top
    verdict(TAG, name, [("max-abs/sum|gs|", err(ref32), err(got))], existing)


def total(rows):
    """the row sum the trainer's rpb_reduce_partials forms (that kernel has its own tests)"""
    return rows.double().sum(0)


def _ex(existing, kernel):
    return (existing or {}).get(kernel)


def _stat(g, C):
    """(mean, invstd, gamma, beta) of a BatchNorm layer, none of them near 0"""
    return (_rn(g, C, scale=0.2), torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) + 0.5, _rn(g, C, scale=0.3))


# ================================================================================================ axis_gemm
# (G, K, O, N, k_valid, mode): mode = "" plain, "xf" BN, "xfg" BN + GELU, "dense", "acc" (dense, accumulate), "odd" (in_g odd)
AXG_CASES = [(3, 33, 5, 64, None, ""), (5, 134, 32, 64, None, ""), (5, 134, 32, 64, None, "xfg"), (2, 70, 48, 128, None, "xf"),
             (2, 96, 134, 64, None, ""), (3, 48, 134, 64, None, ""), (2, 64, 70, 128, 29, ""), (2, 134, 32, 64, 128, ""),
             (4, 7, 5, 32, None, "acc"), (2, 52, 16, 96, None, ""), (3, 48, 268, 64, None, "odd"),
             (2, 5, 5, 64, None, "acc"), (3, 9, 40, 128, None, "acc")]          # accumulate at N % 64 == 0 / N % 128 == 0: the NV = 2 / 4 bodies
AXG_KERNELS = ["axg<1>", "axg<2>", "axg<2,xf>", "axg<3,xf>", "axg<4>+passes", "axg_resident", "axg_resident", "axg<2>",
               "fp32<NV1>", "fp32<NV1>", "fp32<NV1>", "fp32<NV2>", "fp32<NV4>"]


def axg_trip_cases(cus=MI355X_CUS):
    """G = 8 CUs + 3 one-strip items: three waves take a second trip; the plain and the resident kernel"""
    return [(8 * cus + 3, 8, 8, 64, None, "dense"), (8 * cus + 3, 8, 70, 64, None, "dense")]


def axg_strides(G, K, O, N, mode):
    if mode in ("dense", "acc"):
        return K * N, N, O * N, N
    in_k, out_o = N + 64, N + 64
    return K * in_k + (9 if mode == "odd" else 8), in_k, O * out_o + 4, out_o


def axg_case(G, K, O, N, kv, mode):
    g = _gen(41, G, K, O, N, kv or 0, len(mode))
    xf = None
    if mode.startswith("xf"):
        xf = _stat(g, N) + (mode == "xfg",)
    i = dict(dims=(G, K, O, N, kv), mode=mode, strides=axg_strides(G, K, O, N, mode), x=_rn(g, G, K, N, scale=1.5, shift=0.3),
             Mt=_rn(g, K, O), xf=xf, old=_rn(g, G, O, N) if mode == "acc" else None)
    i["kernel"] = axg_kernel(K, O, N, *i["strides"], K if kv is None else kv, mode == "acc", xf is not None)

    def ref(dt):
        out = axis_gemm(i["x"], i["Mt"], kv, xf, dt)
        return dict(out=out + i["old"].to(dt) if mode == "acc" else out)
    return Case(f"axis_gemm G={G} K={K} O={O} N={N} kv={kv} {mode or 'gapped'} [{i['kernel']}]", i, ref)


def run_axis_gemm(kern, c, existing=None):
    G, K, O, N, kv = c.dims
    in_g, in_k, out_g, out_o = c.strides
    r64, r32 = c.refs()
    xbuf = torch.full((G * in_g,), NAN)                           # stride gaps and the rows k >= k_valid hold NaN: nobody reads them
    xbuf.as_strided((G, K, N), (in_g, in_k, 1))[:, :K if kv is None else kv] = c.x[:, :K if kv is None else kv]
    a = guarded.Arena(kern.dev)
    x, Mt = a.inp(xbuf, "in", ld=in_k, guard=32 * in_k + 1024), a.inp(c.Mt, "Mt")      # a K-step of 32 rows is how far a read can overreach
    xf = None if c.xf is None else _ops_of(a, c.xf[:4], STAT_NAMES) + (c.xf[4],)
    if c.mode == "acc":
        out = a.inout(c.old, "out")
    else:
        gaps = torch.ones(G * out_g, dtype=torch.bool)
        gaps.as_strided((G, O, N), (out_g, out_o, 1))[:] = False
        out = a.out(G * out_g, name="out", ld=out_o, unwritten=gaps)
    kern.axis_gemm(x.op, out.op, Mt.op, G, K, O, N, in_g, in_k, out_g, out_o, kv, c.mode == "acc", _opd(xf))
    a.check()
    got = out.get().reshape(-1).as_strided((G, O, N), (out_g, out_o, 1))
    judge(c.name, got, r64["out"], r32["out"], _ex(existing, "axis_gemm"))


# ================================================================================================ mode_contract
MODE_CASES = [(64, 3, 10), (64, 32, 6), (64, 33, 6), (64, 70, 3), (64, 1, 4), (128, 5, 4), (128, 32, 3), (128, 70, 2), (32, 3, 10)]


def mode_trip_case(cus=MI355X_CUS):
    """M = 2 CUs + 5: five workgroups of the persistent kernel walk (and prefetch the weights of) a second mode"""
    return (64, 5, 2 * cus + 5)


def mode_case(C, B, M):
    g = _gen(42, C, B, M)
    i = dict(dims=(C, B, M), X=_rn(g, B, 2, M, C), W=_rn(g, M, C, C, 2, scale=1 / math.sqrt(C)), GY=_rn(g, B, 2, M, C), old=_rn(g, M, C, C, 2))

    def ref(dt):
        r = mode_contract(i["X"], i["W"], i["GY"], dt)
        r["GWacc"] = r["GW"] + i["old"].to(dt)
        return r
    return Case(f"mode_contract C={C} B={B} M={M}", i, ref)


def run_mode_contract(kern, c, existing=None):
    C, B, M = c.dims
    r64, r32 = c.refs()
    for which in ("Y", "GX", "GW", "GWacc"):
        a = guarded.Arena(kern.dev)
        if which == "Y":
            X, W, out = a.inp(c.X, "X"), a.inp(c.W, "W", ld=C * C * 2), a.out(B, 2, M, C, name="Y")
            kern.mode_contract_fwd(X.op, W.op, out.op, B, M, C)
        elif which == "GX":
            GY, W, out = a.inp(c.GY, "GY"), a.inp(c.W, "W", ld=C * C * 2), a.out(B, 2, M, C, name="GX")
            kern.mode_contract_dgrad(GY.op, W.op, out.op, B, M, C)
        else:
            acc = which == "GWacc"
            X, GY = a.inp(c.X, "X"), a.inp(c.GY, "GY")
            out = a.inout(c.old, "GW", ld=C * C * 2) if acc else a.out(M, C, C, 2, name="GW", ld=C * C * 2)
            kern.mode_contract_wgrad(X.op, GY.op, out.op, B, M, C, acc)
        a.check()
        judge(f"{c.name} {which}", out.get(), r64[which], r32[which], _ex(existing, "mode_contract"))


# ================================================================================================ cell_mix (C = 64, csrc/rpb_cmx.hip)
CMX_SHAPES = [(32, 1, 1), (33, 3, 7), (63, 9, 32), (134, 5, 32)]
CMX_MODES = ["fwd", "fwd+bn", "fwd+bn+gelu", "oxf", "bwd", "bwd+gelu", "bwd+gelu+gz", "plain"]
CLAIM_MODES = [0, 1, 2]


CMX128_SHAPES = [(33, 3, 7), (70, 11, 32)]
CELL_FP32_SHAPES = [(18, 11, 8, 32), (13, 9, 7, 64)]               # (Wp, lines, K2, C) on csrc/rpb_cell.hip: C = 32, or lines shorter than a tile
CELL_FP32_MODES = ["fwd", "fwd+bn", "fwd+bn+gelu", "oxf", "bwd", "bwd+gelu", "plain"]     # (that kernel does not store gz)


def cmx_trip_shape(cus=MI355X_CUS):
    return (32, 8 * cus + 5, 32)


def cmx128_trip_shape(cus=MI355X_CUS):
    return (32, 4 * cus + 5, 32)


def _well_conditioned_gradient(g, s, stat, Wc, ncell, C):
    """an incoming gradient whose image g Wc carries 0.5 shat + 0.3: sum gz and sum gz shat are then sums of terms of one sign mostly,
    not of uncorrelated ones (an analytically ~0 sum has no relative error to speak of)"""
    sh = (s.double() - stat[0].double()) * stat[1].double()
    return (_rn(g, ncell, C).double() + (0.5 * sh + 0.3) @ torch.linalg.inv(Wc.double())).float()


def cmx_case(Wp, lines, K2, cus=MI355X_CUS, C=64):
    g = _gen(43, Wp, lines, K2, C)
    ncell = lines * Wp
    Wc = 0.7 * torch.eye(C) + _rn(g, C, C, scale=0.5 / math.sqrt(C))   # far from symmetric, and safely invertible
    s, stat = _rn(g, ncell, C, scale=1.5, shift=0.3), _stat(g, C)
    i = dict(dims=(Wp, lines, K2, C), x=_rn(g, ncell, C, scale=1.5, shift=0.3), Wc=Wc, bias=_rn(g, C, scale=0.3, shift=1.0),
             z2=_rn(g, lines, K2, C), GWt=_rn(g, K2, Wp, scale=1 / math.sqrt(K2)), s=s, stat=stat, ostat=_stat(g, C),
             g=_well_conditioned_gradient(g, s, stat, Wc, ncell, C))
    fp32 = C == 32 or Wp < 32                                     # rpb_cmx_supported, restated: everything else runs on rpb_cell.hip
    if fp32:                                                      # 32-cell tiles of the flat cell list; fewer waves with the BN-backward sums
        i.update(fp32=True, item=32, modes=CELL_FP32_MODES, rows=cell_fp32_rows(ncell, C, C, K2, Wp, True, False, cus),
                 rows_bwd=cell_fp32_rows(ncell, C, C, K2, Wp, True, True, cus))
    else:
        i.update(fp32=False, item=Wp, modes=CMX_MODES, rows=cmx_rows(lines, Wp, C, cus), rows_bwd=cmx_rows(lines, Wp, C, cus))

    def ref(dt):
        r = {}
        for mode in i["modes"]:
            r.update({f"{mode}:{k}": v for k, v in cmx_mode(i, mode, dt).items()})
        return r
    return Case(f"cell_mix C={C} Wp={Wp} lines={lines} K2={K2}" + (" fp32" if fp32 else ""), i, ref)


def cmx_mode(i, mode, dt):
    gelu = "gelu" in mode
    if mode.startswith("fwd"):
        return cell_mix_fwd(i["x"], i["Wc"], i["bias"], i["z2"], i["GWt"], i["stat"] + (gelu,) if "bn" in mode else None, None, i["rows"], dt,
                            i["item"])
    if mode == "oxf":
        return cell_mix_fwd(i["x"], i["Wc"], i["bias"], i["z2"], i["GWt"], i["stat"] + (True,), i["ostat"] + (True,), 0, dt)
    bnb = None if mode == "plain" else (i["s"],) + i["stat"] + (gelu,)
    return cell_mix_bwd(i["g"], i["Wc"], i["z2"], i["GWt"], bnb, mode.endswith("gz"), i["rows_bwd"], dt, item=i["item"])


def _ops_of(a, tensors, names):
    return tuple(a.inp(t, n) for t, n in zip(tensors, names))


def _opd(group):
    """an argument group of operands and flags -> what the kernel gets"""
    return None if group is None else tuple(t.op if isinstance(t, guarded.Operand) else t for t in group)


STAT_NAMES = ("mean", "invstd", "gamma", "beta")


def run_cell_mix(kern, c, mode, existing=None, with_stats=True):
    """one launch of ``mode``; forward modes without ``with_stats`` run the launch whose lines may be claimed"""
    Wp, lines, K2, C = c.dims
    ncell, gelu = lines * Wp, "gelu" in mode
    r64, r32 = c.refs()
    assert kern.cell_mix_writes_gz(ncell, C, C, K2, Wp) == (not c.fp32), f"{c.name}: not on the kernel it is meant for"
    rows = kern.cell_mix_stat_rows(ncell, C, K2, Wp, mode.startswith("bwd"))
    assert rows == (c.rows_bwd if mode.startswith("bwd") else c.rows), (rows, c.rows, c.rows_bwd)
    a = guarded.Arena(kern.dev)
    fwd = mode.startswith("fwd") or mode == "oxf"
    x, Wc, z2, GW = a.inp(c.x if fwd else c.g, "x"), a.inp(c.Wc, "Wc"), a.inp(c.z2, "z2"), a.inp(c.GWt, "GWt")
    bias = a.inp(c.bias, "bias") if fwd else None
    xf = bnb = oxf = None                                         # (operands are declared before the first .op: _opd converts at the call)
    if "bn" in mode or mode == "oxf":
        xf = _ops_of(a, c.stat, STAT_NAMES) + (gelu or mode == "oxf",)
    if mode == "oxf":
        oxf = _ops_of(a, c.ostat, STAT_NAMES) + (True,)
    if mode.startswith("bwd"):
        bnb = (a.inp(c.s, "s"),) + _ops_of(a, c.stat, STAT_NAMES) + (gelu,)
    out = a.out(ncell, C, name="out")
    stats = with_stats and mode not in ("oxf", "plain")
    part = a.out(rows, 2, C, name="part") if stats else None
    kern.cell_mix(x.op, Wc.op, bias.op if bias else None, z2.op, GW.op, out.op, part.op if part else None, ncell, C, K2, Wp,
                  transpose_w=not fwd, xf=_opd(xf), bnb=_opd(bnb), oxf=_opd(oxf), write_gz=mode.endswith("gz"))
    a.check()                                                     # every cell, and every promised partial row, is written
    tag = f"{c.name} {mode}" + ("" if stats or mode in ("oxf", "plain") else " no-stats")
    judge(tag + " out", out.get(), r64[f"{mode}:out"], r32[f"{mode}:out"], _ex(existing, "cell_mix"))
    if stats:
        p, k = part.get(), "cell_mix_stats" if fwd else "cell_mix_bnb_stats"
        idle = p[ceil_div(ncell, c.item):]
        assert not idle.any(), f"{tag}: {int((idle != 0).sum())} non-zero element(s) in the partial rows of waves without a work item"
        t64, t32 = total(r64[f"{mode}:part"]), total(r32[f"{mode}:part"])
        for j, what in enumerate(("first sums", "second sums")):
            judge(f"{tag} {what} rows={rows}", total(p)[j], t64[j], t32[j], _ex(existing, k))


# ---- the gather launch (fc1 data gradient into the padded layout) with the BatchNorm-backward sums of the last layer, csrc/rpb_cell.hip
GATHER_DIMS = (2, 3, 5, 7, 2)                                      # B, T, H, W, pad
GATHER_KC, GATHER_CO = 128, 64


def gather_case(gelu, cus=MI355X_CUS):
    B, T, H, W, pad = GATHER_DIMS
    g = _gen(48, gelu)
    KC, CO, ncrop, ncell = GATHER_KC, GATHER_CO, B * T * H * W, B * (T + pad) * (H + pad) * (W + pad)
    Wm, s, stat = _rn(g, KC, CO, scale=1 / math.sqrt(KC)), _rn(g, ncell, CO, scale=1.5, shift=0.3), _stat(g, CO)
    sh = ((s.double() - stat[0].double()) * stat[1].double()).view(B, T + pad, H + pad, W + pad, CO)[:, :T, :H, :W].reshape(ncrop, CO)
    # gu Wm carries 0.5 shat + 0.3 (the pseudo-inverse of the full-column-rank Wm): well-conditioned sums, as for the spectral launches
    gu = (_rn(g, ncrop, KC).double() + (0.5 * sh + 0.3) @ torch.linalg.pinv(Wm.double())).float()
    i = dict(gelu=gelu, gu=gu, Wm=Wm, s=s, stat=stat, rows=cell_fp32_rows(ncell, KC, CO, 0, 1, False, True, cus))
    return Case(f"cell_mix gather KC={KC} CO={CO} gelu={int(gelu)}", i,
                lambda dt: cell_mix_gather(gu, Wm, s, stat, gelu, GATHER_DIMS, i["rows"], dt))


def run_cell_mix_gather(kern, c, existing=None):
    B, T, H, W, pad = GATHER_DIMS
    KC, CO, ncell = GATHER_KC, GATHER_CO, B * (T + pad) * (H + pad) * (W + pad)
    r64, r32 = c.refs()
    rows = kern.cell_mix_gather_rows(ncell, KC, CO)
    assert rows == c.rows, (rows, c.rows)
    a = guarded.Arena(kern.dev)
    gu, Wm, s = a.inp(c.gu, "gu"), a.inp(c.Wm, "Wm"), a.inp(c.s, "s")
    st = _ops_of(a, c.stat, STAT_NAMES)
    out, part = a.out(ncell, CO, name="g"), a.out(rows, 2, CO, name="part")
    kern.cell_mix_gather(gu.op, Wm.op, out.op, part.op, ncell, KC, CO, GATHER_DIMS, _opd((s,) + st + (c.gelu,)))
    a.check()                                                     # the margin is written, and every partial row
    got = out.get()
    inside = torch.zeros(B, T + pad, H + pad, W + pad, dtype=torch.bool)
    inside[:, :T, :H, :W] = True
    margin = got.view(B, T + pad, H + pad, W + pad, CO)[~inside]
    assert not margin.view(torch.int32).any(), f"{c.name}: {int((margin.view(torch.int32) != 0).sum())} margin element(s) are not +0.0"
    judge(c.name + " g", got, r64["out"], r32["out"], _ex(existing, "cell_mix"))
    p = part.get()
    assert not p[ceil_div(ncell, 32):].any(), f"{c.name}: non-zero partial rows of waves without a tile"
    for j, what in enumerate(("sum gz", "sum gz*shat")):
        judge(f"{c.name} {what} rows={rows}", total(p)[j], total(r64["part"])[j], total(r32["part"])[j], _ex(existing, "cell_mix_bnb_stats"))


# ---- layer 0 on the feature tensor (rpb_cell_mix_feat: the bf16-pipe kernel reading FW fields per cell instead of 64 channels)
FEAT_SHAPES = [(8, 33, 3, 7), (32, 40, 5, 16)]                     # (FW, Wp, lines, K2)


def feat_case(FW, Wp, lines, K2, cus=MI355X_CUS):
    g = _gen(49, FW, Wp, lines, K2)
    C, ncell = 64, lines * Wp
    phi = _rn(g, ncell, FW, scale=1.2, shift=0.2)
    phi[:, FW - 1] = 0.0                                          # the feature tensor ends in a constant 1 and zero fields
    phi[:, FW - 2] = 1.0
    i = dict(dims=(FW, Wp, lines, K2), phi=phi, Wcomp=_rn(g, C, FW, scale=1 / math.sqrt(FW)), bias=_rn(g, C, scale=0.3, shift=1.0),
             z2=_rn(g, lines, K2, C), GWt=_rn(g, K2, Wp, scale=1 / math.sqrt(K2)), ostat=_stat(g, C), rows=cmx_stat_rows(lines, cus))

    def ref(dt):
        a = cell_mix_fwd(phi, i["Wcomp"], i["bias"], i["z2"], i["GWt"], None, None, i["rows"], dt)
        b = cell_mix_fwd(phi, i["Wcomp"], i["bias"], i["z2"], i["GWt"], None, i["ostat"] + (True,), 0, dt)
        return {"fwd:out": a["out"], "fwd:part": a["part"], "oxf:out": b["out"]}
    return Case(f"cell_mix_feat FW={FW} Wp={Wp} lines={lines} K2={K2}", i, ref)


def run_cell_mix_feat(kern, c, mode, existing=None):
    FW, Wp, lines, K2 = c.dims
    C, ncell = 64, lines * Wp
    r64, r32 = c.refs()
    rows = kern.cell_mix_stat_rows(ncell, C, K2, Wp, False)
    assert rows == c.rows, (rows, c.rows)
    a = guarded.Arena(kern.dev)
    phi, Wc, bias, z2, GW = a.inp(c.phi, "phi", ld=FW), a.inp(c.Wcomp, "Wcomp"), a.inp(c.bias, "bias"), a.inp(c.z2, "z2"), a.inp(c.GWt, "GWt")
    oxf = _ops_of(a, c.ostat, STAT_NAMES) + (True,) if mode == "oxf" else None
    out = a.out(ncell, C, name="out")
    part = a.out(rows, 2, C, name="part") if mode == "fwd" else None
    kern.cell_mix_feat(phi.op, Wc.op, bias.op, z2.op, GW.op, out.op, part.op if part else None, ncell, FW, K2, Wp, _opd(oxf))
    a.check()
    judge(f"{c.name} {mode} out", out.get(), r64[f"{mode}:out"], r32[f"{mode}:out"], _ex(existing, "cell_mix"))
    if part:
        p = part.get()
        assert not p[lines:].any(), f"{c.name}: non-zero partial rows of waves without a line"
        for j, what in enumerate(("first sums", "second sums")):
            judge(f"{c.name} {what} rows={rows}", total(p)[j], total(r64["fwd:part"])[j], total(r32["fwd:part"])[j], _ex(existing, "cell_mix_stats"))


# ================================================================================================ cell_mix_wgrad
WG_SHAPES = [(33, 3, 7), (134, 1, 32)]
WG_MODES = [(True, True), (True, False), (False, False)]                    # (gelu, write_gz)


def wg_trip_shape(cus=MI355X_CUS):
    return (32, 4 * cus + 3, 32)


def wg_case(Wp, lines, K2, gelu, write_gz, cus=MI355X_CUS):
    g = _gen(44, Wp, lines, K2, gelu, write_gz)
    C, ncell = 64, lines * Wp
    Wc = 0.7 * torch.eye(C) + _rn(g, C, C, scale=1 / 16)
    s, stat = _rn(g, ncell, C, scale=1.5, shift=0.3), _stat(g, C)
    # per-channel scales on the incoming gradient: a transposed dWc would not match
    gs = _well_conditioned_gradient(g, s, stat, Wc, ncell, C) * torch.linspace(0.5, 2.0, C)
    i = dict(dims=(Wp, lines, K2), gelu=gelu, write_gz=write_gz, gs=gs, Wc=Wc, z2=_rn(g, lines, K2, C),
             GWt=_rn(g, K2, Wp, scale=1 / math.sqrt(K2)), s=s, stat=stat, slots=cmx_wg_slots(lines, cus))
    return Case(f"cell_mix_wgrad Wp={Wp} lines={lines} K2={K2} gelu={int(gelu)} gz={int(write_gz)}", i,
                lambda dt: cell_mix_wgrad(gs, Wc, i["z2"], i["GWt"], (s,) + stat + (gelu,), write_gz, i["slots"], dt))


def run_cell_mix_wgrad(kern, c, existing=None):
    Wp, lines, K2 = c.dims
    C, ncell = 64, lines * Wp
    r64, r32 = c.refs()
    slots = kern.cell_mix_wgrad_slots(ncell, Wp)
    assert slots == c.slots, (slots, c.slots)
    a = guarded.Arena(kern.dev)
    gs, Wc, z2, GW, s = a.inp(c.gs, "gs"), a.inp(c.Wc, "Wc"), a.inp(c.z2, "z2"), a.inp(c.GWt, "GWt"), a.inp(c.s, "s")
    st = _ops_of(a, c.stat, STAT_NAMES)
    out, sp, wp = a.out(ncell, C, name="out"), a.out(slots, 2, C, name="stats_part"), a.out(slots, C, C, name="wg_part", ld=C * C)
    kern.cell_mix_wgrad(gs.op, Wc.op, z2.op, GW.op, out.op, sp.op, wp.op, ncell, K2, Wp, _opd((s,) + st + (c.gelu,)), c.write_gz)
    a.check()
    judge(c.name + " out", out.get(), r64["out"], r32["out"], _ex(existing, "cell_mix_wgrad"))
    t64, t32, tk = total(r64["part"]), total(r32["part"]), total(sp.get())
    for j, what in enumerate(("sum gz", "sum gz*shat")):
        judge(f"{c.name} {what} slots={slots}", tk[j], t64[j], t32[j], _ex(existing, "cell_mix_wgrad_stats"))
    judge(f"{c.name} dWc", total(wp.get()), total(r64["dW"]), total(r32["dW"]), _ex(existing, "cell_mix_wgrad"))


# ================================================================================================ bn_bwd_row (C = 64, csrc/rpb_bwr.hip)
BWR_SHAPES = [(1, 32, 1), (13, 22, 32), (3, 33, 7), (5, 134, 32)]
# (x operand, its transform, gelu) x (in place, out of place)
BWR_MODES = [("nox", None, True), ("nox", None, False), ("x", None, True), ("x", "bn", False), ("x", "bn+gelu", True)]
BWR_VARIANTS = [m + (inplace,) for m in BWR_MODES for inplace in (True, False)]
BWR_TRIP_VARIANTS = [("nox", None, True, True), ("x", "bn+gelu", True, True)]
# the fp32 kernel (csrc/rpb_bwd_row.hip): C = 32, where the layer input is always read; one wave per promised row
BWR32_SHAPE = (13, 22, 8)
BWR32_VARIANTS = [("x", None, True, False), ("x", "bn+gelu", False, True)]
# layer 0 (rpb_bn_bwd_row_feat, the fp32 kernel at C = 64): the weight-gradient operand is the feature tensor; (FW, gelu, gs stored in place)
BWRF_SHAPE = (3, 33, 7)
BWRF_VARIANTS = [(8, False, True), (32, True, False)]


def bwr_trip_shape(cus=MI355X_CUS):
    return (4 * cus + 3, 33, 32)


def bwr_case(G, Wp, K2, xmode, xfm, gelu, inplace, cus=MI355X_CUS, C=64, FW=0):
    """``FW`` > 0: the layer-0 form, x = the feature tensor [ncell][FW], ``inplace`` False = gs is not stored at all (gs == NULL)"""
    g = _gen(45, G, Wp, K2, len(xmode), len(xfm or ""), gelu, C, FW)
    ncell = G * Wp
    s, gy = _rn(g, ncell, C, scale=1.3, shift=0.2), _rn(g, ncell, C)
    stat = (s.double().mean(0).float(), (s.double().var(0, unbiased=False) + 1e-5).rsqrt().float()) + _stat(g, C)[2:]
    xf = None if xfm is None else _stat(g, C) + (xfm == "bn+gelu",)
    # the layer input carries a mixed copy of gy: gs^T x is then a sum of correlated terms, not sqrt(n) noise around 0 (gs has zero column
    # means), and the mixing matrix is far from symmetric, so that a transposed dWc does not match
    x = _rn(g, ncell, FW or C, shift=0.3) + 0.7 * gy @ _rn(g, C, FW or C, scale=1 / math.sqrt(C)) if xmode == "x" else None
    rows = bn_bwd_row_slots(G, cus)
    pipe = C == 64 and not FW                                     # rpb_bwr_supported, restated; else the fp32 kernel, one wave per promised row
    i = dict(dims=(G, Wp, K2), C=C, FW=FW, pipe=pipe, xmode=xmode, gelu=gelu, inplace=inplace, s=s, gy=gy, x=x,
             stat=stat, xf=xf, sums=bn_sums(s, gy, stat, gelu), GWt=_rn(g, K2, Wp, scale=1 / math.sqrt(Wp)),
             slots=bwr_slots(G, cus) if pipe else rows, rows=rows)
    what = f"feat{FW} {'gs in place' if inplace else 'gs not stored'}" if FW else f"{'in-place' if inplace else 'out-of-place'}"
    return Case(f"bn_bwd_row C={C} G={G} Wp={Wp} K2={K2} {xmode}{'+' + xfm if xfm else ''} gelu={int(gelu)} {what}", i,
                lambda dt: bn_bwd_row(s, gy, i["x"], stat, i["sums"], gelu, xf, i["GWt"], i["slots"], i["rows"], dt))


def run_bn_bwd_row(kern, c, existing=None):
    G, Wp, K2 = c.dims
    C, FW, ncell = c.C, c.FW, G * Wp
    r64, r32 = c.refs()
    rows = kern.bn_bwd_row_slots(G)
    assert rows == c.rows, (rows, c.rows)
    a = guarded.Arena(kern.dev)
    s = a.inp(c.s, "s")
    gy = a.inout(c.gy, "gy|gs") if c.inplace else a.inp(c.gy, "gy")
    x = a.inp(c.x, "x", ld=FW or C) if c.x is not None else None
    st, sums, GW = _ops_of(a, c.stat, STAT_NAMES), a.inp(c.sums, "sums"), a.inp(c.GWt.t().contiguous(), "GW")
    xf = None if c.xf is None else _ops_of(a, c.xf[:4], STAT_NAMES) + (c.xf[4],)
    gs = gy if c.inplace else (None if FW else a.out(ncell, C, name="gs"))
    unw = None
    if x is None:                                                 # include/rpb.h: the C x C block of the kernel's own rows stays unwritten
        unw = torch.zeros(rows, C * C + C, dtype=torch.bool)
        unw[:c.slots, :C * C] = True
    if FW:                                                        # include/rpb.h: the field moments fill columns 0 .. 31 of the block's rows
        unw = torch.zeros(rows, C * C + C, dtype=torch.bool)
        unw[:, :C * C].view(rows, C, C)[:, :, 32:] = True
    Y1, part = a.out(G, K2, C, name="Y1"), a.out(rows, C * C + C, name="part", unwritten=unw)
    if FW:
        kern.bn_bwd_row_feat(s.op, gy.op, x.op, gs.op if gs else None, _opd(st), sums.op, ncell, c.gelu, GW.op, Y1.op, part.op, G, Wp, C, K2, FW)
    else:
        kern.bn_bwd_row(s.op, gy.op, x.op if x else None, gs.op, _opd(st), sums.op, ncell, c.gelu, _opd(xf), GW.op, Y1.op, part.op, G, Wp, C, K2)
    a.check()                                                     # every promised row is written, the memset ones included; gy intact where gs is not stored
    if gs is not None:
        judge(c.name + " gs", gs.get(), r64["gs"], r32["gs"], _ex(existing, "bn_bwd_row"))
    judge(c.name + " Y1", Y1.get(), r64["Y1"], r32["Y1"], _ex(existing, "bn_bwd_row"))
    p = part.get()
    idle = p[min(G, c.slots):, C * C:]
    assert not idle.any(), f"{c.name}: non-zero bias sums in the partial rows of waves without a line"
    if FW:
        blk = p[:, :C * C].view(rows, C, C)
        assert not blk[:, :, FW:32].any(), f"{c.name}: the columns FW .. 31 of the field-moment block are not zero"
        judge(f"{c.name} field moments rows={rows}", total(blk[:, :, :FW]), total(r64["dW"]), total(r32["dW"]), _ex(existing, "bn_bwd_row"))
    elif x is not None:
        judge(f"{c.name} dWc rows={rows}", total(p[:, :C * C]).view(C, C), total(r64["dW"]), total(r32["dW"]), _ex(existing, "bn_bwd_row"))
    judge_against(f"{c.name} bias sums rows={rows}", total(p[:, C * C:]), total(r64["bias"]), total(r32["bias"]), r64["abs"],
                  _ex(existing, "bn_bwd_row_bias"))


# ---- width 128: the C = 64 row kernel on each 64-channel half of the 512-byte rows, no weight gradient
BWR128_SHAPES = [(7, 45, 48), (11, 70, 32)]                       # three 16-mode row tiles (K2 > 32), and two
BWR128_VARIANTS = [(True, True), (False, False)]                   # (gelu, in place)


def bwr128_case(G, Wp, K2, gelu, inplace, cus=MI355X_CUS):
    g = _gen(47, G, Wp, K2, gelu)
    C, ncell = 128, G * Wp
    s, gy = _rn(g, ncell, C, scale=1.3, shift=0.2), _rn(g, ncell, C)
    stat = (s.double().mean(0).float(), (s.double().var(0, unbiased=False) + 1e-5).rsqrt().float()) + _stat(g, C)[2:]
    i = dict(dims=(G, Wp, K2), gelu=gelu, inplace=inplace, s=s, gy=gy, stat=stat, sums=bn_sums(s, gy, stat, gelu),
             GWt=_rn(g, K2, Wp, scale=1 / math.sqrt(Wp)), slots=bwr_slots(G, cus), rows=bn_bwd_row_slots(G, cus))
    return Case(f"bn_bwd_row_c128 G={G} Wp={Wp} K2={K2} gelu={int(gelu)} {'in-place' if inplace else 'out-of-place'}", i,
                lambda dt: bn_bwd_row(s, gy, None, stat, i["sums"], gelu, None, i["GWt"], i["slots"], i["rows"], dt))


def run_bn_bwd_row_c128(kern, c, existing=None):
    G, Wp, K2 = c.dims
    C, ncell, L = 128, G * Wp, 64 * 64 + 64
    r64, r32 = c.refs()
    rows = kern.bn_bwd_row_slots(G)
    assert rows == c.rows and kern.bn_bwd_row_c128_supported(Wp, K2), (rows, c.rows)
    a = guarded.Arena(kern.dev)
    s = a.inp(c.s, "s")
    gy = a.inout(c.gy, "gy|gs") if c.inplace else a.inp(c.gy, "gy")
    st, sums, GW = _ops_of(a, c.stat, STAT_NAMES), a.inp(c.sums, "sums"), a.inp(c.GWt.t().contiguous(), "GW")
    gs = gy if c.inplace else a.out(ncell, C, name="gs")
    unw = torch.zeros(2, rows, L, dtype=torch.bool)               # per half: [64] sum gs behind an unwritten 64 x 64 block (include/rpb.h)
    unw[:, :c.slots, :64 * 64] = True
    Y1, part = a.out(G, K2, C, name="Y1"), a.out(2, rows, L, name="part", ld=L, unwritten=unw)
    kern.bn_bwd_row_c128(s.op, gy.op, gs.op, _opd(st), sums.op, ncell, c.gelu, GW.op, Y1.op, part.op, G, Wp, K2)
    a.check()
    judge(c.name + " gs", gs.get(), r64["gs"], r32["gs"], _ex(existing, "bn_bwd_row"))
    judge(c.name + " Y1", Y1.get(), r64["Y1"], r32["Y1"], _ex(existing, "bn_bwd_row"))
    p = part.get()[:, :, 64 * 64:]
    assert not p[:, min(G, c.slots):].any(), f"{c.name}: non-zero bias sums in the partial rows of waves without a line"
    judge_against(f"{c.name} bias sums rows=2x{rows}", p.double().sum(1).reshape(C), total(r64["bias"]), total(r32["bias"]), r64["abs"],
                  _ex(existing, "bn_bwd_row_bias"))


# ================================================================================================ the head (csrc/rpb_pjf.hip, rpb_pjg.hip)
HID = 128
HEAD_SHAPES = [(1, 1, 1, 1, 1, 1), (1, 2, 3, 33, 2, 2), (2, 3, 5, 32, 2, 2), (1, 2, 3, 40, 6, 3), (1, 3, 2, 7, 6, 4)]
GSCALE = 0.37


def head_slots(lines, cus=MI355X_CUS):
    """rpb_head_bwd_slots: PF_WAVES = 4 waves, one workgroup per CU; lines = B T H"""
    return _persistent(lines, 4, cus)


def head_row(DO):
    """rpb_head_bwd_row: M = gh^T shat [128][64] | d fc2.weight [DO][128] | d fc1.bias [128] | d fc2.bias [DO]"""
    return HID * 64 + DO * HID + HID + DO


def head_trip_shapes(cus=MI355X_CUS):
    """T H just above 4 CUs lines of 5 cells: three waves take a second line; fc2 width 2 (rpb_pjg.hip) and 4 (rpb_pjf.hip)"""
    return [(1, 13, (4 * cus + 3 + 12) // 13, 5, 2, DO) for DO in (2, 4)]


def head(s, stat, w1, b1, w2, b2, gout, target, dims, nslots, dt):
    """fno.py's projection head on the cropped cells, backwards: a = gamma shat + beta, u = a fc1^T + b1, out = gelu(u) fc2^T + b2;
    ``target`` given: gout = GSCALE (out - target) and loss[w] = sum (out - target)^2 over wave w's lines.  g = d/d a, scattered into the
    padded tensor (exact zeros elsewhere); part[w] = (gh^T shat | gout^T gelu(u) | sum gh | sum gout) over wave w's lines; then what
    rpb_head_bwd_finalize derives from the row sum"""
    B, T, H, W, pad, DO = dims
    Tp, Hp, Wp, C, L = T + pad, H + pad, W + pad, 64, B * T * H
    mean, invstd, gamma, beta = (t.to(dt) for t in stat)
    w1, b1, w2 = w1.to(dt), b1.to(dt), w2.to(dt)
    sh = ((s.to(dt).view(B, Tp, Hp, Wp, C)[:, :T, :H, :W] - mean) * invstd).reshape(L, W, C)
    u = (sh * gamma + beta) @ w1.t() + b1
    v = torch.nn.functional.gelu(u)
    r = {}
    if target is not None:
        diff = v @ w2.t() + b2.to(dt) - target.to(dt).view(L, W, DO)
        r["loss"] = _rows((diff * diff).sum((1, 2)), nslots)
        gout = GSCALE * diff
    else:
        gout = gout.to(dt).view(L, W, DO)
    gh = (gout @ w2) * gelu_grad(u)
    g = torch.zeros(B, Tp, Hp, Wp, C, dtype=dt)
    g[:, :T, :H, :W] = (gh @ w1).view(B, T, H, W, C)
    r["g"] = g.view(-1, C)
    per_line = torch.cat((torch.einsum("lwh,lwc->lhc", gh, sh).reshape(L, -1), torch.einsum("lwd,lwh->ldh", gout, v).reshape(L, -1),
                          gh.sum(1), gout.sum(1)), 1)
    r["part"] = _rows(per_line, nslots)
    r.update(head_finalize(r["part"].double().sum(0).to(dt), w1, gamma, beta, DO))
    return r


def head_finalize(tot, w1, gamma, beta, DO):
    M, dw2 = tot[:HID * 64].view(HID, 64), tot[HID * 64:HID * 64 + DO * HID].view(DO, HID)
    db1, db2 = tot[HID * 64 + DO * HID:HID * 64 + DO * HID + HID], tot[HID * 64 + DO * HID + HID:]
    return dict(dw1=gamma * M + beta * db1[:, None], dw2=dw2, db1=db1, db2=db2, bn_sums=torch.stack(((w1 * db1[:, None]).sum(0), (w1 * M).sum(0))))


def head_case(B, T, H, W, pad, DO, cus=MI355X_CUS):
    g = _gen(46, B, T, H, W, pad, DO)
    C, L = 64, B * T * H
    ncell = B * (T + pad) * (H + pad) * (W + pad)
    stat = _stat(g, C)
    stat[2][3], stat[3][5] = 0.0, 0.0                             # the algebra behind d fc1 / the sums must not divide by gamma
    i = dict(dims=(B, T, H, W, pad, DO), s=_rn(g, ncell, C, scale=1.2, shift=0.2), stat=stat, w1=_rn(g, HID, C, scale=1 / 8), b1=_rn(g, HID),
             w2=_rn(g, DO, HID, scale=1 / 11), b2=_rn(g, DO), gout=_rn(g, L * W, DO, shift=0.5),
             target=_rn(g, L * W, DO, shift=2.0), slots=head_slots(L, cus))         # the target is drawn independently of the output

    def ref(dt):
        a = head(i["s"], stat, i["w1"], i["b1"], i["w2"], i["b2"], i["gout"], None, i["dims"], i["slots"], dt)
        b = head(i["s"], stat, i["w1"], i["b1"], i["w2"], i["b2"], None, i["target"], i["dims"], i["slots"], dt)
        return {**{f"bwd:{k}": v for k, v in a.items()}, **{f"loss:{k}": v for k, v in b.items()}}
    return Case(f"head B={B} mesh={T}x{H}x{W} pad={pad} DO={DO}", i, ref)


def run_head(kern, c, existing=None):
    B, T, H, W, pad, DO = c.dims
    Tp, Hp, Wp, C, L = T + pad, H + pad, W + pad, 64, B * T * H
    ncell, row = B * Tp * Hp * Wp, head_row(DO)
    r64, r32 = c.refs()
    slots = kern.head_bwd_slots(c.dims)
    assert slots == c.slots and kern.head_bwd_row(DO) == row, (slots, c.slots)
    smask = c.s.clone().view(B, Tp, Hp, Wp, C)                    # the margin of the layer output is never read: it holds NaN
    inside = torch.zeros(B, Tp, Hp, Wp, dtype=torch.bool)
    inside[:, :T, :H, :W] = True
    smask[~inside] = NAN
    for which in ("bwd", "loss"):
        a = guarded.Arena(kern.dev)
        s, w1, b1, w2 = a.inp(smask, "s", ld=C), a.inp(c.w1, "w1"), a.inp(c.b1, "b1"), a.inp(c.w2, "w2")
        st = _ops_of(a, c.stat, STAT_NAMES)
        b2, other = (a.inp(c.b2, "b2"), a.inp(c.target, "target")) if which == "loss" else (None, a.inp(c.gout, "gout"))
        g, part = a.out(ncell, C, name="g"), a.out(slots, row, name="part")
        lpart = a.out(slots, name="loss_part") if which == "loss" else None
        if which == "loss":
            kern.head_fwd_bwd(s.op, w1.op, b1.op, w2.op, b2.op, other.op, GSCALE, g.op, part.op, lpart.op, c.dims, DO, _opd(st))
        else:
            kern.head_bwd(s.op, w1.op, b1.op, w2.op, other.op, g.op, part.op, c.dims, DO, _opd(st))
        a.check()                                                 # the whole padded tensor and every partial row is written
        tag, gg = f"{c.name} {which}", g.get()
        margin = gg.view(B, Tp, Hp, Wp, C)[~inside]
        assert not margin.view(torch.int32).any(), f"{tag}: {int((margin.view(torch.int32) != 0).sum())} margin element(s) are not +0.0"
        judge(tag + " g", gg, r64[f"{which}:g"], r32[f"{which}:g"], _ex(existing, "head"))
        p = part.get()
        assert not p[L:].any(), f"{tag}: non-zero partial rows of waves without a line"
        judge(f"{tag} partial rows slots={slots}", total(p), total(r64[f"{which}:part"]), total(r32[f"{which}:part"]), _ex(existing, "head"))
        if which == "loss":
            judge(tag + " loss", total(lpart.get()).reshape(1), total(r64["loss:loss"]).reshape(1), total(r32["loss:loss"]).reshape(1),
                  _ex(existing, "head"))
        # ---- the trainer's reduction and rpb_head_bwd_finalize on the kernel's own rows
        a = guarded.Arena(kern.dev)
        pin, w1, gam, bet = a.inp(p, "part"), a.inp(c.w1, "w1"), a.inp(c.stat[2], "gamma"), a.inp(c.stat[3], "beta")
        tot = a.out(row, name="tot")
        outs = dict(dw1=a.out(HID, C, name="dw1"), dw2=a.out(DO, HID, name="dw2"), db1=a.out(HID, name="db1"), db2=a.out(DO, name="db2"),
                    bn_sums=a.out(2, C, name="bn_sums"))
        kern.reduce_partials(pin.op, slots, row, tot.op)
        kern.head_bwd_finalize(tot.op, w1.op, gam.op, bet.op, DO, *(outs[k].op for k in ("dw1", "dw2", "db1", "db2", "bn_sums")))
        a.check()
        for k, o in outs.items():
            judge(f"{tag} {k}", o.get(), r64[f"{which}:{k}"], r32[f"{which}:{k}"], _ex(existing, "head_finalize"))


# ================================================================================================ every case, for the host test
def all_cases(cus=MI355X_CUS):
    out = [(axg_case, s) for s in AXG_CASES + axg_trip_cases(cus)]
    out += [(mode_case, s) for s in MODE_CASES + [mode_trip_case(cus)]]
    out += [(cmx_case, s + (cus,)) for s in CMX_SHAPES + [cmx_trip_shape(cus)]]
    out += [(cmx_case, s + (cus, 128)) for s in CMX128_SHAPES + [cmx128_trip_shape(cus)]]
    out += [(wg_case, s + m + (cus,)) for s in WG_SHAPES for m in WG_MODES] + [(wg_case, wg_trip_shape(cus) + (True, True, cus))]
    out += [(bwr_case, s + v + (cus,)) for s in BWR_SHAPES for v in BWR_VARIANTS]
    out += [(bwr_case, bwr_trip_shape(cus) + v + (cus,)) for v in BWR_TRIP_VARIANTS]
    out += [(bwr_case, BWR32_SHAPE + v + (cus, 32)) for v in BWR32_VARIANTS]
    out += [(bwr_case, BWRF_SHAPE + ("x", None, gelu, inplace, cus, 64, FW)) for FW, gelu, inplace in BWRF_VARIANTS]
    out += [(cmx_case, s[:3] + (cus, s[3])) for s in CELL_FP32_SHAPES] + [(gather_case, (gelu, cus)) for gelu in (True, False)]
    out += [(feat_case, s + (cus,)) for s in FEAT_SHAPES]
    out += [(bwr128_case, s + v + (cus,)) for s in BWR128_SHAPES for v in BWR128_VARIANTS]
    out += [(head_case, s + (cus,)) for s in HEAD_SHAPES + head_trip_shapes(cus)]
    return out
