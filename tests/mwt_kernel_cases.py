"""TEST INFRASTRUCTURE ONLY -- the shapes, inputs, references and the verdict of the per-kernel MWT3d tests, shared by
tests/test_gpu_mwt_kernels.py (which runs the HIP kernels of csrc/rpb_mwt.hip and csrc/rpb_mwt3x.hip on them) and
tests/test_mwt_kernels_host.py (which checks, without a GPU, that every case is well conditioned, that the shapes reach the paths they
were chosen for and that a wrong formula would be noticed).  ``Case`` is that of tests/unet_kernel_cases.py, the verdict that of
tests/kernel_verdict.py.

Inputs are uniform in (-1, 1) from seeded generators, the seeds of tests/test_gpu_mwt.py; weights are those of its case "a"
(``MWT_CZ.0.{A,B,C}.*``, ``Lk``) and the filter maps of ``cz_buffers(3)``.  Where a shape needs a weight the fixture has not (a lift
from Cin != 3, a coarse map of another K, the head) it is seeded uniform as well.  References are the functions of
tests/mwt_restatement.py in fp64 and in fp32.

The verdict: every output against the fp64 restatement on Rel-L2 and on max |error| / max |reference|, bound max(8 * e32, floor), e32 the
same measure of the fp32 restatement; floor 1e-6, and 2e-6 for "f16x2", which drops a term of at most 2^-22 |a b| per product (the
bound tests/test_gpu_mwt_arith.py asserts for that kernel); "bf16x3" forms exact fp32 products and gets the fp32 rule.  A case with
8 * e32 > 1e-5 is rejected as badly conditioned.  ``EXISTING_BOUND`` is what another test already asserts for a kernel, for the
``EXISTING`` table of the GPU test."""
import functools
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import mwt_common as MC                      # noqa: E402
import mwt_restatement as R                  # noqa: E402
from kernel_verdict import BADLY_CONDITIONED, MEASURES, bound_of, measures, verdict          # noqa: E402,F401
from unet_kernel_cases import F32, F64, MI355X_CUS, Case                                      # noqa: E402,F401
from realpdebench_amd.model.mwt import LevelPlan, cz_buffers                                  # noqa: E402

C = 36
MODES = 5
FLOOR = {"f32": 1e-6, "bf16x3": 1e-6, "f16x2": 2e-6}
EXISTING_BOUND = {"f32": 1e-5, "bf16x3": 1e-5, "f16x2": 2e-6}      # tests/test_gpu_mwt.py, tests/test_gpu_mwt_arith.py
PLANES = {"bf16x3": 3, "f16x2": 2}


def judge(name, got, ref64, ref32, existing=None, floor=1e-6):
    """``got`` against the fp64 restatement on both measures; prints every figure before it asserts"""
    assert tuple(got.shape) == tuple(ref64.shape), (name, got.shape, ref64.shape)
    verdict("mwt-kernels", name, zip(MEASURES, measures(ref32, ref64), measures(got, ref64)), existing, floor)


def _u(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


@functools.lru_cache(maxsize=None)
def sd():
    shape_in, shape_out, nCZ, _ = MC.CASES["a"]
    return MC.seeded_weights(shape_in, shape_out, nCZ)


# ================================================================================================ guard sizes
# an operand addressed by cell: a kernel that mistakes its cell count by a whole wave (64 cells of 36 floats) must still land in the guard
CELL_GUARD = 64 * C + 1024


def fine_guard(Ny, T):
    """the ``x`` of decompose and the ``out`` of reconstruct, addressed on the fine grid [2Nx][2Ny][T][36]: a kernel that mistakes a
    fine row index by two (one coarse row) must still land in the guard"""
    return max(CELL_GUARD, 2 * 2 * Ny * T * C)


# ================================================================================================ conv3 / conv3x
CONV_SHAPES = [(1, 1, 1, 8), (1, 1, 2, 20), (3, 1, 1, 9), (2, 3, 5, 2), (2, 2, 2, 1), (3, 2, 4, 11), (1, 4, 4, 20)]
CONV_IDS = ["one-partial-tile", "native-coarsest-W=2H", "odd-T-two-sample-borders-in-a-tile", "non-pow2-T=2", "T=1", "full-block+8-cells",
            "full-last-wave"]
CONV_SCALED = [(3, 1, 1, 9), (3, 2, 4, 11)]                          # conv3x also runs the zero input and two input scales here
SCALES = (("x2^-20", 2.0 ** -20), ("x2^12", 2.0 ** 12))             # those of tests/test_gpu_mwt_arith.py


def conv_weights(which="B"):
    p = f"MWT_CZ.0.{which}."
    return tuple(sd()[p + n].float().contiguous() for n in ("conv.0.weight", "conv.0.bias", "Lo.weight", "Lo.bias"))


def conv_case(B, Nx, Ny, T, which="B"):
    v, base = _u(3, B, Nx, Ny, T, C), _u(4, B, Nx, Ny, T, C)
    i = dict(v=v, base=base)

    def ref(dt):
        w = [t.to(dt) for t in conv_weights(which)]
        plain = R.conv3(v.to(dt), *w)
        out = dict(plain=plain, acc=plain + base.to(dt))
        if (B, Nx, Ny, T) in CONV_SCALED:
            out["zero"] = R.conv3(torch.zeros_like(v, dtype=dt), *w)
            for tag, s in SCALES:
                out[tag] = R.conv3((v * s).to(dt), *w)
        return out
    return Case(f"conv3[{which}] ({B},{Nx},{Ny},{T})", i, ref)


def conv_waves(ncell):
    """[block][wave] -> the number of valid cells in each of the wave's four 16-cell column tiles, or None for a wave that exits early
    (mwt_conv3_k / mwt_conv3x_k: 256 threads = 4 waves of 64 consecutive cells)"""
    out = []
    for b in range((ncell + 255) // 256):
        out.append([None if (b * 4 + w) * 64 >= ncell else [max(0, min(16, ncell - (b * 4 + w) * 64 - 16 * n)) for n in range(4)]
                    for w in range(4)])
    return out


def conv3_layouts(cw, lw):
    """the documented lane-order layouts of rpb_mwt_conv3_wprep as a host gather: wp [27 taps][9 j][3 row tiles][64 lanes] holds
    w[co = 16 t + (lane & 15)][ci = 9 (lane >> 4) + j][tap], lop [3 t][4 r][3 u][64] holds lo[o = 16 u + (lane & 15)][c = 16 t +
    4 (lane >> 4) + r]; zeros on the pad rows 36..47"""
    w = cw.reshape(C, C, 27)
    i = torch.arange(27 * 9 * 3 * 64)
    lane, t, j, tap = i & 63, (i >> 6) % 3, (i // 192) % 9, i // (192 * 9)
    co, ci = 16 * t + (lane & 15), 9 * (lane >> 4) + j
    wp = torch.where(co < C, w[co.clamp(max=C - 1), ci, tap], torch.zeros(()))
    k = torch.arange(3 * 4 * 3 * 64)
    lane, u, r, t = k & 63, (k >> 6) % 3, (k // 192) % 4, k // (192 * 4)
    o, c = 16 * u + (lane & 15), 16 * t + 4 * (lane >> 4) + r
    lop = torch.where((o < C) & (c < C), lw[o.clamp(max=C - 1), c.clamp(max=C - 1)], torch.zeros(()))
    return wp.contiguous(), lop.contiguous()


def cb48(cb):
    out = torch.zeros(48)
    out[:C] = cb
    return out


# ================================================================================================ lift
LIFT_SHAPES = [(2, 3, 2, 5, 3), (1, 2, 4, 2, 5), (1, 1, 2, 2, 16), (2, 2, 2, 2, 1), (1, 2, 2, 2, 64)]       # (B, T, H, W, Cin)
LIFT_REFUSED_CIN = 65


def lift_case(B, T, H, W, Cin):
    w = sd()["Lk.weight"].float() if Cin == 3 else _u(14, C, Cin) * Cin ** -0.5
    i = dict(x=_u(1, B, T, H, W, Cin), w=w.contiguous(), b=sd()["Lk.bias"].float())
    return Case(f"lift ({B},{T},{H},{W},{Cin})", i, lambda dt: dict(out=R.lift(i["x"].to(dt), i["w"].to(dt), i["b"].to(dt))))


# ================================================================================================ decompose / reconstruct
DR_SHAPES = [(1, 1, 1, 8), (3, 1, 2, 9), (2, 2, 4, 11), (2, 3, 5, 2)]           # output level (B, Nx, Ny, T) of decompose, input level of reconstruct
BROADCAST_NY = (2, 4)


def rc_maps():
    buf = cz_buffers(3)
    return torch.stack([buf["rc_ee"], buf["rc_eo"], buf["rc_oe"], buf["rc_oo"]]).contiguous()


def dr_case(B, Nx, Ny, T):
    buf = cz_buffers(3)
    i = dict(h=_u(2, B, 2 * Nx, 2 * Ny, T, C), us=_u(5, B, Nx, Ny, T, C), ud=_u(6, B, Nx, Ny, T, C), x=_u(7, B, Nx, Ny, T, C),
             ec_d=buf["ec_d"].contiguous(), ec_s=buf["ec_s"].contiguous(), rc=rc_maps())
    if Ny in BROADCAST_NY:
        i["xb"] = _u(7, B, Nx, 1, T, C)

    def ref(dt):
        d, s = R.decompose(i["h"].to(dt), i["ec_d"].to(dt), i["ec_s"].to(dt))
        out = dict(d=d, s=s)
        for key in ("x", "xb"):
            if key in i:
                for relu in (0, 1):
                    out[f"rec_{key}_relu{relu}"] = R.reconstruct(i[key].to(dt), i["us"].to(dt), i["ud"].to(dt), i["rc"].to(dt), bool(relu))
        return out
    return Case(f"decompose/reconstruct ({B},{Nx},{Ny},{T})", i, ref)


# ================================================================================================ coarse
COARSE_CASES = [(K, rows) for K in (36, 72, 144) for rows in (1, 9, 40)]
COARSE_REFUSED_K = 40


def coarse_case(K, rows):
    i = dict(x=_u(8, rows, K), w=_u(9, C, K), b=sd()["MWT_CZ.0.A.Lo.bias"].float())
    # R.coarse reads [B][1][mult][T][36] as rows of K = 36 mult floats in row-major order: the flat buffer of ``rows`` rows, B = 1
    return Case(f"coarse K={K} rows={rows}", i,
                lambda dt: dict(out=R.coarse(i["x"].to(dt).reshape(1, 1, K // C, rows, C), i["w"].to(dt), i["b"].to(dt)).reshape(rows, C)))


# ================================================================================================ axis, modes, spec_out
AXIS_CASES = [(11, 3, 5, 7), (1, 1, 1, 1)]                           # (outer, O, K, inner)


def axis_case(outer, O, K, inner):
    i = dict(x=_u(20, outer, K, inner), M=_u(21, O, K))
    return Case(f"axis ({outer},{O},{K},{inner})", i, lambda dt: dict(out=R.axis(i["x"].to(dt).reshape(-1), i["M"].to(dt), outer, inner)))


LEVELS = [(1, 1, 8), (1, 2, 20), (2, 4, 11), (8, 16, 8)]             # (Nx, Ny, T) of a spectral level
LEVEL_B = 2
STAGES = ("FT", "FY", "FX", "modes", "GX", "GY", "spec_out")        # the seven launches of MWT3d.k_spectral, in order
NAN_BLOCK = 500                                                      # the extra weight block a stray ``tab`` entry would select


@functools.lru_cache(maxsize=None)
def spectral_weights():
    """(Wt [500][36 in][36 out][2], loT [36 in][36 out], lb) of kernel A, as MWT3d._build_prep lays them out"""
    ws = [sd()[f"MWT_CZ.0.A.weights{j}"] for j in range(1, 5)]
    Wt = torch.view_as_real(torch.stack(ws).permute(0, 3, 4, 5, 1, 2).contiguous()).reshape(4 * MODES ** 3, C, C, 2).float().contiguous()
    return Wt, sd()["MWT_CZ.0.A.Lo.weight"].float().t().contiguous(), sd()["MWT_CZ.0.A.Lo.bias"].float().contiguous()


def axis_overlaps(n, modes=MODES):
    """the low rows [:l] and the high rows [-l:] of a two-sided axis of length n share a row"""
    return n < 2 * min(modes, n // 2 + 1)


def first_wins_tab(Nx, Ny, modes=MODES):
    """the corner table with the FIRST, not the last, of the four sequential assignments winning where they overlap (mutation (e))"""
    def rows(n):
        l = min(modes, n // 2 + 1)
        return [(0, r) if r < l else (1, r - (n - l)) for r in sorted(set(range(l)) | set(range(n - l, n)))]
    tab = [[(hx + 2 * hy) * modes ** 3 + (ix * modes + iy) * modes + kt for kt in range(modes)] for hx, ix in rows(Nx) for hy, iy in rows(Ny)]
    return torch.tensor(tab, dtype=torch.int32).reshape(-1)


def level_case(Nx, Ny, T, B=LEVEL_B):
    """every launch of k_spectral on its own: a later stage takes the fp64 result of the earlier one rounded to fp32 (``ins[stage]``)"""
    plan = LevelPlan(Nx, Ny, T, MODES)
    Wt, loT, lb = spectral_weights()
    d, base = _u(3, B, Nx, Ny, T, C), _u(4, B, Nx, Ny, T, C)
    keep = []
    R.spectral_by_stages(d.double(), Wt.double(), loT.double(), lb.double(), plan, keep)
    ins = dict(zip(STAGES, [d.reshape(-1)] + [t.float() for t in keep[:-1]]))
    NB, calls = plan.KX * plan.KY * MODES, R.spectral_stage_calls(B, plan)
    i = dict(d=d, base=base, plan=plan, ins=ins, NB=NB, calls=dict(zip(("FT", "FY", "FX", "GX", "GY"), calls)), B=B)

    def ref(dt):
        out = {}
        for name, outer, inner in calls:
            out[name] = R.axis(ins[name].to(dt), getattr(plan, name).to(dt), outer, inner)
        out["modes"] = R.modes(ins["modes"].to(dt), Wt.to(dt), plan.tab, B, NB)
        out["spec_out"] = R.spec_out(ins["spec_out"].to(dt), plan.GT.to(dt), loT.to(dt), lb.to(dt), B * Nx * Ny, T)
        out["spec_out_acc"] = out["spec_out"] + base.to(dt).reshape(-1, C)
        return out
    return Case(f"spectral level ({Nx},{Ny},{T}) B={B}", i, ref)


SPEC_OUT_CASES = [(1, 5), (7, 1), (1, 8), (2, 10), (24, 11)]         # (lines, T): 5, 7, 8, 20 and 264 cells around the 7 cells of a block
SPEC_OUT_BLOCK = 7


def spec_out_case(lines, T, K2=2 * MODES):
    _, loT, lb = spectral_weights()
    i = dict(S=_u(30, lines, K2, C), GT=_u(31, T, K2), base=_u(4, lines * T, C), K2=K2)

    def ref(dt):
        out = R.spec_out(i["S"].to(dt), i["GT"].to(dt), loT.to(dt), lb.to(dt), lines, T)
        return dict(out=out, acc=out + i["base"].to(dt))
    return Case(f"spec_out lines={lines} T={T}", i, ref)


# ================================================================================================ head
HEAD_DOUT = [(3, 1), (2, 2), (16, 1)]                                # (Cout, r)
HEAD_MESHES = [(1, 1, 1, 5), (1, 2, 2, 2), (1, 13, 1, 1), (3, 2, 4, 11)]        # 5, 8, 13 and 264 cells
HEAD_STRIDE_DOUT = (2, 2)


def head_stride_mesh(cus):
    """129 CUs cells: ceil(129 CUs / 8) groups of 8 cells exceed the 16 CUs blocks of the grid for every CU count, so the first blocks of
    mwt_head_k take a second grid-stride trip and the rest do not"""
    return (1, 43, cus, 3)


def head_trips(ncell, cus):
    """trip count of every block of mwt_head_k"""
    blocks = min((ncell + 7) // 8, 16 * cus)
    return [len(range(b * 8, ncell, blocks * 8)) for b in range(blocks)]


def head_case(B, Nx, Ny, T, Cout, r):
    i = dict(v=_u(3, B, Nx, Ny, T, C), w0=_u(10, 128, C) * 0.3, b0=_u(11, 128), w1=(_u(12, Cout * r, 128) * 0.2).contiguous(),
             b1=_u(13, Cout * r))
    i["w0t"] = i["w0"].t().contiguous()

    def ref(dt):
        return dict(out=R.head(i["v"].to(dt), i["w0"].to(dt), i["b0"].to(dt), i["w1"].to(dt), i["b1"].to(dt), (T, Nx, Ny, 3),
                               (T * r, Nx, Ny, Cout)))
    return Case(f"head ({B},{Nx},{Ny},{T}) Cout={Cout} r={r}", i, ref)


def all_cases(cus=MI355X_CUS):
    """(case constructor, arguments) of every GPU case, for the host tests"""
    out = [(conv_case, s) for s in CONV_SHAPES] + [(conv_case, (3, 2, 4, 11, "C"))] + [(lift_case, s) for s in LIFT_SHAPES]
    out += [(dr_case, s) for s in DR_SHAPES] + [(coarse_case, s) for s in COARSE_CASES] + [(axis_case, s) for s in AXIS_CASES]
    out += [(level_case, s) for s in LEVELS] + [(spec_out_case, s) for s in SPEC_OUT_CASES]
    out += [(head_case, (*m, *d)) for m in HEAD_MESHES for d in HEAD_DOUT] + [(head_case, (*head_stride_mesh(cus), *HEAD_STRIDE_DOUT))]
    return out
