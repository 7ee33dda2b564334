"""Host side (no GPU) of the per-kernel MWT3d tests:
* the in/out operand of tests/guarded.py trips on a stray write and on a NaN, and a cell it cannot see skipped is caught by the verdict
  -- proven with fake "kernels" written in torch on CPU arenas, as tests/test_unet_kernels_host.py does for the other operand kinds;
* every case of tests/test_gpu_mwt_kernels.py is well conditioned: 8 * e32 <= 1e-5 on every output and both measures;
* the per-launch restatements of the spectral kernel (tests/mwt_restatement.py: axis, modes, spec_out) compose to ``R.spectral``
  (``R.conv3``, ``R.head``, ``R.decompose``, ``R.reconstruct`` and ``R.lift`` rest on tests/test_mwt_host.py);
* the block, wave and tile arithmetic the shapes were chosen for, from the shapes alone;
* the cases would notice: a deliberately wrong restatement, or a fake kernel on a CPU arena, judged exactly as a kernel's output is,
  fails the bound or ``check()`` -- mutations (a) to (i) below, each for the stated reason."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import guarded                              # noqa: E402
import mwt_kernel_cases as K                # noqa: E402
import mwt_restatement as R                 # noqa: E402

F32, F64 = torch.float32, torch.float64
TOL = 1e-12                                   # fp64 against fp64
CUS = K.MI355X_CUS
C = K.C


@functools.lru_cache(maxsize=None)
def case_of(make, args):
    return make(*args)                        # the references of a case are computed once for all the tests of this file


def _past(view, n):
    """the view's storage from its first element on, ``n`` elements long -- how a kernel with a wrong bound sees its pointer"""
    return torch.as_strided(view, (n,), (1,), view.storage_offset())


def rejected(*args, **kw):
    with pytest.raises(AssertionError, match="kernel error"):
        K.judge(*args, **kw)


# ================================================================================================ the in/out operand
def _inout_arena():
    a = guarded.Arena("cpu")
    x, y = a.inp(torch.arange(12.0).view(3, 4), name="x"), a.inout(torch.full((3, 4), 10.0), name="y")
    return a, x, y


def test_inout_operand_passes_a_correct_accumulation():
    a, x, y = _inout_arena()
    assert torch.equal(y.op, torch.full((12,), 10.0))             # the kernel finds the preloaded values
    y.op[:] += 2 * x.op
    a.check()
    assert torch.equal(y.get(), 10.0 + 2 * torch.arange(12.0).view(3, 4))
    assert y.off % 4 == 0 and y.guard >= 4096


def test_inout_operand_sees_a_stray_write_next_to_it():
    a, x, y = _inout_arena()
    _past(y.op, 13)[12:] = 1.0
    with pytest.raises(AssertionError, match="guard after operand 'y'.*the first 1 element"):
        a.check()
    a, x, y = _inout_arena()
    torch.as_strided(y.op, (1,), (1,), y.op.storage_offset() - 1)[:] = 1.0
    with pytest.raises(AssertionError, match="guard before operand 'y'.*the first 1 element"):
        a.check()


def test_inout_operand_sees_a_nan():
    a, x, y = _inout_arena()
    y.op[:] += _past(x.op, 13)[1:]                                # reads one element past the input
    with pytest.raises(AssertionError, match="in/out operand 'y'.*NaN"):
        a.check()


def test_a_cell_skipped_in_an_inout_operand_is_caught_by_judge():
    """check() cannot see it (the cell keeps its preloaded value); the max-error measure does"""
    c = case_of(K.conv_case, (3, 2, 4, 11))
    r64, r32 = c.refs()
    a = guarded.Arena("cpu")
    out = a.inout(c.base, guard=K.CELL_GUARD)
    out.op.view(-1, C)[:-1] += r32["plain"].reshape(-1, C)[:-1]   # the last cell is skipped
    a.check()
    rejected(f"{c.name} acc, one cell skipped", out.get(), r64["acc"], r32["acc"])


# ================================================================================================ conditioning of the GPU cases
def _ids(v):
    return getattr(v, "__name__", None) or "-".join(str(a) for a in v)


@pytest.mark.parametrize("make,args", K.all_cases(), ids=_ids)
def test_gpu_cases_are_well_conditioned(make, args):
    case = case_of(make, args)
    r64, r32 = case.refs()
    assert set(r64) == set(r32)
    for key in r64:
        for kind, e32 in zip(K.MEASURES, K.measures(r32[key], r64[key])):
            print(f"[mwt-cases] {case.name} {key} {kind}: e32 {e32:.3e}")
            assert 8 * e32 <= K.BADLY_CONDITIONED, f"{case.name} {key}: the fp32 restatement itself is off by {e32:.3e} ({kind})"


# ================================================================================================ restatements
@pytest.mark.parametrize("Nx,Ny,T", K.LEVELS)
def test_stage_restatements_compose_to_spectral(Nx, Ny, T):
    c = case_of(K.level_case, (Nx, Ny, T))
    Wt, loT, lb = (t.double() for t in K.spectral_weights())
    ws = [K.sd()[f"MWT_CZ.0.A.weights{j}"] for j in range(1, 5)]
    want = R.spectral(c.d.double(), ws, loT.t(), lb, c.plan)
    got = R.spectral_by_stages(c.d.double(), Wt, loT, lb, c.plan)
    e = float((got - want).norm() / want.norm())
    print(f"stages against R.spectral at ({Nx},{Ny},{T}): {e:.2e}")
    assert e < TOL


def test_conv3_layouts_carry_every_weight_once():
    """the host gather of the documented lane order: every weight appears exactly once, the pad rows are zero"""
    cw, _, lw, _ = K.conv_weights("B")
    wp, lop = K.conv3_layouts(cw, lw)
    assert wp.numel() == 27 * 9 * 3 * 64 and lop.numel() == 3 * 4 * 3 * 64
    assert torch.equal(wp[wp != 0].sort().values, cw.reshape(-1)[cw.reshape(-1) != 0].sort().values)
    assert torch.equal(lop[lop != 0].sort().values, lw.reshape(-1)[lw.reshape(-1) != 0].sort().values)
    assert int((wp == 0).sum()) >= 27 * 9 * 12 * 4 and int((lop == 0).sum()) >= 3 * 4 * 3 * 64 - 36 * 36


# ================================================================================================ what the shapes reach
def test_conv_tiles_and_waves_of_the_named_shapes():
    """which 16-cell column tiles are partial and which waves are dead, from the shapes alone.  (3,1,1,9): the sample borders 8|9 and
    17|18 fall inside the first and the second column tile of one and the same wave."""
    cells = lambda s: s[0] * s[1] * s[2] * s[3]
    assert [cells(s) for s in K.CONV_SHAPES] == [8, 40, 27, 60, 8, 264, 320]
    full, dead = [16, 16, 16, 16], None
    want = [[[[8, 0, 0, 0], dead, dead, dead]],
            [[[16, 16, 8, 0], dead, dead, dead]],
            [[[16, 11, 0, 0], dead, dead, dead]],
            [[[16, 16, 16, 12], dead, dead, dead]],
            [[[8, 0, 0, 0], dead, dead, dead]],
            [[full] * 4, [[8, 0, 0, 0], dead, dead, dead]],
            [[full] * 4, [full, dead, dead, dead]]]
    assert [K.conv_waves(cells(s)) for s in K.CONV_SHAPES] == want
    B, Nx, Ny, T = K.CONV_SHAPES[0]
    assert Nx == 1 and Ny == 1                                    # every x and y tap masked
    B, Nx, Ny, T = K.CONV_SHAPES[1]
    assert (B, Nx, 2 * Nx, T) == (1, 1, Ny, 20)                   # the coarsest level of the W = 2H configs at B = 1
    B, Nx, Ny, T = K.CONV_SHAPES[2]
    assert T % 2 == 1 and 0 < (Nx * Ny * T) % 16 and {(Nx * Ny * T * b) // 16 for b in (1, 2)} == {0, 1}
    B, Nx, Ny, T = K.CONV_SHAPES[3]
    assert T == 2 and Nx & (Nx - 1) and Ny & (Ny - 1)             # every cell on a T border, neither extent a power of two
    assert K.CONV_SHAPES[4][3] == 1                               # both T taps masked everywhere
    B, Nx, Ny, T = K.CONV_SHAPES[5]
    assert (Nx * Ny * T) % 16 == 8                                # samples unaligned to the column tiles
    assert set(K.CONV_SCALED) <= set(K.CONV_SHAPES) and all(cells(s) % 16 for s in K.CONV_SCALED)
    existing = {(2, 8, 16, 8), (3, 4, 8, 10), (3, 1, 2, 8)}       # tests/test_gpu_mwt.py: all multiples of 16 cells, not repeated here
    assert not existing & set(K.CONV_SHAPES) and all(cells(s) % 16 == 0 for s in existing)


def test_spec_out_blocks_and_head_trips():
    cells = [lines * T for lines, T in K.SPEC_OUT_CASES]
    assert cells == [5, 7, 8, 20, 264]
    blocks = lambda n: [min(K.SPEC_OUT_BLOCK, n - b) for b in range(0, n, K.SPEC_OUT_BLOCK)]
    assert [blocks(n) for n in cells[:4]] == [[5], [7], [7, 1], [7, 7, 6]] and blocks(264) == [7] * 37 + [5]
    assert [m[0] * m[1] * m[2] * m[3] for m in K.HEAD_MESHES] == [5, 8, 13, 264]
    for m in K.HEAD_MESHES:                                       # one trip each, the last group ragged but for the 8 and 264 cells
        assert set(K.head_trips(m[0] * m[1] * m[2] * m[3], CUS)) == {1}
    B, Nx, Ny, T = K.head_stride_mesh(CUS)
    trips = K.head_trips(B * Nx * Ny * T, CUS)
    assert B * Nx * Ny * T == 33024 and len(trips) == 16 * CUS == 4096 and trips == [2] * 32 + [1] * 4064
    for cus in (64, 104, 228, 304):                               # some blocks take a second trip and the rest do not, for every CU count
        t = K.head_trips(129 * cus, cus)
        assert len(t) == 16 * cus and set(t) == {1, 2}
    assert B * Nx * Ny * T * C * 4 < 5e6                          # the input stays under 5 MB


def test_which_levels_overlap_their_corner_blocks():
    """every level of the GPU cases overlaps on at least one axis ((1, 1): the single row is the low and the high row at once); an axis
    of 10 or more rows does not, which the host-only level (16, 16) of mutation (e) uses"""
    assert [(K.axis_overlaps(Nx), K.axis_overlaps(Ny)) for Nx, Ny, _ in K.LEVELS] == [(True, True), (True, True), (True, True), (True, False)]
    assert [n for n in range(1, 20) if K.axis_overlaps(n)] == list(range(1, 10))
    for Nx, Ny, T in K.LEVELS + [NO_OVERLAP]:
        plan = K.LevelPlan(Nx, Ny, T, K.MODES)
        differs = not torch.equal(K.first_wins_tab(Nx, Ny), plan.tab)
        assert differs == (K.axis_overlaps(Nx) or K.axis_overlaps(Ny))
        assert 0 <= int(plan.tab.min()) and int(plan.tab.max()) < K.NAN_BLOCK and plan.tab.numel() == plan.KX * plan.KY * K.MODES
    assert [K.LevelPlan(n, n, 8, K.MODES).KX for n in (1, 8, 16)] == [1, 8, 10]          # (1, 1) has a single row


NO_OVERLAP = (16, 16, 8)


# ================================================================================================ the cases would notice
def _conv3_mutant(v, which, mode):
    cw, cb, lw, lb = K.conv_weights(which)
    B, Nx, Ny, T, _ = v.shape
    if mode == "circular_T":                                      # (a)
        x = v.permute(0, 4, 1, 2, 3)
        x = F.pad(torch.cat([x[..., -1:], x, x[..., :1]], -1), (0, 0, 1, 1, 1, 1))
        h = F.conv3d(x, cw, cb)
    elif mode == "next_sample":                                   # (b): the x border of a sample is no border
        h = F.conv3d(v.reshape(1, B * Nx, Ny, T, C).permute(0, 4, 1, 2, 3), cw, cb, padding=1)
    elif mode == "pad_reads_cell_0":                              # (a): the masked lanes keep what they loaded (cell 0 of the tensor)
        bb, xx, yy, tt = torch.meshgrid(torch.arange(B), torch.arange(Nx), torch.arange(Ny), torch.arange(T), indexing="ij")
        taps = []
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dt in (-1, 0, 1):
                    ok = (xx + dx >= 0) & (xx + dx < Nx) & (yy + dy >= 0) & (yy + dy < Ny) & (tt + dt >= 0) & (tt + dt < T)
                    taps.append(torch.where(ok, ((bb * Nx + xx + dx) * Ny + yy + dy) * T + tt + dt, 0))
        nb = v.reshape(-1, C)[torch.stack(taps, -1)]              # [B][Nx][Ny][T][27 taps][ci]
        h = (torch.einsum("bxytkc,ock->bxyto", nb, cw.reshape(C, C, 27)) + cb).permute(0, 4, 1, 2, 3)
    h = F.relu(h).permute(0, 2, 3, 4, 1).reshape(B, Nx, Ny, T, C)
    return F.linear(h, lw, lb)


@pytest.mark.parametrize("shape", K.CONV_SHAPES, ids=K.CONV_IDS)
def test_mutations_a_b_c_g_of_the_convolution(shape):
    B, Nx, Ny, T = shape
    c = case_of(K.conv_case, shape)
    r64, r32 = c.refs()
    # (a) circular instead of zero padding along T: what deleting the ``ok ?`` select on the pad would amount to
    bad = _conv3_mutant(c.v, "B", "circular_T")
    rejected(f"(a) {c.name}", bad, r64["plain"], r32["plain"])
    rejected(f"(a) {c.name} acc", bad + c.base, r64["acc"], r32["acc"])
    bad = _conv3_mutant(c.v, "B", "pad_reads_cell_0")            # ... and that deletion itself, restated: every cell here has a masked tap
    rejected(f"(a) {c.name}, pad = cell 0", bad, r64["plain"], r32["plain"])
    # (b) the x neighbour of a border cell reads the next sample: wrong wherever there is a next sample
    bad = _conv3_mutant(c.v, "B", "next_sample")
    if B > 1:
        rejected(f"(b) {c.name}", bad, r64["plain"], r32["plain"])
    else:
        K.judge(f"(b) {c.name} (one sample: the same operator)", bad, r64["plain"], r32["plain"])
    # (c) the last ncell % 16 cells left unwritten: what a tile-granular store guard would do
    ncell, tail = B * Nx * Ny * T, (B * Nx * Ny * T) % 16
    a = guarded.Arena("cpu")
    out = a.out(B, Nx, Ny, T, C, guard=K.CELL_GUARD)
    out.op.view(-1, C)[:ncell - tail] = r32["plain"].reshape(-1, C)[:ncell - tail]
    if tail:
        with pytest.raises(AssertionError, match=f"{tail * C} element.s. were never written, the first at flat index {(ncell - tail) * C}"):
            a.check()
        a = guarded.Arena("cpu")                                  # ... and in the accumulating call, where check() cannot see it
        out = a.inout(c.base, guard=K.CELL_GUARD)
        out.op.view(-1, C)[:ncell - tail] += r32["plain"].reshape(-1, C)[:ncell - tail]
        a.check()
        rejected(f"(c) {c.name} acc", out.get(), r64["acc"], r32["acc"])
    else:
        assert shape == (1, 4, 4, 20)
        a.check()
    # (g) overwriting where it should accumulate
    rejected(f"(g) {c.name} acc", r32["plain"], r64["acc"], r32["acc"])


@pytest.mark.parametrize("shape", [s for s in K.DR_SHAPES if s[2] in K.BROADCAST_NY])
def test_mutation_d_reconstruct_ignores_the_broadcast(shape):
    """reads column y of a one-column x: rows of the next x line, and past the end of x at the last lines"""
    B, Nx, Ny, T = shape
    c = case_of(K.dr_case, shape)
    r64, r32 = c.refs()
    a = guarded.Arena("cpu")
    x, out = a.inp(c.xb, guard=K.CELL_GUARD), a.out(B, 2 * Nx, 2 * Ny, T, C, guard=K.fine_guard(Ny, T))
    bb, xx, y, t = torch.meshgrid(torch.arange(B), torch.arange(Nx), torch.arange(Ny), torch.arange(T), indexing="ij")
    xq = ((bb * Nx + xx) * 1 + y) * T + t                         # the kernel has (xNy == Ny ? y : 0) for y
    rows = _past(x.op, (int(xq.max()) + 1) * C).view(-1, C)[xq]
    out.op[:] = R.reconstruct(rows, c.us, c.ud, c.rc, False).reshape(-1)
    with pytest.raises(AssertionError, match="NaN"):
        a.check()
    inside = R.reconstruct(c.xb.reshape(-1, C)[xq.clamp(max=B * Nx * T - 1)], c.us, c.ud, c.rc, False)     # the reads that stay inside x
    rejected(f"(d) {c.name}", inside, r64["rec_xb_relu0"], r32["rec_xb_relu0"])


@pytest.mark.parametrize("level", K.LEVELS + [NO_OVERLAP], ids=str)
def test_mutation_e_modes_take_the_first_corner_assignment(level):
    Nx, Ny, T = level
    c = case_of(K.level_case, (Nx, Ny, T) + ((1,) if level == NO_OVERLAP else ()))
    r64, r32 = c.refs()
    Wt = K.spectral_weights()[0]
    bad = R.modes(c.ins["modes"], Wt, K.first_wins_tab(Nx, Ny), c.B, c.NB)
    if K.axis_overlaps(Nx) or K.axis_overlaps(Ny):
        rejected(f"(e) {c.name} modes", bad, r64["modes"], r32["modes"])
    else:
        assert level == NO_OVERLAP
        K.judge(f"(e) {c.name} modes (no overlap: the same table)", bad, r64["modes"], r32["modes"])


@pytest.mark.parametrize("Cout,r", K.HEAD_DOUT)
def test_mutation_f_head_writes_j_T_plus_t(Cout, r):
    B, Nx, Ny, T = mesh = K.HEAD_MESHES[-1]
    c = case_of(K.head_case, (*mesh, Cout, r))
    r64, r32 = c.refs()
    y = r32["out"].reshape(B, T, r, Nx, Ny, Cout)                 # out[b][t r + j][x][y][co]
    bad = y.permute(0, 2, 1, 3, 4, 5).reshape(B, r * T, Nx, Ny, Cout)          # ... written at j T + t
    if r > 1:
        rejected(f"(f) {c.name}", bad, r64["out"], r32["out"])
    else:
        K.judge(f"(f) {c.name} (r = 1: the same index)", bad, r64["out"], r32["out"])


@pytest.mark.parametrize("lines,T", K.SPEC_OUT_CASES)
def test_mutation_g_spec_out_overwrites(lines, T):
    c = case_of(K.spec_out_case, (lines, T))
    r64, r32 = c.refs()
    rejected(f"(g) {c.name} acc", r32["out"], r64["acc"], r32["acc"])


def test_mutation_h_head_without_the_second_trip():
    """the cells of the second grid-stride trip are never written"""
    B, Nx, Ny, T = mesh = K.head_stride_mesh(CUS)
    Cout, r = K.HEAD_STRIDE_DOUT
    c = case_of(K.head_case, (*mesh, Cout, r))
    r64, r32 = c.refs()
    first = 16 * CUS * 8                                          # cells of the first trip
    cell = torch.arange(B * Nx * Ny * T).reshape(B, Nx, Ny, T, 1, 1).expand(B, Nx, Ny, T, Cout, r)
    done = (cell < first).permute(0, 3, 5, 1, 2, 4).reshape(B, T * r, Nx, Ny, Cout)           # the output permute of R.head
    a = guarded.Arena("cpu")
    out = a.out(B, T * r, Nx, Ny, Cout)
    out.op[done.reshape(-1)] = r32["out"].reshape(-1)[done.reshape(-1)]
    missing = (B * Nx * Ny * T - first) * Cout * r
    with pytest.raises(AssertionError, match=f"{missing} element.s. were never written"):
        a.check()
    a = guarded.Arena("cpu")
    out = a.out(B, T * r, Nx, Ny, Cout)
    out.op[:] = r32["out"].reshape(-1)
    a.check()
    K.judge(f"{c.name} (the fp32 restatement itself)", out.get(), r64["out"], r32["out"])


def test_mutation_i_one_wrong_tap_weight_in_one_border_cell():
    """passes the old global Rel-L2 < 1e-5 and fails the max-error measure: why there are two measures"""
    shape = B, Nx, Ny, T = (3, 2, 4, 11)
    c = case_of(K.conv_case, shape)
    r64, r32 = c.refs()
    cw, cb, lw, lb = K.conv_weights("B")
    cw2 = cw.clone()
    cw2[:, :, 1, 1, 2] *= 1 + 2.0 ** -13                          # the tap (0, 0, +1), every channel pair
    wrong = R.conv3(c.v, cw2, cb, lw, lb)
    bad = r32["plain"].clone()
    bad[1, 0, 3, 0] = wrong[1, 0, 3, 0]                           # one cell on the x, y and T border of the second sample
    rel, mx = K.measures(bad, r64["plain"])
    print(f"(i) one cell with a wrong tap weight: rel-l2 {rel:.3e}, max-abs {mx:.3e}")
    assert rel < 1e-5 and mx > K.bound_of(K.measures(r32["plain"], r64["plain"])[1])
    rejected(f"(i) {c.name}", bad, r64["plain"], r32["plain"])
