"""Host side (no GPU) of the per-kernel tests of the DeepONet evaluation kernels (tests/deeponet_kernel_cases.py):
* every case of tests/test_gpu_deeponet_kernels.py is well conditioned: the drivers run here on ``TorchKernels``, a torch stand-in for
  the library on CPU arenas that computes the fp32 restatement FROM THE OPERANDS THE KERNEL GETS -- the point MLP's weights decoded
  from their bf16 / fp16 planes in lane order, the pool's folded (sc, sh) --, and the verdict rejects a case whose 8 * e32 exceeds 1e-5;
* the planes decode to the weights they were made from (bf16: exactly; fp16: to 2^-21), through the inverse of the lane permutations;
* the restated pool grid takes its second trip at the MI355X's 256 compute units, and stage 1 at native shape does from B = 4 up;
* the drivers would notice: with ONE wrong term or ONE out-of-range access the stand-in trips ``Arena.check()``, a bit comparison or
  the verdict in at least one case of its kernel -- the same driver code the GPU test runs."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import deeponet_kernel_cases as K            # noqa: E402
import deeponet_restatement as R             # noqa: E402

F32, F64 = torch.float32, torch.float64
CUS = K.MI355X_CUS


def _past_the_end(t, n, count=1):
    """elements ``n .. n + count - 1`` of a flat operand view of ``n`` elements: the first elements of the guard behind it"""
    return t.as_strided((n + count,), (1,))[n:]


def _planes(z, half):
    """int32 pairs -> the fp64 values of the int16 planes"""
    h = z.view(torch.int16)
    return h.view(torch.float16).double() if half else (h.to(torch.int32) << 16).view(F32).double()


def decode_point_weights(w, sc, p, cout):
    """(W1, b1, W2, b2, W3, b3) from the kernel's operands: the planes summed, the lane order of ``point_weights`` inverted"""
    w1z, b1z, w2z, b2z, w3z, b3 = w
    half = sc is not None
    npl, KS = (2 if half else 3), p // 16
    s = [float(sc[i]) for i in range(3)] if half else [1.0] * 3
    w1 = (_planes(w1z[:16 * KS * npl * 256], half).view(16, KS, npl, 64, 8).sum(2) * s[0]).float()
    w2 = (_planes(w2z[:16 * 8 * npl * 256], half).view(16, 2, 4, npl, 64, 8).sum(3) * s[1]).float()
    w3 = (_planes(w3z[:8 * npl * 256], half).view(4, 2, npl, 64, 8).sum(2) * s[2]).float()
    W1 = w1.reshape(16, KS, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(512, p)
    W2 = w2.reshape(16, 2, 4, 2, 32, 2, 4).permute(2, 4, 0, 1, 5, 3, 6).reshape(128, 512)
    W3 = w3.reshape(4, 2, 2, 32, 2, 4).permute(3, 0, 1, 4, 2, 5).reshape(32, 128)[:cout]
    regs = lambda b, tiles: b[:tiles * 32].view(tiles, 2, 4, 4).permute(0, 2, 1, 3).reshape(-1)
    return W1, regs(b1z, 16), W2, regs(b2z, 4), W3, b3[:cout]


def _adaptive(y, floor):
    """R.adaptive_pool; ``floor``: the wrong upper bin edge"""
    B, T, H, W, C = y.shape
    bins = (lambda n: [(i * n // 4, (i + 1) * n // 4) for i in range(4)]) if floor else (lambda n: R.bins(n, 4))
    out = torch.empty(B, 1, 4, 4, C, dtype=y.dtype)
    for i, (h0, h1) in enumerate(bins(H)):
        for j, (w0, w1) in enumerate(bins(W)):
            out[:, 0, i, j] = y[:, :, h0:h1, w0:w1].mean(dim=(1, 2, 3))
    return out


class TorchKernels:
    """the entry points the drivers call, in fp32 torch on the views of CPU arenas; ``mut`` = one wrong term or out-of-range access"""
    dev = "cpu"

    def __init__(self, mut=None, cus=CUS):
        self.mut, self.cus = mut, cus

    def don_point_mlp(self, t, b, w, sc, out, B, N, p, cout):
        ws = decode_point_weights(w, sc, p, cout)
        tv = t[:N * p].view(N, p)
        if self.mut == "row_N_of_t_read":                         # the tail clamps to row N instead of N - 1
            tv = torch.cat((tv[:N - 1], t.as_strided((N + 1, p), (p, 1))[N:]))
        r = R.point_mlp(K.AH.sd_of(ws), tv, b[:B * p].view(B, p))
        ov = out[:B * N * cout].view(B, N, cout)
        if self.mut == "last_tail_point_unwritten":
            ov[:, :N - 1] = r[:, :N - 1]
        else:
            ov[:] = r
        if self.mut == "column_C_out_written":                    # of the last point: the float behind the operand
            _past_the_end(out, B * N * cout)[:] = 0.0

    def don_trunk(self, axes, wb, out, T, H, W, p):
        N = T * H * W
        grid = torch.stack(torch.meshgrid(axes[0][:T], axes[1][:H], axes[2][:W], indexing="ij"), -1).reshape(N, 3)
        if self.mut == "H_and_W_axes_swapped":
            grid = grid[:, [0, 2, 1]]
        layers = [(wb[2 * i][:k * n].view(k, n).t(), wb[2 * i + 1][:n]) for i, (k, n) in enumerate(((3, 64), (64, 128), (128, p)))]
        r = R._mlp(grid, layers)
        out[:N * p] = r.reshape(-1)
        if self.mut == "tail_point_written_at_row_N":
            _past_the_end(out, N * p, p)[:] = r[-1]

    def don_bn_relu_pool(self, x, sc, sh, out, B, T, H, W, C, ldx, ldo, mode):
        if mode == 0 and min(T, H, W) < 2:
            raise RuntimeError(f"don_bn_relu_pool: mode={mode} with T={T} H={H} W={W} (MaxPool3d(2) needs extents >= 2)")
        xv = x[:B * T * H * W * ldx].view(B, T, H, W, ldx)
        y = F.relu(xv[..., :C] * sc[:C] + sh[:C])
        if self.mut == "column_C_of_x_read" and ldx > C:
            y[..., C - 1] += 0.0 * xv[..., C]
        if mode == 0:
            r = R.max_pool(y)
            if self.mut == "trailing_odd_frame_included" and T % 2:
                r[:, -1] = torch.maximum(r[:, -1], R.max_pool(y[:, T - 1:].expand(-1, 2, -1, -1, -1))[:, 0])
        else:
            r = _adaptive(y, self.mut == "bin_ceil_replaced_by_floor")
        cells = r.numel() // C
        full = torch.zeros(cells, ldo)
        full[:, :C] = r.reshape(cells, C)
        ov = out[:cells * ldo].view(cells, ldo)
        if self.mut == "columns_past_C_left_unwritten":
            ov[:, :C] = full[:, :C]
        elif self.mut == "second_trip_items_dropped":
            n = min(4 * 256 * K.pool_grid((B, T, H, W, C, ldx, ldo), mode, self.cus)[1], cells * ldo)
            out[:n] = full.reshape(-1)[:n]
        else:
            ov[:] = full


GOOD = TorchKernels()
CAUGHT = "kernel error|never written|were written|was written|NaN|differ in their bits"


def rejected(driver, mut, *args, match=CAUGHT):
    """the driver fails on the mutated stand-in: an assertion of Arena.check(), of a bit comparison or of the verdict"""
    with pytest.raises(AssertionError, match=match):
        driver(TorchKernels(mut), *args)


def _ids(v):
    return "-".join(str(a) for a in v) if isinstance(v, tuple) else str(v)


# ================================================================================================ the planes and the launch arithmetic
@pytest.mark.parametrize("shape", [(64, 1), (128, 16), (256, 2)], ids=_ids)
def test_planes_decode_to_the_weights(shape):
    from realpdebench_amd.model.deeponet import point_weights, point_weights_f16x2
    p, cout = shape
    ws, _, _ = K.AH.point_inputs(p, cout, 1, 1)
    pw = point_weights(*ws)
    got = decode_point_weights((K.as_i32(pw[0]), pw[1].reshape(-1), K.as_i32(pw[2]), pw[3].reshape(-1), K.as_i32(pw[4]), pw[5]), None, p, cout)
    for a, b in zip(got, ws):
        assert torch.equal(a, b)                                  # hi + mid + lo == x exactly
    ph = point_weights_f16x2(*ws)
    got = decode_point_weights((K.as_i32(ph[0]), ph[1].reshape(-1), K.as_i32(ph[2]), ph[3].reshape(-1), K.as_i32(ph[4]), ph[5]), ph[6], p, cout)
    for i, (a, b) in enumerate(zip(got, ws)):
        assert float((a - b).abs().max()) <= (2.0 ** -21 * float(b.abs().max()) if i % 2 == 0 else 0.0)


def test_cases_reach_the_paths_they_claim():
    assert [(N + 127) // 128 * 128 - N for _, _, N, _ in K.POINT_CASES] == [97, 0, 95, 63, 127]      # tail lanes of the last workgroup
    assert {p for p, _, _, _ in K.POINT_CASES} == {64, 128, 256} and {c for _, c, _, _ in K.POINT_CASES} >= {1, 16}
    assert [T * H * W for T, H, W, _ in K.TRUNK_CASES] == [1, 63, 64, 195] and {p for _, _, _, p in K.TRUNK_CASES} == {64, 128, 256}
    dims, mode = K.POOL_SECOND_TRIP
    assert K.pool_grid(dims, mode, CUS) == (1064960, 4096) and K.pool_trips(dims, mode, CUS) == 2
    assert all(K.pool_trips(d, m, CUS) == 1 for d, m in K.POOL_RUNS if (d, m) != K.POOL_SECOND_TRIP)
    # stage 1 at the cylinder shape (20, 64, 128) with ldo = 64: the second trip from B = 4 up
    assert [K.pool_trips((B, 20, 64, 128, 32, 64, 64), 0, CUS) for B in (1, 3, 4, 12)] == [1, 1, 2, 4]


# ================================================================================================ the stand-in passes, its mutations fail
@pytest.mark.parametrize("arith", ["f32", "f16x2"])
@pytest.mark.parametrize("shape", K.POINT_CASES, ids=_ids)
def test_standin_point_mlp(shape, arith):
    c = K.point_case(*shape)
    K.run_point_mlp_twice(GOOD, c, arith)
    rejected(K.run_point_mlp, "last_tail_point_unwritten", c, arith)
    rejected(K.run_point_mlp, "column_C_out_written", c, arith)
    rejected(K.run_point_mlp, "row_N_of_t_read", c, arith)


def test_a_weight_read_past_its_operand_poisons_the_result():
    """the guard value of the int32 arenas is a NaN in both halves, for both plane formats"""
    for fill, half in ((K.BF16_NAN_PAIR, False), (K.F16_NAN_PAIR, True)):
        a = K.guarded.Arena("cpu", dtype=torch.int32, fill=fill)
        w = a.inp(torch.zeros(8, dtype=torch.int32), "w")
        assert bool(torch.isnan(_planes(_past_the_end(w.op, 8, 4), half)).all())


@pytest.mark.parametrize("shape", K.TRUNK_CASES, ids=_ids)
def test_standin_trunk(shape):
    c = K.trunk_case(*shape)
    K.run_trunk(GOOD, c)
    rejected(K.run_trunk, "tail_point_written_at_row_N", c)
    if shape[1] != shape[2]:
        rejected(K.run_trunk, "H_and_W_axes_swapped", c)


@pytest.mark.parametrize("dims,mode", K.POOL_RUNS, ids=_ids)
def test_standin_pool(dims, mode):
    B, T, H, W, C, ldx, ldo = dims
    c = K.pool_case(*dims)
    K.run_pool(GOOD, c, mode)
    if ldo > C:
        rejected(K.run_pool, "columns_past_C_left_unwritten", c, mode)
    if ldx > C:
        rejected(K.run_pool, "column_C_of_x_read", c, mode)
    if mode == 0 and T % 2:
        rejected(K.run_pool, "trailing_odd_frame_included", c, mode)
    if mode == 1 and (H % 4 or W % 4):
        rejected(K.run_pool, "bin_ceil_replaced_by_floor", c, mode)
    if K.pool_trips(dims, mode, CUS) > 1:
        rejected(K.run_pool, "second_trip_items_dropped", c, mode)


def test_standin_pool_refusal_and_nan_rule():
    K.run_pool_refused(GOOD, K.pool_case(*K.POOL_REFUSED[0]), K.POOL_REFUSED[1])
    for mode in (0, 1):
        for at in K.NAN_AT:
            K.run_pool_nan(GOOD, mode, at)
