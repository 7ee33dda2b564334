"""Host side (no GPU) of the per-kernel tests of the DMD kernels (tests/dmd_kernel_cases.py):
* every case of tests/test_gpu_dmd_kernels.py is well conditioned: the drivers run here on ``TorchKernels``, a torch stand-in for the
  library on CPU arenas that forms the fp64 products chunk by chunk and rounds as the kernels round;
* the restated launch arithmetic (``dmd_pts``, the Gram groups) puts the cases on the paths they claim at the MI355X's 256 compute
  units: the partial last tile, both staging widths, the second and third trips of the gram-only cases;
* the cancelling inputs tell fp64 arithmetic from fp32 arithmetic: the correct stand-in stays under the 1e-6 bound, ``M`` rounded to
  fp32 and fp32 accumulation exceed it, at three shapes -- and the inputs of tests/test_gpu_dmd.py (the ``random`` family) do not;
* the drivers would notice: with ONE wrong term or ONE out-of-range access the stand-in trips ``Arena.check()``, a bit comparison or
  the verdict in at least one case -- the same driver code the GPU test runs."""
import os
import sys

import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import dmd_kernel_cases as K                 # noqa: E402

F32, F64 = torch.float32, torch.float64
CUS = K.MI355X_CUS


def _past_the_end(t, n, count=1):
    """elements ``n .. n + count - 1`` of a flat operand view of ``n`` elements: the first elements of the guard behind it"""
    return t.as_strided((n + count,), (1,))[n:]


class TorchKernels:
    """the entry points the drivers call, in torch on the views of CPU arenas; ``mut`` = one wrong term or out-of-range access"""
    dev = "cpu"

    def __init__(self, mut=None, cus=CUS):
        self.mut, self.cus = mut, cus

    def dmd_gram_groups(self, B, P, f):
        return K.gram_groups(B, P, f, self.cus)

    def _frames(self, x, B, T, P, C, f):
        """[B][T][P][f] fp64: the gathered channels of every cell"""
        n = B * T * P * C
        keep = min(f + 1, C) if self.mut == "channel_past_f_kept" else f
        X = x[:n].view(B, T, P, C)[..., :keep].double()
        if self.mut == "point_at_P_read":                         # the last frame's staging runs one cell past the row
            X = X.clone()
            X[B - 1, T - 1, P - 1, 0] += 0.0 * _past_the_end(x, n)[0].double()
        return X

    def dmd_gram(self, x, G, part, B, T, P, C, f):
        NG, pts = self.dmd_gram_groups(B, P, f), K.dmd_pts(f)
        X = self._frames(x, B, T, P, C, f)
        acc = torch.zeros(B, NG, T, T, dtype=F64)
        for ch in range(K.nchunk(P, f)):                          # workgroup g walks chunks g, g + NG, ...
            if self.mut == "second_trip_chunks_dropped" and ch >= NG:
                continue
            Xc = X[:, :, ch * pts:(ch + 1) * pts].reshape(B, T, -1)
            acc[:, ch % NG] += Xc @ Xc.transpose(1, 2)
        low = torch.ones(T, T, dtype=torch.bool).tril()
        pv = part[:B * NG * T * T].view(B, NG, T, T)
        if self.mut == "upper_triangle_of_part_written":
            pv[:] = acc
        else:
            pv[:, :, low] = acc[:, :, low]
        s = acc[:, 0].clone()
        for g in range(1, NG):
            s = s + acc[:, g]
        s = torch.where(low, s, s.transpose(1, 2))                # the lower triangle, mirrored
        Gv = G[:B * T * T].view(B, T, T)
        if self.mut == "mirror_missing":
            Gv[:, low] = s[:, low]
        else:
            Gv[:] = s

    def dmd_predict(self, x, M, out, B, T, P, C, f, S):
        n, pts = P * f, K.dmd_pts(f)
        X = self._frames(x, B, T, P, C, f)[:, 1:, :, :f].reshape(B, T - 1, n)
        Mv = M[:B * (T - 1) * S].view(B, T - 1, S)
        if self.mut == "M_rounded_to_fp32":
            Mv = Mv.float().double()
        if self.mut == "fp32_accumulation":
            r = torch.einsum("bks,bkn->bsn", Mv.float(), X.float())
        else:
            r = torch.einsum("bks,bkn->bsn", Mv, X).float()
        ov = out[:B * S * n].view(B, S, n)
        if self.mut == "elements_240_to_251_of_a_chunk_not_written":
            e = torch.arange(n) % (pts * f)
            ov[:, :, e < 240] = r[:, :, e < 240]
        else:
            ov[:] = r
        if self.mut == "row_S_written":                           # of the last sample: the n floats behind the operand
            _past_the_end(out, B * S * n, n)[:] = 0.0


GOOD = TorchKernels()
CAUGHT = "kernel error|never written|were written|was written|NaN|differ in their bits|an entry is off"


def rejected(driver, mut, *args, match=CAUGHT):
    """the driver fails on the mutated stand-in: an assertion of Arena.check(), of a bit comparison or of the verdict"""
    with pytest.raises(AssertionError, match=match):
        driver(TorchKernels(mut), *args)


def _ids(v):
    return "-".join(str(a) for a in v)


# ================================================================================================ launch arithmetic
def test_cases_reach_the_paths_they_claim():
    assert [K.dmd_pts(f) for f in (1, 2, 3, 4, 6, 16, 64)] == [256, 128, 84, 64, 40, 16, 4]
    pf = {c: K.dmd_pts(c[4]) * c[4] for c in K.CASES}
    assert pf[K.CASES[0]] == 252 and pf[K.CASES[1]] == 252 and pf[K.CASES[4]] == 240        # a partial 16-column tile; 15 whole ones
    assert [K.nchunk(c[2], c[4]) for c in K.CASES] == [2, 1, 1, 3, 1, 1]
    assert 88 - K.dmd_pts(3) == 4 and 9 - 2 * K.dmd_pts(64) == 1                            # the tails of the last chunks
    assert [K.vec(c[2], c[3]) for c in K.CASES] == [4, 4, 1, 4, 4, 1] and K.vec(88, 3, misaligned=True) == 1
    assert {c[1] for c in K.CASES} >= {2, 16, 17, 32} and {c[5] for c in K.CASES} >= {1, 16, 17, 32}
    # the gram-only cases: more chunks than workgroups at 256 compute units
    assert [K.nchunk(P, f) for _, _, P, _, f in K.GRAM_ONLY] == [66, 69, 130]
    assert [K.gram_groups(B, P, f, CUS) for B, _, P, _, f in K.GRAM_ONLY] == [64, 64, 64]
    for B, T, P, C, f in K.GRAM_ONLY:
        assert K.nchunk(P, f) > K.gram_groups(B, P, f, CUS)
    assert K.ceil_div(130, 64) == 3                                                         # a third trip
    # the benchmark batch: B = 12 on 256 compute units walks 64 chunks of P = 8192, f = 2 with 43 workgroups
    assert K.gram_groups(12, 8192, 2, CUS) == 43 and K.nchunk(8192, 2) == 64
    assert K.gram_groups(2, 8192, 2, CUS) == 64 and K.gram_groups(2, 4099, 2, CUS) == 33    # tests/test_gpu_dmd.py: one trip each


# ================================================================================================ the stand-in passes, its mutations fail
@pytest.mark.parametrize("dims", [c[:5] for c in K.CASES] + K.GRAM_ONLY, ids=_ids)
def test_standin_gram(dims):
    B, T, P, C, f = dims
    c = K.gram_case(*dims)
    K.run_gram_twice(GOOD, c)
    rejected(K.run_gram, "mirror_missing", c)
    rejected(K.run_gram, "upper_triangle_of_part_written", c)
    rejected(K.run_gram, "point_at_P_read", c)
    if C > f:
        rejected(K.run_gram, "channel_past_f_kept", c)
    if K.nchunk(P, f) > K.gram_groups(B, P, f, CUS):
        rejected(K.run_gram, "second_trip_chunks_dropped", c)


def test_standin_gram_misaligned():
    K.run_gram_misaligned(GOOD, K.gram_case(*K.MISALIGNED[:5]))
    rejected(K.run_gram, "point_at_P_read", K.gram_case(*K.MISALIGNED[:5]), True)


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("dims", K.CASES, ids=_ids)
def test_standin_predict(dims, family):
    B, T, P, C, f, S = dims
    c = K.predict_case(*dims, family)
    K.run_predict_twice(GOOD, c)
    rejected(K.run_predict, "row_S_written", c)
    rejected(K.run_predict, "point_at_P_read", c)
    if K.dmd_pts(f) * f == 252:
        rejected(K.run_predict, "elements_240_to_251_of_a_chunk_not_written", c)


@pytest.mark.parametrize("family", K.FAMILIES)
def test_standin_predict_misaligned(family):
    K.run_predict_misaligned(GOOD, K.predict_case(*K.MISALIGNED, family))


# ================================================================================================ fp64 against fp32 arithmetic
WRONG_ARITHMETIC = ["M_rounded_to_fp32", "fp32_accumulation"]


@pytest.mark.parametrize("dims", [K.CASES[0], K.CASES[3], K.CASES[4]], ids=_ids)
def test_cancelling_inputs_tell_fp64_from_fp32_arithmetic(dims):
    """correct arithmetic under the 1e-6 bound (the GOOD run asserts it), both wrong ones over it on both measures"""
    c = K.predict_case(*dims, "cancelling")
    K.run_predict(GOOD, c)
    for mut in WRONG_ARITHMETIC:
        rejected(K.run_predict, mut, c, match="kernel error")
        got = torch.empty(c.want.shape)
        TorchKernels(mut).dmd_predict(c.x.reshape(-1).nan_to_num(0.0), c.M.reshape(-1), got.view(-1), *c.dims)
        for kind, e in zip(K.MEASURES, K.measures(got, c.want)):
            print(f"[{K.TAG}] {c.name} {mut} {kind}: {e:.3e}")
            assert e > K.PREDICT_BOUND, (mut, kind, e)


@pytest.mark.parametrize("dims", K.CASES, ids=_ids)
def test_random_inputs_do_not(dims):
    """why the cancelling family exists: on the inputs of tests/test_gpu_dmd.py both wrong arithmetics pass the 1e-6 bound"""
    c = K.predict_case(*dims, "random")
    for mut in WRONG_ARITHMETIC:
        K.run_predict(TorchKernels(mut), c)
