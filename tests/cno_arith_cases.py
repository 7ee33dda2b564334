"""Shared by tests/test_cno_arith_host.py and tests/test_gpu_cno_arith.py (a plain module, not a test file): the operands of the
rpb_cno_conv3x_f16x2 kernel cases -- ``_kernel_case`` of tests/test_gpu_cno.py restated without a device -- and the f16x2 arithmetic
restated in fp64: the exponent rule, both planes rounded to nearest even, three products, one fp32 rounding of the sum, the epilogue.

Bounds.  GPU kernel against fp64 ``conv3d``: Rel-L2 < 2e-6, the bound tests/test_gpu_conv3h.py holds this arithmetic to (with or without a
residual).  The restatement against the same fp64 result must stay under one eighth of it, 2.5e-7: what the arithmetic itself loses
(dropped lo*lo term <= 2^-22 |a b|, one fp32 rounding of the sum and of each epilogue step) leaves the rest to the summation order of
the MFMA chain."""
import functools
import struct

import torch
import torch.nn.functional as F

B_K, MESH_K = 2, (3, 5, 7)
M_K = B_K * MESH_K[0] * MESH_K[1] * MESH_K[2]             # 210: two tiles, a tail, the sample border (105) inside a tile
SHAPES = [(64, 64), (128, 128), (64, 128), (128, 64)]    # (Ci, N)
# (act, residual, narrow): the four epilogue rows of tests/test_gpu_cno.py.  narrow: nvalid = 16 at a non-zero column offset of wider
# rows (fp32 columns 8..23 of 48; residual columns 4..19 of 40); otherwise nvalid = N and the rows are N wide
EPILOGUES = [(1, False, False), (0, True, True), (1, True, False), (0, False, True)]
GPU_BOUND = 2e-6
HOST_BOUND = GPU_BOUND / 8
# the boundary values of test_split2h_reconstructs_and_exponent_range (tests/test_gpu_conv3h.py): an fp32 subnormal maximum and every
# power-of-two / just-below boundary of the exponent choice
BOUNDARY_VALUES = (2.0 ** -140, 3.0 * 2.0 ** -130, 2.0 ** -87, 2.0 ** -88 * (2 - 2 ** -23), 1.0, 2.0 ** 100)


def _u(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def conv_fp64(x, w, Ci, N):
    """x [M_K][Ci], w [N][27 * Ci] (tap-major rows) -> Conv3d(Ci, N, 3, padding=1) as rows [M_K][N], in fp64"""
    T, H, W = MESH_K
    xr = x.view(B_K, T, H, W, Ci).permute(0, 4, 1, 2, 3).double()
    wr = w.view(N, 3, 3, 3, Ci).permute(0, 4, 1, 2, 3).double()
    return F.conv3d(xr, wr, padding=1).permute(0, 2, 3, 4, 1).reshape(M_K, N)


@functools.lru_cache(maxsize=None)
def kernel_case(Ci, N):
    """x, weights, affine, residual and the fp64 convolution of one (Ci, N): the values of tests/test_gpu_cno.py, computed once."""
    x = _u(Ci + N, M_K, Ci)
    w = _u(Ci + N + 1, N, 27 * Ci) * (3.0 / (27 * Ci)) ** 0.5 * 1.4
    sc, sh, res = _u(3, N) * 0.5 + 1.0, _u(4, N) * 0.5, _u(5, M_K, N)
    return dict(x=x, w=w, sc=sc, sh=sh, res=res, y=conv_fp64(x, w, Ci, N))


def expected(c, act, with_res, nv):
    """the exact fp64 result of the first nv channels"""
    v = c["y"][:, :nv] * c["sc"][:nv].double() + c["sh"][:nv].double()
    if act:
        v = F.leaky_relu(v, 0.2)
    if with_res:
        v = v + c["res"][:, :nv].double()
    return v


# ----------------------------------------------------------------------------------------------------------- the arithmetic, restated
def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def exponent_of_bits(b):
    """The rule of amax_exp_finish_kernel: b = max |x| as an fp32 bit pattern -> e with max * 2^e in [2^14, 2^15); 0 for zero or a
    non-finite maximum.  The binary exponent is read from the bits (normal: biased exponent - 127; subnormal: position of the leading
    one - 149)."""
    if b == 0 or b >= 0x7F800000:
        return 0
    return 14 - ((b >> 23) - 127 if b >= 0x00800000 else (b.bit_length() - 1) - 149)


def exponent(t):
    """the exponent of an fp32 tensor"""
    return exponent_of_bits(int((t.float().contiguous().view(torch.int32) & 0x7FFFFFFF).max()))


def split2h(t, e):
    """fp32 tensor -> (hi, lo) in fp64: the two fp16 planes of t * 2^e, both rounded to nearest even (t * 2^e and v - hi are exact)"""
    v = t.double() * 2.0 ** e
    hi = v.to(torch.float16).double()
    lo = (v - hi).to(torch.float16).double()
    return hi, lo


def restated(c, Ci, N, act, with_res, nv):
    """rpb_cno_conv3x_f16x2 in fp64 on the operands of ``kernel_case``: the three products exactly, one fp32 rounding of their sum, then
    each epilogue step rounded once to fp32 (the fma is one rounding)."""
    ea, ew = exponent(c["x"]), exponent(c["w"])
    xh, xl = split2h(c["x"], ea)
    wh, wl = split2h(c["w"], ew)
    acc = (conv_fp64(xl, wh, Ci, N) + conv_fp64(xh, wl, Ci, N) + conv_fp64(xh, wh, Ci, N)).float()
    acc = (acc.double() * 2.0 ** -(ea + ew)).float()                    # exact: a power of two
    v = (acc.double() * c["sc"].double() + c["sh"].double()).float()[:, :nv]
    if act:
        v = torch.where(v > 0, v, (v.double() * float(torch.tensor(0.2, dtype=torch.float32))).float())
    if with_res:
        v = (v.double() + c["res"][:, :nv].double()).float()
    return v


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())
