"""Shared by tests/test_deeponet_arith_host.py and tests/test_gpu_deeponet_arith.py (a plain module, not a test file): a numpy emulation
of rpb_don_point_mlp_f16x2's data flow (csrc/rpb_deeponet_h.hip) from the operands ``point_weights_f16x2`` builds, the kernel's exponent
rule restated, and the input variants both files use."""
import numpy as np
import torch

F16_MAX = 65504.0


def u(seed, *shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1


def point_inputs(p, cout, N, B):
    """The seeded inputs of tests/test_gpu_deeponet.py::test_point_mlp_kernel: (W1, b1, W2, b2, W3, b3), t [N][p], b [B][p]."""
    ws = (u(1, 512, p) * (3 / p) ** 0.5, u(2, 512) * 0.2, u(3, 128, 512) * (3 / 512) ** 0.5, u(4, 128) * 0.2,
          u(5, cout, 128) * (3 / 128) ** 0.5, u(6, cout) * 0.2)
    return ws, u(7, N, p), u(8, B, p) * 2


def sd_of(ws):
    return dict(zip(("output_net.0.weight", "output_net.0.bias", "output_net.3.weight", "output_net.3.bias", "output_net.6.weight",
                     "output_net.6.bias"), ws))


def adversarial(W1, t, b, row=0, c=3.0):
    """(t, b) with sample 0's branch vector all ones and point ``row`` of t = c sign(W1[u]), u the row of W1 with the largest 1-norm:
    h1_u of that point is c ||W1_u||_1 + b1_u, the kernel's bound up to max|b1| - b1_u."""
    t, b = t.clone(), b.clone()
    uu = int(W1.double().abs().sum(1).argmax())
    sign = torch.where(W1[uu] < 0, -torch.ones_like(W1[uu]), torch.ones_like(W1[uu]))
    b[0] = 1.0
    t[row] = c * sign
    return t, b


def col_exp(m, top):
    """The kernel's rule: e with m 2^e in [2^top, 2^(top + 1)) for finite fp32 m > 0, capped at 62; 0 for m == 0."""
    m = np.ascontiguousarray(m, dtype=np.float32)
    e = np.minimum(top + 127 - (m.view(np.int32) >> 23), 62)
    return np.where(m == 0, 0, e).astype(np.int64)


def planes_of(v):
    """fp64 values that are exact fp32 numbers -> (hi, lo) as fp64, both rounded to nearest even fp16 (inf past fp16's range)."""
    with np.errstate(over="ignore"):
        v32 = v.astype(np.float32)
        hi = v32.astype(np.float16)
        lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def decode(z):
    """int16 fp16 bit patterns [..., 2 planes, 64, 8] -> (hi, lo) fp64 arrays [..., 64, 8]"""
    hi, lo = z.view(torch.float16).double().unbind(-3)
    return hi.numpy(), lo.numpy()


def emulate_point_kernel_f16x2(t, b, pw, stats=None):
    """One 32-point tile (t [32][p], b [1][p]) through the v_mfma_f32_32x32x16_f16 register layout: A / B lane (row or column =
    lane % 32, kg = lane // 32) holds k = 8 kg + e; accumulator register r of lane (column, kg) is row 8 (r // 4) + 4 kg + r % 4.
    Planes decoded from their bit patterns, the per-point exponents of the kernel, three products (lo hi, hi lo, hi hi), exact products
    accumulated in fp64, the epilogues relu(acc 2^-(ew + e) + bias).  ``stats`` (a dict) receives the largest |plane value| of the
    activations and the exponents (ex, e1, e2) per point."""
    w1h, b1z, w2h, b2z, w3h, b3, sc = pw
    w1, w2, w3 = decode(w1h), decode(w2h), decode(w3h)
    b1z, b2z, sc = b1z.double().numpy(), b2z.double().numpy(), sc.numpy().astype(np.float32)
    lanes = np.arange(64)
    col, kg = lanes % 32, lanes // 32
    rows = np.array([[8 * (r // 4) + 4 * g + r % 4 for r in range(16)] for g in range(2)])      # [kg][r]
    peak = [0.0]

    def mfma(A, Bop, D):                       # A, Bop [64 lanes][8]; D [64 lanes][16]
        a = np.zeros((32, 16)); bm = np.zeros((16, 32))
        for l in range(64):
            a[col[l], 8 * kg[l]:8 * kg[l] + 8] = A[l]
            bm[8 * kg[l]:8 * kg[l] + 8, col[l]] = Bop[l]
        prod = a @ bm
        for l in range(64):
            D[l] += prod[rows[kg[l]], col[l]]

    def mma3(w, x, D):                         # w, x: (hi, lo)
        mfma(w[1], x[0], D)
        mfma(w[0], x[1], D)
        mfma(w[0], x[0], D)

    def split(v):                              # [64 lanes][8] scaled values -> (hi, lo)
        hi, lo = planes_of(v)
        peak[0] = max(peak[0], float(np.abs(hi).max()), float(np.abs(lo).max()))
        return hi, lo

    p = t.shape[1]
    x = (t.float() * b.float()).numpy()        # [32 points][p], fp32 as the kernel forms it
    m = np.abs(x).max(1)
    ex = col_exp(m, 14)
    e1 = col_exp((np.float64(sc[3]) * m + np.float64(sc[4])).astype(np.float32), 13)      # the kernel's fmaf
    c1 = (float(sc[0]) * 2.0 ** -ex)[col][:, None]
    c2 = (float(sc[1]) * 2.0 ** -e1)[col][:, None]
    xs = x.astype(np.float64) * (2.0 ** ex)[:, None]
    xop = [split(np.stack([xs[col[l], 16 * ks + 8 * kg[l]:16 * ks + 8 * kg[l] + 8] for l in range(64)])) for ks in range(p // 16)]
    acc2 = [np.zeros((64, 16)) for _ in range(4)]
    for blk in range(16):
        acc1 = np.zeros((64, 16))
        for ks in range(p // 16):
            mma3((w1[0][blk, ks], w1[1][blk, ks]), xop[ks], acc1)
        v = np.maximum(acc1 * c1 + b1z[blk][kg], 0).astype(np.float32).astype(np.float64) * (2.0 ** e1)[col][:, None]
        hp = [split(v[:, 8 * s:8 * s + 8]) for s in range(2)]
        for s in range(2):
            for mt in range(4):
                mma3((w2[0][blk, s, mt], w2[1][blk, s, mt]), hp[s], acc2[mt])
    h2 = [np.maximum(acc2[mt] * c2 + b2z[mt][kg], 0).astype(np.float32) for mt in range(4)]
    m2 = np.max(np.stack([h.max(1) for h in h2]), 0)                       # per lane
    m2 = np.maximum(m2[:32], m2[32:])                                      # lane ^ 32 -> per point
    e2 = col_exp(m2, 14)
    c3 = (float(sc[2]) * 2.0 ** -e2)[col][:, None]
    acc3 = np.zeros((64, 16))
    for mt in range(4):
        v = h2[mt].astype(np.float64) * (2.0 ** e2)[col][:, None]
        for s in range(2):
            mma3((w3[0][mt, s], w3[1][mt, s]), split(v[:, 8 * s:8 * s + 8]), acc3)
    o = acc3 * c3
    out = np.zeros((32, b3.shape[0]))
    for l in range(64):
        for r in range(8):
            c = rows[kg[l]][r]
            if c < b3.shape[0]:
                out[col[l], c] = o[l, r] + float(b3[c])
    if stats is not None:
        stats.update(peak=peak[0], ex=ex, e1=e1, e2=e2)
    return out
