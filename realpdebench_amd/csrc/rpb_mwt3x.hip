// MWT3d sparseKernel3d (3x3x3 convolution at 36 channels + bias + ReLU + Linear(36, 36) + bias, optional +=) on the split-operand
// arithmetic of rpb_mma.h: the opt-in modes of MWT3d.set_arith.  Contract of rpb_mwt_conv3 (csrc/rpb_mwt.hip): channels-last fp32
// [B][Nx][Ny][T][36] in and out, zero padding at the mesh borders, no atomics (two calls are bit-equal).
//   "bf16x3"  operands as three bf16 planes (hi + mid + lo exact), six products per fp32 product, fp32 accumulation (split8 / mfma16);
//   "f16x2"   operands as two fp16 planes of the tensor scaled by 2^e (e from rpb_amax_exp, read from device memory: no host
//             synchronisation), three products (split8h / mfma16h), dropped term <= 2^-22 |a b|; the epilogue undoes both scales.
// One kernel body, templated on the plane scheme.  v_mfma_f32_16x16x32_{bf16,f16}: rows = output channel (3 tiles, 36 of 48 used),
// columns = cells (one wave = 64 consecutive cells = 4 column tiles).  K = 27 taps x 36 channels is FLAT: 243 groups of four channels
// (16 bytes, never straddling a tap), eight groups per K step, 31 steps (the last five groups are zero: K = 992 for 972).  Lane group
// kg = l >> 4 of step s supplies groups G = 8 s + 2 kg + {0, 1}: tap G / 9, channels 4 (G % 9) .. + 3 -- two 16-byte loads of the
// neighbour cell(s) per column tile, split into planes in registers; no plane tensor exists in HBM.  The weights are split once per
// weight change into the A operand in lane order, wpx [31][3 row tiles][P planes][64 lanes] x 16 bytes (rpb_mwt_conv3x_wprep).
// The D layout is that of the fp32 instruction (register r of lane group g = row 4 g + r), so the epilogue is rpb_mwt_conv3's: the
// ReLU'd accumulator feeds the small Lo product (3.7 % of the FLOPs) on v_mfma_f32_16x16x4_f32 with the same `lop`, and a lane ends
// with four consecutive output channels of one cell = one 16-byte store.
#include "rpb_mma.h"

#define MWX_C 36
#define MWX_GROUPS 243      // 27 taps x 9 groups of four channels
#define MWX_STEPS 31        // ceil(243 / 8)

__device__ __forceinline__ f32x4 mwx_mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// H = false: three bf16 planes; H = true: two fp16 planes of x * 2^ea[0] and w * 2^ew[0]
template <bool H>
__global__ __launch_bounds__(256) void mwt_conv3x_k(const float* __restrict__ x, const u32x4* __restrict__ wpx, const float* __restrict__ cb,
                                                    const float* __restrict__ lop, const float* __restrict__ lb, float* __restrict__ out,
                                                    long ncell, int Nx, int Ny, int T, int accumulate, const int* __restrict__ ea,
                                                    const int* __restrict__ ew) {
    constexpr int P = H ? 2 : 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, cl = lane & 15;
    const long base = (blockIdx.x * 4L + wave) * 64;
    if (base >= ncell) return;                       // wave-uniform
    int ex = 0, eo = 0;
    if constexpr (H) {
        ex = ea[0];
        eo = -(ex + ew[0]);
    }
    long cq[4];
    unsigned mask[4];                                // bit `tap`: that neighbour of the cell lies inside the mesh (0 for a tail column)
    bool cv[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const long q = base + n * 16 + cl;
        cv[n] = q < ncell;
        cq[n] = cv[n] ? q : ncell - 1;
        long r = cq[n];
        const int ct = (int)(r % T);
        r /= T;
        const int cy = (int)(r % Ny);
        r /= Ny;
        const int cx = (int)(r % Nx);
        unsigned mt = 0, my = 0, mx = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) mt |= (unsigned)(ct + j - 1) < (unsigned)T ? 1u << j : 0u;
#pragma unroll
        for (int j = 0; j < 3; ++j) my |= (unsigned)(cy + j - 1) < (unsigned)Ny ? mt << (3 * j) : 0u;
#pragma unroll
        for (int j = 0; j < 3; ++j) mx |= (unsigned)(cx + j - 1) < (unsigned)Nx ? my << (9 * j) : 0u;
        mask[n] = cv[n] ? mx : 0u;
    }
    f32x4 acc[3][4];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int s = 0; s < MWX_STEPS; ++s) {
        // this lane's two channel groups: offset (floats) from the cell to the neighbour's four channels, and the tap as a mask bit
        long off[2];
        unsigned bit[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int G = 8 * s + 2 * g + h;
            const int tap = G / 9, c4 = G - 9 * tap;
            const int dx = tap / 9 - 1, dy = (tap / 3) % 3 - 1, dt = tap % 3 - 1;
            off[h] = ((long)(dx * Ny + dy) * T + dt) * MWX_C + 4 * c4;
            bit[h] = G < MWX_GROUPS ? 1u << tap : 0u;
        }
        bf16x8 a[3][P];
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int p = 0; p < P; ++p) a[t][p] = __builtin_bit_cast(bf16x8, wpx[((s * 3 + t) * P + p) * 64 + lane]);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            float v[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bool ok = (mask[n] & bit[h]) != 0u;
                // a neighbour inside the mesh is inside the same sample; everything else reads cell 0 and is replaced by the zero pad
                const f32x4 q = *reinterpret_cast<const f32x4*>(x + (ok ? cq[n] * MWX_C + off[h] : 0L));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float z = ok ? q[i] : 0.f;
                    v[4 * h + i] = H ? ldexpf(z, ex) : z;             // exact: max|x| 2^ex < 2^15
                }
            }
            if constexpr (H) {
                bf16x8 bh, bl;
                split8h<true>(v, bh, bl);
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    acc[t][n] = mfma16h(a[t][0], bl, acc[t][n]);
                    acc[t][n] = mfma16h(a[t][1], bh, acc[t][n]);
                    acc[t][n] = mfma16h(a[t][0], bh, acc[t][n]);
                }
            } else {
                bf16x8 bh, bm, bl;
                split8(v, bh, bm, bl);
#pragma unroll
                for (int t = 0; t < 3; ++t) {                         // small terms first
                    acc[t][n] = mfma16(a[t][0], bl, acc[t][n]);
                    acc[t][n] = mfma16(a[t][2], bh, acc[t][n]);
                    acc[t][n] = mfma16(a[t][1], bm, acc[t][n]);
                    acc[t][n] = mfma16(a[t][0], bm, acc[t][n]);
                    acc[t][n] = mfma16(a[t][1], bh, acc[t][n]);
                    acc[t][n] = mfma16(a[t][0], bh, acc[t][n]);
                }
            }
        }
    }
    // undo the scales, bias + ReLU on the rows 16 t + 4 g + r (cb is padded to 48 with zeros, so the pad rows stay 0)
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(cb + 16 * t + 4 * g);
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float c = H ? ldexpf(acc[t][n][r], eo) : acc[t][n][r];
                acc[t][n][r] = fmaxf(c + b4[r], 0.f);
            }
    }
    // Lo on the fp32 MFMA, fed from the accumulator as it stands (rpb_mwt_conv3's second product and its `lop`)
    f32x4 o2[3][4];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int n = 0; n < 4; ++n) o2[u][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const float a2 = lop[((t * 4 + r) * 3 + u) * 64 + lane];
#pragma unroll
                for (int n = 0; n < 4; ++n) o2[u][n] = mwx_mfma4(a2, acc[t][n][r], o2[u][n]);
            }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int o0 = 16 * u + 4 * g;
        if (o0 >= MWX_C) continue;                   // rows 36..47 are padding
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(lb + o0);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (!cv[n]) continue;
            f32x4* dst = reinterpret_cast<f32x4*>(out + cq[n] * MWX_C + o0);
            f32x4 v = o2[u][n] + b4;
            if (accumulate) v += *dst;
            *dst = v;
        }
    }
}

// weights [36 co][36 ci][27] -> wpx [31][3][P][64] x 16 bytes: lane (m = l & 15, kg = l >> 4) of row tile t holds row 16 t + m,
// k = 8 kg + e = channel 4 (G % 9) + (e & 3) of tap G / 9, G = 8 s + 2 kg + (e >> 2); zeros on the pad rows and the pad groups
template <bool H>
__global__ __launch_bounds__(256) void mwt_conv3x_wprep_k(const float* __restrict__ w, u32x4* __restrict__ wpx, const int* __restrict__ ew) {
    constexpr int P = H ? 2 : 3;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= MWX_STEPS * 3 * 64) return;
    const int lane = i & 63, t = (i >> 6) % 3, s = i / 192;
    const int co = 16 * t + (lane & 15), kg = lane >> 4;
    int e = 0;
    if constexpr (H) e = ew[0];
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int G = 8 * s + 2 * kg + (k >> 2);
        const int tap = G / 9, ci = 4 * (G - 9 * tap) + (k & 3);
        const float z = (co < MWX_C && G < MWX_GROUPS) ? w[(co * MWX_C + ci) * 27 + tap] : 0.f;
        v[k] = H ? ldexpf(z, e) : z;
    }
    u32x4* dst = wpx + ((s * 3 + t) * P) * 64 + lane;
    if constexpr (H) {
        bf16x8 h, l;
        split8h<false>(v, h, l);
        dst[0] = __builtin_bit_cast(u32x4, h);
        dst[64] = __builtin_bit_cast(u32x4, l);
    } else {
        bf16x8 h, m, l;
        split8(v, h, m, l);
        dst[0] = __builtin_bit_cast(u32x4, h);
        dst[64] = __builtin_bit_cast(u32x4, m);
        dst[128] = __builtin_bit_cast(u32x4, l);
    }
}

// ---------------------------------------------------------------------------------- C ABI
#define MWX_STREAM (static_cast<hipStream_t>(stream))

extern "C" int rpb_mwt_conv3x_wprep(const float* w, void* wpx, int planes, const int* ew, void* stream) {
    RPB_REQUIRE(w && wpx, "rpb_mwt_conv3x_wprep: null pointer");
    RPB_REQUIRE(planes == 3 || (planes == 2 && ew), "rpb_mwt_conv3x_wprep: planes = 3 (bf16x3) or 2 (f16x2, with its exponent), got %d", planes);
    const dim3 grid((MWX_STEPS * 3 * 64 + 255) / 256), block(256);
    if (planes == 2)
        hipLaunchKernelGGL(mwt_conv3x_wprep_k<true>, grid, block, 0, MWX_STREAM, w, static_cast<u32x4*>(wpx), ew);
    else
        hipLaunchKernelGGL(mwt_conv3x_wprep_k<false>, grid, block, 0, MWX_STREAM, w, static_cast<u32x4*>(wpx), ew);
    RPB_CHECK_LAUNCH("rpb_mwt_conv3x_wprep");
}

extern "C" int rpb_mwt_conv3x(const float* x, const void* wpx, const float* cb48, const float* lop, const float* lb, float* out, int B,
                              int Nx, int Ny, int T, int accumulate, int planes, const int* ea, const int* ew, void* stream) {
    RPB_REQUIRE(x && wpx && cb48 && lop && lb && out, "rpb_mwt_conv3x: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0, "rpb_mwt_conv3x: bad shape B=%d Nx=%d Ny=%d T=%d", B, Nx, Ny, T);
    RPB_REQUIRE(x != out, "rpb_mwt_conv3x: in-place convolution is not possible");
    RPB_REQUIRE(planes == 3 || (planes == 2 && ea && ew), "rpb_mwt_conv3x: planes = 3 (bf16x3) or 2 (f16x2, with both exponents), got %d",
                planes);
    const long ncell = (long)B * Nx * Ny * T;
    const dim3 grid((unsigned)((ncell + 255) / 256)), block(256);
    const u32x4* wz = static_cast<const u32x4*>(wpx);
    if (planes == 2)
        hipLaunchKernelGGL(mwt_conv3x_k<true>, grid, block, 0, MWX_STREAM, x, wz, cb48, lop, lb, out, ncell, Nx, Ny, T, accumulate, ea, ew);
    else
        hipLaunchKernelGGL(mwt_conv3x_k<false>, grid, block, 0, MWX_STREAM, x, wz, cb48, lop, lb, out, ncell, Nx, Ny, T, accumulate, ea, ew);
    RPB_CHECK_LAUNCH("rpb_mwt_conv3x");
}
