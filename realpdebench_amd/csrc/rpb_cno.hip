// CNO3d (realpdebench/model/cno.py with activation = 'LeakyReLU'): every layer is Conv3d(3, padding=1) followed by an eval BatchNorm,
// LeakyReLU(0.2), a residual add or a channel concat, all at full resolution.  rpb_cno_conv3x is the implicit GEMM of conv3x_kernel
// (csrc/rpb_conv3x.hip: same plane input P[3][M][Ci], same rpb_conv3x_wprep weights, same tiling, same six bf16 products per fp32
// product, same accumulation order) with the CNO epilogue
//     v = acc * sc[n] + sh[n];  if (act) v = v > 0 ? v : 0.2 v;  if (res) v += res[m][n]
// and two optional outputs of the first nvalid channels: fp32 rows out[m * ldo + n] and the three bf16 planes of v at
// out_planes[pl * M * ldp + m * ldp + n] -- bit-equal to rpb_split3 of the fp32 v.  Both pointers arrive at the first column the launch
// owns: two producers write disjoint column ranges of one plane buffer and the next convolution reads it directly, so neither a
// torch.cat nor an rpb_split3 pass exists in the model.  rpb_cno_pack writes the first layer's planes from the raw input.
// `res` may alias `out` element for element (same address, ldr == ldo): the lane that reads res[m][n] is the one that writes out[m][n]
// afterwards and no other lane touches that element -- the training step accumulates data gradients into one buffer that way.
// The main loop and the K-split reduction are conv3x_kernel's own text, csrc/rpb_conv3x_loop.h, included into both kernels (as text and
// not as a __device__ template: profiles/conv3_fwd_unify.txt; both files' device code is unchanged by it:
// profiles/conv3x_loop_share.txt).  What is written here is what differs: the arguments, the epilogue, the first layer's pack.
#include "rpb_mma.h"
#include <stdlib.h>

// ---------------------------------------------------------------------------------- the first layer's planes
// x [M][Cin] fp32 (1 <= Cin <= 64) -> P[3][M][64] bf16 with columns Cin..63 zero; one thread = 8 channels
__global__ __launch_bounds__(256) void cno_pack_kernel(const float* __restrict__ x, uint16_t* __restrict__ P, long M, int Cin) {
    const long total = M * 8;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long m = idx >> 3;
        const int c0 = (int)(idx & 7) * 8;
        unsigned h[8], md[8], lo[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float v = c0 + i < Cin ? x[m * Cin + c0 + i] : 0.f;
            split3(v, h[i], md[i], lo[i]);
        }
        u32x4 oh, om, ol;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            oh[q] = h[2 * q] | (h[2 * q + 1] << 16);
            om[q] = md[2 * q] | (md[2 * q + 1] << 16);
            ol[q] = lo[2 * q] | (lo[2 * q + 1] << 16);
        }
        const long o = m * 64 + c0;
        *reinterpret_cast<u32x4*>(P + o) = oh;
        *reinterpret_cast<u32x4*>(P + M * 64 + o) = om;
        *reinterpret_cast<u32x4*>(P + 2 * M * 64 + o) = ol;
    }
}

extern "C" int rpb_cno_pack(const float* x, void* planes, long M, int Cin, void* stream) {
    RPB_REQUIRE(x && planes && M > 0 && M < (1L << 31) && Cin >= 1 && Cin <= 64 && (uintptr_t)planes % 16 == 0,
                "cno_pack: bad arguments (M=%ld Cin=%d; 1 <= Cin <= 64, planes 16-byte aligned)", M, Cin);
    long grid = (M * 8 + 255) / 256;
    const long cap = (long)rpb_num_cus() * 16;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(cno_pack_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)planes, M, Cin);
    RPB_CHECK_LAUNCH("cno_pack");
}

// ---------------------------------------------------------------------------------- the convolution
struct CnoArgs {
    const uint16_t* P;     // [3][M][Ci] bf16 planes of the input tokens
    const uint16_t* Wz;    // B-operand order (rpb_conv3x_wprep)
    const float* sc;       // [N] folded BatchNorm scale (1 without BatchNorm, 0 on pad channels)
    const float* sh;       // [N] folded shift (bias without BatchNorm, 0 on pad channels)
    const float* res;      // [M][ldr] residual added after the activation step, or null
    float* out;            // [M][ldo], already at the first column this launch owns, or null
    uint16_t* op;          // [3][M][ldp] bf16 planes of the result, already at the first column, or null
    long M;
    int N, Ci, nvalid, act, ldr, ldo, ldp, T, H, W;
};

template <int WN>
__global__ __launch_bounds__(256, 1) void cno_conv3x_kernel(CnoArgs a) {
#include "rpb_conv3x_loop.h"      // leaves acc, red, CX_KSPLIT_SUM and the indices used below
    // ---- the CNO epilogue on the tiles this wave owns.  The owner's first K-split slot (8 KB = 32 tokens x 64 channels of fp32, read by
    // nobody else) is free once its partials are summed: the result goes through it so that a lane leaves with 8 consecutive channels
    // of one token -- 16 B per plane -- instead of one channel of 16 tokens (2-byte stores 2 * ldp apart).
    static_assert(KS > 1, "the plane transpose reuses the owner's first K-split slot");
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
        if (kp != tm % KS) continue;
        float* slot0 = red + ((nw * 4 + tm) * (KS - 1)) * 2048;
        CX_KSPLIT_SUM(tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int n = n0 + tn * 32 + col;
            const bool nok = n < a.nvalid;
            const float sc = a.sc[n], sh = a.sh[n];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + tm * 32 + mfma_row(lane, r);
                const bool ok = nok && m < a.M;
                float v = __builtin_fmaf(acc[tm][tn][r], sc, sh);
                if (a.act) v = v > 0.f ? v : 0.2f * v;
                if (a.res && ok) v += a.res[m * a.ldr + n];
                if (a.out && ok) a.out[m * a.ldo + n] = v;
                acc[tm][tn][r] = v;
            }
        }
        if (a.op) {
            // [32 tokens][64 channels]; tokens 4 apart (the two lane halves of one store) go to opposite bank halves
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mfma_row(lane, r);
                    slot0[row * 64 + ((tn * 32 + col) ^ ((row & 4) << 3))] = acc[tm][tn][r];
                }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the slot is this wave's own: no workgroup barrier
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = j * 8 + (lane >> 3), c8 = (lane & 7) * 8;
                const float* src = slot0 + row * 64 + (c8 ^ ((row & 4) << 3));
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
                unsigned h[8], md[8], lo[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    split3(v0[i], h[i], md[i], lo[i]);
                    split3(v1[i], h[4 + i], md[4 + i], lo[4 + i]);
                }
                u32x4 oh, om, ol;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    oh[q] = h[2 * q] | (h[2 * q + 1] << 16);
                    om[q] = md[2 * q] | (md[2 * q + 1] << 16);
                    ol[q] = lo[2 * q] | (lo[2 * q + 1] << 16);
                }
                const long m = m0 + tm * 32 + row;
                const int n = n0 + c8;
                if (m < a.M && n < a.nvalid) {                          // nvalid % 8 == 0 here: a run of 8 is inside or outside
                    uint16_t* dst = a.op + m * a.ldp + n;
                    const long pstride = a.M * (long)a.ldp;
                    *reinterpret_cast<u32x4*>(dst) = oh;
                    *reinterpret_cast<u32x4*>(dst + pstride) = om;
                    *reinterpret_cast<u32x4*>(dst + 2 * pstride) = ol;
                }
            }
            __builtin_amdgcn_wave_barrier();                            // (WN = 2: the next owned tile has its own slot)
        }
    }
}

extern "C" int rpb_cno_conv3x(const void* planes, const void* Wz, const float* sc, const float* sh, const float* res, float* out,
                              void* out_planes, long M, int N, int Ci, int nvalid, int act, int ldr, int ldo, int ldp, int Hc, int Wc,
                              int Dc, void* stream) {
    RPB_REQUIRE(planes && Wz && sc && sh && (out || out_planes) && M > 0 && M < (1L << 31), "cno_conv3x: bad arguments");
    RPB_REQUIRE(Ci > 0 && Ci % 64 == 0 && (N == 64 || N == 128) && nvalid >= 1 && nvalid <= N && (act == 0 || act == 1),
                "cno_conv3x: N=%d Ci=%d nvalid=%d act=%d unsupported (Ci %% 64, N = 64 or 128, 1 <= nvalid <= N, act 0 / 1)", N, Ci, nvalid, act);
    RPB_REQUIRE((uintptr_t)planes % 16 == 0 && (uintptr_t)Wz % 16 == 0, "cno_conv3x: planes and weights must be 16-byte aligned");
    RPB_REQUIRE(!out || ((uintptr_t)out % 4 == 0 && ldo >= nvalid), "cno_conv3x: ldo=%d < nvalid=%d", ldo, nvalid);
    RPB_REQUIRE(!res || ((uintptr_t)res % 4 == 0 && ldr >= nvalid), "cno_conv3x: ldr=%d < nvalid=%d", ldr, nvalid);
    RPB_REQUIRE(!out_planes || ((uintptr_t)out_planes % 16 == 0 && ldp % 8 == 0 && nvalid % 8 == 0 && ldp >= nvalid),
                "cno_conv3x: plane output needs a 16-byte aligned first column, ldp %% 8 == 0 and nvalid %% 8 == 0 (ldp=%d nvalid=%d)", ldp, nvalid);
    RPB_REQUIRE(Hc > 0 && Wc > 0 && Dc > 0 && M % ((long)Hc * Wc * Dc) == 0, "cno_conv3x: bad mesh");
    CnoArgs a{(const uint16_t*)planes, (const uint16_t*)Wz, sc, sh, res, out, (uint16_t*)out_planes, M, N, Ci, nvalid, act, ldr, ldo, ldp,
              Hc, Wc, Dc};
    const size_t lds = (size_t)2 * 24 * CX_ROWS * 16 + 9 * CX_ROWS + 16;
    const unsigned gx = (unsigned)(((M + CX_BM - 1) / CX_BM + 7) / 8 * 8);
    hipStream_t st = (hipStream_t)stream;
    (void)hipFuncSetAttribute((const void*)cno_conv3x_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)cno_conv3x_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (N == 64) {
        hipLaunchKernelGGL(cno_conv3x_kernel<1>, dim3(gx, 1), dim3(256), lds, st, a);
    } else {
        hipLaunchKernelGGL(cno_conv3x_kernel<2>, dim3(gx, 1), dim3(256), lds, st, a);
    }
    RPB_CHECK_LAUNCH("cno_conv3x");
}
