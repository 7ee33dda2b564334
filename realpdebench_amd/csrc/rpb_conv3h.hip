// 3x3x3 convolution (padding 1) on the opt-in "f16x2" eval arithmetic: the implicit GEMM of rpb_conv3x.hip with every fp32
// operand written as TWO fp16 numbers, both rounded to nearest even, after an exact power-of-two rescale per tensor:
//   x * 2^e = hi + lo   (11 + 11 significand bits and the sign of lo: x to one fp32 unit in the last place)
// and a product accumulated in fp32 from the three fp16 x fp16 products hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16 (the
// bf16 rate on gfx950); the dropped term lo*lo is <= 2^-22 |a b|.  Three MFMAs instead of the six of the bf16x3 split.
// fp16 has 5 exponent bits, so each tensor is first scaled by 2^e with max|x| * 2^e in [2^14, 2^15) (rpb_amax_exp, computed and
// kept on the device: no host synchronisation); the lo plane of every element within 2^-16 of the maximum is then a normal or
// exactly representable subnormal fp16.  The epilogue undoes both scales: out = ldexp(acc, -(ea + ew)) + bias.
// Evaluation forward only (Transolver.set_arith / Unet3d.set_arith); training and data gradients stay on rpb_conv3x.
//
// Layout and tiling are those of conv3x_kernel: a workgroup owns 128 consecutive tokens, stages the 130 rows of each (kt, kh) and
// 64-channel chunk in LDS (two planes: 2 x 33 KB per stage buffer instead of 2 x 50 KB), the w boundary is applied to the A operand,
// weights are pre-arranged in MFMA B-operand order Wz[tap][Ci/16][2 planes][N/32][64 lanes][8] fp16.
// The kernel stays a second text next to conv3x_kernel on purpose.  One body for both plane schemes was tried two ways with hipcc 7.2
// (profiles/conv3_fwd_unify.txt): as a forced-inline __device__ template it is optimised on its own before it is inlined, without
// the kernel's launch bounds, and every instance came out differently (other loop duplication, 1.5x the v_accvgpr moves); as one
// text included into both kernels the bf16x3 instances kept their code and speed, but conv3x_f16x2_kernel<1> went from
// 368 VGPRs + 128 AGPRs to 496 + 256 and from 1.85 to 2.15 ms at the U-Net 64 -> 64 shape.  Outputs were bit-equal in both forms.
// The bf16x3 loop is shared in that second form since: csrc/rpb_conv3x_loop.h is the one text of conv3x_kernel and cno_conv3x_kernel.
// The f16x2 loop likewise: csrc/rpb_conv3h_loop.h is the one text of conv3x_f16x2_kernel here and cno_conv3x_f16x2_kernel
// (csrc/rpb_cno3h.hip); the tile constants and split2h are in csrc/rpb_conv3h.h.  This file's device code is unchanged by either.
#include "rpb_conv3h.h"
#include <stdlib.h>

// ---------------------------------------------------------------------------------- per-tensor exponent
// bits = max over the tensor of (|x| as an unsigned fp32 pattern): for non-negative floats the integer order is the float order,
// and NaN / inf patterns sort above every finite value
__global__ __launch_bounds__(256) void amax_bits_kernel(const float* __restrict__ x, long M, int C, int ldx, unsigned* __restrict__ bits) {
    const int c4n = C >> 2;
    const long total = M * c4n;
    unsigned mx = 0;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long m = idx / c4n;
        const int c4 = (int)(idx - m * c4n);
        // loaded as unsigned: a bit cast of each element of an f32x4 compiled to a compare of element 0 only
        const u32x4 v = *reinterpret_cast<const u32x4*>(x + m * ldx + c4 * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned u = v[i] & 0x7FFFFFFFu;
            mx = u > mx ? u : mx;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = __shfl_xor(mx, o);
        mx = t > mx ? t : mx;
    }
    __shared__ unsigned wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned r = wm[0];
        for (int w = 1; w < 4; ++w) r = wm[w] > r ? wm[w] : r;
        atomicMax(bits, r);
    }
}

// bits -> e with max|x| * 2^e in [2^14, 2^15); 0 for an all-zero or non-finite tensor.  The binary exponent is read from the bits
// (normal: biased exponent - 127; subnormal: position of the leading one - 149).
__global__ void amax_exp_finish_kernel(int* e) {
    const unsigned b = (unsigned)e[0];
    int r = 0;
    if (b != 0 && b < 0x7F800000u) r = 14 - (b >= 0x00800000u ? (int)(b >> 23) - 127 : (31 - __builtin_clz(b)) - 149);
    e[0] = r;
}

extern "C" int rpb_amax_exp(const float* x, long M, int C, int ldx, int* e, void* stream) {
    RPB_REQUIRE(x && e && M > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldx >= C, "amax_exp: bad arguments (C=%d ldx=%d)", C, ldx);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(e, 0, sizeof(int), st) != hipSuccess) RPB_FAIL(RPB_ERR_LAUNCH, "amax_exp: memset failed");
    const long total = M * (C / 4);
    long grid = (total + 255) / 256;
    const long cap = (long)rpb_num_cus() * 4;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(amax_bits_kernel, dim3((unsigned)grid), dim3(256), 0, st, x, M, C, ldx, (unsigned*)e);
    hipLaunchKernelGGL(amax_exp_finish_kernel, dim3(1), dim3(1), 0, st, e);
    RPB_CHECK_LAUNCH("amax_exp");
}

// the second half of rpb_amax_exp on its own: e[0] holds the maximum of |x| bit patterns that several launches formed with atomicMax
// (the epilogue of rpb_cno_conv3x_f16x2, csrc/rpb_cno3h.hip) and becomes the exponent
extern "C" int rpb_amax_exp_finish(int* e, void* stream) {
    RPB_REQUIRE(e, "amax_exp_finish: null pointer");
    hipLaunchKernelGGL(amax_exp_finish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, e);
    RPB_CHECK_LAUNCH("amax_exp_finish");
}

// ---------------------------------------------------------------------------------- activation planes
// x [M][ldx] fp32 (C channels used) -> P[2][M][C] fp16 of x * 2^e; one thread = 8 channels (32 B in, 2 x 16 B out)
__global__ __launch_bounds__(256) void split2h_kernel(const float* __restrict__ x, uint16_t* __restrict__ P, long M, int C, int ldx,
                                                      const int* __restrict__ ep) {
    const int e = *ep;
    const int c8n = C >> 3;
    const long total = M * c8n;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long m = idx / c8n;
        const int c8 = (int)(idx - m * c8n);
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + m * ldx + c8 * 8);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(x + m * ldx + c8 * 8 + 4);
        unsigned h[8], lo[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            split2h(v0[i], e, h[i], lo[i]);
            split2h(v1[i], e, h[4 + i], lo[4 + i]);
        }
        uint4 oh, ol;
        oh.x = h[0] | (h[1] << 16); oh.y = h[2] | (h[3] << 16); oh.z = h[4] | (h[5] << 16); oh.w = h[6] | (h[7] << 16);
        ol.x = lo[0] | (lo[1] << 16); ol.y = lo[2] | (lo[3] << 16); ol.z = lo[4] | (lo[5] << 16); ol.w = lo[6] | (lo[7] << 16);
        const long o = m * C + c8 * 8;
        *reinterpret_cast<uint4*>(P + o) = oh;
        *reinterpret_cast<uint4*>(P + M * C + o) = ol;
    }
}

extern "C" int rpb_split2h(const float* x, void* planes, long M, int C, int ldx, const int* e, void* stream) {
    RPB_REQUIRE(x && planes && e && M > 0 && C > 0 && C % 8 == 0 && ldx % 4 == 0 && ldx >= C, "split2h: bad arguments (C=%d ldx=%d)", C, ldx);
    const long total = M * (C / 8);
    long grid = (total + 255) / 256;
    const long cap = (long)rpb_num_cus() * 16;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(split2h_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)planes, M, C, ldx, e);
    RPB_CHECK_LAUNCH("split2h");
}

// ---------------------------------------------------------------------------------- weights in B-operand order
// W [N][27 * Ci] fp32 -> Wz[tap][Ci/16][2 planes][N/32][64 lanes][8] fp16 of W * 2^e, lane = (co & 31) + 32 * k-half,
// element j <-> ci = 16 cc + 8 half + j (the order of conv3x_wprep with two planes)
__global__ __launch_bounds__(256) void conv3x_wprep_f16x2_kernel(const float* __restrict__ W, uint16_t* __restrict__ Wz, int N, int Ci,
                                                                 const int* __restrict__ ep) {
    const int NT = N >> 5, NCC = Ci >> 4;
    const long total = 27L * NCC * NT * 64;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int e = *ep;
    const int lane = (int)(idx & 63);
    long r = idx >> 6;
    const int nt = (int)(r % NT);
    r /= NT;
    const int cc = (int)(r % NCC);
    const int tap = (int)(r / NCC);
    const int co = nt * 32 + (lane & 31), half = lane >> 5;
    const float* src = W + (long)co * 27 * Ci + (long)tap * Ci + cc * 16 + half * 8;
    unsigned h[8], lo[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) split2h(src[j], e, h[j], lo[j]);
    uint4 o[2];
    o[0].x = h[0] | (h[1] << 16); o[0].y = h[2] | (h[3] << 16); o[0].z = h[4] | (h[5] << 16); o[0].w = h[6] | (h[7] << 16);
    o[1].x = lo[0] | (lo[1] << 16); o[1].y = lo[2] | (lo[3] << 16); o[1].z = lo[4] | (lo[5] << 16); o[1].w = lo[6] | (lo[7] << 16);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const long dst = (((((long)tap * NCC + cc) * 2 + p) * NT + nt) * 64 + lane) * 8;
        *reinterpret_cast<uint4*>(Wz + dst) = o[p];
    }
}

extern "C" int rpb_conv3x_wprep_f16x2(const float* W, void* Wz, int N, int Ci, const int* e, void* stream) {
    RPB_REQUIRE(W && Wz && e && N > 0 && N % 32 == 0 && Ci > 0 && Ci % 16 == 0, "conv3x_wprep_f16x2: N=%d Ci=%d unsupported", N, Ci);
    const long total = 27L * (Ci / 16) * (N / 32) * 64;
    hipLaunchKernelGGL(conv3x_wprep_f16x2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W,
                       (uint16_t*)Wz, N, Ci, e);
    RPB_CHECK_LAUNCH("conv3x_wprep_f16x2");
}

// ---------------------------------------------------------------------------------- the convolution
struct Conv3hArgs {
    const uint16_t* P;     // [2][M][Ci] fp16 planes of the scaled input tokens
    const uint16_t* Wz;    // B-operand order, see above
    const float* bias;     // [N] or null
    float* out;            // [M][ldo]
    const int* ea;         // exponent of the activations
    const int* ew;         // exponent of the weights
    long M;
    int N, Ci, ldo, T, H, W;
};

// WN: waves over co (64 each), KS = 4 / WN split the 16-channel chunks of a stage.  One workgroup per CU, one wave per SIMD, as
// conv3x_kernel: the two-plane stage pair (66.6 KB of LDS) would fit two workgroups per CU, but at the 256 registers per wave that
// allows the N >= 128 instances spill 35 / 46 VGPRs to scratch (-Rpass-analysis=kernel-resource-usage: 128 accumulators + 36 staging
// + 48 operand registers); with the whole register file they hold 168-239 VGPRs + 128 AGPRs and no spill.
template <int WN>
__global__ __launch_bounds__(256, 1) void conv3x_f16x2_kernel(Conv3hArgs a) {
#include "rpb_conv3h_loop.h"     // leaves acc, red (the parked K-split partials) and the indices used below
    const int esum = -(*a.ea + *a.ew);
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
        if (KS > 1 && kp != tm % KS) continue;
        if (KS > 1) {
#pragma unroll
            for (int k2 = 0; k2 < KS - 1; ++k2) {
                const float* slot = red + ((nw * 4 + tm) * (KS - 1) + k2) * 2048;
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[tm][tn][r] += slot[(tn * 16 + r) * 64 + lane];
            }
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int n = n0 + tn * 32 + col;
            const float bv = a.bias ? a.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + tm * 32 + mfma_row(lane, r);
                if (m < a.M) a.out[m * a.ldo + n] = ldexpf(acc[tm][tn][r], esum) + bv;
            }
        }
    }
}

// bytes of dynamic LDS: the two stage buffers + validity table, or the K-split reduction if larger (N = 64: 4 tiles x 3 sources x 8 KB)
static size_t conv3h_lds(int WN) {
    const size_t stage = (size_t)2 * 16 * CH_ROWS * 16 + 9 * CH_ROWS + 16;
    const size_t red = (size_t)WN * 4 * (4 / WN - 1) * 2048 * 4;
    return stage > red ? stage : red;
}

template <int WN>
static void conv3h_launch(const Conv3hArgs& a, unsigned gx, unsigned gy, hipStream_t st) {
    const size_t lds = conv3h_lds(WN);
    (void)hipFuncSetAttribute((const void*)conv3x_f16x2_kernel<WN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(conv3x_f16x2_kernel<WN>, dim3(gx, gy), dim3(256), lds, st, a);
}

extern "C" int rpb_conv3x_f16x2(const void* planes, const void* Wz, const float* bias, float* out, long M, int N, int Ci, int ldo,
                                int Hc, int Wc, int Dc, const int* ea, const int* ew, void* stream) {
    RPB_REQUIRE(planes && Wz && out && ea && ew && M > 0 && M < (1L << 31), "conv3x_f16x2: bad arguments");
    RPB_REQUIRE(Ci % 64 == 0 && (N == 64 || N == 128 || N % 256 == 0) && ldo >= N,
                "conv3x_f16x2: N=%d Ci=%d unsupported (Ci %% 64, N = 64, 128 or a multiple of 256)", N, Ci);
    RPB_REQUIRE(Hc > 0 && Wc > 0 && Dc > 0 && M % ((long)Hc * Wc * Dc) == 0, "conv3x_f16x2: bad mesh");
    Conv3hArgs a{(const uint16_t*)planes, (const uint16_t*)Wz, bias, out, ea, ew, M, N, Ci, ldo, Hc, Wc, Dc};
    const unsigned gx = (unsigned)(((M + CH_BM - 1) / CH_BM + 7) / 8 * 8);
    hipStream_t st = (hipStream_t)stream;
    if (N == 64) conv3h_launch<1>(a, gx, 1, st);
    else if (N == 128) conv3h_launch<2>(a, gx, 1, st);
    else conv3h_launch<4>(a, gx, N / 256, st);
    RPB_CHECK_LAUNCH("conv3x_f16x2");
}
