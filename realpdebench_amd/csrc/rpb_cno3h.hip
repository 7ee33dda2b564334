// CNO3d on the opt-in "f16x2" eval arithmetic (CNO3d.set_arith("f16x2")): rpb_cno_conv3x_f16x2 is the implicit GEMM of
// conv3x_f16x2_kernel (csrc/rpb_conv3h.hip: same plane input P[2][M][Ci] fp16, same rpb_conv3x_wprep_f16x2 weights, same tiling, same
// three products hi*hi + hi*lo + lo*hi per fp32 product, exponents read from device memory) with the CNO epilogue of csrc/rpb_cno.hip
//     v = fmaf(acc * 2^-(ea + ew), sc[n], sh[n]);  if (act) v = v > 0 ? v : 0.2 v;  if (res) v += res[m][n]
// and fp32 rows out[m * ldo + n] of the first nvalid channels, at the first column the launch owns.
// There is no plane output.  The fp16 planes of an activation need max|v| * 2^e in fp16 range and that maximum exists only when every
// producer of the buffer has finished, so the epilogue cannot write them as the bf16x3 kernel does; what it can do is form the
// maximum: `amax` (a device word, may be null) receives atomicMax of bits(v) & 0x7fffffff over exactly the elements the launch writes
// (m < M, n < nvalid), reduced inside the wave first -- at most one atomic per wave.  The ordering rule is amax_bits_kernel's: for
// non-negative floats the integer order is the float order, NaN / inf patterns sort on top.  A maximum does not depend on the order of
// its operands, so outputs stay bit-reproducible.  Several producers (a concat) max into one word; rpb_amax_exp_finish then turns
// the word into the exponent and rpb_split2h writes the planes, once per buffer (model/cno.py).
// `res` may alias `out` element for element, as in rpb_cno_conv3x: the lane that reads res[m][n] is the one that writes out[m][n].
// The main loop is conv3x_f16x2_kernel's own text, csrc/rpb_conv3h_loop.h, included into both kernels; that kernel's device code is
// unchanged by it (profiles/cno_arith_probe.txt).  What is written here is what differs: the arguments, the epilogue, the first
// layer's pack.
#include "rpb_conv3h.h"
#include <stdlib.h>

extern "C" int rpb_amax_exp_finish(int* e, void* stream);

// ---------------------------------------------------------------------------------- the first layer's planes
// bits = max over x[0 .. total) of (|x| as an unsigned fp32 pattern); scalar loads: M * Cin is any number (Cin = 3, 5, ...)
__global__ __launch_bounds__(256) void cno_amax_flat_kernel(const float* __restrict__ x, long total, unsigned* __restrict__ bits) {
    unsigned mx = 0;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const unsigned u = __builtin_bit_cast(unsigned, x[idx]) & 0x7FFFFFFFu;
        mx = u > mx ? u : mx;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = __shfl_xor(mx, o);
        mx = t > mx ? t : mx;
    }
    if ((threadIdx.x & 63) == 0 && mx) atomicMax(bits, mx);
}

// x [M][Cin] fp32 (1 <= Cin <= 64) -> P[2][M][64] fp16 of x * 2^e with columns Cin..63 zero; one thread = 8 channels
__global__ __launch_bounds__(256) void cno_pack_f16x2_kernel(const float* __restrict__ x, uint16_t* __restrict__ P, long M, int Cin,
                                                             const int* __restrict__ ep) {
    const int e = *ep;
    const long total = M * 8;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long m = idx >> 3;
        const int c0 = (int)(idx & 7) * 8;
        unsigned h[8], lo[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float v = c0 + i < Cin ? x[m * Cin + c0 + i] : 0.f;
            split2h(v, e, h[i], lo[i]);
        }
        u32x4 oh, ol;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            oh[q] = h[2 * q] | (h[2 * q + 1] << 16);
            ol[q] = lo[2 * q] | (lo[2 * q + 1] << 16);
        }
        const long o = m * 64 + c0;
        *reinterpret_cast<u32x4*>(P + o) = oh;
        *reinterpret_cast<u32x4*>(P + M * 64 + o) = ol;
    }
}

extern "C" int rpb_cno_pack_f16x2(const float* x, void* planes, long M, int Cin, int* e, void* stream) {
    RPB_REQUIRE(x && planes && e && M > 0 && M < (1L << 31) && Cin >= 1 && Cin <= 64 && (uintptr_t)planes % 16 == 0,
                "cno_pack_f16x2: bad arguments (M=%ld Cin=%d; 1 <= Cin <= 64, planes 16-byte aligned)", M, Cin);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(e, 0, sizeof(int), st) != hipSuccess) RPB_FAIL(RPB_ERR_LAUNCH, "cno_pack_f16x2: memset failed");
    const long cap = (long)rpb_num_cus() * 16;
    long grid = (M * Cin + 255) / 256;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(cno_amax_flat_kernel, dim3((unsigned)grid), dim3(256), 0, st, x, M * Cin, (unsigned*)e);
    const int rc = rpb_amax_exp_finish(e, stream);
    if (rc != RPB_OK) return rc;
    grid = (M * 8 + 255) / 256;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(cno_pack_f16x2_kernel, dim3((unsigned)grid), dim3(256), 0, st, x, (uint16_t*)planes, M, Cin, e);
    RPB_CHECK_LAUNCH("cno_pack_f16x2");
}

// ---------------------------------------------------------------------------------- the convolution
struct Cno3hArgs {
    const uint16_t* P;     // [2][M][Ci] fp16 planes of the scaled input tokens
    const uint16_t* Wz;    // B-operand order (rpb_conv3x_wprep_f16x2)
    const float* sc;       // [N] folded BatchNorm scale (1 without BatchNorm, 0 on pad channels)
    const float* sh;       // [N] folded shift (bias without BatchNorm, 0 on pad channels)
    const float* res;      // [M][ldr] residual added after the activation step, or null
    float* out;            // [M][ldo], already at the first column this launch owns
    unsigned* amax;        // max of |v| bit patterns over what this launch writes, or null
    const int* ea;         // exponent of the activations
    const int* ew;         // exponent of the weights
    long M;
    int N, Ci, nvalid, act, ldr, ldo, T, H, W;
};

// One workgroup per CU, one wave per SIMD, as conv3x_f16x2_kernel (the comment there has the register count that decides it).
template <int WN>
__global__ __launch_bounds__(256, 1) void cno_conv3x_f16x2_kernel(Cno3hArgs a) {
#include "rpb_conv3h_loop.h"      // leaves acc, red, CH_KSPLIT_SUM and the indices used below
    static_assert(KS > 1, "every wave owns 4 / KS of the four row tiles");
    const int esum = -(*a.ea + *a.ew);
    unsigned mx = 0;
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
        if (kp != tm % KS) continue;
        CH_KSPLIT_SUM(tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int n = n0 + tn * 32 + col;
            const bool nok = n < a.nvalid;
            const float sc = a.sc[n], sh = a.sh[n];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + tm * 32 + mfma_row(lane, r);
                if (nok && m < a.M) {
                    float v = __builtin_fmaf(ldexpf(acc[tm][tn][r], esum), sc, sh);
                    if (a.act) v = v > 0.f ? v : 0.2f * v;
                    if (a.res) v += a.res[m * a.ldr + n];
                    a.out[m * a.ldo + n] = v;
                    const unsigned u = __builtin_bit_cast(unsigned, v) & 0x7FFFFFFFu;
                    mx = u > mx ? u : mx;
                }
            }
        }
    }
    if (a.amax) {                                                       // wave-uniform; every lane of the wave arrives here
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned t = __shfl_xor(mx, o);
            mx = t > mx ? t : mx;
        }
        if (lane == 0 && mx) atomicMax(a.amax, mx);
    }
}

// bytes of dynamic LDS: the two stage buffers + validity table, or the K-split reduction if larger (N = 64: 4 tiles x 3 sources x 8 KB)
static size_t cno3h_lds(int WN) {
    const size_t stage = (size_t)2 * 16 * CH_ROWS * 16 + 9 * CH_ROWS + 16;
    const size_t red = (size_t)WN * 4 * (4 / WN - 1) * 2048 * 4;
    return stage > red ? stage : red;
}

template <int WN>
static void cno3h_launch(const Cno3hArgs& a, unsigned gx, hipStream_t st) {
    const size_t lds = cno3h_lds(WN);
    (void)hipFuncSetAttribute((const void*)cno_conv3x_f16x2_kernel<WN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(cno_conv3x_f16x2_kernel<WN>, dim3(gx, 1), dim3(256), lds, st, a);
}

extern "C" int rpb_cno_conv3x_f16x2(const void* planes, const void* Wz, const float* sc, const float* sh, const float* res, float* out,
                                    int* amax, long M, int N, int Ci, int nvalid, int act, int ldr, int ldo, int Hc, int Wc, int Dc,
                                    const int* ea, const int* ew, void* stream) {
    RPB_REQUIRE(planes && Wz && sc && sh && out && ea && ew && M > 0 && M < (1L << 31), "cno_conv3x_f16x2: bad arguments");
    RPB_REQUIRE(Ci > 0 && Ci % 64 == 0 && (N == 64 || N == 128) && nvalid >= 1 && nvalid <= N && (act == 0 || act == 1),
                "cno_conv3x_f16x2: N=%d Ci=%d nvalid=%d act=%d unsupported (Ci %% 64, N = 64 or 128, 1 <= nvalid <= N, act 0 / 1)", N, Ci,
                nvalid, act);
    RPB_REQUIRE((uintptr_t)planes % 16 == 0 && (uintptr_t)Wz % 16 == 0, "cno_conv3x_f16x2: planes and weights must be 16-byte aligned");
    RPB_REQUIRE((uintptr_t)out % 4 == 0 && ldo >= nvalid, "cno_conv3x_f16x2: ldo=%d < nvalid=%d", ldo, nvalid);
    RPB_REQUIRE(!res || ((uintptr_t)res % 4 == 0 && ldr >= nvalid), "cno_conv3x_f16x2: ldr=%d < nvalid=%d", ldr, nvalid);
    RPB_REQUIRE((uintptr_t)amax % 4 == 0 && (uintptr_t)ea % 4 == 0 && (uintptr_t)ew % 4 == 0, "cno_conv3x_f16x2: misaligned amax / exponent word");
    RPB_REQUIRE(Hc > 0 && Wc > 0 && Dc > 0 && M % ((long)Hc * Wc * Dc) == 0, "cno_conv3x_f16x2: bad mesh");
    Cno3hArgs a{(const uint16_t*)planes, (const uint16_t*)Wz, sc, sh, res, out, (unsigned*)amax, ea, ew, M, N, Ci, nvalid, act, ldr, ldo,
                Hc, Wc, Dc};
    const unsigned gx = (unsigned)(((M + CH_BM - 1) / CH_BM + 7) / 8 * 8);
    hipStream_t st = (hipStream_t)stream;
    if (N == 64) cno3h_launch<1>(a, gx, st);
    else cno3h_launch<2>(a, gx, st);
    RPB_CHECK_LAUNCH("cno_conv3x_f16x2");
}
