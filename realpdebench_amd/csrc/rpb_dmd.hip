// DMD baseline (realpdebench/model/dmd.py) -- the two passes over the input that are all of the model's device work
// (DESIGN.md section 18).  Everything the reference computes from its [n, T-1] snapshot matrices is a function of the T x T Gram
// matrix of the input frames, so the device forms G = X X^T, the host solves a problem of order T - 1, and the device applies the
// resulting [T-1, S] coefficient matrix to the frames:
//
//   rpb_dmd_gram     x [B][T][P][C] fp32, f <= C  ->  G [B][T][T] fp64,  G[b][i][j] = sum_{p, c < f} x[b][i][p][c] x[b][j][p][c]
//   rpb_dmd_predict  out[b][s][p][c] = sum_{k < T-1} M[b][k][s] x[b][k+1][p][c]  (c < f),  M fp64 [B][T-1][S], out fp32 [B][S][P][f]
//
// Both accumulate in fp64 on v_mfma_f64_16x16x4_f64 (the product of two fp32 values is exact in fp64; M has entries that cancel).
// Lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15], one double each; register r of the result holds
// D[row = (l >> 4) + 4 r][col = l & 15] -- NOT the row map of the other 16x16 MFMAs.
//
// Staging is shared: a workgroup of 4 waves copies a chunk of PTS points of every frame into LDS, reading whole C-wide cells with
// coalesced (16-byte where the row length allows) loads and keeping channels c < f, so that the LDS image is the gathered matrix
// [frame][PTS * f] in fp32; slots past the last point hold zeros.  The waves then read it in MFMA operand order and convert.
//   gram:    T <= 32 is a 2 x 2 grid of 16 x 16 tiles, three by symmetry; the diagonal tiles take the SAME register as A and B.
//            Rows >= T are zero at the operand read and never read from memory.  A workgroup walks chunks g, g + NG, ...; its four
//            waves' tiles are summed in wave order into part[b][g][T][T] (lower triangle), and rpb_dmd_gram's second launch sums the
//            NG partials in order and mirrors the lower triangle: no atomics, two calls are bit-equal, G is symmetric bit for bit.
//   predict: one workgroup per chunk; rows = S (two tiles), columns = 16 gathered elements, K = T - 1 padded to a multiple of 4 with
//            zero coefficients.  The coefficients of a lane stay in registers for the whole workgroup.
#include "rpb_common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define DMD_THREADS 256
#define DMD_WAVES 4
#define DMD_KC 256            // gathered elements (points x kept channels) of a frame per chunk, at the most
#define DMD_TMAX 32
#define DMD_KS_GRAM 260       // LDS row strides in floats: operand reads of 16 rows x 4 columns (gram) and of 4 rows x 16 columns
#define DMD_KS_PRED 272       // (predict) each touch 64 different banks

__device__ __forceinline__ f64x4 mfma64(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

static int dmd_pts(int f) { return (DMD_KC / f) & ~3; }      // points per chunk: a multiple of 4, so that pts * f is one too

// Frames [t0, t1) of one sample, source floats [src0, src0 + nsrc) of each (whole cells: src0 and nsrc are multiples of C), channels
// c < f kept: lds[(t - t0) * KS + cell * f + c].  Floats at or past rowlen read as zero.  VEC = 4 needs rowlen % 4 == 0, x 16-byte aligned.
template <int VEC, int KS>
__device__ __forceinline__ void dmd_stage(float* lds, const float* __restrict__ xb, int t0, int t1, long rowlen, long src0, int nsrc,
                                          int C, int f) {
    for (int t = t0; t < t1; ++t) {
        const float* row = xb + (long)t * rowlen;
        float* dst = lds + (t - t0) * KS;
        for (int e = threadIdx.x * VEC; e < nsrc; e += DMD_THREADS * VEC) {
            const long s = src0 + e;
            float v[VEC];
            if (VEC == 4) {
                f32x4 q = {0.f, 0.f, 0.f, 0.f};
                if (s + 3 < rowlen) q = RPB_SLD4(row + s);
#pragma unroll
                for (int i = 0; i < VEC; ++i) v[i] = q[i];
            } else {
                v[0] = s < rowlen ? __builtin_nontemporal_load(row + s) : 0.f;
            }
            unsigned cell = (unsigned)e / (unsigned)C;
            int c = e - (int)cell * C;
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                if (c < f) dst[cell * f + c] = v[i];
                if (++c == C) { c = 0; ++cell; }
            }
        }
    }
}

// ---------------------------------------------------------------------------------- Gram matrix
template <int VEC>
__global__ __launch_bounds__(DMD_THREADS) void dmd_gram_kernel(const float* __restrict__ x, double* __restrict__ part, int T, long P,
                                                               int C, int f, int pts, int NG) {
    __shared__ float stage[DMD_TMAX * DMD_KS_GRAM];
    __shared__ double red[DMD_WAVES][3][256];
    const int b = blockIdx.y, g = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rowlen = P * C;
    const float* xb = x + (long)b * T * rowlen;
    const int r0 = lane & 15, r1 = 16 + (lane & 15), kq = lane >> 4;
    const bool two = T > 16;
    f64x4 a00 = {0., 0., 0., 0.}, a10 = a00, a11 = a00;
    const long nchunk = (P + pts - 1) / pts;
    const int ksteps = pts * f / 4;
    for (long ch = g; ch < nchunk; ch += NG) {
        __syncthreads();                                   // the previous chunk's operand reads are done
        dmd_stage<VEC, DMD_KS_GRAM>(stage, xb, 0, T, rowlen, ch * pts * C, pts * C, C, f);
        __syncthreads();
        for (int ks = wave; ks < ksteps; ks += DMD_WAVES) {
            const int k = ks * 4 + kq;
            const double v0 = r0 < T ? (double)stage[r0 * DMD_KS_GRAM + k] : 0.;
            a00 = mfma64(v0, v0, a00);
            if (two) {                                     // uniform
                const double v1 = r1 < T ? (double)stage[r1 * DMD_KS_GRAM + k] : 0.;
                a10 = mfma64(v1, v0, a10);                 // rows 16.., columns 0..15
                a11 = mfma64(v1, v1, a11);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                          // red[wave][tile][row * 16 + col]
        const int o = (kq + 4 * r) * 16 + (lane & 15);
        red[wave][0][o] = a00[r];
        red[wave][1][o] = a10[r];
        red[wave][2][o] = a11[r];
    }
    __syncthreads();
    double* dst = part + ((long)b * NG + g) * T * T;
    for (int e = threadIdx.x; e < T * T; e += DMD_THREADS) {
        const int i = e / T, j = e - i * T;
        if (i < j) continue;                               // the finish reads the lower triangle only
        const int tile = i < 16 ? 0 : (j < 16 ? 1 : 2);
        const int o = (i & 15) * 16 + (j & 15);
        double s = red[0][tile][o];
#pragma unroll
        for (int w = 1; w < DMD_WAVES; ++w) s += red[w][tile][o];
        dst[e] = s;
    }
}

__global__ __launch_bounds__(DMD_THREADS) void dmd_gram_finish_kernel(const double* __restrict__ part, double* __restrict__ G, int T, int NG) {
    const int b = blockIdx.x;
    const double* src = part + (long)b * NG * T * T;
    double* dst = G + (long)b * T * T;
    for (int e = threadIdx.x; e < T * T; e += DMD_THREADS) {
        const int i = e / T, j = e - i * T;
        if (i < j) continue;
        double s = src[e];
        for (int g = 1; g < NG; ++g) s += src[(long)g * T * T + e];
        dst[i * T + j] = s;
        dst[j * T + i] = s;
    }
}

static bool dmd_shape_ok(int B, int T, long P, int C, int f) {
    return B > 0 && T >= 2 && T <= DMD_TMAX && P > 0 && C > 0 && f > 0 && f <= C && f <= 64 && C <= 4096 && P * C < (1L << 40);
}

extern "C" int rpb_dmd_gram_groups(int B, long P, int f) {
    if (B <= 0 || P <= 0 || f <= 0 || f > 64) return -1;
    const int pts = dmd_pts(f);
    const long nchunk = (P + pts - 1) / pts;
    long ng = (2L * rpb_num_cus() + B - 1) / B;            // about two workgroups per CU over the batch
    if (ng > 64) ng = 64;
    if (ng > nchunk) ng = nchunk;
    return (int)(ng < 1 ? 1 : ng);
}

extern "C" int rpb_dmd_gram(const float* x, double* G, double* part, int B, int T, long P, int C, int f, void* stream) {
    RPB_REQUIRE(x && G && part, "dmd_gram: null pointer");
    RPB_REQUIRE(dmd_shape_ok(B, T, P, C, f), "dmd_gram: needs 2 <= T <= 32, 1 <= f <= min(C, 64), C <= 4096 (B=%d T=%d P=%ld C=%d f=%d)", B, T,
                P, C, f);
    RPB_REQUIRE(B <= 65535, "dmd_gram: B = %d above 65535", B);
    const int pts = dmd_pts(f), NG = rpb_dmd_gram_groups(B, P, f);
    const bool vec = (P * C) % 4 == 0 && ((uintptr_t)x & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(dmd_gram_kernel<4>, dim3(NG, B), dim3(DMD_THREADS), 0, (hipStream_t)stream, x, part, T, P, C, f, pts, NG);
    else
        hipLaunchKernelGGL(dmd_gram_kernel<1>, dim3(NG, B), dim3(DMD_THREADS), 0, (hipStream_t)stream, x, part, T, P, C, f, pts, NG);
    hipLaunchKernelGGL(dmd_gram_finish_kernel, dim3(B), dim3(DMD_THREADS), 0, (hipStream_t)stream, part, G, T, NG);
    RPB_CHECK_LAUNCH("dmd_gram");
}

// ---------------------------------------------------------------------------------- prediction
template <int VEC>
__global__ __launch_bounds__(DMD_THREADS) void dmd_predict_kernel(const float* __restrict__ x, const double* __restrict__ M,
                                                                  float* __restrict__ out, int T, long P, int C, int f, int S, int pts) {
    __shared__ float stage[(DMD_TMAX - 1) * DMD_KS_PRED];
    const int b = blockIdx.y;
    const long ch = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long rowlen = P * C;
    const int K = T - 1, nks = (K + 3) / 4, kq = lane >> 4, col = lane & 15;
    const bool two = S > 16;
    // A operand: A[i = s][k] = M[b][k][s], zero outside [K) x [S)
    double m0[8], m1[8];
    const double* Mb = M + (long)b * K * S;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int k = ks * 4 + kq;
        m0[ks] = (k < K && col < S) ? Mb[(long)k * S + col] : 0.;
        m1[ks] = (k < K && 16 + col < S) ? Mb[(long)k * S + 16 + col] : 0.;
    }
    dmd_stage<VEC, DMD_KS_PRED>(stage, x + (long)b * T * rowlen, 1, T, rowlen, ch * pts * C, pts * C, C, f);
    __syncthreads();
    const long n = P * f, n0 = ch * pts * f;               // gathered elements of a frame; this chunk's first
    float* ob = out + (long)b * S * n;
    for (int ct = wave; ct * 16 < pts * f; ct += DMD_WAVES) {
        f64x4 d0 = {0., 0., 0., 0.}, d1 = d0;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            if (ks < nks) {                                // uniform
                const int k = ks * 4 + kq;
                const double v = k < K ? (double)stage[k * DMD_KS_PRED + ct * 16 + col] : 0.;
                d0 = mfma64(m0[ks], v, d0);
                if (two) d1 = mfma64(m1[ks], v, d1);
            }
        }
        const long e = n0 + ct * 16 + col;
        if (ct * 16 + col < pts * f && e < n) {            // pts * f is a multiple of 4, not of 16: the last tile may be partial
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int s0 = kq + 4 * r;
                if (s0 < S) ob[(long)s0 * n + e] = (float)d0[r];
                if (two && 16 + s0 < S) ob[(long)(16 + s0) * n + e] = (float)d1[r];
            }
        }
    }
}

extern "C" int rpb_dmd_predict(const float* x, const double* M, float* out, int B, int T, long P, int C, int f, int S, void* stream) {
    RPB_REQUIRE(x && M && out, "dmd_predict: null pointer");
    RPB_REQUIRE(dmd_shape_ok(B, T, P, C, f) && S >= 1 && S <= 32,
                "dmd_predict: needs 2 <= T <= 32, 1 <= S <= 32, 1 <= f <= min(C, 64), C <= 4096 (B=%d T=%d P=%ld C=%d f=%d S=%d)", B, T, P, C, f, S);
    RPB_REQUIRE(B <= 65535, "dmd_predict: B = %d above 65535", B);
    const int pts = dmd_pts(f);
    const long nchunk = (P + pts - 1) / pts;
    RPB_REQUIRE(nchunk < (1L << 31), "dmd_predict: P = %ld too large", P);
    const bool vec = (P * C) % 4 == 0 && ((uintptr_t)x & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(dmd_predict_kernel<4>, dim3((unsigned)nchunk, B), dim3(DMD_THREADS), 0, (hipStream_t)stream, x, M, out, T, P, C, f, S,
                           pts);
    else
        hipLaunchKernelGGL(dmd_predict_kernel<1>, dim3((unsigned)nchunk, B), dim3(DMD_THREADS), 0, (hipStream_t)stream, x, M, out, T, P, C, f, S,
                           pts);
    RPB_CHECK_LAUNCH("dmd_predict");
}
