// MWT3d (multiwavelet operator, reference realpdebench/model/MWT_libs/models.py:498-790) -- evaluation forward.
// Activations are channels-last fp32 [B][Nx][Ny][T][36] (36 = c * k^2 = 4 * 9; one cell = 144 B), so no reference permute exists here.
// The FLOP carrier is rpb_mwt_conv3 (3x3x3 convolution at 36 channels + ReLU + Linear(36, 36)) on v_mfma_f32_16x16x4_f32: the 36 output
// channels are padded to 48 = 3 row tiles in REGISTERS (never in HBM), cells are the MFMA columns.  Everything else is a streaming or a
// tiny kernel on the vector unit.  No kernel uses atomics: two calls give bit-equal results.
#include "rpb_common.h"
#include "rpb_mwt_conv3.h"      // MWT_C = 36 = c * k^2; mwt_conv3_k, mwt_spec_out_k

#define MWT_K2 9       // k^2
#define MWT_NC 4       // c

static inline unsigned mwt_blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }

// ---------------------------------------------------------------------------------- lift: [B,T,H,W,Cin] permute + Lk
__global__ __launch_bounds__(256) void mwt_lift_k(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                  float* __restrict__ out, long ncell, int T, int H, int W, int Cin) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= ncell * MWT_C) return;
    const int o = (int)(i % MWT_C);
    long q = i / MWT_C;                       // output cell (b, h, w, t)
    const int t = (int)(q % T);
    q /= T;
    const int yw = (int)(q % W);
    q /= W;
    const int xh = (int)(q % H);
    const long bb = q / H;
    const float* xi = x + (((bb * T + t) * H + xh) * W + yw) * Cin;
    float acc = b[o];
    for (int c = 0; c < Cin; ++c) acc = fmaf(xi[c], w[o * Cin + c], acc);
    out[i] = acc;
}

// ---------------------------------------------------------------------------------- wavelet_transform (models.py:683-691)
// x [B][2Nx][2Ny][T][4][9] -> d, s [B][Nx][Ny][T][4][9]; ecd / ecs [36][9], rows = (quadrant ee|eo|oe|oo, n)
__global__ __launch_bounds__(256) void mwt_decompose_k(const float* __restrict__ x, const float* __restrict__ ecd,
                                                       const float* __restrict__ ecs, float* __restrict__ d, float* __restrict__ s,
                                                       long nout, int Nx, int Ny, int T) {
    __shared__ float sd[MWT_C * MWT_K2], ss[MWT_C * MWT_K2];
    for (int i = threadIdx.x; i < MWT_C * MWT_K2; i += 256) {
        sd[i] = ecd[i];
        ss[i] = ecs[i];
    }
    __syncthreads();
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= nout * MWT_C) return;
    const int m = (int)(i % MWT_K2), cc = (int)((i / MWT_K2) % MWT_NC);
    long q = i / MWT_C;
    const int t = (int)(q % T);
    q /= T;
    const int y = (int)(q % Ny);
    q /= Ny;
    const int xx = (int)(q % Nx);
    const long bb = q / Nx;
    float ad = 0.f, as = 0.f;
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const int dx = qd >> 1, dy = qd & 1;
        const float* src = x + ((((bb * 2 * Nx + 2 * xx + dx) * (2L * Ny) + 2 * y + dy) * T + t) * MWT_C + cc * MWT_K2);
#pragma unroll
        for (int n = 0; n < MWT_K2; ++n) {
            const float v = src[n];
            ad = fmaf(v, sd[(qd * MWT_K2 + n) * MWT_K2 + m], ad);
            as = fmaf(v, ss[(qd * MWT_K2 + n) * MWT_K2 + m], as);
        }
    }
    d[i] = ad;
    s[i] = as;
}

// ---------------------------------------------------------------------------------- evenOdd (models.py:676-678, 694-709)
// x [B][Nx][xNy][T][36] (xNy = Ny, or 1 = broadcast along Ny: the coarsest level of a W = 2H grid), us / ud [B][Nx][Ny][T][36],
// rc [4 (ee|eo|oe|oo)][18][9] -> out [B][2Nx][2Ny][T][36], ReLU when `relu`
__global__ __launch_bounds__(256) void mwt_reconstruct_k(const float* __restrict__ x, const float* __restrict__ us,
                                                         const float* __restrict__ ud, const float* __restrict__ rc,
                                                         float* __restrict__ out, long ncell, int Nx, int Ny, int T, int xNy, int relu) {
    __shared__ float sr[4 * 18 * MWT_K2];
    for (int i = threadIdx.x; i < 4 * 18 * MWT_K2; i += 256) sr[i] = rc[i];
    __syncthreads();
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= ncell * MWT_C) return;
    const int m = (int)(i % MWT_K2), cc = (int)((i / MWT_K2) % MWT_NC);
    const long cell = i / MWT_C;
    long q = cell;
    const int t = (int)(q % T);
    q /= T;
    const int y = (int)(q % Ny);
    q /= Ny;
    const int xx = (int)(q % Nx);
    const long bb = q / Nx;
    const long xq = ((bb * Nx + xx) * xNy + (xNy == Ny ? y : 0)) * T + t;
    float in[18];
#pragma unroll
    for (int n = 0; n < MWT_K2; ++n) {
        in[n] = x[xq * MWT_C + cc * MWT_K2 + n] + us[cell * MWT_C + cc * MWT_K2 + n];
        in[MWT_K2 + n] = ud[cell * MWT_C + cc * MWT_K2 + n];
    }
#pragma unroll
    for (int qd = 0; qd < 4; ++qd) {
        const int dx = qd >> 1, dy = qd & 1;
        float acc = 0.f;
#pragma unroll
        for (int n = 0; n < 18; ++n) acc = fmaf(in[n], sr[(qd * 18 + n) * MWT_K2 + m], acc);
        if (relu) acc = fmaxf(acc, 0.f);
        out[(((bb * 2 * Nx + 2 * xx + dx) * (2L * Ny) + 2 * y + dy) * T + t) * MWT_C + cc * MWT_K2 + m] = acc;
    }
}

// ---------------------------------------------------------------------------------- T0 on the coarsest view (models.py:666-672)
// in: rows of K = 36 * shape_multiplier floats (the row-major reinterpretation of [B][1][mult][T][36]); w [36][K]
__global__ __launch_bounds__(256) void mwt_coarse_k(const float* __restrict__ in, const float* __restrict__ w, const float* __restrict__ b,
                                                    float* __restrict__ out, long rows, int K) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= rows * MWT_C) return;
    const int o = (int)(i % MWT_C);
    const float* src = in + (i / MWT_C) * K;
    float acc = b[o];
    for (int k = 0; k < K; ++k) acc = fmaf(src[k], w[o * K + k], acc);
    out[i] = acc;
}

// ---------------------------------------------------------------------------------- one truncated-DFT stage along a strided axis
// out[outer][o][inner] = sum_k M[o][k] in[outer][k][inner]   (the dft.py stage convention; M is [O][K] real)
__global__ __launch_bounds__(256) void mwt_axis_k(const float* __restrict__ in, const float* __restrict__ M, float* __restrict__ out,
                                                  long total, int O, int K, long inner) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= total) return;
    const long in_ = i % inner;
    const int o = (int)((i / inner) % O);
    const long ou = i / (inner * O);
    const float* src = in + ou * K * inner + in_;
    const float* mr = M + (long)o * K;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) acc = fmaf(mr[k], src[k * inner], acc);
    out[i] = acc;
}

// ---------------------------------------------------------------------------------- per-bin 36 x 36 complex contraction
// X, Y [B][2 (re|im)][NB][36]; Wt [4 blocks * 125 modes][36 in][36 out][2]; tab[bin] = block * 125 + (ix * 5 + iy) * 5 + kt -- the weight
// element that the LAST of the four sequential corner assignments of models.py:569-576 puts on that bin
__global__ __launch_bounds__(256) void mwt_modes_k(const float* __restrict__ X, const float* __restrict__ Wt, const int* __restrict__ tab,
                                                   float* __restrict__ Y, int B, int NB) {
    const long i = blockIdx.x * 256L + threadIdx.x;
    if (i >= (long)B * NB * MWT_C) return;
    const int o = (int)(i % MWT_C);
    const int bin = (int)((i / MWT_C) % NB);
    const long bb = i / ((long)MWT_C * NB);
    const float* xr = X + ((bb * 2 + 0) * NB + bin) * MWT_C;
    const float* xi = X + ((bb * 2 + 1) * NB + bin) * MWT_C;
    const float* w = Wt + (long)tab[bin] * MWT_C * MWT_C * 2;
    float yr = 0.f, yi = 0.f;
    for (int c = 0; c < MWT_C; ++c) {
        const float wr = w[(c * MWT_C + o) * 2], wi = w[(c * MWT_C + o) * 2 + 1];
        const float a = xr[c], b = xi[c];
        yr = fmaf(a, wr, yr);
        yr = fmaf(-b, wi, yr);
        yi = fmaf(a, wi, yi);
        yi = fmaf(b, wr, yi);
    }
    Y[((bb * 2 + 0) * NB + bin) * MWT_C + o] = yr;
    Y[((bb * 2 + 1) * NB + bin) * MWT_C + o] = yi;
}

// ---------------------------------------------------------------------------------- last inverse stage (c2r along T) + ReLU + Lo (+=),
// ---------------------------------------------------------------------------------- 3x3x3 conv + bias + ReLU + Lo + bias (+=):
// mwt_spec_out_k<false> and mwt_conv3_k<MWT_CONV_EVAL> of rpb_mwt_conv3.h: the kernel texts are shared with the training step
// (rpb_mwt_train.hip), whose variants keep one more tensor each; the instances here are the evaluation forward's.

// weights [36 co][36 ci][27] , lo [36][36] -> wp [27][9][3][64], lop [3][4][3][64] (zeros on the pad rows)
__global__ void mwt_conv3_wprep_k(const float* __restrict__ w, const float* __restrict__ lo, float* __restrict__ wp, float* __restrict__ lop) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int NW = 27 * 9 * 3 * 64, NL = 3 * 4 * 3 * 64;
    if (i < NW) {
        const int lane = i & 63, t = (i >> 6) % 3, j = (i / 192) % 9, tap = i / (192 * 9);
        const int co = 16 * t + (lane & 15), ci = 9 * (lane >> 4) + j;
        wp[i] = co < MWT_C ? w[(co * MWT_C + ci) * 27 + tap] : 0.f;
    } else if (i < NW + NL) {
        const int k = i - NW;
        const int lane = k & 63, u = (k >> 6) % 3, r = (k / 192) % 4, t = k / (192 * 4);
        const int o = 16 * u + (lane & 15), c = 16 * t + 4 * (lane >> 4) + r;
        lop[k] = (o < MWT_C && c < MWT_C) ? lo[o * MWT_C + c] : 0.f;
    }
}

// ---------------------------------------------------------------------------------- head: Lc0, ReLU, Lc1, output permute (models.py:770-779)
// x [B][Nx][Ny][T][36]; w0t [36][128]; w1 [dout = Cout * r][128] -> out [B][T * r][Nx][Ny][Cout], out[.., t r + j, .., co] = y[co r + j]
#define MWT_HID 128
__global__ __launch_bounds__(256) void mwt_head_k(const float* __restrict__ x, const float* __restrict__ w0t, const float* __restrict__ b0,
                                                  const float* __restrict__ w1, const float* __restrict__ b1, float* __restrict__ out,
                                                  long ncell, int Nx, int Ny, int T, int Cout, int r) {
    __shared__ float xin[8][MWT_C];
    __shared__ float hid[8][MWT_HID + 1];
    const int tid = threadIdx.x, h = tid & 127, half = tid >> 7;
    float w0[MWT_C];
#pragma unroll
    for (int c = 0; c < MWT_C; ++c) w0[c] = w0t[c * MWT_HID + h];
    const float bh = b0[h];
    const int dout = Cout * r;
    for (long g0 = blockIdx.x * 8L; g0 < ncell; g0 += gridDim.x * 8L) {       // block-uniform trip count
        for (int i = tid; i < 8 * MWT_C; i += 256) {
            const long q = g0 + i / MWT_C;
            xin[i / MWT_C][i % MWT_C] = q < ncell ? x[q * MWT_C + i % MWT_C] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ci = half; ci < 8; ci += 2) {
            float acc = bh;
#pragma unroll
            for (int c = 0; c < MWT_C; ++c) acc = fmaf(w0[c], xin[ci][c], acc);
            hid[ci][h] = fmaxf(acc, 0.f);
        }
        __syncthreads();
        const int ci = tid >> 5, l32 = tid & 31;
        long q = g0 + ci;
        const bool ok = q < ncell;
        const int t = (int)(q % T);
        q /= T;
        const int y = (int)(q % Ny);
        q /= Ny;
        const int xx = (int)(q % Nx);
        const long bb = q / Nx;
        for (int od = 0; od < dout; ++od) {
            float p = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) p = fmaf(w1[od * MWT_HID + l32 + 32 * k], hid[ci][l32 + 32 * k], p);
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) p += __shfl_xor(p, off, 64);
            if (ok && l32 == 0) {
                const int co = od / r, j = od % r;
                out[(((bb * T * r + (long)t * r + j) * Nx + xx) * Ny + y) * Cout + co] = p + b1[od];
            }
        }
        __syncthreads();
    }
}

// ================================================================================== C ABI
#define MWT_STREAM (static_cast<hipStream_t>(stream))

extern "C" int rpb_mwt_lift(const float* x, const float* w, const float* b, float* out, int B, int T, int H, int W, int Cin, void* stream) {
    RPB_REQUIRE(x && w && b && out, "rpb_mwt_lift: null pointer");
    RPB_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && Cin > 0 && Cin <= 64, "rpb_mwt_lift: bad shape B=%d T=%d H=%d W=%d Cin=%d", B, T, H, W, Cin);
    const long ncell = (long)B * T * H * W;
    hipLaunchKernelGGL(mwt_lift_k, dim3(mwt_blocks(ncell * MWT_C, 256)), dim3(256), 0, MWT_STREAM, x, w, b, out, ncell, T, H, W, Cin);
    RPB_CHECK_LAUNCH("rpb_mwt_lift");
}

extern "C" int rpb_mwt_decompose(const float* x, const float* ec_d, const float* ec_s, float* d, float* s, int B, int Nx, int Ny, int T,
                                 void* stream) {
    RPB_REQUIRE(x && ec_d && ec_s && d && s, "rpb_mwt_decompose: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0, "rpb_mwt_decompose: bad output shape B=%d Nx=%d Ny=%d T=%d", B, Nx, Ny, T);
    const long nout = (long)B * Nx * Ny * T;
    hipLaunchKernelGGL(mwt_decompose_k, dim3(mwt_blocks(nout * MWT_C, 256)), dim3(256), 0, MWT_STREAM, x, ec_d, ec_s, d, s, nout, Nx, Ny, T);
    RPB_CHECK_LAUNCH("rpb_mwt_decompose");
}

extern "C" int rpb_mwt_reconstruct(const float* x, const float* us, const float* ud, const float* rc, float* out, int B, int Nx, int Ny,
                                   int T, int xNy, int relu, void* stream) {
    RPB_REQUIRE(x && us && ud && rc && out, "rpb_mwt_reconstruct: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0, "rpb_mwt_reconstruct: bad shape B=%d Nx=%d Ny=%d T=%d", B, Nx, Ny, T);
    RPB_REQUIRE(xNy == Ny || xNy == 1, "rpb_mwt_reconstruct: x spans %d columns, needs %d or 1 (broadcast)", xNy, Ny);
    const long ncell = (long)B * Nx * Ny * T;
    hipLaunchKernelGGL(mwt_reconstruct_k, dim3(mwt_blocks(ncell * MWT_C, 256)), dim3(256), 0, MWT_STREAM, x, us, ud, rc, out, ncell, Nx, Ny,
                       T, xNy, relu);
    RPB_CHECK_LAUNCH("rpb_mwt_reconstruct");
}

extern "C" int rpb_mwt_coarse(const float* in, const float* w, const float* b, float* out, long rows, int K, void* stream) {
    RPB_REQUIRE(in && w && b && out, "rpb_mwt_coarse: null pointer");
    RPB_REQUIRE(rows > 0 && K > 0 && K % MWT_C == 0, "rpb_mwt_coarse: rows=%ld K=%d (K must be a multiple of 36)", rows, K);
    hipLaunchKernelGGL(mwt_coarse_k, dim3(mwt_blocks(rows * MWT_C, 256)), dim3(256), 0, MWT_STREAM, in, w, b, out, rows, K);
    RPB_CHECK_LAUNCH("rpb_mwt_coarse");
}

extern "C" int rpb_mwt_axis(const float* in, const float* M, float* out, long outer, int O, int K, long inner, void* stream) {
    RPB_REQUIRE(in && M && out, "rpb_mwt_axis: null pointer");
    RPB_REQUIRE(outer > 0 && O > 0 && K > 0 && inner > 0, "rpb_mwt_axis: bad shape outer=%ld O=%d K=%d inner=%ld", outer, O, K, inner);
    const long total = outer * O * inner;
    hipLaunchKernelGGL(mwt_axis_k, dim3(mwt_blocks(total, 256)), dim3(256), 0, MWT_STREAM, in, M, out, total, O, K, inner);
    RPB_CHECK_LAUNCH("rpb_mwt_axis");
}

extern "C" int rpb_mwt_modes(const float* X, const float* Wt, const int* tab, float* Y, int B, int NB, void* stream) {
    RPB_REQUIRE(X && Wt && tab && Y, "rpb_mwt_modes: null pointer");
    RPB_REQUIRE(B > 0 && NB > 0, "rpb_mwt_modes: bad shape B=%d NB=%d", B, NB);
    hipLaunchKernelGGL(mwt_modes_k, dim3(mwt_blocks((long)B * NB * MWT_C, 256)), dim3(256), 0, MWT_STREAM, X, Wt, tab, Y, B, NB);
    RPB_CHECK_LAUNCH("rpb_mwt_modes");
}

extern "C" int rpb_mwt_spec_out(const float* S, const float* GT, const float* loT, const float* lb, float* out, long lines, int T, int K2,
                                int accumulate, void* stream) {
    RPB_REQUIRE(S && GT && loT && lb && out, "rpb_mwt_spec_out: null pointer");
    RPB_REQUIRE(lines > 0 && T > 0 && K2 > 0, "rpb_mwt_spec_out: bad shape lines=%ld T=%d K2=%d", lines, T, K2);
    const long ncell = lines * T;
    hipLaunchKernelGGL(mwt_spec_out_k<false>, dim3(mwt_blocks(ncell, MWT_SO_CELLS)), dim3(MWT_SO_CELLS * MWT_C), 0, MWT_STREAM, S, GT, loT, lb,
                       out, static_cast<float*>(nullptr), ncell, T, K2, accumulate);
    RPB_CHECK_LAUNCH("rpb_mwt_spec_out");
}

extern "C" int rpb_mwt_conv3_wprep(const float* w, const float* lo, float* wp, float* lop, void* stream) {
    RPB_REQUIRE(w && lo && wp && lop, "rpb_mwt_conv3_wprep: null pointer");
    const int n = 27 * 9 * 3 * 64 + 3 * 4 * 3 * 64;
    hipLaunchKernelGGL(mwt_conv3_wprep_k, dim3(mwt_blocks(n, 256)), dim3(256), 0, MWT_STREAM, w, lo, wp, lop);
    RPB_CHECK_LAUNCH("rpb_mwt_conv3_wprep");
}

extern "C" int rpb_mwt_conv3(const float* x, const float* wp, const float* cb48, const float* lop, const float* lb, float* out, int B,
                             int Nx, int Ny, int T, int accumulate, void* stream) {
    RPB_REQUIRE(x && wp && cb48 && lop && lb && out, "rpb_mwt_conv3: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0, "rpb_mwt_conv3: bad shape B=%d Nx=%d Ny=%d T=%d", B, Nx, Ny, T);
    RPB_REQUIRE(x != out, "rpb_mwt_conv3: in-place convolution is not possible");
    const long ncell = (long)B * Nx * Ny * T;
    hipLaunchKernelGGL(mwt_conv3_k<MWT_CONV_EVAL>, dim3(mwt_blocks(ncell, 256)), dim3(256), 0, MWT_STREAM, x, wp, cb48, lop, lb, out,
                       static_cast<float*>(nullptr), ncell, Nx, Ny, T, accumulate);
    RPB_CHECK_LAUNCH("rpb_mwt_conv3");
}

extern "C" int rpb_mwt_head(const float* x, const float* w0t, const float* b0, const float* w1, const float* b1, float* out, int B, int Nx,
                            int Ny, int T, int Cout, int r, void* stream) {
    RPB_REQUIRE(x && w0t && b0 && w1 && b1 && out, "rpb_mwt_head: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0 && Cout > 0 && r > 0, "rpb_mwt_head: bad shape");
    const long ncell = (long)B * Nx * Ny * T;
    const long groups = (ncell + 7) / 8;
    const long cap = 16L * rpb_num_cus();
    hipLaunchKernelGGL(mwt_head_k, dim3((unsigned)(groups < cap ? groups : cap)), dim3(256), 0, MWT_STREAM, x, w0t, b0, w1, b1, out, ncell, Nx,
                       Ny, T, Cout, r);
    RPB_CHECK_LAUNCH("rpb_mwt_head");
}
