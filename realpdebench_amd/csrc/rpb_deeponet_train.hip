// DeepONet training step (realpdebench/model/deeponet.py in train() mode; opt-in: DeepONet.enable_training()).  The convolutions and
// Linear layers stay rpb_im2col / rpb_gemm3x / rpb_split3 / rpb_conv3x (data gradients: the same kernels on transposed / flipped weights),
// the weight gradients stay rpb_gemm_tn / rpb_gemm3x_tn / rpb_conv3x_wgrad, the batch statistics and the BatchNorm backward apply are the
// rpb_rowbn_* family (rpb_rowbn.hip; the forward statistics at C = 256 as two column halves) and the forward pooling is
// rpb_don_bn_relu_pool with (a, b) of the batch statistics.  Here are the memory-bound row passes that are DeepONet's own:
//
//   rpb_don_pool_bwd        gz = d loss / d (y a + b) from the gradient of the pooled stage output, y = the saved convolution output:
//                           mode 0  MaxPool3d(2): one window per output cell; the gradient goes to the FIRST maximum in (t, h, w) scan order of
//                                   v = relu(fmaf(y, a, b)), nothing where that maximum is <= 0, nothing to the trailing frame / row / column
//                                   the flooring pool drops;
//                           mode 1  AdaptiveAvgPool3d((1, 4, 4)): gather form, a cell adds g_bin / |bin| over the (overlapping or replicated)
//                                   bins that contain it, gated by v > 0.
//                           The same launch leaves fp64 partials of (sum gz, sum gz xhat), xhat = (y - mean) rstd, per workgroup, for
//                           rpb_rowbn_sum64 and rpb_rowbn_act_bwd_apply (has_bn = 1, act = 0, in place on gz).
//   rpb_don_point_mul       x[r] = b[s] (.) t[n] for the points q = q0 + r, s = q / N, n = q % N of one chunk of the output net
//   rpb_don_point_mul_bwd   one sample's rows of a chunk: gt[n] += gx (.) b[s] and fp32 partials (summed in fp64) of gb[s] = sum_n gx (.) t[n]
//
// Every kernel is grid-stride with 16-byte accesses, fp64 only in the partial sums, no atomics and a fixed summation order: two calls
// are bit-equal.  The ReLU gate and the arg-max are recomputed from fmaf(y, a, b) -- the expression rpb_don_bn_relu_pool evaluates -- so
// neither a mask nor an index tensor is stored.
#include "rpb_rowbn.h"

// ---------------------------------------------------------------------------------- pooling backward + BatchNorm backward sums
// A thread owns 4 channels and every nsub-th item of its workgroup's share (item = one 2 x 2 x 2 window, or one cell in mode 1); the nsub
// sub-sums of a workgroup are added in index order through LDS.  part[block][2 C] = (sum gz [C], sum gz xhat [C]).
struct DtPoolArgs {
    const float* y;        // [B][T][H][W][ldy]  saved convolution output
    const float* g;        // mode 0: [B][T/2][H/2][W/2][ldg]; mode 1: [B][4][4][ldg]
    const float *a, *b, *mean, *rstd;      // [C]
    float* gz;             // [B][T][H][W][ldz]
    double* part;          // [gridDim.x][2 C]
    int B, T, H, W, C, ldy, ldg, ldz, mode;
};

__global__ __launch_bounds__(ROWBN_THREADS) void dt_pool_bwd_kernel(DtPoolArgs p) {
    __shared__ double red[ROWBN_THREADS * 8];                           // [nsub][2 C] = 256 / (C / 4) * 2 C doubles = 16 KB
    const int c4n = p.C >> 2;
    const int c4 = threadIdx.x % c4n, sub = threadIdx.x / c4n, nsub = ROWBN_THREADS / c4n;
    const int c0 = 4 * c4;
    const f32x4 a4 = *reinterpret_cast<const f32x4*>(p.a + c0), b4 = *reinterpret_cast<const f32x4*>(p.b + c0);
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    double mu[4], rs[4], s0[4] = {0., 0., 0., 0.}, s1[4] = {0., 0., 0., 0.};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mu[i] = (double)p.mean[c0 + i];
        rs[i] = (double)p.rstd[c0 + i];
    }
    if (p.mode == 0) {
        const int Tw = (p.T + 1) / 2, Hw = (p.H + 1) / 2, Ww = (p.W + 1) / 2;   // windows, the partial ones at the far faces included
        const int To = p.T / 2, Ho = p.H / 2, Wo = p.W / 2;
        const long items = (long)p.B * Tw * Hw * Ww;
        for (long it = (long)blockIdx.x * nsub + sub; it < items; it += (long)gridDim.x * nsub) {
            long r = it;
            const int ww = (int)(r % Ww);
            r /= Ww;
            const int wh = (int)(r % Hw);
            r /= Hw;
            const int wt = (int)(r % Tw);
            const long bb = r / Tw;
            const bool whole = wt < To && wh < Ho && ww < Wo;
            f32x4 yv[8], gz[8];
            int arg[4] = {0, 0, 0, 0};
            f32x4 best = zero4, g4 = zero4;
            if (whole) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int t = 2 * wt + (k >> 2), h = 2 * wh + ((k >> 1) & 1), w = 2 * ww + (k & 1);
                    yv[k] = RPB_SLD4(p.y + (((bb * p.T + t) * p.H + h) * (long)p.W + w) * p.ldy + c0);
                }
                g4 = *reinterpret_cast<const f32x4*>(p.g + (((bb * To + wt) * Ho + wh) * (long)Wo + ww) * p.ldg + c0);
#pragma unroll
                for (int k = 0; k < 8; ++k)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v = __builtin_fmaf(yv[k][i], a4[i], b4[i]);
                        v = v > 0.f ? v : 0.f;
                        if (k == 0 || v > best[i]) {                     // strict: the first maximum in scan order keeps the gradient
                            best[i] = v;
                            arg[i] = k;
                        }
                    }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                gz[k] = zero4;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (whole && arg[i] == k && best[i] > 0.f) {
                        gz[k][i] = g4[i];
                        s0[i] += (double)g4[i];
                        s1[i] += (double)g4[i] * (((double)yv[k][i] - mu[i]) * rs[i]);
                    }
                const int t = 2 * wt + (k >> 2), h = 2 * wh + ((k >> 1) & 1), w = 2 * ww + (k & 1);
                if (t < p.T && h < p.H && w < p.W)
                    *reinterpret_cast<f32x4*>(p.gz + (((bb * p.T + t) * p.H + h) * (long)p.W + w) * p.ldz + c0) = gz[k];
            }
        }
    } else {
        const long items = (long)p.B * p.T * p.H * p.W;
        const long thw = (long)p.T * p.H * p.W;
        for (long it = (long)blockIdx.x * nsub + sub; it < items; it += (long)gridDim.x * nsub) {
            const long bb = it / thw;
            const long r = it - bb * thw;
            const int w = (int)(r % p.W), h = (int)((r / p.W) % p.H);
            const f32x4 y4 = RPB_SLD4(p.y + it * p.ldy + c0);
            f32x4 acc = zero4;
            for (int i = 0; i < 4; ++i) {
                const int h0 = i * p.H / 4, h1 = ((i + 1) * p.H + 3) / 4;
                if (h < h0 || h >= h1) continue;
                for (int j = 0; j < 4; ++j) {
                    const int w0 = j * p.W / 4, w1 = ((j + 1) * p.W + 3) / 4;
                    if (w < w0 || w >= w1) continue;
                    const float inv = 1.0f / (float)(p.T * (h1 - h0) * (w1 - w0));
                    acc += *reinterpret_cast<const f32x4*>(p.g + ((bb * 4 + i) * 4 + j) * (long)p.ldg + c0) * inv;
                }
            }
            f32x4 gz4 = zero4;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (__builtin_fmaf(y4[i], a4[i], b4[i]) > 0.f) {
                    gz4[i] = acc[i];
                    s0[i] += (double)acc[i];
                    s1[i] += (double)acc[i] * (((double)y4[i] - mu[i]) * rs[i]);
                }
            *reinterpret_cast<f32x4*>(p.gz + it * p.ldz + c0) = gz4;
        }
    }
    rowbn_block_sums<2>(red, s0, s1, p.C, c0, sub, nsub, p.part);
}

extern "C" int rpb_don_pool_bwd(const float* y, int ldy, const float* g, int ldg, const float* a, const float* b, const float* mean,
                                const float* rstd, float* gz, int ldz, int B, int T, int H, int W, int C, int mode, double* part,
                                void* stream) {
    RPB_REQUIRE(y && g && a && b && mean && rstd && gz && part && B > 0 && T > 0 && H > 0 && W > 0 && rowbn_chan_ok(C, 32, 256) && (mode == 0 || mode == 1),
                "don_pool_bwd: bad arguments (B=%d T=%d H=%d W=%d C=%d mode=%d; C in {32, 64, 128, 256})", B, T, H, W, C, mode);
    RPB_REQUIRE((long)B * T * H * W < (1L << 31), "don_pool_bwd: B T H W = %ld cells (< 2^31)", (long)B * T * H * W);
    RPB_REQUIRE(mode == 1 || (T >= 2 && H >= 2 && W >= 2), "don_pool_bwd: MaxPool3d(2) needs extents >= 2 (T=%d H=%d W=%d)", T, H, W);
    RPB_REQUIRE(ldy >= C && ldy % 4 == 0 && ldg >= C && ldg % 4 == 0 && ldz >= C && ldz % 4 == 0 && rowbn_al16(y) && rowbn_al16(g) && rowbn_al16(gz) &&
                    rowbn_al16(a) && rowbn_al16(b),
                "don_pool_bwd: ldy=%d ldg=%d ldz=%d must be >= C and %% 4 == 0, y / g / gz / a / b 16-byte aligned", ldy, ldg, ldz);
    DtPoolArgs p{y, g, a, b, mean, rstd, gz, part, B, T, H, W, C, ldy, ldg, ldz, mode};
    hipLaunchKernelGGL(dt_pool_bwd_kernel, dim3(rowbn_rows()), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("don_pool_bwd");
}

// ---------------------------------------------------------------------------------- the output net's input and its backward
__global__ __launch_bounds__(ROWBN_THREADS) void dt_point_mul_kernel(const float* __restrict__ t, const float* __restrict__ b, float* __restrict__ x,
                                                                  long q0, long R, long N, int p) {
    const int c4n = p >> 2;
    const long total = R * c4n;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long r = idx / c4n;
        const int c = (int)(idx - r * c4n) * 4;
        const long q = q0 + r, s = q / N, n = q - s * N;
        const f32x4 v = *reinterpret_cast<const f32x4*>(b + s * p + c) * RPB_SLD4(t + n * p + c);
        *reinterpret_cast<f32x4*>(x + r * p + c) = v;
    }
}

extern "C" int rpb_don_point_mul(const float* t, const float* b, float* x, long q0, long R, int B, long N, int p, void* stream) {
    RPB_REQUIRE(t && b && x && q0 >= 0 && R > 0 && B > 0 && N > 0 && q0 + R <= (long)B * N && (p == 64 || p == 128 || p == 256) && rowbn_al16(t) &&
                    rowbn_al16(b) && rowbn_al16(x),
                "don_point_mul: bad arguments (q0=%ld R=%ld B=%d N=%ld p=%d; q0 + R <= B N, p in {64, 128, 256}, 16-byte aligned)", q0, R, B, N, p);
    hipLaunchKernelGGL(dt_point_mul_kernel, dim3(rowbn_grid(R * (p / 4))), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, t, b, x, q0, R, N, p);
    RPB_CHECK_LAUNCH("don_point_mul");
}

// gx [R][p]: the rows of points n0 .. n0 + R - 1 of ONE sample (b: that sample's branch vector).  gt[n0 + r] += gx[r] (.) b; part[block][p] =
// sum over the block's rows of gx[r] (.) t[n0 + r] (fp64 sums, stored as fp32; rpb_reduce_partials finishes them in fp64).
__global__ __launch_bounds__(ROWBN_THREADS) void dt_point_mul_bwd_kernel(const float* __restrict__ gx, const float* __restrict__ t,
                                                                      const float* __restrict__ b, float* gt, float* __restrict__ part,
                                                                      long n0, long R, int p) {
    __shared__ double red[ROWBN_THREADS * 4];                           // [nsub][p] = 256 / (p / 4) * p doubles = 8 KB
    const int c4n = p >> 2;
    const int c4 = threadIdx.x % c4n, sub = threadIdx.x / c4n, nsub = ROWBN_THREADS / c4n;
    const int c0 = 4 * c4;
    const f32x4 b4 = *reinterpret_cast<const f32x4*>(b + c0);
    double s[4] = {0., 0., 0., 0.};
    for (long r = (long)blockIdx.x * nsub + sub; r < R; r += (long)gridDim.x * nsub) {
        const f32x4 g4 = RPB_SLD4(gx + r * p + c0);
        const f32x4 t4 = RPB_SLD4(t + (n0 + r) * p + c0);
        float* dst = gt + (n0 + r) * p + c0;
        *reinterpret_cast<f32x4*>(dst) = *reinterpret_cast<const f32x4*>(dst) + g4 * b4;
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += (double)g4[i] * (double)t4[i];
    }
    rowbn_block_sums<1>(red, s, nullptr, p, c0, sub, nsub, part);
}

extern "C" int rpb_don_point_mul_bwd(const float* gx, const float* t, const float* b, float* gt, float* part, long n0, long R, long N, int p,
                                     void* stream) {
    RPB_REQUIRE(gx && t && b && gt && part && n0 >= 0 && R > 0 && n0 + R <= N && (p == 64 || p == 128 || p == 256) && rowbn_al16(gx) && rowbn_al16(t) &&
                    rowbn_al16(b) && rowbn_al16(gt),
                "don_point_mul_bwd: bad arguments (n0=%ld R=%ld N=%ld p=%d; n0 + R <= N, p in {64, 128, 256}, 16-byte aligned)", n0, R, N, p);
    hipLaunchKernelGGL(dt_point_mul_bwd_kernel, dim3(rowbn_rows()), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, gx, t, b, gt, part, n0, R, p);
    RPB_CHECK_LAUNCH("don_point_mul_bwd");
}
