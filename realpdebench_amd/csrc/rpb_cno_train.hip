// CNO3d training step (realpdebench/model/cno.py:96-100, 146-152, 222-231 in train() mode): batch-statistics BatchNorm3d on channels-last
// rows [M][C], M = B * T * H * W, with LeakyReLU(0.2) and the residual add, forward and backward.  The convolutions themselves stay
// rpb_cno_conv3x (forward with sc = 1, sh = bias, act = 0; data gradient with the flipped, transposed taps -- seven of the 34 on the
// exact-fp32 rpb_gemm_nt, model/cno.py EXACT_DGRAD) and the weight gradient stays
// rpb_gemm_tn / rpb_conv3x_wgrad: what is new here are the memory-bound row passes around them.
//
//   forward    y = conv(x) + bias                           (rpb_cno_conv3x)
//              (sum y, sum y^2) per channel                 rpb_cno_bn_stats  -> fp64 partials
//              mean, rstd, a = gamma rstd, b = beta - mean a; running statistics      rpb_cno_bn_finish
//              z = y a + b;  v = act ? lrelu(z) : z;  v += res                        rpb_cno_bn_act_fwd  (fp32 rows and / or bf16 planes)
//   backward   dz = gv (z > 0 ? 1 : 0.2);  (sum dz, sum dz xhat), xhat = (y - mean) rstd   rpb_cno_bn_act_bwd_stats -> fp64 partials
//              fixed-order sum of the partials              rpb_cno_sum64
//              dy = a (dz - dbeta / M - xhat dgamma / M);  dgamma, dbeta              rpb_cno_bn_act_bwd_apply (fp32 rows + bf16 planes)
//
// Every kernel is grid-stride with 16-byte accesses, uses no atomics and sums in a fixed order: two calls are bit-equal.  Every pointer
// arrives at the first column the launch owns, with a leading dimension (producers own column ranges of shared buffers).  The gate of the
// backward pass is recomputed from fmaf(y, a, b) -- the expression the forward pass evaluates -- so no mask is stored.
#include "rpb_mma.h"
#include <stdint.h>

#define CT_THREADS 256

__device__ __forceinline__ float ct_lrelu(float z) { return z > 0.f ? z : 0.2f * z; }

// ---------------------------------------------------------------------------------- per-channel fp64 partial sums
// A thread owns 4 channels (one 16 B load per row) and every nsub-th row of its workgroup's share; the nsub sub-rows of a workgroup are
// added in index order through LDS.  part[block][2 C] = (s0[0..C), s1[0..C)).
//   MODE 0  s0 = sum y,   s1 = sum y^2
//   MODE 1  s0 = sum dz,  s1 = sum dz xhat     (dz = gv or 0.2 gv by the sign of fmaf(y, a, b); xhat = (y - mean) rstd, formed in fp64)
struct CtStatArgs {
    const float* y;        // [M][ldy]
    const float* gv;       // [M][ldg]  (MODE 1)
    const float *a, *b, *mean, *rstd;      // [C]  (MODE 1)
    double* part;          // [gridDim.x][2 C]
    long M;
    int C, ldy, ldg, act;
};

template <int MODE>
__global__ __launch_bounds__(CT_THREADS) void ct_stats_kernel(CtStatArgs p) {
    __shared__ double red[CT_THREADS * 8];                              // [nsub][2 C] = 256 / (C / 4) * 2 C doubles = 16 KB
    const int c4n = p.C >> 2;
    const int c4 = threadIdx.x % c4n, sub = threadIdx.x / c4n, nsub = CT_THREADS / c4n;
    const int c0 = 4 * c4;
    double s0[4] = {0., 0., 0., 0.}, s1[4] = {0., 0., 0., 0.};
    f32x4 a4, b4;
    double mu[4], rs[4];
    if (MODE == 1) {
        a4 = *reinterpret_cast<const f32x4*>(p.a + c0);
        b4 = *reinterpret_cast<const f32x4*>(p.b + c0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            mu[i] = (double)p.mean[c0 + i];
            rs[i] = (double)p.rstd[c0 + i];
        }
    }
    for (long m = (long)blockIdx.x * nsub + sub; m < p.M; m += (long)gridDim.x * nsub) {
        const f32x4 y4 = RPB_SLD4(p.y + m * p.ldy + c0);
        if (MODE == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double yd = (double)y4[i];
                s0[i] += yd;
                s1[i] += yd * yd;
            }
        } else {
            const f32x4 g4 = RPB_SLD4(p.gv + m * p.ldg + c0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float z = __builtin_fmaf(y4[i], a4[i], b4[i]);
                const double dz = (p.act && !(z > 0.f)) ? 0.2 * (double)g4[i] : (double)g4[i];
                s0[i] += dz;
                s1[i] += dz * (((double)y4[i] - mu[i]) * rs[i]);
            }
        }
    }
    double* mine = red + (long)sub * 2 * p.C;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mine[c0 + i] = s0[i];
        mine[p.C + c0 + i] = s1[i];
    }
    __syncthreads();
    for (int n = threadIdx.x; n < 2 * p.C; n += CT_THREADS) {
        double s = 0.;
        for (int k = 0; k < nsub; ++k) s += red[(long)k * 2 * p.C + n];
        p.part[(long)blockIdx.x * 2 * p.C + n] = s;
    }
}

static bool ct_chan_ok(int C) { return C == 16 || C == 32 || C == 64 || C == 128; }
static bool ct_al16(const void* p) { return (uintptr_t)p % 16 == 0; }

extern "C" int rpb_cno_bn_rows(void) { return rpb_num_cus() * 4; }

extern "C" int rpb_cno_bn_stats(const float* y, int ld, long M, int C, double* part, void* stream) {
    RPB_REQUIRE(y && part && M > 0 && M < (1L << 31) && ct_chan_ok(C) && ld >= C && ld % 4 == 0 && ct_al16(y),
                "cno_bn_stats: bad arguments (M=%ld C=%d ld=%d; C in {16, 32, 64, 128}, ld %% 4 == 0, y 16-byte aligned)", M, C, ld);
    CtStatArgs p{y, nullptr, nullptr, nullptr, nullptr, nullptr, part, M, C, ld, 0, 0};
    hipLaunchKernelGGL(ct_stats_kernel<0>, dim3(rpb_cno_bn_rows()), dim3(CT_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("cno_bn_stats");
}

extern "C" int rpb_cno_bn_act_bwd_stats(const float* gv, int ldg, const float* y, int ldy, const float* a, const float* b, const float* mean,
                                        const float* rstd, long M, int C, int act, double* part, void* stream) {
    RPB_REQUIRE(gv && y && a && b && mean && rstd && part && M > 0 && M < (1L << 31) && ct_chan_ok(C) && (act == 0 || act == 1),
                "cno_bn_act_bwd_stats: bad arguments (M=%ld C=%d act=%d; C in {16, 32, 64, 128})", M, C, act);
    RPB_REQUIRE(ldg >= C && ldg % 4 == 0 && ldy >= C && ldy % 4 == 0 && ct_al16(gv) && ct_al16(y) && ct_al16(a) && ct_al16(b),
                "cno_bn_act_bwd_stats: ldg=%d ldy=%d must be >= C and %% 4 == 0, gv / y / a / b 16-byte aligned", ldg, ldy);
    CtStatArgs p{y, gv, a, b, mean, rstd, part, M, C, ldy, ldg, act};
    hipLaunchKernelGGL(ct_stats_kernel<1>, dim3(rpb_cno_bn_rows()), dim3(CT_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("cno_bn_act_bwd_stats");
}

// ---------------------------------------------------------------------------------- the partials' fixed-order sum, and the statistics
// One workgroup per 16 channels: thread = (row group g of 8, statistic s of 2, channel c of 16) adds rows g, g + 8, ... of its column;
// the 8 groups are added in index order through LDS.
struct CtFinArgs {
    const double* part;    // [rows][2 C]
    double* sums;          // [2 C] or null
    const float *gamma, *beta;
    float *rmean, *rvar, *a, *b, *mean, *rstd;
    long M;
    int rows, C;
    double eps, momentum;
};

template <bool FINISH>
__global__ __launch_bounds__(CT_THREADS) void ct_sum_kernel(CtFinArgs p) {
    __shared__ double red[8][32];
    const int ch = threadIdx.x & 15, st = (threadIdx.x >> 4) & 1, g = threadIdx.x >> 5;
    const int c = blockIdx.x * 16 + ch;
    const long colm = (long)st * p.C + c;
    double s = 0.;
    for (int r = g; r < p.rows; r += 8) s += p.part[(long)r * 2 * p.C + colm];
    red[g][st * 16 + ch] = s;
    __syncthreads();
    if (threadIdx.x >= 32) return;
    double t = 0.;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += red[k][threadIdx.x];
    if (!FINISH) {
        p.sums[colm] = t;
        return;
    }
    const double t2 = __shfl(t, (threadIdx.x & 15) + 16, 64);           // lane c < 16 holds sum y, lane 16 + c holds sum y^2
    if (threadIdx.x >= 16) return;
    const double n = (double)p.M;
    const double mean = t / n;
    double var = t2 / n - mean * mean;                                  // biased; fp64 sums of fp32 values: no cancellation to speak of
    if (var < 0.) var = 0.;
    const double rstd = 1.0 / sqrt(var + p.eps);
    const double a = (double)p.gamma[c] * rstd;
    p.mean[c] = (float)mean;
    p.rstd[c] = (float)rstd;
    p.a[c] = (float)a;
    p.b[c] = (float)((double)p.beta[c] - mean * a);
    p.rmean[c] = (float)((1.0 - p.momentum) * (double)p.rmean[c] + p.momentum * mean);
    p.rvar[c] = (float)((1.0 - p.momentum) * (double)p.rvar[c] + p.momentum * var * (n / (n - 1.0)));
}

extern "C" int rpb_cno_bn_finish(const double* part, int rows, long M, int C, const float* gamma, const float* beta, float* running_mean,
                                 float* running_var, double eps, double momentum, float* a, float* b, float* mean, float* rstd,
                                 void* stream) {
    RPB_REQUIRE(part && gamma && beta && running_mean && running_var && a && b && mean && rstd && rows > 0 && M > 1 && ct_chan_ok(C) &&
                    eps > 0. && momentum >= 0. && momentum <= 1.,
                "cno_bn_finish: bad arguments (rows=%d M=%ld C=%d; M > 1, C in {16, 32, 64, 128})", rows, M, C);
    CtFinArgs p{part, nullptr, gamma, beta, running_mean, running_var, a, b, mean, rstd, M, rows, C, eps, momentum};
    hipLaunchKernelGGL(ct_sum_kernel<true>, dim3(C / 16), dim3(CT_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("cno_bn_finish");
}

extern "C" int rpb_cno_sum64(const double* part, int rows, int C, double* sums, void* stream) {
    RPB_REQUIRE(part && sums && rows > 0 && ct_chan_ok(C), "cno_sum64: bad arguments (rows=%d C=%d; C in {16, 32, 64, 128})", rows, C);
    CtFinArgs p{part, sums, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, rows, C, 0., 0.};
    hipLaunchKernelGGL(ct_sum_kernel<false>, dim3(C / 16), dim3(CT_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("cno_sum64");
}

// ---------------------------------------------------------------------------------- forward apply
// v = fmaf(y, a, b); LeakyReLU; + res.  One thread = 8 channels of one token (2 x 16 B in, 2 x 16 B fp32 and 3 x 16 B bf16 out).
__global__ __launch_bounds__(CT_THREADS) void ct_act_fwd_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ a,
                                                                const float* __restrict__ b, const float* res, int ldr, float* out,
                                                                int ldo, uint16_t* op, int ldp, long M, int C, int act) {
    const int c8n = C >> 3;
    const long total = M * c8n, pstride = M * (long)ldp;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long m = idx / c8n;
        const int c0 = (int)(idx - m * c8n) * 8;
        const f32x4 y0 = RPB_SLD4(y + m * ldy + c0), y1 = RPB_SLD4(y + m * ldy + c0 + 4);
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + c0), a1 = *reinterpret_cast<const f32x4*>(a + c0 + 4);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(b + c0), b1 = *reinterpret_cast<const f32x4*>(b + c0 + 4);
        f32x4 v0, v1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v0[i] = __builtin_fmaf(y0[i], a0[i], b0[i]);
            v1[i] = __builtin_fmaf(y1[i], a1[i], b1[i]);
            if (act) {
                v0[i] = ct_lrelu(v0[i]);
                v1[i] = ct_lrelu(v1[i]);
            }
        }
        if (res) {
            v0 += *reinterpret_cast<const f32x4*>(res + m * ldr + c0);
            v1 += *reinterpret_cast<const f32x4*>(res + m * ldr + c0 + 4);
        }
        if (out) {
            *reinterpret_cast<f32x4*>(out + m * ldo + c0) = v0;
            *reinterpret_cast<f32x4*>(out + m * ldo + c0 + 4) = v1;
        }
        if (op) split3_store(op, m * ldp + c0, pstride, v0, v1);
    }
}

static unsigned ct_grid(long total) {
    long grid = (total + CT_THREADS - 1) / CT_THREADS;
    const long cap = (long)rpb_num_cus() * 16;
    return (unsigned)(grid > cap ? cap : grid);
}

extern "C" int rpb_cno_bn_act_fwd(const float* y, int ldy, const float* a, const float* b, const float* res, int ldr, float* out, int ldo,
                                  void* out_planes, int ldp, long M, int C, int act, void* stream) {
    RPB_REQUIRE(y && a && b && (out || out_planes) && M > 0 && M < (1L << 31) && ct_chan_ok(C) && (act == 0 || act == 1),
                "cno_bn_act_fwd: bad arguments (M=%ld C=%d act=%d; C in {16, 32, 64, 128})", M, C, act);
    RPB_REQUIRE(ldy >= C && ldy % 4 == 0 && ct_al16(y) && ct_al16(a) && ct_al16(b), "cno_bn_act_fwd: ldy=%d (>= C, %% 4 == 0, 16-byte aligned)", ldy);
    RPB_REQUIRE(!res || (ldr >= C && ldr % 4 == 0 && ct_al16(res)), "cno_bn_act_fwd: ldr=%d (>= C, %% 4 == 0, 16-byte aligned)", ldr);
    RPB_REQUIRE(!out || (ldo >= C && ldo % 4 == 0 && ct_al16(out)), "cno_bn_act_fwd: ldo=%d (>= C, %% 4 == 0, 16-byte aligned)", ldo);
    RPB_REQUIRE(!out_planes || (ldp >= C && ldp % 8 == 0 && ct_al16(out_planes)),
                "cno_bn_act_fwd: plane output needs a 16-byte aligned first column and ldp %% 8 == 0 (ldp=%d)", ldp);
    hipLaunchKernelGGL(ct_act_fwd_kernel, dim3(ct_grid(M * (C / 8))), dim3(CT_THREADS), 0, (hipStream_t)stream, y, ldy, a, b, res, ldr, out,
                       ldo, (uint16_t*)out_planes, ldp, M, C, act);
    RPB_CHECK_LAUNCH("cno_bn_act_fwd");
}

// ---------------------------------------------------------------------------------- backward apply
// has_bn:  dy = a (dz - dbeta / M - xhat dgamma / M),  dz = gv or 0.2 gv by the sign of fmaf(y, a, b)
// else:    dy = dz, the gate from the sign of `y` itself (the saved LeakyReLU output, or conv + bias: same sign)
// Columns C..Cpad-1 of the rows and planes are written as zero (the 64-wide operands of the narrow layers).
struct CtBwdArgs {
    const float *gv, *y, *a, *b, *mean, *rstd;
    const double* sums;    // [2 C]: (sum dz, sum dz xhat)
    float* dy;             // [M][ldd] or null
    uint16_t* dp;          // [3][M][ldp] or null
    float *dgamma, *dbeta; // [C] or null
    long M;
    int C, Cpad, ldg, ldy, ldd, ldp, act, has_bn;
};

__global__ __launch_bounds__(CT_THREADS) void ct_act_bwd_kernel(CtBwdArgs p) {
    const int c8n = p.Cpad >> 3;
    const long total = p.M * c8n, pstride = p.M * (long)p.ldp;
    if (p.has_bn && p.dgamma && blockIdx.x == 0)
        for (int c = threadIdx.x; c < p.C; c += CT_THREADS) {
            p.dbeta[c] = (float)p.sums[c];
            p.dgamma[c] = (float)p.sums[p.C + c];
        }
    const double inv_m = 1.0 / (double)p.M;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long m = idx / c8n;
        const int c0 = (int)(idx - m * c8n) * 8;
        f32x4 d[2] = {z4, z4};
        if (c0 < p.C) {                                                 // C % 8 == 0: a run of 8 is inside or outside
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = c0 + 4 * h;
                const f32x4 g4 = RPB_SLD4(p.gv + m * p.ldg + c);
                f32x4 y4 = z4;
                if (p.has_bn || p.act) y4 = RPB_SLD4(p.y + m * p.ldy + c);
                if (p.has_bn) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(p.a + c), b4 = *reinterpret_cast<const f32x4*>(p.b + c);
                    const f32x4 mu = *reinterpret_cast<const f32x4*>(p.mean + c), rs = *reinterpret_cast<const f32x4*>(p.rstd + c);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float k1 = (float)(p.sums[c + i] * inv_m), k2 = (float)(p.sums[p.C + c + i] * inv_m);
                        const float z = __builtin_fmaf(y4[i], a4[i], b4[i]);
                        const float dz = (p.act && !(z > 0.f)) ? 0.2f * g4[i] : g4[i];
                        const float xh = (y4[i] - mu[i]) * rs[i];
                        d[h][i] = a4[i] * (dz - k1 - xh * k2);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) d[h][i] = (p.act && !(y4[i] > 0.f)) ? 0.2f * g4[i] : g4[i];
                }
            }
        }
        if (p.dy) {
            *reinterpret_cast<f32x4*>(p.dy + m * p.ldd + c0) = d[0];
            *reinterpret_cast<f32x4*>(p.dy + m * p.ldd + c0 + 4) = d[1];
        }
        if (p.dp) split3_store(p.dp, m * p.ldp + c0, pstride, d[0], d[1]);
    }
}

extern "C" int rpb_cno_bn_act_bwd_apply(const float* gv, int ldg, const float* y, int ldy, const float* a, const float* b, const float* mean,
                                        const float* rstd, const double* sums, long M, int C, int Cpad, int act, int has_bn, float* dy,
                                        int ldd, void* dy_planes, int ldp, float* dgamma, float* dbeta, void* stream) {
    RPB_REQUIRE(gv && (dy || dy_planes) && M > 0 && M < (1L << 31) && ct_chan_ok(C) && Cpad >= C && Cpad % 8 == 0 && (act == 0 || act == 1) &&
                    (has_bn == 0 || has_bn == 1),
                "cno_bn_act_bwd_apply: bad arguments (M=%ld C=%d Cpad=%d act=%d has_bn=%d; C in {16, 32, 64, 128}, Cpad >= C, Cpad %% 8 == 0)",
                M, C, Cpad, act, has_bn);
    RPB_REQUIRE(ldg >= C && ldg % 4 == 0 && ct_al16(gv), "cno_bn_act_bwd_apply: ldg=%d (>= C, %% 4 == 0, gv 16-byte aligned)", ldg);
    RPB_REQUIRE(!(has_bn || act) || (y && ldy >= C && ldy % 4 == 0 && ct_al16(y)), "cno_bn_act_bwd_apply: y / ldy=%d (>= C, %% 4 == 0, 16-byte aligned)", ldy);
    RPB_REQUIRE(!has_bn || (a && b && mean && rstd && sums && ct_al16(a) && ct_al16(b) && ct_al16(mean) && ct_al16(rstd) && (!dgamma == !dbeta)),
                "cno_bn_act_bwd_apply: has_bn needs a, b, mean, rstd (16-byte aligned) and sums; dgamma and dbeta come together");
    RPB_REQUIRE(!dy || (ldd >= Cpad && ldd % 4 == 0 && ct_al16(dy)), "cno_bn_act_bwd_apply: ldd=%d (>= Cpad, %% 4 == 0, dy 16-byte aligned)", ldd);
    RPB_REQUIRE(!dy_planes || (ldp >= Cpad && ldp % 8 == 0 && ct_al16(dy_planes)),
                "cno_bn_act_bwd_apply: plane output needs a 16-byte aligned first column and ldp %% 8 == 0 (ldp=%d)", ldp);
    CtBwdArgs p{gv, y, a, b, mean, rstd, sums, dy, (uint16_t*)dy_planes, dgamma, dbeta, M, C, Cpad, ldg, ldy, ldd, ldp, act, has_bn};
    hipLaunchKernelGGL(ct_act_bwd_kernel, dim3(ct_grid(M * (Cpad / 8))), dim3(CT_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("cno_bn_act_bwd_apply");
}
