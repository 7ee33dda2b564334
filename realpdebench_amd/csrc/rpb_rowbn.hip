// Batch-statistics BatchNorm on channels-last rows [M][ld], forward and backward, with the LeakyReLU(0.2) gate and the residual add of the
// CNO3d layers: the memory-bound row passes of the opt-in training steps of CNO3d (model/cno.py; realpdebench/model/cno.py:96-100,
// 146-152, 222-231 in train() mode) and DeepONet (model/deeponet.py; its pooling backward writes the backward partials itself,
// rpb_deeponet_train.hip).  The convolutions, their data gradients and weight gradients are the callers'.
//
//   forward    (sum y, sum y^2) per channel                 rpb_rowbn_stats  -> fp64 partials
//              mean, rstd, a = gamma rstd, b = beta - mean a; running statistics      rpb_rowbn_finish
//              z = y a + b;  v = act ? lrelu(z) : z;  v += res                        rpb_rowbn_act_fwd  (fp32 rows and / or bf16 planes)
//   backward   dz = gv (z > 0 ? 1 : 0.2);  (sum dz, sum dz xhat), xhat = (y - mean) rstd   rpb_rowbn_act_bwd_stats -> fp64 partials
//              fixed-order sum of the partials              rpb_rowbn_sum64
//              dy = a (dz - dbeta / M - xhat dgamma / M);  dgamma, dbeta              rpb_rowbn_act_bwd_apply (fp32 rows and / or bf16 planes)
//   SyncBN     the statistics from sums the caller all-reduced over its ranks      rpb_rowbn_finish_sums
//              dy from the all-reduced sums and M_total, dgamma and dbeta from this rank's own      rpb_rowbn_act_bwd_apply_sync
//
// Every kernel is grid-stride with 16-byte accesses, uses no atomics and sums in a fixed order: two calls are bit-equal.  Every pointer
// arrives at the first column the launch owns, with a leading dimension (producers own column ranges of shared buffers).  The gate of the
// backward pass is recomputed from fmaf(y, a, b) -- the expression the forward pass evaluates -- so no mask is stored.
#include "rpb_rowbn.h"

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
__global__ __launch_bounds__(ROWBN_THREADS) void ct_stats_kernel(CtStatArgs p) {
    __shared__ double red[ROWBN_THREADS * 8];                           // [nsub][2 C] = 256 / (C / 4) * 2 C doubles = 16 KB
    const int c4n = p.C >> 2;
    const int c4 = threadIdx.x % c4n, sub = threadIdx.x / c4n, nsub = ROWBN_THREADS / c4n;
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
    rowbn_block_sums<2>(red, s0, s1, p.C, c0, sub, nsub, p.part);
}

extern "C" int rpb_rowbn_rows(void) { return rowbn_rows(); }

extern "C" int rpb_rowbn_stats(const float* y, int ld, long M, int C, double* part, void* stream) {
    RPB_REQUIRE(y && part && M > 0 && M < (1L << 31) && rowbn_chan_ok(C, 16, 128) && ld >= C && ld % 4 == 0 && rowbn_al16(y),
                "rowbn_stats: bad arguments (M=%ld C=%d ld=%d; C in {16, 32, 64, 128}, ld %% 4 == 0, y 16-byte aligned)", M, C, ld);
    CtStatArgs p{y, nullptr, nullptr, nullptr, nullptr, nullptr, part, M, C, ld, 0, 0};
    hipLaunchKernelGGL(ct_stats_kernel<0>, dim3(rowbn_rows()), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("rowbn_stats");
}

extern "C" int rpb_rowbn_act_bwd_stats(const float* gv, int ldg, const float* y, int ldy, const float* a, const float* b, const float* mean,
                                       const float* rstd, long M, int C, int act, double* part, void* stream) {
    RPB_REQUIRE(gv && y && a && b && mean && rstd && part && M > 0 && M < (1L << 31) && rowbn_chan_ok(C, 16, 128) && (act == 0 || act == 1),
                "rowbn_act_bwd_stats: bad arguments (M=%ld C=%d act=%d; C in {16, 32, 64, 128})", M, C, act);
    RPB_REQUIRE(ldg >= C && ldg % 4 == 0 && ldy >= C && ldy % 4 == 0 && rowbn_al16(gv) && rowbn_al16(y) && rowbn_al16(a) && rowbn_al16(b),
                "rowbn_act_bwd_stats: ldg=%d ldy=%d must be >= C and %% 4 == 0, gv / y / a / b 16-byte aligned", ldg, ldy);
    CtStatArgs p{y, gv, a, b, mean, rstd, part, M, C, ldy, ldg, act};
    hipLaunchKernelGGL(ct_stats_kernel<1>, dim3(rowbn_rows()), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("rowbn_act_bwd_stats");
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
__global__ __launch_bounds__(ROWBN_THREADS) void ct_sum_kernel(CtFinArgs p) {
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

extern "C" int rpb_rowbn_finish(const double* part, int rows, long M, int C, const float* gamma, const float* beta, float* running_mean,
                                float* running_var, double eps, double momentum, float* a, float* b, float* mean, float* rstd,
                                void* stream) {
    RPB_REQUIRE(part && gamma && beta && running_mean && running_var && a && b && mean && rstd && rows > 0 && M > 1 && rowbn_chan_ok(C, 16, 128) &&
                    eps > 0. && momentum >= 0. && momentum <= 1.,
                "rowbn_finish: bad arguments (rows=%d M=%ld C=%d; M > 1, C in {16, 32, 64, 128})", rows, M, C);
    CtFinArgs p{part, nullptr, gamma, beta, running_mean, running_var, a, b, mean, rstd, M, rows, C, eps, momentum};
    hipLaunchKernelGGL(ct_sum_kernel<true>, dim3(C / 16), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("rowbn_finish");
}

// The finish from sums a caller reduced itself (SyncBN: the all-reduced sums of W ranks, M_total = W M): ct_sum_kernel<true> on the one
// row `sums`.  Row group 0 holds the sum, the other seven add 0: with sums = rpb_rowbn_sum64(part) and M_total = M every output has the bits
// of rpb_rowbn_finish(part, rows, M, ...).
extern "C" int rpb_rowbn_finish_sums(const double* sums, long M_total, int C, const float* gamma, const float* beta, float* running_mean,
                                     float* running_var, double eps, double momentum, float* a, float* b, float* mean, float* rstd,
                                     void* stream) {
    RPB_REQUIRE(sums && gamma && beta && running_mean && running_var && a && b && mean && rstd && M_total > 1 && rowbn_chan_ok(C, 16, 128) &&
                    eps > 0. && momentum >= 0. && momentum <= 1.,
                "rowbn_finish_sums: bad arguments (M_total=%ld C=%d; M_total > 1, C in {16, 32, 64, 128})", M_total, C);
    CtFinArgs p{sums, nullptr, gamma, beta, running_mean, running_var, a, b, mean, rstd, M_total, 1, C, eps, momentum};
    hipLaunchKernelGGL(ct_sum_kernel<true>, dim3(C / 16), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("rowbn_finish_sums");
}

extern "C" int rpb_rowbn_sum64(const double* part, int rows, int C, double* sums, void* stream) {
    RPB_REQUIRE(part && sums && rows > 0 && rowbn_chan_ok(C, 16, 256), "rowbn_sum64: bad arguments (rows=%d C=%d; C in {16, 32, 64, 128, 256})", rows, C);
    CtFinArgs p{part, sums, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, rows, C, 0., 0.};
    hipLaunchKernelGGL(ct_sum_kernel<false>, dim3(C / 16), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("rowbn_sum64");
}

// ---------------------------------------------------------------------------------- forward apply
// v = fmaf(y, a, b); LeakyReLU; + res.  One thread = 8 channels of one token (2 x 16 B in, 2 x 16 B fp32 and 3 x 16 B bf16 out).
__global__ __launch_bounds__(ROWBN_THREADS) void ct_act_fwd_kernel(const float* __restrict__ y, int ldy, const float* __restrict__ a,
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

extern "C" int rpb_rowbn_act_fwd(const float* y, int ldy, const float* a, const float* b, const float* res, int ldr, float* out, int ldo,
                                 void* out_planes, int ldp, long M, int C, int act, void* stream) {
    RPB_REQUIRE(y && a && b && (out || out_planes) && M > 0 && M < (1L << 31) && rowbn_chan_ok(C, 16, 128) && (act == 0 || act == 1),
                "rowbn_act_fwd: bad arguments (M=%ld C=%d act=%d; C in {16, 32, 64, 128})", M, C, act);
    RPB_REQUIRE(ldy >= C && ldy % 4 == 0 && rowbn_al16(y) && rowbn_al16(a) && rowbn_al16(b), "rowbn_act_fwd: ldy=%d (>= C, %% 4 == 0, 16-byte aligned)", ldy);
    RPB_REQUIRE(!res || (ldr >= C && ldr % 4 == 0 && rowbn_al16(res)), "rowbn_act_fwd: ldr=%d (>= C, %% 4 == 0, 16-byte aligned)", ldr);
    RPB_REQUIRE(!out || (ldo >= C && ldo % 4 == 0 && rowbn_al16(out)), "rowbn_act_fwd: ldo=%d (>= C, %% 4 == 0, 16-byte aligned)", ldo);
    RPB_REQUIRE(!out_planes || (ldp >= C && ldp % 8 == 0 && rowbn_al16(out_planes)),
                "rowbn_act_fwd: plane output needs a 16-byte aligned first column and ldp %% 8 == 0 (ldp=%d)", ldp);
    hipLaunchKernelGGL(ct_act_fwd_kernel, dim3(rowbn_grid(M * (C / 8))), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, y, ldy, a, b, res, ldr, out,
                       ldo, (uint16_t*)out_planes, ldp, M, C, act);
    RPB_CHECK_LAUNCH("rowbn_act_fwd");
}

// ---------------------------------------------------------------------------------- backward apply
// has_bn:  dy = a (dz - gsums[c] / Mtot - xhat gsums[C + c] / Mtot),  dz = gv or 0.2 gv by the sign of fmaf(y, a, b);  dbeta, dgamma = sums.
//          One rank: gsums = sums, Mtot = M.  SyncBN (rpb_rowbn_act_bwd_apply_sync): gsums = the sums of all ranks, Mtot = the rows of all
//          ranks, sums = this rank's own (the trainer's mean over the ranks makes them the global gradients).
// else:    dy = dz, the gate from the sign of `y` itself (the saved LeakyReLU output, or conv + bias: same sign)
// Columns C..Cpad-1 of the rows and planes are written as zero (the 64-wide operands of the narrow layers).  One thread = RUN channels
// of one row: 8 (what a 16 B plane store takes) when Cpad % 8 == 0, else 4 (rows only); the expression per element is the same.  dy may
// be gv itself (same address, ldd == ldg): a thread reads all its elements of a row before it writes them.
struct CtBwdArgs {
    const float *gv, *y, *a, *b, *mean, *rstd;
    const double* sums;    // [2 C]: (sum dz, sum dz xhat) of these M rows -> dbeta, dgamma
    const double* gsums;   // [2 C]: the same sums over all Mtot rows -> k1, k2
    float* dy;             // [M][ldd] or null
    uint16_t* dp;          // [3][M][ldp] or null
    float *dgamma, *dbeta; // [C] or null
    long M, Mtot;
    int C, Cpad, ldg, ldy, ldd, ldp, act, has_bn;
};

template <int RUN>
__global__ __launch_bounds__(ROWBN_THREADS) void ct_act_bwd_kernel(CtBwdArgs p) {
    const int runs = p.Cpad / RUN;
    const long total = p.M * runs, pstride = p.M * (long)p.ldp;
    if (p.has_bn && p.dgamma && blockIdx.x == 0)
        for (int c = threadIdx.x; c < p.C; c += ROWBN_THREADS) {
            p.dbeta[c] = (float)p.sums[c];
            p.dgamma[c] = (float)p.sums[p.C + c];
        }
    const double inv_m = 1.0 / (double)p.Mtot;
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long m = idx / runs;
        const int c0 = (int)(idx - m * runs) * RUN;
        f32x4 d[2] = {z4, z4};
        if (c0 < p.C) {                                                 // C % 16 == 0, RUN <= 8: a run is inside C or outside
#pragma unroll
            for (int h = 0; h < RUN / 4; ++h) {
                const int c = c0 + 4 * h;
                const f32x4 g4 = RPB_SLD4(p.gv + m * p.ldg + c);
                f32x4 y4 = z4;
                if (p.has_bn || p.act) y4 = RPB_SLD4(p.y + m * p.ldy + c);
                if (p.has_bn) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(p.a + c), b4 = *reinterpret_cast<const f32x4*>(p.b + c);
                    const f32x4 mu = *reinterpret_cast<const f32x4*>(p.mean + c), rs = *reinterpret_cast<const f32x4*>(p.rstd + c);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float k1 = (float)(p.gsums[c + i] * inv_m), k2 = (float)(p.gsums[p.C + c + i] * inv_m);
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
            if (RUN == 8) *reinterpret_cast<f32x4*>(p.dy + m * p.ldd + c0 + 4) = d[1];
        }
        if (RUN == 8 && p.dp) split3_store(p.dp, m * p.ldp + c0, pstride, d[0], d[1]);
    }
}

// The argument checks and the launch of both backward applies; `who` names the entry point in the messages.  A refused call writes nothing.
static int rowbn_bwd_apply(const char* who, const float* gv, int ldg, const float* y, int ldy, const float* a, const float* b, const float* mean,
                           const float* rstd, const double* sums, const double* gsums, long M, long Mtot, int C, int Cpad, int act,
                           int has_bn, float* dy, int ldd, void* dy_planes, int ldp, float* dgamma, float* dbeta, void* stream) {
    RPB_REQUIRE(gv && (dy || dy_planes) && M > 0 && M < (1L << 31) && rowbn_chan_ok(C, 16, 256) && Cpad >= C && Cpad % 4 == 0 && (act == 0 || act == 1) &&
                    (has_bn == 0 || has_bn == 1),
                "%s: bad arguments (M=%ld C=%d Cpad=%d act=%d has_bn=%d; C in {16, 32, 64, 128, 256}, Cpad >= C, Cpad %% 4 == 0)", who, M, C, Cpad,
                act, has_bn);
    RPB_REQUIRE(Mtot >= M, "%s: M_total=%ld must be >= M=%ld (the rows of all ranks, this rank's included)", who, Mtot, M);
    RPB_REQUIRE(ldg >= C && ldg % 4 == 0 && rowbn_al16(gv), "%s: ldg=%d (>= C, %% 4 == 0, gv 16-byte aligned)", who, ldg);
    RPB_REQUIRE(!(has_bn || act) || (y && ldy >= C && ldy % 4 == 0 && rowbn_al16(y)), "%s: y / ldy=%d (>= C, %% 4 == 0, 16-byte aligned)", who, ldy);
    RPB_REQUIRE(!has_bn || (a && b && mean && rstd && sums && gsums && rowbn_al16(a) && rowbn_al16(b) && rowbn_al16(mean) && rowbn_al16(rstd) &&
                            (!dgamma == !dbeta)),
                "%s: has_bn needs a, b, mean, rstd (16-byte aligned) and sums; dgamma and dbeta come together", who);
    RPB_REQUIRE(!dy || (ldd >= Cpad && ldd % 4 == 0 && rowbn_al16(dy)), "%s: ldd=%d (>= Cpad, %% 4 == 0, dy 16-byte aligned)", who, ldd);
    RPB_REQUIRE(!dy_planes || (Cpad % 8 == 0 && ldp >= Cpad && ldp % 8 == 0 && rowbn_al16(dy_planes)),
                "%s: plane output needs a 16-byte aligned first column, Cpad %% 8 == 0 and ldp %% 8 == 0 (Cpad=%d ldp=%d)", who, Cpad, ldp);
    CtBwdArgs p{gv, y, a, b, mean, rstd, sums, gsums, dy, (uint16_t*)dy_planes, dgamma, dbeta, M, Mtot, C, Cpad, ldg, ldy, ldd, ldp, act, has_bn};
    if (Cpad % 8 == 0)
        hipLaunchKernelGGL(ct_act_bwd_kernel<8>, dim3(rowbn_grid(M * (Cpad / 8))), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(ct_act_bwd_kernel<4>, dim3(rowbn_grid(M * (Cpad / 4))), dim3(ROWBN_THREADS), 0, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH(who);
}

extern "C" int rpb_rowbn_act_bwd_apply(const float* gv, int ldg, const float* y, int ldy, const float* a, const float* b, const float* mean,
                                       const float* rstd, const double* sums, long M, int C, int Cpad, int act, int has_bn, float* dy,
                                       int ldd, void* dy_planes, int ldp, float* dgamma, float* dbeta, void* stream) {
    return rowbn_bwd_apply("rowbn_act_bwd_apply", gv, ldg, y, ldy, a, b, mean, rstd, sums, sums, M, M, C, Cpad, act, has_bn, dy, ldd, dy_planes,
                           ldp, dgamma, dbeta, stream);
}

// The BatchNorm form (has_bn = 1) over the rows of several ranks.  With sums_global == sums_local and M_total == M it has the bits of
// rpb_rowbn_act_bwd_apply: the same kernel, the same expression per element.
extern "C" int rpb_rowbn_act_bwd_apply_sync(const float* gv, int ldg, const float* y, int ldy, const float* a, const float* b,
                                            const float* mean, const float* rstd, const double* sums_local, const double* sums_global, long M,
                                            long M_total, int C, int Cpad, int act, float* dy, int ldd, void* dy_planes, int ldp,
                                            float* dgamma, float* dbeta, void* stream) {
    return rowbn_bwd_apply("rowbn_act_bwd_apply_sync", gv, ldg, y, ldy, a, b, mean, rstd, sums_local, sums_global, M, M_total, C, Cpad, act, 1,
                           dy, ldd, dy_planes, ldp, dgamma, dbeta, stream);
}
