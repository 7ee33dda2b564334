// nn.Conv3d(Ci, N, KS, padding = KS / 2), KS odd and <= 7, as an implicit GEMM on the bf16 MFMA with the default (fp32-grade) split-operand
// arithmetic of rpb_mma.h: three bf16 planes per operand, six products per fp32 product, fp32 accumulation -- as rpb_conv3x.  Written for the
// 7x7x7 init_conv of WDNO's denoiser (Ci = 8 (C_in + C_out r), 48 at the cylinder shape): K = KS^3 Ci = 16 464 there, and the column matrix
// rpb_im2col would write is 1.6 GB per sample.  Here it never exists: the A operand is gathered from x [B][T][H][W][Ci] with the zero halo
// formed on load.
//
// K order.  K is walked as (kt, kh) row pairs x 64-channel chunks x (kw, 8-channel group): one MFMA k-step (16 values) is two 8-channel
// groups, one per lane half, so Ci only has to be a multiple of 8 (a chunk's odd last group is paired with a zero group).
// Input reuse.  For one (kt, kh, chunk) a workgroup stages the C7_BM + KS - 1 input rows its 128 output tokens touch -- split into planes on
// the way into LDS, [plane][8-channel group][row] x 16 B -- and all KS taps along W read them at row offsets 0..KS - 1: every input row is
// loaded once per (kt, kh), not once per tap.  The next stage's global loads are in flight during the current stage's MFMAs.
// Weights.  343 Ci x 64 values per N tile do not fit LDS and are read once per workgroup: they are STREAMED from L2 in MFMA B-operand
// order (rpb_conv7x_wprep: one coalesced 1 KB load per plane and 32-wide co tile, straight into registers).
// Work split.  A workgroup owns 128 tokens x 64 co; its four waves split the k-steps round-robin (each holds the whole 128 x 64 tile: 48
// MFMAs per 6 KB of weights) and reduce through LDS in one round at the end, in a fixed order: two calls are bit-equal, no atomics.
// Validity (t, h, w inside the mesh) is a property of the output token and the tap and is applied to the A operand in registers; rows
// whose flat index falls outside [0, M) are zero in LDS, so nothing outside x is read.
#include "rpb_mma.h"

#define C7_BM 128
#define C7_ROWS (C7_BM + 6)
#define C7_NLD ((C7_ROWS * 8 + 255) / 256)

struct Conv7xArgs {
    const float* x;        // [M][Ci]
    const uint16_t* Wz;    // rpb_conv7x_wprep order
    const float* bias;     // [N] or null
    float* out;            // [M][ldo]
    long M;
    int N, Ci, KS, T, H, W, ldo;
};

// k-steps of a full 64-channel chunk, and of all chunks of one (kt, kh)
static __host__ __device__ inline int c7_s64(int KS) { return (KS * 8 + 1) >> 1; }
static __host__ __device__ inline int c7_steps(int Ci, int KS) {
    const int nch = (Ci + 63) >> 6, last = (Ci - (nch - 1) * 64) >> 3;
    return (nch - 1) * c7_s64(KS) + ((KS * last + 1) >> 1);
}

// W [N][Ci][KS][KS][KS] fp32 (nn.Conv3d's own layout) -> Wz[kt][kh][step][3 planes][N / 32][64 lanes][8] bf16; lane = (co & 31) + 32 half,
// element e of (step s of chunk c, half) <-> group g = 2 s + half = kw ng + c8 (ng = the chunk's 8-channel groups), ci = 64 c + 8 c8 + e;
// zero where g is past the chunk's last group
__global__ __launch_bounds__(256) void conv7x_wprep_kernel(const float* __restrict__ W, uint16_t* __restrict__ Wz, int N, int Ci, int KS) {
    const int NT = N >> 5, SP = c7_steps(Ci, KS), S64 = c7_s64(KS), nch = (Ci + 63) >> 6;
    const long total = (long)KS * KS * SP * NT * 64;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    long r = idx >> 6;
    const int nt = (int)(r % NT);
    r /= NT;
    const int sl = (int)(r % SP), tap2 = (int)(r / SP);
    const int kt = tap2 / KS, kh = tap2 - kt * KS;
    int c = sl / S64;
    if (c >= nch) c = nch - 1;
    const int s = sl - c * S64;
    const int chn = Ci - c * 64 < 64 ? Ci - c * 64 : 64, ng = chn >> 3;
    const int g = 2 * s + (lane >> 5);
    const int co = nt * 32 + (lane & 31);
    unsigned h[8], md[8], lo[8];
    if (g < KS * ng) {
        const int kw = g / ng, c8 = g - kw * ng;
        const long KV = (long)KS * KS * KS;
        const float* src = W + ((long)co * Ci + c * 64 + c8 * 8) * KV + ((long)kt * KS + kh) * KS + kw;
#pragma unroll
        for (int e = 0; e < 8; ++e) split3(src[e * KV], h[e], md[e], lo[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = md[e] = lo[e] = 0u;
    }
    u32x4 o[3];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        o[0][q] = h[2 * q] | (h[2 * q + 1] << 16);
        o[1][q] = md[2 * q] | (md[2 * q + 1] << 16);
        o[2][q] = lo[2 * q] | (lo[2 * q + 1] << 16);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const long dst = (((((long)tap2 * SP + sl) * 3 + p) * NT + nt) * 64 + lane) * 8;
        *reinterpret_cast<u32x4*>(Wz + dst) = o[p];
    }
}

__global__ __launch_bounds__(256, 1) void conv7x_kernel(Conv7xArgs a) {
    extern __shared__ u32x4 lds4[];                    // staging [3 planes][8 groups][C7_ROWS] x 16 B; at the end the K-split slots
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int kp = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long m0 = (long)blockIdx.x * C7_BM;
    const int n0 = blockIdx.y * 64;
    const int KS = a.KS, pd = KS >> 1, NT = a.N >> 5;
    const int nch = (a.Ci + 63) >> 6, S64 = c7_s64(KS), SP = c7_steps(a.Ci, KS);
    const int nrows = C7_BM + 2 * pd;                  // rows a stage holds

    int tq[4], hq[4], wq[4];
    bool live[4];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
        const long m = m0 + tm * 32 + col;
        live[tm] = m < a.M;
        const long mm = live[tm] ? m : 0;
        wq[tm] = (int)(mm % a.W);
        const long r = mm / a.W;
        hq[tm] = (int)(r % a.H);
        tq[tm] = (int)((r / a.H) % a.T);
    }
    f32x16 acc[4][2];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) acc[tm][0] = acc[tm][1] = zero16();
    const u32x4 z4 = {0u, 0u, 0u, 0u};
    const f32x4 zf = {0.f, 0.f, 0.f, 0.f};
    const uint16_t* wbase = a.Wz + ((long)(n0 >> 5) * 64 + lane) * 8;
    const long wplane = (long)NT * 512, wstep = 3 * wplane;

    // ---- staging: rows x 8-channel groups, 32 B per item, consecutive threads = consecutive groups of one row (coalesced)
    f32x4 sv[C7_NLD][2];
    bool ok[C7_NLD];
    auto stage_load = [&](int kt, int kh, int c) __attribute__((always_inline)) {
        const int chn = a.Ci - c * 64 < 64 ? a.Ci - c * 64 : 64, ng = chn >> 3;
        const long rowbase = m0 - pd + ((long)(kt - pd) * a.H + (kh - pd)) * a.W;
#pragma unroll
        for (int j = 0; j < C7_NLD; ++j) {
            const int idx = tid + j * 256, row = idx / ng, c8 = idx - row * ng;
            const long q = rowbase + row;
            ok[j] = row < nrows && q >= 0 && q < a.M;
            const float* src = a.x + (ok[j] ? q * a.Ci + c * 64 + c8 * 8 : 0);
            sv[j][0] = *reinterpret_cast<const f32x4*>(src);
            sv[j][1] = *reinterpret_cast<const f32x4*>(src + 4);
        }
    };
    auto stage_store = [&](int c) __attribute__((always_inline)) {
        const int chn = a.Ci - c * 64 < 64 ? a.Ci - c * 64 : 64, ng = chn >> 3;
#pragma unroll
        for (int j = 0; j < C7_NLD; ++j) {
            const int idx = tid + j * 256, row = idx / ng, c8 = idx - row * ng;
            if (row < nrows) {
                const f32x4 v0 = ok[j] ? sv[j][0] : zf, v1 = ok[j] ? sv[j][1] : zf;
                const float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                bf16x8 h, m, l;
                split8(v, h, m, l);
                lds4[(0 * 8 + c8) * C7_ROWS + row] = __builtin_bit_cast(u32x4, h);
                lds4[(1 * 8 + c8) * C7_ROWS + row] = __builtin_bit_cast(u32x4, m);
                lds4[(2 * 8 + c8) * C7_ROWS + row] = __builtin_bit_cast(u32x4, l);
            }
        }
    };

    const int nstage = KS * KS * nch;
    stage_load(0, 0, 0);
    stage_store(0);
    __syncthreads();
    int gcount = 0;                                     // k-steps before this stage: step s of the launch belongs to wave s & 3
    for (int st = 0; st < nstage; ++st) {
        const int tap2 = st / nch, c = st - tap2 * nch;
        const int kt = tap2 / KS, kh = tap2 - kt * KS;
        const bool more = st + 1 < nstage;
        int cn = c + 1, tap2n = tap2;
        if (cn == nch) {
            cn = 0;
            ++tap2n;
        }
        if (more) stage_load(tap2n / KS, tap2n % KS, cn);               // in flight during the MFMAs below
        const int chn = a.Ci - c * 64 < 64 ? a.Ci - c * 64 : 64, ng = chn >> 3;
        const int G = KS * ng, S = (G + 1) >> 1;
        bool vth[4];
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
            vth[tm] = live[tm] && (unsigned)(tq[tm] + kt - pd) < (unsigned)a.T && (unsigned)(hq[tm] + kh - pd) < (unsigned)a.H;
        const uint16_t* wst = wbase + ((long)tap2 * SP + (long)c * S64) * wstep;
        for (int s = (kp - gcount) & 3; s < S; s += 4) {
            const uint16_t* wp = wst + (long)s * wstep;
            u32x4 b[2][3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn) b[tn][p] = *reinterpret_cast<const u32x4*>(wp + p * wplane + tn * 512);
            const int g = 2 * s + half;
            const bool gok = g < G;
            const int kw = gok ? g / ng : 0, c8 = gok ? g - kw * ng : 0;
#pragma unroll
            for (int tm = 0; tm < 4; ++tm) {
                const bool v = gok && vth[tm] && (unsigned)(wq[tm] + kw - pd) < (unsigned)a.W;
                u32x4 av[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    av[p] = lds4[(p * 8 + c8) * C7_ROWS + tm * 32 + col + kw];
                    if (!v) av[p] = z4;
                }
                const u32x4 ah = av[0], am = av[1], al = av[2];
                // small terms first; the two co tiles alternate so consecutive MFMAs are independent
                acc[tm][0] = mfma32b(al, b[0][0], acc[tm][0]);
                acc[tm][1] = mfma32b(al, b[1][0], acc[tm][1]);
                acc[tm][0] = mfma32b(ah, b[0][2], acc[tm][0]);
                acc[tm][1] = mfma32b(ah, b[1][2], acc[tm][1]);
                acc[tm][0] = mfma32b(am, b[0][1], acc[tm][0]);
                acc[tm][1] = mfma32b(am, b[1][1], acc[tm][1]);
                acc[tm][0] = mfma32b(am, b[0][0], acc[tm][0]);
                acc[tm][1] = mfma32b(am, b[1][0], acc[tm][1]);
                acc[tm][0] = mfma32b(ah, b[0][1], acc[tm][0]);
                acc[tm][1] = mfma32b(ah, b[1][1], acc[tm][1]);
                acc[tm][0] = mfma32b(ah, b[0][0], acc[tm][0]);
                acc[tm][1] = mfma32b(ah, b[1][0], acc[tm][1]);
            }
        }
        gcount += S;
        __syncthreads();                                                // everyone has read this stage
        if (more) stage_store(cn);
        __syncthreads();
    }

    // ---- K-split reduction in one round (as rpb_conv3x): row tile tm belongs to wave tm, the others park their partials
    float* red = reinterpret_cast<float*>(lds4);                        // [4 tiles][3 sources][2 co tiles][16 regs][64 lanes]
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
        if (kp != tm) {
            const int rank = kp < tm ? kp : kp - 1;
            float* slot = red + (tm * 3 + rank) * 2048;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) slot[(tn * 16 + r) * 64 + lane] = acc[tm][tn][r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
        if (kp != tm) continue;
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) {
            const float* slot = red + (tm * 3 + k2) * 2048;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tm][tn][r] += slot[(tn * 16 + r) * 64 + lane];
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int n = n0 + tn * 32 + col;
            const float bv = a.bias ? a.bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + tm * 32 + mfma_row(lane, r);
                if (m < a.M) a.out[m * a.ldo + n] = acc[tm][tn][r] + bv;
            }
        }
    }
}

static bool c7_ok(long M, int N, int Ci, int KS) {
    return M > 0 && M < (1L << 31) && (N == 64 || N == 128 || N == 256) && Ci % 8 == 0 && Ci >= 8 && Ci <= 256 && KS >= 1 && KS <= 7 &&
           (KS & 1);
}

extern "C" int rpb_conv7x_supported(long M, int N, int Ci, int KS) { return c7_ok(M, N, Ci, KS) ? 1 : 0; }

extern "C" long rpb_conv7x_wz_elems(int N, int Ci, int KS) {
    if (!c7_ok(1, N, Ci, KS)) return -1;
    return (long)KS * KS * c7_steps(Ci, KS) * 3 * (N / 32) * 512;
}

extern "C" int rpb_conv7x_wprep(const float* W, void* Wz, int N, int Ci, int KS, void* stream) {
    RPB_REQUIRE(W && Wz && c7_ok(1, N, Ci, KS), "conv7x_wprep: N=%d Ci=%d KS=%d unsupported", N, Ci, KS);
    const long total = (long)KS * KS * c7_steps(Ci, KS) * (N / 32) * 64;
    hipLaunchKernelGGL(conv7x_wprep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, (uint16_t*)Wz, N,
                       Ci, KS);
    RPB_CHECK_LAUNCH("conv7x_wprep");
}

extern "C" int rpb_conv7x(const float* x, const void* Wz, const float* bias, float* out, int B, int T, int H, int W, int Ci, int N, int KS,
                          int ldo, void* stream) {
    RPB_REQUIRE(x && Wz && out && B > 0 && T > 0 && H > 0 && W > 0, "conv7x: bad arguments");
    const long M = (long)B * T * H * W;
    RPB_REQUIRE(c7_ok(M, N, Ci, KS) && ldo >= N,
                "conv7x: M=%ld N=%d Ci=%d KS=%d ldo=%d unsupported (N = 64, 128 or 256; Ci %% 8, 8..256; KS odd <= 7)", M, N, Ci, KS, ldo);
    Conv7xArgs a{x, (const uint16_t*)Wz, bias, out, M, N, Ci, KS, T, H, W, ldo};
    const size_t lds = (size_t)4 * 3 * 2048 * sizeof(float);           // the K-split slots (98 304 B) exceed the staging (51 456 B)
    static_assert((size_t)3 * 8 * C7_ROWS * 16 <= (size_t)4 * 3 * 2048 * 4, "staging fits the reduction's LDS");
    (void)hipFuncSetAttribute((const void*)conv7x_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(conv7x_kernel, dim3((unsigned)((M + C7_BM - 1) / C7_BM), N / 64), dim3(256), lds, (hipStream_t)stream, a);
    RPB_CHECK_LAUNCH("conv7x");
}
