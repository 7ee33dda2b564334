// Backward of the projection head on the bf16 matrix pipe, without the gu round trips ("pjx"):
//
//   fno.py:121-125    u = fc1 a + b1 (64 -> 128),  v = gelu(u),  out = fc2 v + b2        a = crop(act(BN(s_{L-1})))
//   autograd          gh = (fc2^T gout) * gelu'(u);   g_a = fc1^T gh (scattered into the padded layout, + the BatchNorm-backward
//                     sums of the last Fourier layer);   d fc1 = gh^T a,  d b1 = sum gh,  d fc2 = gout^T v,  d b2 = sum gout
//
// Round 1 ran this as three kernels chained through gu = gh in HBM ([ncrop][128] fp32, written by proj_bwd with dword stores,
// read by the fc1-dgrad cell_mix and again by cell_wgrad, all on the fp32 matrix pipe).  Here:
//
//   pjx_dgrad  (lane = cell):    reads gh from gu (rows written by pjx_head_kernel<true>) as the B operand of  g_a^T = W1^T gh^T;
//                                16 B stores of g_a into the padded tensor (zeros in the pad margin), BatchNorm-backward sums of the
//                                last layer from the x registers the kernel already holds.
//   pjx_head   (lane = cell):    the head's forward, and its backward up to gu and the fc2 / bias gradient partials.
// (Recomputing gh inside the dgrad and weight-gradient kernels instead of storing gu was built and measured slower: 3.4 against 2.2 ms
// for the dgrad at B = 32, the second evaluation of act' on 128 hidden units per cell costs more VALU time than the 5.4 GB it saves.)
#include "rpb_mma.h"
#include "rpb_pjx.h"
#include <stdlib.h>

#define PJ_HID 128
#define PJ_WAVES 8
#define PJ_DOMAX 4

namespace {
// six products of the three-plane split, small terms first
#define PJ_MAC6(ACC, AH, AM, AL, BH, BM, BL) \
    ACC = mfma16(AH, BL, ACC);                \
    ACC = mfma16(AL, BH, ACC);                \
    ACC = mfma16(AM, BM, ACC);                \
    ACC = mfma16(AH, BM, ACC);                \
    ACC = mfma16(AM, BH, ACC);                \
    ACC = mfma16(AH, BH, ACC);

// d/du of the head's activation: exact-erf GELU (fno.py:124) or SiLU (Galerkin SpectralRegressor); v = act(u) as well
__device__ __forceinline__ void act_pair(float u, bool silu, float& v, float& d) {
    if (silu) {
        const float sig = 1.0f / (1.0f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * u));
        v = u * sig;
        d = sig * (1.0f + u * (1.0f - sig));
    } else {
        const float cdf = 0.5f * (1.0f + fast_erf(u * 0.70710678118654752440f));
        const float pdf = 0.39894228040143267794f * __builtin_amdgcn_exp2f(-0.72134752044448170368f * u * u);
        v = u * cdf;
        d = cdf + u * pdf;
    }
}
// channel of contraction index (ks, kg, e) under the 4 x 16 B-per-cell load pattern (see rpb_cmx.hip)
__device__ __forceinline__ int chan_of(int ks, int kg, int e) { return 16 * (2 * ks + (e >> 2)) + 4 * kg + (e & 3); }
}  // namespace

struct PjxArgs {
    const float* s;       // padded pre-BN tensor of the last Fourier layer [B*Tp*Hp*Wp][64]  (a = xf(s) on the cropped cells)
    const float* w1;      // fc1.weight [128][64]
    const float* gu;      // gh [ncrop][128] as written by rpb_proj_bwd
    float* g;             // [ncell][64] gradient w.r.t. the layer output, padded layout
    float* stats_part;    // [slots][2][64] BatchNorm-backward sums (sum gz, sum gz*shat)
    int B;
    CropMap cm;
    XForm xf;             // BatchNorm (+GELU flag) of the last layer: mean, invstd, gamma, beta
};

// ------------------------------------------------------------------------------------------------------------ dgrad
// gh is READ from p.gu ([ncrop][128] fp32, written by rpb_proj_bwd): the kernel is the fc1-dgrad "gather" (one GEMM, no activation),
// with the lane's 2 x 16 B per K-step as its contraction values (k = (s, kg, e) <-> hidden 32 s + 8 kg + e).  Measured at B = 32:
// 2.2 ms, round-1 fp32 kernel 3.3 ms.
__global__ __launch_bounds__(PJ_WAVES * 64) void pjx_dgrad_kernel(PjxArgs p) {
    extern __shared__ u32x4 lds4[];
    u32x4* W1T = lds4;                              // [s 4][plane 3][mt2 4][lane]   A of g^T = W1^T gh^T   (rows = channel)
    float* xfl = reinterpret_cast<float*>(W1T + 4 * 3 * 4 * 64);     // [4][64] mean, invstd, gamma, beta
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, kg = lane >> 4;
    for (int idx = tid; idx < 4 * 4 * 64; idx += blockDim.x) {
        const int l = idx & 63, mt2 = (idx >> 6) & 3, s = idx >> 8;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p.w1[(32 * s + 8 * (l >> 4) + e) * 64 + 16 * mt2 + (l & 15)];
        bf16x8 h, m, lo;
        split8(v, h, m, lo);
        W1T[((s * 3 + 0) * 4 + mt2) * 64 + l] = __builtin_bit_cast(u32x4, h);
        W1T[((s * 3 + 1) * 4 + mt2) * 64 + l] = __builtin_bit_cast(u32x4, m);
        W1T[((s * 3 + 2) * 4 + mt2) * 64 + l] = __builtin_bit_cast(u32x4, lo);
    }
    if (tid < 64) {
        xfl[tid] = p.xf.mean[tid];
        xfl[64 + tid] = p.xf.invstd[tid];
        xfl[128 + tid] = p.xf.gamma[tid];
        xfl[192 + tid] = p.xf.beta[tid];
    }
    __syncthreads();

    const CropMap cm = p.cm;
    const long G = (long)p.B * cm.Tp * cm.Hp;
    const long nslots = (long)gridDim.x * PJ_WAVES;
    const long slot = (long)blockIdx.x * PJ_WAVES + wave;
    const int TQ = (cm.Wp + 15) >> 4;
    const unsigned line_bytes = (unsigned)cm.Wp * 256u;
    // the lane's 16 channels 16 i + 4 kg + c (as loaded) == 16 mt2 + 4 mg + r (as produced): sums live per lane, reduced at the end
    f32x4 ssum[4], ssq[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ssum[i] = ssq[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long g = slot; g < G; g += nslots) {
        const int h = (int)(g % cm.Hp);
        const long r2 = g / cm.Hp;
        const int t = (int)(r2 % cm.Tp);
        const long b = r2 / cm.Tp;
        const rsrc_t ro = make_rsrc(p.g + g * cm.Wp * 64, line_bytes);
        if (h >= cm.H || t >= cm.T) {                            // uniform: the whole line is padding -> zeros
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            for (int off = lane * 16; off < (int)line_bytes; off += 1024) st16<0>(z, ro, off);
            continue;
        }
        const long rc = (b * cm.T + t) * cm.H + h;               // cropped line
        const rsrc_t rx = make_rsrc(p.s + g * cm.Wp * 64, (unsigned)cm.W * 256u);            // cells >= W read as 0
        const rsrc_t rg = make_rsrc(p.gu + rc * cm.W * PJ_HID, (unsigned)(cm.W * PJ_HID) * 4u);    // cells >= W read as 0
        for (int q = 0; q < TQ; ++q) {
            asm volatile("" ::: "memory");
            const bool live = 16 * q < cm.W;                     // uniform: the tile holds cropped cells
            if (!live) {                                         // margin cells W .. Wp-1: zeros
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int i = 0; i < 4; ++i) st16<0>(z, ro, (16 * q + n16) * 256 + i * 64 + kg * 16);
                continue;
            }
            u32x4 xa[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) xa[i] = ld16<0>(rx, (16 * q + n16) * 256 + i * 64 + kg * 16);
            f32x4 shat[4];                                       // (s - mean) * invstd at the lane's 16 channels: reused by the sums
            f32x4 acc[8];                                        // gh rows of the lane's cell: 32 B per K-step
#pragma unroll
            for (int i = 0; i < 8; ++i)
                acc[i] = __builtin_bit_cast(f32x4, ld16<0>(rg, (16 * q + n16) * 512 + (i >> 1) * 128 + kg * 32 + (i & 1) * 16));
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 xv = __builtin_bit_cast(f32x4, xa[i]);
                const f32x4 mu = *reinterpret_cast<const f32x4*>(xfl + 16 * i + 4 * kg);
                const f32x4 is = *reinterpret_cast<const f32x4*>(xfl + 64 + 16 * i + 4 * kg);
                shat[i] = (xv - mu) * is;
            }
            // ---- g^T = W1^T gh^T: the contraction values of lane-group mg in K-step s are hidden units 32 s + 8 mg + e
            f32x4 acc2[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                float v[8];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = acc[2 * s][r];
                    v[4 + r] = acc[2 * s + 1][r];
                }
                bf16x8 Bh, Bm, Bl;
                split8(v, Bh, Bm, Bl);
#pragma unroll
                for (int mt2 = 0; mt2 < 4; ++mt2) {
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, W1T[((s * 3 + 0) * 4 + mt2) * 64 + lane]);
                    const bf16x8 am = __builtin_bit_cast(bf16x8, W1T[((s * 3 + 1) * 4 + mt2) * 64 + lane]);
                    const bf16x8 al = __builtin_bit_cast(bf16x8, W1T[((s * 3 + 2) * 4 + mt2) * 64 + lane]);
                    PJ_MAC6(acc2[mt2], ah, am, al, Bh, Bm, Bl)
                }
            }
            // ---- store 4 x 16 B (channels 16 mt2 + 4 mg ..) of the lane's cell; BatchNorm-backward sums (cells >= W carry g == 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                st16<0>(acc2[i], ro, (16 * q + n16) * 256 + i * 64 + kg * 16);
                ssum[i] += acc2[i];
                ssq[i] += acc2[i] * shat[i];
            }
        }
    }
    // per-channel totals: sum over the 16 cell lanes of a lane group, then lane n16 == 0 of group mg writes channels 16 i + 4 mg + c
    float* part = p.stats_part + slot * 128;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float a = ssum[i][c], q2 = ssq[i][c];
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                a += __shfl_xor(a, off, 64);
                q2 += __shfl_xor(q2, off, 64);
            }
            if (n16 == 0) {
                part[16 * i + 4 * kg + c] = a;
                part[64 + 16 * i + 4 * kg + c] = q2;
            }
        }
}

static size_t pjx_dgrad_lds() { return (size_t)(4 * 3 * 4 * 64) * 16 + 256 * 4; }

static bool pjx_off() {
    static const bool off = getenv("RPB_PROJ_F32") && atoi(getenv("RPB_PROJ_F32")) == 1;       // round-1 fp32 kernels through gu
    return off;
}

extern "C" int rpb_proj_bwd_fused_supported(int C, int DO, int W, int Wp) {
    return !pjx_off() && C == 64 && DO >= 1 && DO <= PJ_DOMAX && W >= 16 && Wp >= W;
}

extern "C" long rpb_proj_dgrad_slots(int B, int Tp, int Hp) {
    const long G = (long)B * Tp * Hp;
    long grid = 2L * rpb_num_cus();                  // the load flavour needs 128 registers and 50 KB of LDS: two workgroups per CU
    const long need = (G + PJ_WAVES - 1) / PJ_WAVES;
    if (grid > need) grid = need;
    return grid * PJ_WAVES;
}

// g [ncell][64] = crop-scatter( fc1^T gu ),  gu = gh [ncrop][128] as written by rpb_proj_bwd; stats_part [rpb_proj_dgrad_slots][2][64]
// = partial (sum g, sum g * shat) over all cells, shat = (s - mean) * invstd  (the last layer has no GELU after its BatchNorm, so gz = g)
extern "C" int rpb_proj_dgrad(const float* s, const float* w1, const float* gu, float* g, float* stats_part, int B, int DO, int T,
                              int H, int W, int Tp, int Hp, int Wp, const float* xf_mean, const float* xf_invstd, const float* xf_gamma,
                              const float* xf_beta, int xf_gelu, void* stream) {
    RPB_REQUIRE(s && w1 && gu && g && stats_part && xf_mean && xf_invstd && xf_gamma && xf_beta, "proj_dgrad: null pointer");
    RPB_REQUIRE(rpb_proj_bwd_fused_supported(64, DO, W, Wp), "proj_dgrad: unsupported shape (DO=%d W=%d Wp=%d)", DO, W, Wp);
    PjxArgs p{};
    p.s = s; p.w1 = w1; p.gu = gu; p.g = g; p.stats_part = stats_part; p.B = B;
    p.cm = CropMap{T, H, W, Tp, Hp, Wp};
    p.xf = XForm{xf_mean, xf_invstd, xf_gamma, xf_beta, xf_gelu};
    const int grid = (int)(rpb_proj_dgrad_slots(B, Tp, Hp) / PJ_WAVES);
    const size_t lds = pjx_dgrad_lds();
    (void)hipFuncSetAttribute((const void*)pjx_dgrad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(pjx_dgrad_kernel, dim3(grid), dim3(PJ_WAVES * 64), lds, (hipStream_t)stream, p);
    RPB_CHECK_LAUNCH("proj_dgrad");
}

// ------------------------------------------------------------------------------------------------------------ head forward / gu
// The projection head itself on the bf16 matrix pipe (replaces the fp32-MFMA kernels of rpb_proj.hip for C = 64):
//   BWD = false:  out[cell][j] = b2[j] + sum_hid w2[j][hid] act(u[hid]),  u = fc1 a + b1           (fno.py:123-125)
//   BWD = true :  gu[cell][hid] = (sum_j gout[cell][j] w2[j][hid]) act'(u[hid])  + partial sums of d fc2.weight, d fc1.bias, d fc2.bias
// u^T = W1 a^T is computed as in the data-gradient kernel above (hidden units = MFMA rows, the lane's cell = MFMA column), so a lane
// holds the 32 hidden units {16 mt + 4 mg + r} of ONE cell: the fc2 contraction is 32 FMAs per output + two cross-group adds, the
// gu rows are 16 B stores, and the parameter-gradient sums are per-lane accumulators reduced over the 16 cell lanes once at the end.
struct PjhArgs {
    const float* s;
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    const float* gout;    // BWD: [ncrop][DO]
    float* out;           // FWD: [ncrop][DO]
    float* gu;            // BWD: [ncrop][128]
    float* part;          // BWD: [slots][DO*128 + 128 + DO]
    int B, DO, act;
    CropMap cm;
    XForm xf;
};

// DOT = 16 (forward only: the combustion configurations have 16 output features): fc2 runs on the matrix pipe as well -- the
//   activated hidden units in the accumulators are the B operand of out^T = W2 v^T (rows {4 mg + r, 16 + 4 mg + r} of a 32-row
//   K-step, the same accumulator-as-operand trick as the data gradient), W2 sits in LDS in A-operand order.
// BFIN: the input is STORED as bf16 [ncell][64] (BASELINE.json configs[4]): one 16 B load is the exact B operand of a K-step
//   (channel 32 ks + 8 kg + e), three products instead of six, no lazy transform.
template <bool BWD, int DOT, bool BFIN = false>
__global__ __launch_bounds__(PJ_WAVES * 64) void pjx_head_kernel(PjhArgs p) {
    static_assert(!(BWD && (BFIN || DOT > 4)), "gu producer: fp32 input, <= 4 outputs");
    constexpr bool FC2M = DOT > 4;
    extern __shared__ u32x4 lds4[];
    u32x4* W1A = lds4;                                              // [ks 2][plane 3][mt 8][lane]
    float* xfl = reinterpret_cast<float*>(W1A + 2 * 3 * 8 * 64);    // [4][64]
    float* b1l = xfl + 256;                                         // [128]
    float* w2l = b1l + PJ_HID;                                      // [DOT][128]            (FC2M: unused)
    u32x4* W2A = reinterpret_cast<u32x4*>(w2l + (FC2M ? 0 : DOT * PJ_HID));   // FC2M: [s 4][plane 3][lane]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, kg = lane >> 4;
    const int DO = p.DO;
    for (int idx = tid; idx < 2 * 8 * 64; idx += blockDim.x) {
        const int l = idx & 63, mt = (idx >> 6) & 7, ks = idx >> 9;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = p.w1[(16 * mt + (l & 15)) * 64 + (BFIN ? 32 * ks + 8 * (l >> 4) + e : chan_of(ks, l >> 4, e))];
        bf16x8 h, m, lo;
        split8(v, h, m, lo);
        W1A[((ks * 3 + 0) * 8 + mt) * 64 + l] = __builtin_bit_cast(u32x4, h);
        W1A[((ks * 3 + 1) * 8 + mt) * 64 + l] = __builtin_bit_cast(u32x4, m);
        W1A[((ks * 3 + 2) * 8 + mt) * 64 + l] = __builtin_bit_cast(u32x4, lo);
    }
    for (int idx = tid; idx < PJ_HID; idx += blockDim.x) b1l[idx] = p.b1[idx];
    if (FC2M) {
        for (int idx = tid; idx < 4 * 64; idx += blockDim.x) {
            const int l = idx & 63, s = idx >> 6;
            const int j = l & 15;
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = j < DO ? p.w2[j * PJ_HID + 32 * s + 16 * (e >> 2) + 4 * (l >> 4) + (e & 3)] : 0.f;
            bf16x8 h, m, lo;
            split8(v, h, m, lo);
            W2A[(s * 3 + 0) * 64 + l] = __builtin_bit_cast(u32x4, h);
            W2A[(s * 3 + 1) * 64 + l] = __builtin_bit_cast(u32x4, m);
            W2A[(s * 3 + 2) * 64 + l] = __builtin_bit_cast(u32x4, lo);
        }
    } else {
        for (int idx = tid; idx < DOT * PJ_HID; idx += blockDim.x) w2l[idx] = idx < DO * PJ_HID ? p.w2[idx] : 0.f;
    }
    const bool has_xf = !BFIN && p.xf.mean != nullptr;
    if (tid < 64) {
        xfl[tid] = has_xf ? p.xf.mean[tid] : 0.f;
        xfl[64 + tid] = has_xf ? p.xf.invstd[tid] : 1.f;
        xfl[128 + tid] = has_xf ? p.xf.gamma[tid] : 1.f;
        xfl[192 + tid] = has_xf ? p.xf.beta[tid] : 0.f;
    }
    __syncthreads();

    const CropMap cm = p.cm;
    const long GL = (long)p.B * cm.T * cm.H;                        // cropped lines
    const long nslots = (long)gridDim.x * PJ_WAVES;
    const long slot = (long)blockIdx.x * PJ_WAVES + wave;
    const int TQ = (cm.W + 15) >> 4;
    const bool xgelu = has_xf && p.xf.gelu != 0, silu = p.act == 1;
    float b2v[DOT];
#pragma unroll
    for (int j = 0; j < DOT; ++j) b2v[j] = (!BWD && j < DO) ? p.b2[j] : 0.f;
    f32x4 db1[BWD ? 8 : 1], dw2[BWD ? DOT : 1][BWD ? 8 : 1];
    float db2[DOT];
#pragma unroll
    for (int j = 0; j < DOT; ++j) db2[j] = 0.f;
    if (BWD) {
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            db1[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < DOT; ++j) dw2[j][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    auto line_of = [&](long gl) {                                   // cropped line -> padded line
        const int h = (int)(gl % cm.H);
        const long r2 = gl / cm.H;
        return ((r2 / cm.T) * cm.Tp + r2 % cm.T) * cm.Hp + h;
    };
    u32x4 xa[BFIN ? 2 : 4];
    auto issue = [&](long gl, int q) {
        if (BFIN) {                                                  // 128 B per cell: loads ks = 0, 1 are the two K-steps
            const rsrc_t rx = make_rsrc(p.s + line_of(gl) * cm.Wp * 32, (unsigned)cm.W * 128u);
#pragma unroll
            for (int i = 0; i < 2; ++i) xa[i] = ld16<0>(rx, (16 * q + n16) * 128 + i * 64 + kg * 16);
        } else {
            const rsrc_t rx = make_rsrc(p.s + line_of(gl) * cm.Wp * 64, (unsigned)cm.W * 256u);      // cells >= W read as 0
#pragma unroll
            for (int i = 0; i < 4; ++i) xa[i] = ld16<0>(rx, (16 * q + n16) * 256 + i * 64 + kg * 16);
        }
    };
    if (slot < GL) issue(slot, 0);
    for (long gl = slot; gl < GL; gl += nslots) {
        const rsrc_t rgo = make_rsrc((BWD ? p.gout : p.out) + gl * cm.W * DO, (unsigned)(cm.W * DO) * 4u);
        const rsrc_t rgu = make_rsrc(BWD ? p.gu + gl * cm.W * PJ_HID : p.s, BWD ? (unsigned)(cm.W * PJ_HID) * 4u : 0u);
        for (int q = 0; q < TQ; ++q) {
            asm volatile("" ::: "memory");
            const bool last = q + 1 == TQ;
            const long gn = last ? gl + nslots : gl;
            f32x4 acc[8];
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) acc[mt] = *reinterpret_cast<const f32x4*>(b1l + 16 * mt + 4 * kg);
            float go[DOT];
#pragma unroll
            for (int j = 0; j < DOT; ++j) go[j] = (BWD && j < DO) ? buf_load_f32(rgo, ((16 * q + n16) * DO + j) * 4, 0) : 0.f;
            bf16x8 Bh[2], Bm[2], Bl[2];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                if (BFIN) {
                    Bh[ks] = __builtin_bit_cast(bf16x8, xa[ks]);
                    continue;
                }
                float v[8];
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int i = BFIN ? 0 : 2 * ks + hf;
                    const f32x4 xv = __builtin_bit_cast(f32x4, xa[i]);
                    const f32x4 mu = *reinterpret_cast<const f32x4*>(xfl + 16 * i + 4 * kg);
                    const f32x4 is = *reinterpret_cast<const f32x4*>(xfl + 64 + 16 * i + 4 * kg);
                    const f32x4 ga = *reinterpret_cast<const f32x4*>(xfl + 128 + 16 * i + 4 * kg);
                    const f32x4 be = *reinterpret_cast<const f32x4*>(xfl + 192 + 16 * i + 4 * kg);
                    f32x4 z = bn4(xv, mu, is, ga, be);
                    if (xgelu) z = gelu4(z);
#pragma unroll
                    for (int c = 0; c < 4; ++c) v[4 * hf + c] = z[c];
                }
                split8(v, Bh[ks], Bm[ks], Bl[ks]);
            }
            if (gn < GL) issue(gn, last ? 0 : q + 1);               // the next tile's loads fly during the products below
            // MG row tiles advance together: MG independent accumulation chains per product keep the matrix pipe issuing back to back
            constexpr int MG = BWD ? 2 : 4;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int m0 = 0; m0 < 8; m0 += MG) {
                    bf16x8 ah[MG], am[MG], al[MG];
#pragma unroll
                    for (int u = 0; u < MG; ++u) {
                        ah[u] = __builtin_bit_cast(bf16x8, W1A[((ks * 3 + 0) * 8 + m0 + u) * 64 + lane]);
                        am[u] = __builtin_bit_cast(bf16x8, W1A[((ks * 3 + 1) * 8 + m0 + u) * 64 + lane]);
                        al[u] = __builtin_bit_cast(bf16x8, W1A[((ks * 3 + 2) * 8 + m0 + u) * 64 + lane]);
                    }
#define PJ_ROW(AP, BP) _Pragma("unroll") for (int u = 0; u < MG; ++u) acc[m0 + u] = mfma16(AP[u], BP[ks], acc[m0 + u]);
                    if (BFIN) {
                        if (RPB_BF16_CONST_PLANES > 2) { PJ_ROW(al, Bh) }
                        PJ_ROW(am, Bh) PJ_ROW(ah, Bh)
                    } else {
                        PJ_ROW(ah, Bl) PJ_ROW(al, Bh) PJ_ROW(am, Bm) PJ_ROW(ah, Bm) PJ_ROW(am, Bh) PJ_ROW(ah, Bh)
                    }
#undef PJ_ROW
                }
            if (!BWD && FC2M) {
                // out^T [j][cell] = W2 v^T + b2: K-step s takes hidden rows {32 s + 4 mg + r, 32 s + 16 + 4 mg + r} = acc[2 s], acc[2 s + 1]
                f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = 4 * kg + r < DO ? p.b2[4 * kg + r] : 0.f;
#pragma unroll
                for (int s4 = 0; s4 < 4; ++s4) {
                    f32x4 v0, v1;
                    if (silu) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float a0, a1, d;
                            act_pair(acc[2 * s4][r], true, a0, d);
                            act_pair(acc[2 * s4 + 1][r], true, a1, d);
                            v0[r] = a0;
                            v1[r] = a1;
                        }
                    } else {
                        v0 = gelu4(acc[2 * s4]);
                        v1 = gelu4(acc[2 * s4 + 1]);
                    }
                    float v[8];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        v[r] = v0[r];
                        v[4 + r] = v1[r];
                    }
                    bf16x8 Vh, Vm, Vl;
                    split8(v, Vh, Vm, Vl);
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, W2A[(s4 * 3 + 0) * 64 + lane]);
                    const bf16x8 am = __builtin_bit_cast(bf16x8, W2A[(s4 * 3 + 1) * 64 + lane]);
                    const bf16x8 al = __builtin_bit_cast(bf16x8, W2A[(s4 * 3 + 2) * 64 + lane]);
                    PJ_MAC6(o, ah, am, al, Vh, Vm, Vl)
                }
                // lane (cell n16, group mg) holds outputs j = 4 mg + r of its cell
                if ((DO & 3) == 0) {
                    if (4 * kg < DO) st16<0>(o, rgo, ((16 * q + n16) * DO + 4 * kg) * 4);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (4 * kg + r < DO) buf_store_f32(o[r], rgo, ((16 * q + n16) * DO + 4 * kg + r) * 4, 0);
                }
            } else if (!BWD) {
                float po[DOT];
#pragma unroll
                for (int j = 0; j < DOT; ++j) po[j] = 0.f;
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    f32x4 vv;
                    if (silu) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float v1, d;
                            act_pair(acc[mt][r], true, v1, d);
                            vv[r] = v1;
                        }
                    } else {
                        vv = gelu4(acc[mt]);
                    }
#pragma unroll
                    for (int j = 0; j < DOT; ++j) {
                        const f32x4 w = *reinterpret_cast<const f32x4*>(w2l + j * PJ_HID + 16 * mt + 4 * kg);
                        const f32x4 pr = w * vv;
                        po[j] += (pr[0] + pr[1]) + (pr[2] + pr[3]);
                    }
                }
#pragma unroll
                for (int j = 0; j < DOT; ++j) {
                    float t = po[j];
                    t += __shfl_xor(t, 16, 64);
                    t += __shfl_xor(t, 32, 64);
                    if (kg == 0 && j < DO) buf_store_f32(t + b2v[j], rgo, ((16 * q + n16) * DO + j) * 4, 0);   // cells >= W: dropped
                }
            } else {
#pragma unroll
                for (int mt = 0; mt < 8; ++mt) {
                    f32x4 gp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < DOT; ++j) gp += *reinterpret_cast<const f32x4*>(w2l + j * PJ_HID + 16 * mt + 4 * kg) * go[j];
                    f32x4 vv, dd;
                    if (silu) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            float v1, d1;
                            act_pair(acc[mt][r], true, v1, d1);
                            vv[r] = v1;
                            dd[r] = d1;
                        }
                    } else {                                        // v = u Phi(u), d = Phi(u) + u phi(u): one erf, packed pairs
                        const f32x4 u = acc[mt];
                        const f32x2 e0 = fast_erf2(u.lo * pk2(0.70710678118654752440f)), e1 = fast_erf2(u.hi * pk2(0.70710678118654752440f));
                        const f32x4 cdf = join4(pk2(0.5f) * (pk2(1.0f) + e0), pk2(0.5f) * (pk2(1.0f) + e1));
                        const f32x4 q2 = (f32x4{-0.72134752044448170368f, -0.72134752044448170368f, -0.72134752044448170368f, -0.72134752044448170368f} * u) * u;
                        f32x4 ex;
#pragma unroll
                        for (int r = 0; r < 4; ++r) ex[r] = __builtin_amdgcn_exp2f(q2[r]);
                        vv = u * cdf;
                        dd = cdf + u * (ex * 0.39894228040143267794f);
                    }
                    const f32x4 guv = gp * dd;                     // cells >= W carry gout == 0 -> 0, and their store is dropped
                    st16<0>(guv, rgu, (16 * q + n16) * 512 + (16 * mt + 4 * kg) * 4);
                    db1[mt] += guv;
#pragma unroll
                    for (int j = 0; j < DOT; ++j) dw2[j][mt] += vv * go[j];
                }
#pragma unroll
                for (int j = 0; j < DOT; ++j) db2[j] += kg == 0 ? go[j] : 0.f;
            }
        }
    }
    if (BWD) {      // sums over the 16 cell lanes of each lane group; lane n16 == 0 of group mg writes hidden 16 mt + 4 mg + r
        float* part = p.part + slot * ((long)DO * PJ_HID + PJ_HID + DO);
        auto red16 = [&](float v) {
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) v += __shfl_xor(v, off, 64);
            return v;
        };
#pragma unroll
        for (int mt = 0; mt < 8; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float b = red16(db1[mt][r]);
                if (n16 == 0) part[DO * PJ_HID + 16 * mt + 4 * kg + r] = b;
#pragma unroll
                for (int j = 0; j < DOT; ++j) {
                    const float w = red16(dw2[j][mt][r]);
                    if (n16 == 0 && j < DO) part[j * PJ_HID + 16 * mt + 4 * kg + r] = w;
                }
            }
#pragma unroll
        for (int j = 0; j < DOT; ++j) {
            float b = red16(db2[j]);                                 // only group 0 counted the cells
            if (lane == 0 && j < DO) part[DO * PJ_HID + PJ_HID + j] = b;
        }
    }
}

static size_t pjx_head_lds(int dot) {
    return (size_t)(2 * 3 * 8 * 64) * 16 + (256 + PJ_HID) * 4 + (dot > 4 ? (size_t)(4 * 3 * 64) * 16 : (size_t)dot * PJ_HID * 4);
}

// ------------------------------------------------------------------------------------------------------------ head entry points
// (called by rpb_proj_fwd / rpb_proj_bwd in rpb_proj.hip when the shape is covered; same arguments, same partial-row layout)
// (the gu producer keeps 32 (1 + DO) gradient accumulators per lane: two fc2 outputs fit the register file, four spill)
bool rpb_pjx_head_supported(int C, int DO, bool bwd) { return !pjx_off() && C == 64 && DO >= 1 && DO <= (bwd ? 2 : 16); }

long rpb_pjx_head_slots(int B, int T, int H, bool bwd) {
    const long GL = (long)B * T * H;
    long grid = (bwd ? 1L : 2L) * rpb_num_cus();          // forward: 122 registers, 60 KB of LDS -> two workgroups per CU
    const long need = (GL + PJ_WAVES - 1) / PJ_WAVES;
    if (grid > need) grid = need;
    return grid * PJ_WAVES;
}

int rpb_pjx_head_launch(bool bwd, const float* s, const float* w1, const float* b1, const float* w2, const float* b2, const float* gout,
                        float* out, float* gu, float* part, long part_rows, int DO, int T, int H, int W, int Tp, int Hp, int Wp, long ncrop,
                        const XForm& xf, int act, hipStream_t st, bool a_bf16) {
    if (!bwd && rpb_pjh_supported(64, DO, act, xf, a_bf16))                       // the evaluation forward, third organisation (csrc/rpb_pjh.hip)
        return rpb_pjh_launch(s, w1, b1, w2, b2, out, (int)(ncrop / ((long)T * H * W)), DO, T, H, W, Tp, Hp, Wp, xf, st, false, a_bf16);
    PjhArgs p{};
    p.s = s; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.b2 = b2; p.gout = gout; p.out = out; p.gu = gu; p.part = part;
    p.B = (int)(ncrop / ((long)T * H * W)); p.DO = DO; p.act = act;
    p.cm = CropMap{T, H, W, Tp, Hp, Wp};
    p.xf = xf;
    long slots = rpb_pjx_head_slots(p.B, T, H, bwd);
    if (bwd && slots > part_rows) slots = part_rows / PJ_WAVES * PJ_WAVES;       // never more partial rows than the caller allocated
    RPB_REQUIRE(slots >= PJ_WAVES, "proj (bf16 pipe): no partial rows");
    const int grid = (int)(slots / PJ_WAVES);
    if (bwd && part_rows > slots)                                                 // rows this launch does not write
        (void)hipMemsetAsync(part + slots * ((long)DO * PJ_HID + PJ_HID + DO), 0, (size_t)(part_rows - slots) * ((long)DO * PJ_HID + PJ_HID + DO) * 4, st);
    const int dot = DO <= 2 ? 2 : (DO <= 4 ? 4 : 16);
    const size_t lds = pjx_head_lds(dot);
    if (a_bf16 && bwd) RPB_FAIL(RPB_ERR_UNSUPPORTED, "proj (bf16 pipe): bf16 activation storage is a forward path");
#define RPB_PJH(BWD_, D_)                                                                                                    \
    if (bwd == BWD_ && dot == D_) {                                                                                          \
        (void)hipFuncSetAttribute((const void*)pjx_head_kernel<BWD_, D_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((pjx_head_kernel<BWD_, D_>), dim3(grid), dim3(PJ_WAVES * 64), lds, st, p);                        \
    }
#define RPB_PJHB(D_)                                                                                                        \
    if (a_bf16 && dot == D_) {                                                                                               \
        (void)hipFuncSetAttribute((const void*)pjx_head_kernel<false, D_, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((pjx_head_kernel<false, D_, true>), dim3(grid), dim3(PJ_WAVES * 64), lds, st, p);                 \
        RPB_CHECK_LAUNCH("proj (bf16 pipe, bf16 storage)");                                                                  \
    }
    RPB_PJHB(2) RPB_PJHB(4) RPB_PJHB(16)
#undef RPB_PJHB
    RPB_PJH(false, 2) RPB_PJH(false, 4) RPB_PJH(false, 16) RPB_PJH(true, 2)
#undef RPB_PJH
    RPB_CHECK_LAUNCH("proj (bf16 pipe)");
}
