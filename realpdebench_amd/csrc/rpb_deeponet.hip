// DeepONet (realpdebench/model/deeponet.py) -- the evaluation forward's own kernels.  The branch CNN's convolutions and the two branch
// Linear layers run on rpb_im2col / rpb_gemm3x / rpb_split3 / rpb_conv3x; this file adds what those do not cover:
//   rpb_don_bn_relu_pool   eval-BatchNorm affine + ReLU + MaxPool3d(2) (floor) or AdaptiveAvgPool3d((1, 4, 4)) on channels-last rows
//   rpb_don_trunk          the trunk MLP 3 -> 64 -> 128 -> p over the N = T_out H W grid points (batch-independent, cached by the model)
//   rpb_don_point_mlp      the output net p -> 512 -> 128 -> C_out on b[b] (.) t[n] for every (sample, point): the hot path, one launch,
//                          bf16 MFMA from three-plane split fp32 operands (rpb_mma.h), hidden activations in registers only.
#include "rpb_mma.h"

// ====================================================================================== BN + ReLU + pooling
// x [B][T][H][W][ldx] (channels 0..C-1 live), y = relu(x * sc[c] + sh[c]) with sc = gamma / sqrt(var + eps), sh = beta - mean * sc.
//   mode 0: out [B][T/2][H/2][W/2][ldo] = max over the 2 x 2 x 2 window (floor: a trailing odd frame / row / column is dropped);
//   mode 1: out [B][1][4][4][ldo] = mean over T and over the bins [floor(i In / 4), ceil((i + 1) In / 4)) of H and W.
// Channels C..ldo-1 of the output are written as zeros (the next convolution's zero-padded input channels).
struct PoolArgs {
    const float* x;
    const float* sc;
    const float* sh;
    float* out;
    int B, T, H, W, C, ldx, ldo, mode;
};

__global__ __launch_bounds__(256) void don_pool_kernel(PoolArgs a) {
    const int To = a.mode ? 1 : a.T / 2, Ho = a.mode ? 4 : a.H / 2, Wo = a.mode ? 4 : a.W / 2;
    const int Q = a.ldo / 4;
    const long total = (long)a.B * To * Ho * Wo * Q;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int q = (int)(idx % Q);
        long r = idx / Q;
        const int wo = (int)(r % Wo);
        r /= Wo;
        const int ho = (int)(r % Ho);
        r /= Ho;
        const int to = (int)(r % To);
        const long b = r / To;
        f32x4 res = {0.f, 0.f, 0.f, 0.f};
        if (4 * q < a.C) {
            const f32x4 sc = *reinterpret_cast<const f32x4*>(a.sc + 4 * q), sh = *reinterpret_cast<const f32x4*>(a.sh + 4 * q);
            int t0, t1, h0, h1, w0, w1;
            if (a.mode) {
                t0 = 0, t1 = a.T;
                h0 = ho * a.H / 4, h1 = ((ho + 1) * a.H + 3) / 4;
                w0 = wo * a.W / 4, w1 = ((wo + 1) * a.W + 3) / 4;
            } else {
                t0 = 2 * to, t1 = t0 + 2;
                h0 = 2 * ho, h1 = h0 + 2;
                w0 = 2 * wo, w1 = w0 + 2;
            }
            for (int t = t0; t < t1; ++t)
                for (int h = h0; h < h1; ++h)
                    for (int w = w0; w < w1; ++w) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + (((b * a.T + t) * a.H + h) * (long)a.W + w) * a.ldx + 4 * q);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float y = fmaf(v[e], sc[e], sh[e]);
                            y = (y > 0.f || y != y) ? y : 0.f;                    // ReLU and max keep a NaN, as torch's do (fmaxf drops it)
                            res[e] = a.mode ? res[e] + y : ((y > res[e] || y != y) ? y : res[e]);      // max of ReLU outputs: 0 is a neutral start
                        }
                    }
            if (a.mode) {
                const float inv = 1.0f / (float)((t1 - t0) * (h1 - h0) * (w1 - w0));
#pragma unroll
                for (int e = 0; e < 4; ++e) res[e] *= inv;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * q + e >= a.C) res[e] = 0.f;
        }
        *reinterpret_cast<f32x4*>(a.out + (((b * To + to) * Ho + ho) * (long)Wo + wo) * a.ldo + 4 * q) = res;
    }
}

extern "C" int rpb_don_bn_relu_pool(const float* x, const float* sc, const float* sh, float* out, int B, int T, int H, int W, int C, int ldx,
                                    int ldo, int mode, void* stream) {
    RPB_REQUIRE(x && sc && sh && out && B > 0 && T > 0 && H > 0 && W > 0 && C > 0, "don_bn_relu_pool: bad arguments");
    RPB_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && ldx >= C && ldo >= C, "don_bn_relu_pool: C=%d ldx=%d ldo=%d (multiples of 4, ld >= C)", C, ldx, ldo);
    RPB_REQUIRE(mode == 1 || (mode == 0 && T >= 2 && H >= 2 && W >= 2), "don_bn_relu_pool: mode=%d with T=%d H=%d W=%d (MaxPool3d(2) needs extents >= 2)", mode, T, H, W);
    PoolArgs a{x, sc, sh, out, B, T, H, W, C, ldx, ldo, mode};
    const long total = (long)B * (mode ? 16 : (long)(T / 2) * (H / 2) * (W / 2)) * (ldo / 4);
    long grid = (total + 255) / 256;
    const long cap = (long)rpb_num_cus() * 16;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(don_pool_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    RPB_CHECK_LAUNCH("don_bn_relu_pool");
}

// ====================================================================================== trunk MLP (vector unit)
// 64 grid points per workgroup, lane = point, wave w owns a quarter of every layer's output units; the weights are read at wave-uniform
// addresses (transposed [k][o], so the units of one k are contiguous), the activations go from wave to wave through LDS stored
// unit-major ([unit][64 points]: conflict-free both ways).
struct TrunkArgs {
    const float *gt, *gh, *gw;            // np.linspace(0, 1, n) of the three axes, as float32
    const float *w1t, *b1, *w2t, *b2, *w3t, *b3;   // [3][64], [64], [64][128], [128], [128][p], [p]
    float* t;                             // [N][p]
    long N;
    int H, W, p;
};

__global__ __launch_bounds__(256) void don_trunk_kernel(TrunkArgs a) {
    __shared__ float h1[64 * 64];
    __shared__ float h2[128 * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long n = (long)blockIdx.x * 64 + lane;
    const long nc = n < a.N ? n : a.N - 1;                     // tail lanes compute a valid point and store nothing
    const int iw = (int)(nc % a.W), ih = (int)((nc / a.W) % a.H), it = (int)(nc / ((long)a.W * a.H));
    const float x0 = a.gt[it], x1 = a.gh[ih], x2 = a.gw[iw];
    {
        const int o0 = wave * 16;
#pragma unroll
        for (int o = 0; o < 16; ++o) {
            float v = a.b1[o0 + o];
            v = fmaf(x0, a.w1t[o0 + o], v);
            v = fmaf(x1, a.w1t[64 + o0 + o], v);
            v = fmaf(x2, a.w1t[128 + o0 + o], v);
            h1[(o0 + o) * 64 + lane] = fmaxf(v, 0.f);
        }
    }
    __syncthreads();
    {
        const int o0 = wave * 32;
        float acc[32];
#pragma unroll
        for (int o = 0; o < 32; ++o) acc[o] = a.b2[o0 + o];
        for (int k = 0; k < 64; ++k) {
            const float h = h1[k * 64 + lane];
            const float* w = a.w2t + k * 128 + o0;
#pragma unroll
            for (int o = 0; o < 32; ++o) acc[o] = fmaf(h, w[o], acc[o]);
        }
#pragma unroll
        for (int o = 0; o < 32; ++o) h2[(o0 + o) * 64 + lane] = fmaxf(acc[o], 0.f);
    }
    __syncthreads();
    const int per = a.p >> 2;                                  // p in {64, 128, 256}: 16, 32 or 64 units per wave, 16 at a time
    for (int c = 0; c < per; c += 16) {
        const int o0 = wave * per + c;
        float acc[16];
#pragma unroll
        for (int o = 0; o < 16; ++o) acc[o] = a.b3[o0 + o];
        for (int k = 0; k < 128; ++k) {
            const float h = h2[k * 64 + lane];
            const float* w = a.w3t + (long)k * a.p + o0;
#pragma unroll
            for (int o = 0; o < 16; ++o) acc[o] = fmaf(h, w[o], acc[o]);
        }
        if (n < a.N) {
            float* dst = a.t + n * a.p + o0;
#pragma unroll
            for (int o = 0; o < 16; o += 4) *reinterpret_cast<f32x4*>(dst + o) = f32x4{acc[o], acc[o + 1], acc[o + 2], acc[o + 3]};
        }
    }
}

extern "C" int rpb_don_trunk(const float* gt, const float* gh, const float* gw, const float* w1t, const float* b1, const float* w2t,
                             const float* b2, const float* w3t, const float* b3, float* t, int T, int H, int W, int p, void* stream) {
    RPB_REQUIRE(gt && gh && gw && w1t && b1 && w2t && b2 && w3t && b3 && t && T > 0 && H > 0 && W > 0, "don_trunk: bad arguments");
    RPB_REQUIRE(p == 64 || p == 128 || p == 256, "don_trunk: p=%d unsupported (64, 128 or 256)", p);
    const long N = (long)T * H * W;
    RPB_REQUIRE((N + 63) / 64 < (1L << 31), "don_trunk: too many points");
    TrunkArgs a{gt, gh, gw, w1t, b1, w2t, b2, w3t, b3, t, N, H, W, p};
    hipLaunchKernelGGL(don_trunk_kernel, dim3((unsigned)((N + 63) / 64)), dim3(256), 0, (hipStream_t)stream, a);
    RPB_CHECK_LAUNCH("don_trunk");
}

// ====================================================================================== the output net, per (sample, point)
// out[b][n][:] = W3 relu(W2 relu(W1 (b[b] (.) t[n]) + b1) + b2) + b3,  W1 [512][P], W2 [128][512], W3 [C_out][128].
//
// Everything is computed TRANSPOSED -- hidden units are MFMA rows, points are MFMA columns -- on v_mfma_f32_32x32x16_bf16:
//   A operand = a 32-unit x 16-k tile of a weight (prepared once on the host side of the model as bf16 planes in lane order),
//   B operand = 16 k x 32 points of the previous layer's activation, split into three bf16 planes in registers.
// In that orientation an accumulator tile D (lane = (point, hg), register r = unit 8 (r / 4) + 4 hg + r % 4 of the tile) IS the next
// layer's B operand after bias + ReLU + split: registers 8 s .. 8 s + 7 of a lane are the 8 k-values of k-step s, with k-group = hg.
// The contraction index of that step is therefore the unit bijection u(s, kg, e) = 8 (2 s + e / 4) + 4 kg + e % 4, and the NEXT layer's
// weight planes are stored in exactly that order (point_weights of model/deeponet.py builds them): no LDS, no cross-lane traffic, no
// transposition between the three layers.
//
// One wave = 32 points of one sample; a workgroup = 4 waves = 128 consecutive points.  The 512 hidden units are walked in 16 blocks
// of 32: layer 1 of the block (P / 16 k-steps x 6 products, even / odd k-steps on two accumulators so that consecutive MFMAs are
// independent) -> bias, ReLU, split -> layer 2 accumulates the block's 32 units into the four 32-unit tiles of the 128-wide hidden
// layer (2 k-steps x 4 tiles x 6 products).  Layer 3 pads C_out to one 32-row tile (zero weight rows; 3 % of the MFMA work).
// b is applied to t when the tile is loaded (one multiply per loaded value against per-sample weight copies).
// The weight operands come straight from global memory (L2 / L1: the four waves of a workgroup walk the same addresses, but nothing
// synchronises them -- there is no barrier in the kernel); every wave reads them in 1 KiB contiguous runs, one step ahead of use.
// Products are accumulated small terms first: lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi.
__device__ __forceinline__ f32x16 mma6(const u32x4 (&w)[3], const u32x4 (&x)[3], f32x16 c) {
    c = mfma32b(w[2], x[0], c);
    c = mfma32b(w[0], x[2], c);
    c = mfma32b(w[1], x[1], c);
    c = mfma32b(w[1], x[0], c);
    c = mfma32b(w[0], x[1], c);
    c = mfma32b(w[0], x[0], c);
    return c;
}
// relu(acc + bias) of a D tile -> the B-operand planes of its two k-steps
__device__ __forceinline__ void act_split(const f32x16& acc, const float* __restrict__ bias16, u32x4 (&hp)[2][3]) {
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 bq = *reinterpret_cast<const f32x4*>(bias16 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = fmaxf(acc[4 * q + e] + bq[e], 0.f);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            unsigned h, m, l;
            rpb_split_pair(v[8 * s + 2 * q], v[8 * s + 2 * q + 1], h, m, l);
            hp[s][0][q] = h;
            hp[s][1][q] = m;
            hp[s][2][q] = l;
        }
}

struct PointArgs {
    const float* t;         // [N][P]
    const float* b;         // [B][P]
    const uint16_t* w1z;    // [16 blocks][P / 16 k-steps][3 planes][64 lanes][8]
    const uint16_t* w2z;    // [16 blocks][2 k-steps][4 tiles][3 planes][64 lanes][8]
    const uint16_t* w3z;    // [4 tiles of the 128 units][2 k-steps][3 planes][64 lanes][8], rows >= C_out zero
    const float* b1z;       // [16 blocks][2 hg][16]: bias in D-register order
    const float* b2z;       // [4 tiles][2 hg][16]
    const float* b3;        // [C_out]
    float* out;             // [B][N][C_out]
    long N;
    int Cout;
};

template <int P>
__global__ __launch_bounds__(256, 1) void don_point_kernel(PointArgs a) {
    constexpr int KS = P / 16;
    const int lane = threadIdx.x & 63, pt = lane & 31, hg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long bi = blockIdx.y;
    const long n = (long)blockIdx.x * 128 + wave * 32 + pt;
    const long nc = n < a.N ? n : a.N - 1;                     // tail: a valid row is read, nothing is stored
    // ---- layer-1 B operand: (b (.) t) of my point, k = 16 ks + 8 hg + e, three planes per k-step
    u32x4 xp[KS][3];
    {
        const float* trow = a.t + nc * P + 8 * hg;
        const float* brow = a.b + bi * P + 8 * hg;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(trow + 16 * ks), t1 = *reinterpret_cast<const f32x4*>(trow + 16 * ks + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(brow + 16 * ks), b1 = *reinterpret_cast<const f32x4*>(brow + 16 * ks + 4);
            const f32x4 v0 = t0 * b0, v1 = t1 * b1;
            unsigned h, m, l;
            rpb_split_pair(v0[0], v0[1], h, m, l);
            xp[ks][0][0] = h, xp[ks][1][0] = m, xp[ks][2][0] = l;
            rpb_split_pair(v0[2], v0[3], h, m, l);
            xp[ks][0][1] = h, xp[ks][1][1] = m, xp[ks][2][1] = l;
            rpb_split_pair(v1[0], v1[1], h, m, l);
            xp[ks][0][2] = h, xp[ks][1][2] = m, xp[ks][2][2] = l;
            rpb_split_pair(v1[2], v1[3], h, m, l);
            xp[ks][0][3] = h, xp[ks][1][3] = m, xp[ks][2][3] = l;
        }
    }
    f32x16 acc2[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc2[mt] = zero16();
    auto wld = [&](const uint16_t* base, u32x4 (&w)[3]) __attribute__((always_inline)) {      // base: plane 0 of one operand
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) w[pl] = *reinterpret_cast<const u32x4*>(base + (pl * 64 + lane) * 8);
    };
    // Every weight operand is requested ONE STEP AHEAD of the six MFMAs that use it (wq[0] / wq[1] alternate; a block has KS + 8 steps,
    // an even count, so every block starts on wq[0]): with one wave per SIMD at p >= 128 nobody else covers the L2 latency.
    u32x4 wq[2][3];
    wld(a.w1z, wq[0]);
    for (int blk = 0; blk < 16; ++blk) {
        const uint16_t* w1 = a.w1z + (long)blk * KS * 1536;
        const uint16_t* w2 = a.w2z + (long)blk * 8 * 1536;
        f32x16 acc1[2] = {zero16(), zero16()};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            wld(ks + 1 < KS ? w1 + (ks + 1) * 1536 : w2, wq[(ks + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            acc1[ks & 1] = mma6(wq[ks & 1], xp[ks], acc1[ks & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        u32x4 hp[2][3];
        act_split(acc1[0] + acc1[1], a.b1z + (blk * 2 + hg) * 16, hp);
        // the step after the block's last one: the next block's first layer-1 operand, or layer 3's first
        const uint16_t* nxt = blk < 15 ? w1 + KS * 1536 : a.w3z;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int i = s * 4 + mt;
                wld(i < 7 ? w2 + (i + 1) * 1536 : nxt, wq[(i + 1) & 1]);
                __builtin_amdgcn_sched_barrier(0);
                acc2[mt] = mma6(wq[i & 1], hp[s], acc2[mt]);
                __builtin_amdgcn_sched_barrier(0);
            }
    }
    // ---- layer 3: the 128 hidden units are four tiles = eight k-steps; C_out rows of one 32-row tile are live
    f32x16 acc3[2] = {zero16(), zero16()};
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        u32x4 hp[2][3];
        act_split(acc2[mt], a.b2z + (mt * 2 + hg) * 16, hp);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = mt * 2 + s;
            if (i < 7) wld(a.w3z + (i + 1) * 1536, wq[(i + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            acc3[s] = mma6(wq[i & 1], hp[s], acc3[s]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const f32x16 o = acc3[0] + acc3[1];
    if (n < a.N) {
        float* dst = a.out + (bi * a.N + n) * a.Cout;
#pragma unroll
        for (int r = 0; r < 8; ++r) {                           // rows 0..15 of the tile: C_out <= 16
            const int c = mfma_row(lane, r);
            if (c < a.Cout) dst[c] = o[r] + a.b3[c];
        }
    }
}

extern "C" int rpb_don_point_mlp(const float* t, const float* b, const void* w1z, const float* b1z, const void* w2z, const float* b2z,
                                 const void* w3z, const float* b3, float* out, int B, long N, int p, int Cout, void* stream) {
    RPB_REQUIRE(t && b && w1z && b1z && w2z && b2z && w3z && b3 && out && B > 0 && N > 0, "don_point_mlp: bad arguments");
    RPB_REQUIRE(p == 64 || p == 128 || p == 256, "don_point_mlp: p=%d unsupported (64, 128 or 256)", p);
    RPB_REQUIRE(Cout >= 1 && Cout <= 16, "don_point_mlp: C_out=%d unsupported (1..16)", Cout);
    RPB_REQUIRE(B <= 65535 && (N + 127) / 128 < (1L << 31), "don_point_mlp: B=%d N=%ld exceed the launch grid", B, N);
    PointArgs a{t, b, (const uint16_t*)w1z, (const uint16_t*)w2z, (const uint16_t*)w3z, b1z, b2z, b3, out, N, Cout};
    const dim3 grid((unsigned)((N + 127) / 128), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (p == 64) hipLaunchKernelGGL(don_point_kernel<64>, grid, dim3(256), 0, st, a);
    else if (p == 128) hipLaunchKernelGGL(don_point_kernel<128>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(don_point_kernel<256>, grid, dim3(256), 0, st, a);
    RPB_CHECK_LAUNCH("don_point_mlp");
}
