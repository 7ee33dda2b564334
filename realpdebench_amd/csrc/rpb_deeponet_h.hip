// DeepONet's output net on the opt-in "f16x2" eval arithmetic (DeepONet.set_arith("f16x2")).
//   rpb_don_point_mlp_f16x2   out[b][n][:] = W3 relu(W2 relu(W1 (b[b] (.) t[n]) + b1) + b2) + b3, the contract of rpb_don_point_mlp
//                             (csrc/rpb_deeponet.hip: p in {64, 128, 256}, C_out 1..16, any N, B <= 65535), on v_mfma_f32_32x32x16_f16
//                             from two fp16 planes per operand: three products per fp32 product instead of six.
// The organisation is rpb_don_point_mlp's: hidden units are MFMA rows, points are MFMA columns, a wave owns 32 points and a workgroup
// 128, the 512 hidden units are walked in 16 blocks of 32, an accumulator tile becomes the next layer's B operand in place through the
// unit bijection u(s, kg, e) = 8 (2 s + e / 4) + 4 kg + e % 4, the weight operands are requested ahead of use into a ring of register
// sets (three steps ahead into four sets here, one step into two there).  No LDS allocation, no atomics, no barrier, a fixed summation
// order: two calls give the same bits.
//
// What fp16 needs and the bf16 planes did not is a RANGE.  Every operand is multiplied by an exact power of two before it is split:
//   weights      W1, W2, W3 each by its own 2^ew, max|W| 2^ew in [2^14, 2^15) (point_weights_f16x2 of model/deeponet.py, the rule of
//                rpb_amax_exp); the kernel reads the factors 2^-ew from device memory (sc[0..2]).
//   activations  ONE EXPONENT PER POINT.  Points are MFMA columns, so a B operand may carry a scale per column and the column of the
//                accumulator is rescaled in the epilogue: relu(acc * 2^-(ew + e_point) + bias), one fma per value.
//     x = b (.) t  the exact maximum of the point's p values (a lane holds p / 2 of them, lane ^ 32 the rest: one exchange);
//     h1 (512)     is produced and consumed 32 units at a time and all 16 blocks accumulate into the same four tiles through the MFMA's
//                  C input, so the 16 blocks share one exponent, fixed before the first block: from the bound
//                  |h1_u| <= max_u ||W1_u||_1 max_k |x_k| + max|b1| (sc[3], sc[4]: weight-only constants, rounded up), scaled into
//                  [2^13, 2^14) -- one binade of headroom for the rounding of the bound and of the computed h1.  The bound cannot be
//                  exceeded, so no plane overflows; it is loose (an order of magnitude on random weights), which costs nothing: a pair
//                  of fp16 planes keeps an absolute error of 2^-25 on the scaled column, 2^-22 of the column maximum as long as that
//                  maximum is within 2^18 of the bound;
//     h2 (128)     is complete in the accumulators before layer 3 starts: the exact maximum over the lane's 64 values and one exchange.
//   An all-zero column takes e = 0.  Exponents are capped at 62 (a column maximum below 2^-48 is scaled by 2^62 only: still exact
//   planes, and still 2^-22 of the column maximum down to 2^-65), so that every factor 2^e, 2^-e stays a normal fp32 number.
// Products are accumulated small terms first: lo*hi, hi*lo, hi*hi; lo*lo (<= 2^-22 of the product) is dropped.
// Non-finite inputs (t, b, weights) are outside the contract: an exponent derived from Inf / NaN is meaningless and the output is then
// unspecified (finite or not), where the default kernel propagates them.
#include "rpb_mma.h"

// col_exp, pow2f and mma3h (operand a = the weights here) come from rpb_mma.h
// 8 values of one k-step, already scaled -> (hi, lo) fp16 planes as dwords
__device__ __forceinline__ void split_step(const float (&v)[8], u32x4 (&hp)[2]) {
    bf16x8 h, l;
    split8h<false>(v, h, l);
    hp[0] = __builtin_bit_cast(u32x4, h);
    hp[1] = __builtin_bit_cast(u32x4, l);
}
// v[r] = relu(acc[r] * c + bias[r]) of a D tile (bias in D-register order)
__device__ __forceinline__ void act16(const f32x16& acc, float c, const float* __restrict__ bias16, float (&v)[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 bq = *reinterpret_cast<const f32x4*>(bias16 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * q + e] = fmaxf(fmaf(acc[4 * q + e], c, bq[e]), 0.f);
    }
}
// the B-operand planes of the two k-steps of v * s
__device__ __forceinline__ void scale_split(const float (&v)[16], float s, u32x4 (&hp)[2][2]) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        float w[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[e] = v[8 * st + e] * s;
        split_step(w, hp[st]);
    }
}

struct PointHArgs {
    const float* t;         // [N][P]
    const float* b;         // [B][P]
    const uint16_t* w1z;    // [16 blocks][P / 16 k-steps][2 planes][64 lanes][8]: fp16 (hi, lo) of W1 2^ew1
    const uint16_t* w2z;    // [16 blocks][2 k-steps][4 tiles][2 planes][64 lanes][8]
    const uint16_t* w3z;    // [4 tiles of the 128 units][2 k-steps][2 planes][64 lanes][8], rows >= C_out zero
    const float* b1z;       // [16 blocks][2 hg][16]: bias in D-register order
    const float* b2z;       // [4 tiles][2 hg][16]
    const float* b3;        // [C_out]
    const float* sc;        // [5]: 2^-ew1, 2^-ew2, 2^-ew3, max_u ||W1_u||_1, max|b1| (the last two rounded up)
    float* out;             // [B][N][C_out]
    long N;
    int Cout;
};

// p <= 128 is built for two workgroups per CU = two waves per SIMD (the second wave's MFMAs run under this wave's epilogues and operand
// latency; 190 / 228 registers, no scratch; measured against the one-wave build in DESIGN.md section 16.2); p = 256 needs 334 registers.
template <int P>
__global__ __launch_bounds__(256, P <= 128 ? 2 : 1) void don_point_h_kernel(PointHArgs a) {
    constexpr int KS = P / 16;
    constexpr int OP = 2 * 64 * 8;                             // one operand: two planes of 64 lanes x 8
    const int lane = threadIdx.x & 63, pt = lane & 31, hg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long bi = blockIdx.y;
    const long n = (long)blockIdx.x * 128 + wave * 32 + pt;
    const long nc = n < a.N ? n : a.N - 1;                     // tail: a valid row is read, nothing is stored
    const float iw1 = a.sc[0], iw2 = a.sc[1], iw3 = a.sc[2], l1max = a.sc[3], b1max = a.sc[4];
    // ---- layer-1 B operand: (b (.) t) of my point, k = 16 ks + 8 hg + e, scaled by the point's 2^ex, two planes per k-step
    u32x4 xp[KS][2];
    float c1, c2, s1;                                          // epilogue factors of layers 1 and 2, the scale of h1
    {
        const float* trow = a.t + nc * P + 8 * hg;
        const float* brow = a.b + bi * P + 8 * hg;
        float xv[KS][8];
        float m = 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const f32x4 t0 = *reinterpret_cast<const f32x4*>(trow + 16 * ks), t1 = *reinterpret_cast<const f32x4*>(trow + 16 * ks + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(brow + 16 * ks), b1 = *reinterpret_cast<const f32x4*>(brow + 16 * ks + 4);
            const f32x4 v0 = t0 * b0, v1 = t1 * b1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                xv[ks][e] = v0[e];
                xv[ks][4 + e] = v1[e];
                m = fmaxf(m, fmaxf(fabsf(v0[e]), fabsf(v1[e])));
            }
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));                   // the other half of the point's p values
        const int ex = col_exp<14>(m);
        const int e1 = col_exp<13>(fmaf(l1max, m, b1max));     // |h1| <= l1max m + b1max: one binade of headroom
        const float sx = pow2f(ex);
        s1 = pow2f(e1);
        c1 = iw1 * pow2f(-ex);
        c2 = iw2 * pow2f(-e1);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            float w[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] = xv[ks][e] * sx;
            split_step(w, xp[ks]);
        }
    }
    f32x16 acc2[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc2[mt] = zero16();
    auto wld = [&](const uint16_t* base, u32x4 (&w)[2]) __attribute__((always_inline)) {      // base: plane 0 of one operand
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) w[pl] = *reinterpret_cast<const u32x4*>(base + (pl * 64 + lane) * 8);
    };
    // Every weight operand is requested AHEAD = 3 STEPS before the three MFMAs that use it, into a ring of four register sets (a step is
    // three MFMAs here, half the default kernel's six, so one step of lead covers half the latency it covers there; measured in
    // DESIGN.md section 16.2).  A block has KS + 8 steps, a multiple of four, so every block and layer 3 start on wq[0].
    constexpr int AHEAD = 3, SETS = AHEAD + 1, S = KS + 8;
    static_assert(S % SETS == 0 && AHEAD <= KS && AHEAD <= 8, "the ring must close at every block");
    u32x4 wq[SETS][2];
#pragma unroll
    for (int j = 0; j < AHEAD; ++j) wld(a.w1z + j * OP, wq[j]);
    for (int blk = 0; blk < 16; ++blk) {
        const uint16_t* w1 = a.w1z + (long)blk * KS * OP;
        const uint16_t* w2 = a.w2z + (long)blk * 8 * OP;
        const uint16_t* nxt = blk < 15 ? w1 + KS * OP : a.w3z;  // what follows the block: the next block's layer 1, or layer 3
        auto operand = [&](int j) __attribute__((always_inline)) {      // step j of this block; j >= S: the steps that follow it
            return j < KS ? w1 + j * OP : j < S ? w2 + (j - KS) * OP : nxt + (j - S) * OP;
        };
        f32x16 acc1[2] = {zero16(), zero16()};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            wld(operand(ks + AHEAD), wq[(ks + AHEAD) % SETS]);
            __builtin_amdgcn_sched_barrier(0);
            acc1[ks & 1] = mma3h(wq[ks % SETS], xp[ks], acc1[ks & 1]);
            __builtin_amdgcn_sched_barrier(0);
        }
        u32x4 hp[2][2];
        {
            float v[16];
            act16(acc1[0] + acc1[1], c1, a.b1z + (blk * 2 + hg) * 16, v);
            scale_split(v, s1, hp);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                const int j = KS + s * 4 + mt;
                wld(operand(j + AHEAD), wq[(j + AHEAD) % SETS]);
                __builtin_amdgcn_sched_barrier(0);
                acc2[mt] = mma3h(wq[j % SETS], hp[s], acc2[mt]);
                __builtin_amdgcn_sched_barrier(0);
            }
    }
    // ---- h2 = relu(acc2 2^-(ew2 + e1) + b2) in place, its exact column maximum, the point's 2^e2
    float m2 = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        float v[16];
        act16(acc2[mt], c2, a.b2z + (mt * 2 + hg) * 16, v);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc2[mt][r] = v[r];
            m2 = fmaxf(m2, v[r]);
        }
    }
    m2 = fmaxf(m2, __shfl_xor(m2, 32, 64));
    const int e2 = col_exp<14>(m2);
    const float s2 = pow2f(e2), c3 = iw3 * pow2f(-e2);
    // ---- layer 3: the 128 hidden units are four tiles = eight k-steps; C_out rows of one 32-row tile are live
    f32x16 acc3[2] = {zero16(), zero16()};
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        u32x4 hp[2][2];
        {
            float v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) v[r] = acc2[mt][r];
            scale_split(v, s2, hp);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int i = mt * 2 + s;
            if (i + AHEAD < 8) wld(a.w3z + (i + AHEAD) * OP, wq[(i + AHEAD) % SETS]);
            __builtin_amdgcn_sched_barrier(0);
            acc3[s] = mma3h(wq[i % SETS], hp[s], acc3[s]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    const f32x16 o = acc3[0] + acc3[1];
    if (n < a.N) {
        float* dst = a.out + (bi * a.N + n) * a.Cout;
#pragma unroll
        for (int r = 0; r < 8; ++r) {                           // rows 0..15 of the tile: C_out <= 16
            const int c = mfma_row(lane, r);
            if (c < a.Cout) dst[c] = fmaf(o[r], c3, a.b3[c]);
        }
    }
}

extern "C" int rpb_don_point_mlp_f16x2(const float* t, const float* b, const void* w1z, const float* b1z, const void* w2z, const float* b2z,
                                       const void* w3z, const float* b3, const float* sc, float* out, int B, long N, int p, int Cout,
                                       void* stream) {
    RPB_REQUIRE(t && b && w1z && b1z && w2z && b2z && w3z && b3 && sc && out && B > 0 && N > 0, "don_point_mlp_f16x2: bad arguments");
    RPB_REQUIRE(p == 64 || p == 128 || p == 256, "don_point_mlp_f16x2: p=%d unsupported (64, 128 or 256)", p);
    RPB_REQUIRE(Cout >= 1 && Cout <= 16, "don_point_mlp_f16x2: C_out=%d unsupported (1..16)", Cout);
    RPB_REQUIRE(B <= 65535 && (N + 127) / 128 < (1L << 31), "don_point_mlp_f16x2: B=%d N=%ld exceed the launch grid", B, N);
    PointHArgs a{t, b, (const uint16_t*)w1z, (const uint16_t*)w2z, (const uint16_t*)w3z, b1z, b2z, b3, sc, out, N, Cout};
    const dim3 grid((unsigned)((N + 127) / 128), (unsigned)B);
    hipStream_t st = (hipStream_t)stream;
    if (p == 64) hipLaunchKernelGGL(don_point_h_kernel<64>, grid, dim3(256), 0, st, a);
    else if (p == 128) hipLaunchKernelGGL(don_point_h_kernel<128>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(don_point_h_kernel<256>, grid, dim3(256), 0, st, a);
    RPB_CHECK_LAUNCH("don_point_mlp_f16x2");
}
