// The AFNO block MLP of DPOT on the opt-in "f16x2" eval arithmetic (DPOT.set_arith("f16x2")): the two-fp16-plane
// twin of afno_mlp_kernel's forward mode 0 without `mid` (csrc/rpb_dpot.hip),
//     out = gelu(X Wa + ba) Wb + bb      per (32-token tile, block k),  X, out: [ntok][2][C] rows, the block's slice = columns
//                                        [k bs, + bs) of both halves, K = 2 bs real columns (re | im)
// on v_mfma_f32_32x32x16_f16 with three products per k-step (mma3h of rpb_mma.h: lo*hi, hi*lo, hi*hi; lo*lo <= 2^-22 of the product is
// dropped) where the default kernel issues eight 32x32x2 fp32 MFMAs per 16 columns.
//
// Scales (fp16 has five exponent bits), all exact powers of two formed on the device, no host read:
//   weights   ONE exponent per weight tensor (w1, w2) by rpb_amax_exp's rule, max|w| 2^ew in [2^14, 2^15), capped at 62.  The real
//             composite Wc[(ri, i)][(ro, o)] (re -> re = wr, im -> re = -wi, re -> im = wi, im -> im = wr) holds the same magnitudes, so the
//             exponent of w is the composite's.  rpb_afno_wprep_f16x2 writes the composites of all blocks as (hi, lo) planes in B-operand
//             order, Wz[nb][K / 16][2 planes][K / 32][64 lanes][8], and sc[0] = 2^-ew (sc[1] is its scratch word).
//   X         one exponent per (token, block) from the EXACT maximum of the token's resident 2 bs values (col_exp<14>): spectral tokens
//             span many binades between DC and the high modes, and blocks of one token differ as well.
//   hidden    one exponent per (token, block) from the exact maximum of the 2 bs hidden values AFTER GELU.  The hidden tile lives in LDS
//             (fp32, then as planes) and never reaches HBM.
// A zero token takes exponent 0: its hidden layer is gelu(ba) and its output the second layer of that, as in the default kernel.
//
// One workgroup = (32-token tile, block); wave w owns output columns [32 w, 32 w + 32) of both layers (K / 32 waves: 6 at bs = 96, 8 at
// bs = 128).  LDS: the fp32 tile [32][K + 4] (X, then the hidden layer) and its planes [2][K / 8][34] x 16 B: 69 KB at bs = 128, two
// workgroups per CU.  Fixed summation order, no atomics: two calls give equal bits.  Rows >= ntok are staged as zeros and store nothing;
// nothing is written outside the block's columns of out[tok], tok < ntok.  Non-finite inputs are outside the contract.
#include "rpb_mma.h"

extern "C" int rpb_amax_exp(const float* x, long M, int C, int ldx, int* e, void* stream);

#define AFH_RS 34          // 16-byte units per 8-column group of a plane: 32 token rows + 2

// ---------------------------------------------------------------------------------- weights: composite, scaled, split, operand order
// one thread = one (block, k-step, 32-column tile, lane): 8 consecutive kk of output column n; sc[1] holds rpb_amax_exp's exponent on entry
__global__ __launch_bounds__(256) void afno_wprep_h_kernel(const float* __restrict__ w, uint16_t* __restrict__ Wz, float* sc, int nb, int bs) {
    const int K = 2 * bs, NT = K >> 5, NCC = K >> 4;
    const long total = (long)nb * NCC * NT * 64;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int ew = reinterpret_cast<const int*>(sc)[1];
    ew = ew > 62 ? 62 : ew;
    if (idx == 0) sc[0] = pow2f(-ew);
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    long r = idx >> 6;
    const int nt = (int)(r % NT);
    r /= NT;
    const int cc = (int)(r % NCC), k = (int)(r / NCC);
    const int n = nt * 32 + (lane & 31), ro = n / bs, o = n % bs;
    const float s = pow2f(ew);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int kk = cc * 16 + (lane >> 5) * 8 + e, ri = kk / bs, i = kk % bs;
        const float wr = w[(((long)0 * nb + k) * bs + i) * bs + o], wi = w[(((long)1 * nb + k) * bs + i) * bs + o];
        v[e] = ((ri == ro) ? wr : (ri == 1 ? -wi : wi)) * s;
    }
    bf16x8 h, l;
    split8h<false>(v, h, l);
    const long dst = (((((long)k * NCC + cc) * 2) * NT + nt) * 64 + lane) * 8;
    *reinterpret_cast<u32x4*>(Wz + dst) = __builtin_bit_cast(u32x4, h);
    *reinterpret_cast<u32x4*>(Wz + dst + (long)NT * 512) = __builtin_bit_cast(u32x4, l);
}

struct AfnoHArgs {
    const float* X;
    const uint16_t* Waz;
    const float* sca;
    const float* ba;
    const uint16_t* Wbz;
    const float* scb;
    const float* bb;
    float* out;
    long ntok;
    int nb, bs, C;
};

__global__ __launch_bounds__(512) void afno_mlp_h_kernel(AfnoHArgs a) {
    extern __shared__ u32x4 lds4[];
    const int bs = a.bs, K = 2 * bs, LD = K + 4, NT = K >> 5, nks = K >> 4, nk8 = K >> 3;
    float* const Xs = reinterpret_cast<float*>(lds4);                  // [32][LD] fp32: X, then the hidden layer
    u32x4* const P0 = lds4 + 8 * LD;                                   // [K / 8][AFH_RS] hi plane
    u32x4* const P1 = P0 + nk8 * AFH_RS;                               //                 lo plane
    float* const fac = reinterpret_cast<float*>(P1 + nk8 * AFH_RS);    // [32] 2^-e of the token, [32] 2^e
    const int k = blockIdx.y;
    const long tok0 = (long)blockIdx.x * 32;
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = blockDim.x >> 6;
    const long rowld = 2L * a.C;
    // ---- stage the token tile: Xs[m][ri bs + i] = X[tok0 + m][ri][k bs + i]; rows past the end are zeros
    for (int idx = tid; idx < 32 * K; idx += blockDim.x) {
        const int m = idx / K, kk = idx % K;
        const int ri = kk / bs, i = kk % bs;
        const long tok = tok0 + m;
        Xs[m * LD + kk] = tok < a.ntok ? a.X[tok * rowld + (long)ri * a.C + k * bs + i] : 0.f;
    }
    // the exact maximum of each token's K values -> its exponent; the tile as scaled (hi, lo) planes in A-operand order
    auto to_planes = [&]() __attribute__((always_inline)) {
        __syncthreads();
        for (int m = wave; m < 32; m += nwaves) {
            float mx = 0.f;
            for (int c = lane; c < K; c += 64) mx = fmaxf(mx, fabsf(Xs[m * LD + c]));
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) mx = fmaxf(mx, __shfl_xor(mx, d, 64));
            if (lane == 0) {
                const int ex = col_exp<14>(mx);
                fac[m] = pow2f(-ex);
                fac[32 + m] = pow2f(ex);
            }
        }
        __syncthreads();
        for (int idx = tid; idx < 32 * nk8; idx += blockDim.x) {
            const int m = idx & 31, g = idx >> 5;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(Xs + m * LD + 8 * g), v1 = *reinterpret_cast<const f32x4*>(Xs + m * LD + 8 * g + 4);
            const float s = fac[32 + m];
            float v[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = v0[e] * s;
                v[4 + e] = v1[e] * s;
            }
            bf16x8 h, l;
            split8h<false>(v, h, l);
            P0[g * AFH_RS + m] = __builtin_bit_cast(u32x4, h);
            P1[g * AFH_RS + m] = __builtin_bit_cast(u32x4, l);
        }
        __syncthreads();
    };
    // one layer's 32 x 32 tile of this wave: A from the planes, B from the block's operand-ordered weight planes
    auto layer = [&](const uint16_t* Wz) __attribute__((always_inline)) {
        const uint16_t* wb = Wz + ((((long)k * nks) * 2 * NT + wave) * 64 + lane) * 8;
        const long wplane = (long)NT * 512;
        f32x16 acc = zero16();
        for (int ks = 0; ks < nks; ++ks) {
            const int o = (2 * ks + half) * AFH_RS + col;
            const u32x4 av[2] = {P0[o], P1[o]};
            const uint16_t* s = wb + (long)ks * 2 * wplane;
            const u32x4 bv[2] = {*reinterpret_cast<const u32x4*>(s), *reinterpret_cast<const u32x4*>(s + wplane)};
            acc = mma3h(av, bv, acc);
        }
        return acc;
    };
    const int n = wave * 32 + col;
    const int ro = n / bs, oo = n % bs;                                // this lane's output column -> (re / im half, channel in block)
    // ---- layer A, GELU; the hidden tile replaces X in LDS
    to_planes();
    f32x16 acc = layer(a.Waz);
    {
        const float wsc = a.sca[0];
        const float bav = a.ba ? a.ba[(long)ro * a.C + k * bs + oo] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mfma_row(lane, r);
            Xs[m * LD + n] = gelu_f(fmaf(acc[r], fac[m] * wsc, bav));  // X's fp32 tile was last read before to_planes' final barrier
        }
    }
    // ---- layer B (to_planes starts with a barrier: every wave has left layer A's main loop before the planes are rewritten)
    to_planes();
    acc = layer(a.Wbz);
    {
        const float wsc = a.scb[0];
        const float bbv = a.bb ? a.bb[(long)ro * a.C + k * bs + oo] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = mfma_row(lane, r);
            const long tok = tok0 + m;
            if (tok < a.ntok) a.out[tok * rowld + (long)ro * a.C + k * bs + oo] = fmaf(acc[r], fac[m] * wsc, bbv);
        }
    }
}

extern "C" int rpb_afno_mlp_f16x2_supported(int nb, int bs) { return nb > 0 && bs >= 16 && bs % 16 == 0 && bs <= 128; }

extern "C" int rpb_afno_wprep_f16x2(const float* w, void* Wz, float* sc, int nb, int bs, void* stream) {
    RPB_REQUIRE(w && Wz && sc && rpb_afno_mlp_f16x2_supported(nb, bs), "afno_wprep_f16x2: nb=%d bs=%d unsupported (bs %% 16, bs <= 128)", nb, bs);
    const int rc = rpb_amax_exp(w, (long)2 * nb * bs, bs, bs, reinterpret_cast<int*>(sc) + 1, stream);
    if (rc != RPB_OK) return rc;
    const long total = (long)nb * (2 * bs / 16) * (2 * bs / 32) * 64;
    hipLaunchKernelGGL(afno_wprep_h_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, (uint16_t*)Wz, sc, nb, bs);
    RPB_CHECK_LAUNCH("afno_wprep_f16x2");
}

extern "C" int rpb_afno_mlp_f16x2(const float* X, const void* Waz, const float* sca, const float* ba, const void* Wbz, const float* scb,
                                  const float* bb, float* out, long ntok, int nb, int bs, void* stream) {
    RPB_REQUIRE(X && Waz && sca && Wbz && scb && out && ntok > 0, "afno_mlp_f16x2: bad arguments");
    RPB_REQUIRE(rpb_afno_mlp_f16x2_supported(nb, bs), "afno_mlp_f16x2: nb=%d bs=%d unsupported (bs %% 16, bs <= 128)", nb, bs);
    const int K = 2 * bs, waves = K / 32;
    const size_t lds = (size_t)32 * (K + 4) * 4 + (size_t)2 * (K / 8) * AFH_RS * 16 + 64 * sizeof(float);
    if (hipFuncSetAttribute((const void*)afno_mlp_h_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        RPB_FAIL(RPB_ERR_LAUNCH, "afno_mlp_f16x2: %zu bytes of LDS refused", lds);
    const AfnoHArgs a{X, (const uint16_t*)Waz, sca, ba, (const uint16_t*)Wbz, scb, bb, out, ntok, nb, bs, nb * bs};
    hipLaunchKernelGGL(afno_mlp_h_kernel, dim3((unsigned)((ntok + 31) / 32), nb), dim3(waves * 64), lds, (hipStream_t)stream, a);
    RPB_CHECK_LAUNCH("afno_mlp_f16x2");
}
