// CNO3d (realpdebench/model/cno.py with activation = 'LeakyReLU'): every layer is Conv3d(3, padding=1) followed by an eval BatchNorm,
// LeakyReLU(0.2), a residual add or a channel concat, all at full resolution.  rpb_cno_conv3x is the implicit GEMM of conv3x_kernel
// (csrc/rpb_conv3x.hip: same plane input P[3][M][Ci], same rpb_conv3x_wprep weights, same tiling, same six bf16 products per fp32
// product, same accumulation order) with the CNO epilogue
//     v = acc * sc[n] + sh[n];  if (act) v = v > 0 ? v : 0.2 v;  if (res) v += res[m][n]
// and two optional outputs of the first nvalid channels: fp32 rows out[m * ldo + n] and the three bf16 planes of v at
// out_planes[pl * M * ldp + m * ldp + n] -- bit-equal to rpb_split3 of the fp32 v.  Both pointers arrive at the first column the launch
// owns: two producers write disjoint column ranges of one plane buffer and the next convolution reads it directly, so neither a
// torch.cat nor an rpb_split3 pass exists in the model.  rpb_cno_pack writes the first layer's planes from the raw input.
// `res` may alias `out` element for element (same address, ldr == ldo): the lane that reads res[m][n] is the one that writes out[m][n]
// afterwards and no other lane touches that element -- the training step accumulates data gradients into one buffer that way.
// The kernel is a second text next to conv3x_kernel on purpose (csrc/rpb_conv3h.hip:14-18 records what one shared body did to the
// register counts); the main loop below is conv3x_kernel's, statement for statement.
#include "rpb_mma.h"
#include <stdlib.h>

template <int V>
struct ICn {
    static constexpr int value = V;
};

#define CN_BM 128
#define CN_ROWS (CN_BM + 2)

// the split of rpb_split3 (csrc/rpb_conv3x.hip): round to nearest even at every level, hi + mid + lo == x exactly
__device__ __forceinline__ unsigned cno_bf16_rne(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ void cno_split3(float x, unsigned& h, unsigned& m, unsigned& l) {
    h = cno_bf16_rne(x);
    const float r1 = x - __builtin_bit_cast(float, h << 16);          // exact
    m = cno_bf16_rne(r1);
    const float r2 = r1 - __builtin_bit_cast(float, m << 16);         // exact
    l = cno_bf16_rne(r2);
}

// ---------------------------------------------------------------------------------- the first layer's planes
// x [M][Cin] fp32 (1 <= Cin <= 64) -> P[3][M][64] bf16 with columns Cin..63 zero; one thread = 8 channels
__global__ __launch_bounds__(256) void cno_pack_kernel(const float* __restrict__ x, uint16_t* __restrict__ P, long M, int Cin) {
    const long total = M * 8;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long m = idx >> 3;
        const int c0 = (int)(idx & 7) * 8;
        unsigned h[8], md[8], lo[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float v = c0 + i < Cin ? x[m * Cin + c0 + i] : 0.f;
            cno_split3(v, h[i], md[i], lo[i]);
        }
        u32x4 oh, om, ol;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            oh[q] = h[2 * q] | (h[2 * q + 1] << 16);
            om[q] = md[2 * q] | (md[2 * q + 1] << 16);
            ol[q] = lo[2 * q] | (lo[2 * q + 1] << 16);
        }
        const long o = m * 64 + c0;
        *reinterpret_cast<u32x4*>(P + o) = oh;
        *reinterpret_cast<u32x4*>(P + M * 64 + o) = om;
        *reinterpret_cast<u32x4*>(P + 2 * M * 64 + o) = ol;
    }
}

extern "C" int rpb_cno_pack(const float* x, void* planes, long M, int Cin, void* stream) {
    RPB_REQUIRE(x && planes && M > 0 && M < (1L << 31) && Cin >= 1 && Cin <= 64 && (uintptr_t)planes % 16 == 0,
                "cno_pack: bad arguments (M=%ld Cin=%d; 1 <= Cin <= 64, planes 16-byte aligned)", M, Cin);
    long grid = (M * 8 + 255) / 256;
    const long cap = (long)rpb_num_cus() * 16;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(cno_pack_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, (uint16_t*)planes, M, Cin);
    RPB_CHECK_LAUNCH("cno_pack");
}

// ---------------------------------------------------------------------------------- the convolution
struct CnoArgs {
    const uint16_t* P;     // [3][M][Ci] bf16 planes of the input tokens
    const uint16_t* Wz;    // B-operand order (rpb_conv3x_wprep)
    const float* sc;       // [N] folded BatchNorm scale (1 without BatchNorm, 0 on pad channels)
    const float* sh;       // [N] folded shift (bias without BatchNorm, 0 on pad channels)
    const float* res;      // [M][ldr] residual added after the activation step, or null
    float* out;            // [M][ldo], already at the first column this launch owns, or null
    uint16_t* op;          // [3][M][ldp] bf16 planes of the result, already at the first column, or null
    long M;
    int N, Ci, nvalid, act, ldr, ldo, ldp, T, H, W;
};

template <int WN>
__global__ __launch_bounds__(256, 1) void cno_conv3x_kernel(CnoArgs a) {
    constexpr int KS = 4 / WN;
    extern __shared__ u32x4 lds4[];
    // two stage buffers of [3 planes][4 chunks][2 halves][CN_ROWS] x 16 B, then [9][CN_ROWS] row validity per (kt, kh)
    unsigned char* rv = reinterpret_cast<unsigned char*>(lds4 + 2 * 24 * CN_ROWS);
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nw = wave % WN, kp = wave / WN;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so XCD x walks the
    // contiguous tile range [x * chunk, (x + 1) * chunk): the h +- 1 rows a tile stages are its neighbours' own rows and hit L2
    const unsigned chunk = gridDim.x >> 3;
    const long tile = (long)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    const long m0 = tile * CN_BM;
    if (m0 >= a.M) return;
    const int n0 = blockIdx.y * (64 * WN) + nw * 64;
    const int NT = a.N >> 5, NCC = a.Ci >> 4;
    const unsigned uT = a.T, uH = a.H, uW = a.W;

    for (int idx = tid; idx < 9 * CN_ROWS; idx += 256) {
        const int g = idx / CN_ROWS, j = idx - g * CN_ROWS;
        const int kt = g / 3, kh = g - kt * 3;
        const long q = m0 - 1 + j + ((long)(kt - 1) * a.H + (kh - 1)) * a.W;
        bool ok = q >= 0 && q < a.M;
        if (ok) {
            const unsigned uq = (unsigned)q, r = uq / uW;
            const int hq = (int)(r % uH), tq = (int)((r / uH) % uT);
            const int tt = tq - kt + 1, hh = hq - kh + 1;
            ok = tt >= 0 && tt < a.T && hh >= 0 && hh < a.H;
        }
        rv[idx] = ok ? 1 : 0;
    }
    bool wlo[4], whi[4];                                                // my output tokens at the w boundaries
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
        const unsigned w = (unsigned)(m0 + tm * 32 + col) % uW;
        wlo[tm] = (w == 0);
        whi[tm] = (w == uW - 1);
    }
    f32x16 acc[4][2];
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) acc[tm][0] = acc[tm][1] = zero16();
    const u32x4 z4 = {0u, 0u, 0u, 0u};
    const long MC = a.M * a.Ci;

    // One workgroup per CU, one wave per SIMD with the whole 512-register file, everything software-pipelined by hand:
    //   * the next stage's 13 A loads per thread are issued (unconditionally: invalid rows read a dummy address and are zeroed on
    //     the way into LDS) before the current stage's MFMAs and land in the other LDS buffer afterwards -- one barrier per stage;
    //   * the B operands of the NEXT tap step (kw, then the next 16-channel chunk / stage) are requested before the 48 MFMAs of
    //     the current one (left to itself the compiler put every load next to its use: an L2 latency per tap, 57 % MFMA busy).
    constexpr int SPS = 4 / KS;                                        // my 16-channel chunks per stage
    const int nc64 = a.Ci >> 6;
    const uint16_t* wbase = a.Wz + ((long)(n0 >> 5) * 64 + lane) * 8;
    const long wplane = (long)NT * 512;                                // bf16 elements between the planes of one (tap, chunk)
    const long wchunk = 3 * wplane, wtap = (long)NCC * wchunk;
    auto bload = [&](const uint16_t* src, u32x4 (&b)[2][3]) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) b[tn][p] = *reinterpret_cast<const u32x4*>(src + p * wplane + tn * 512);
    };
    u32x4 bc[2][3], bn[2][3];
    const u32x4* As = lds4;
    u32x4 ac[3], an[3];                                                 // A operands of the current / next 32-token row tile
    auto lda = [&](int s, int kw, int tm, u32x4 (&av)[3]) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 3; ++p) av[p] = As[((p * 4 + s) * 2 + half) * CN_ROWS + tm * 32 + col + kw];
    };
    // one tap step = 4 row tiles x 12 MFMAs; the next tile's A operands (the next step's first tile when `more`) are read from
    // LDS before the current tile's MFMAs are issued -- with one wave per SIMD nobody else hides that latency
    // (the A tiles ping-pong between ac and an -- four tiles per step, so every step starts on ac -- and the B sets between bc and
    // bn by step parity: no register copies)
    auto mfma12 = [&](int tm, int kw, u32x4 (&av)[3], const u32x4 (&b)[2][3]) __attribute__((always_inline)) {
        if ((kw == 0 && wlo[tm]) || (kw == 2 && whi[tm])) av[0] = av[1] = av[2] = z4;
        const bf16x8 ah = __builtin_bit_cast(bf16x8, av[0]), am = __builtin_bit_cast(bf16x8, av[1]),
                     al = __builtin_bit_cast(bf16x8, av[2]);
        const bf16x8 b0h = __builtin_bit_cast(bf16x8, b[0][0]), b0m = __builtin_bit_cast(bf16x8, b[0][1]),
                     b0l = __builtin_bit_cast(bf16x8, b[0][2]), b1h = __builtin_bit_cast(bf16x8, b[1][0]),
                     b1m = __builtin_bit_cast(bf16x8, b[1][1]), b1l = __builtin_bit_cast(bf16x8, b[1][2]);
        // small terms first; the two co tiles alternate so consecutive MFMAs are independent
        acc[tm][0] = mfma32b(al, b0h, acc[tm][0]);
        acc[tm][1] = mfma32b(al, b1h, acc[tm][1]);
        acc[tm][0] = mfma32b(ah, b0l, acc[tm][0]);
        acc[tm][1] = mfma32b(ah, b1l, acc[tm][1]);
        acc[tm][0] = mfma32b(am, b0m, acc[tm][0]);
        acc[tm][1] = mfma32b(am, b1m, acc[tm][1]);
        acc[tm][0] = mfma32b(am, b0h, acc[tm][0]);
        acc[tm][1] = mfma32b(am, b1h, acc[tm][1]);
        acc[tm][0] = mfma32b(ah, b0m, acc[tm][0]);
        acc[tm][1] = mfma32b(ah, b1m, acc[tm][1]);
        acc[tm][0] = mfma32b(ah, b0h, acc[tm][0]);
        acc[tm][1] = mfma32b(ah, b1h, acc[tm][1]);
    };
    auto tap_step = [&](int s, int kw, bool more, const u32x4 (&b)[2][3]) __attribute__((always_inline)) {   // kw: compile-time constant
        lda(s, kw, 1, an);
        __builtin_amdgcn_sched_barrier(0);
        mfma12(0, kw, ac, b);
        __builtin_amdgcn_sched_barrier(0);
        lda(s, kw, 2, ac);
        __builtin_amdgcn_sched_barrier(0);
        mfma12(1, kw, an, b);
        __builtin_amdgcn_sched_barrier(0);
        lda(s, kw, 3, an);
        __builtin_amdgcn_sched_barrier(0);
        mfma12(2, kw, ac, b);
        __builtin_amdgcn_sched_barrier(0);
        if (more) lda(kw == 2 ? s + KS : s, kw == 2 ? 0 : kw + 1, 0, ac);
        __builtin_amdgcn_sched_barrier(0);
        mfma12(3, kw, an, b);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto bsel = [&](auto pc) -> u32x4(&)[2][3] {
        if constexpr (decltype(pc)::value) return bn;
        else return bc;
    };
    // A staging registers: 13 x 16 B per thread, named individually (as an array indexed from helper lambdas they were demoted to
    // scratch memory: load, wait, spill -- one exposed HBM latency per load)
    constexpr int NLD = (CN_ROWS * 24 + 255) / 256;
    static_assert(NLD == 13, "staging macros below are written for 13 loads per thread");
#define CN_FOR13(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
#define CN_DECL(J) u32x4 sv##J = z4; bool ok##J = false;
    CN_FOR13(CN_DECL)
#define CN_LOAD(J)                                                                                            \
    if constexpr (J >= j0 && J < j1) {                                                                        \
        const int idx = tid + J * 256;                                                                        \
        const int row = idx / 24, rem = idx - row * 24;                                                       \
        const int p = rem >> 3, sh = rem & 7; /* sh = 2 * chunk + half: 8 x 16 B = one 128 B line */          \
        ok##J = idx < CN_ROWS * 24 && rv[g * CN_ROWS + (row < CN_ROWS ? row : 0)];                            \
        const long off = ok##J ? (long)p * MC + (rowbase + row) * a.Ci + c * 64 + sh * 8 : 0;                 \
        sv##J = *reinterpret_cast<const u32x4*>(a.P + off);                                                   \
    }
#define CN_STORE(J)                                                                                           \
    {                                                                                                         \
        const int idx = tid + J * 256;                                                                        \
        const int row = idx / 24, rem = idx - row * 24;                                                       \
        if (idx < CN_ROWS * 24) dst[rem * CN_ROWS + row] = ok##J ? sv##J : z4;                                \
    }
    // loads j0 <= j < j1 of the 13 a thread contributes to stage (g, c)
    auto stage_load = [&](int g, int c, auto j0c, auto j1c) __attribute__((always_inline)) {
        constexpr int j0 = decltype(j0c)::value, j1 = decltype(j1c)::value;
        const int kt = g / 3, kh = g - kt * 3;
        const long rowbase = m0 - 1 + ((long)(kt - 1) * a.H + (kh - 1)) * a.W;
        CN_FOR13(CN_LOAD)
    };
    auto stage_store = [&](u32x4* dst) __attribute__((always_inline)) { CN_FOR13(CN_STORE) };
    bload(wbase + (long)kp * wchunk, bc);                               // (g 0, c 0, s = kp, kw 0)
    stage_load(0, 0, ICn<0>{}, ICn<NLD>{});
    stage_store(lds4);
    __syncthreads();
    int buf = 0;
    constexpr int NST = 3 * SPS;                                        // tap steps per stage
    for (int g = 0; g < 9; ++g) {
        for (int c = 0; c < nc64; ++c) {
            int gn = g, cn = c + 1;                                     // next stage
            if (cn == nc64) {
                cn = 0;
                ++gn;
            }
            const bool more = gn < 9;
            As = lds4 + buf * 24 * CN_ROWS;
            lda(kp, 0, 0, ac);
            // the next stage's A loads are spread over this stage's tap steps (13 MB at once from every CU of the chip in
            // lock-step is a burst that the in-order vmcnt of the next B operands would have to wait out)
#define CN_SI_BLOCK(SI)                                                                                        \
    if constexpr (SI < SPS) {                                                                                  \
        const int s = kp + SI * KS;                                                                            \
        const uint16_t* w0 = wbase + (long)(g * 3) * wtap + (long)(c * 4 + s) * wchunk;                        \
        bload(w0 + wtap, bsel(ICn<(SI * 3 + 1) & 1>{}));                                                        \
        if (more) stage_load(gn, cn, ICn<(SI * 3 + 0) * NLD / NST>{}, ICn<(SI * 3 + 1) * NLD / NST>{});          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        tap_step(s, 0, true, bsel(ICn<(SI * 3 + 0) & 1>{}));                                                    \
        bload(w0 + 2 * wtap, bsel(ICn<(SI * 3 + 2) & 1>{}));                                                    \
        if (more) stage_load(gn, cn, ICn<(SI * 3 + 1) * NLD / NST>{}, ICn<(SI * 3 + 2) * NLD / NST>{});          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        tap_step(s, 1, true, bsel(ICn<(SI * 3 + 1) & 1>{}));                                                    \
        /* the step after (s, kw 2): next chunk of this stage, else the next stage's first chunk */            \
        if (SI + 1 < SPS) bload(w0 + (long)KS * wchunk, bsel(ICn<(SI * 3 + 3) & 1>{}));                         \
        else if (more) bload(wbase + (long)(gn * 3) * wtap + (long)(cn * 4 + kp) * wchunk, bsel(ICn<(SI * 3 + 3) & 1>{})); \
        if (more) stage_load(gn, cn, ICn<(SI * 3 + 2) * NLD / NST>{}, ICn<(SI * 3 + 3) * NLD / NST>{});          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        tap_step(s, 2, SI + 1 < SPS, bsel(ICn<(SI * 3 + 2) & 1>{}));                                            \
    }
            CN_SI_BLOCK(0) CN_SI_BLOCK(1) CN_SI_BLOCK(2) CN_SI_BLOCK(3)
            if constexpr (NST & 1) {                                    // odd step count (N = 64): the next stage's first B set is in bn
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int p = 0; p < 3; ++p) bc[tn][p] = bn[tn][p];
            }
            if (more) stage_store(lds4 + (buf ^ 1) * 24 * CN_ROWS);
            __syncthreads();                                            // everyone is done with buf and has filled buf ^ 1
            buf ^= 1;
        }
    }
#undef CN_SI_BLOCK
#undef CN_STORE
#undef CN_LOAD
#undef CN_DECL
#undef CN_FOR13
    // ---- K-split partial sums through LDS in ONE round: the KS waves of a column group own the four 32-token row tiles round-robin
    // (tile tm belongs to wave tm % KS); every wave parks its partials of the tiles it does not own, one barrier, every wave sums
    // and stores its own tiles.  (A first version let the kp == 0 waves reduce and store all four tiles, one tile and two
    // barriers at a time: measured 38 k of the 116 k cycles of a Ci = 64, N = 64 workgroup.)
    float* red = reinterpret_cast<float*>(lds4);                        // [WN][4 tiles][KS - 1 sources][2 col tiles][16 regs][64 lanes]
    {
        __syncthreads();                                                // the last stage's LDS reads are done
#pragma unroll
        for (int tm = 0; tm < 4; ++tm) {
            const int owner = tm % KS;
            if (kp != owner) {
                const int rank = kp < owner ? kp : kp - 1;
                float* slot = red + ((nw * 4 + tm) * (KS - 1) + rank) * 2048;
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int r = 0; r < 16; ++r) slot[(tn * 16 + r) * 64 + lane] = acc[tm][tn][r];
            }
        }
        __syncthreads();
    }
    // ---- the CNO epilogue on the tiles this wave owns.  The owner's first K-split slot (8 KB = 32 tokens x 64 channels of fp32, read by
    // nobody else) is free once its partials are summed: the result goes through it so that a lane leaves with 8 consecutive channels
    // of one token -- 16 B per plane -- instead of one channel of 16 tokens (2-byte stores 2 * ldp apart).
    static_assert(KS > 1, "the plane transpose reuses the owner's first K-split slot");
#pragma unroll
    for (int tm = 0; tm < 4; ++tm) {
        if (kp != tm % KS) continue;
        float* slot0 = red + ((nw * 4 + tm) * (KS - 1)) * 2048;
#pragma unroll
        for (int k2 = 0; k2 < KS - 1; ++k2) {
            const float* slot = slot0 + k2 * 2048;
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[tm][tn][r] += slot[(tn * 16 + r) * 64 + lane];
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int n = n0 + tn * 32 + col;
            const bool nok = n < a.nvalid;
            const float sc = a.sc[n], sh = a.sh[n];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long m = m0 + tm * 32 + mfma_row(lane, r);
                const bool ok = nok && m < a.M;
                float v = __builtin_fmaf(acc[tm][tn][r], sc, sh);
                if (a.act) v = v > 0.f ? v : 0.2f * v;
                if (a.res && ok) v += a.res[m * a.ldr + n];
                if (a.out && ok) a.out[m * a.ldo + n] = v;
                acc[tm][tn][r] = v;
            }
        }
        if (a.op) {
            // [32 tokens][64 channels]; tokens 4 apart (the two lane halves of one store) go to opposite bank halves
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mfma_row(lane, r);
                    slot0[row * 64 + ((tn * 32 + col) ^ ((row & 4) << 3))] = acc[tm][tn][r];
                }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");      // the slot is this wave's own: no workgroup barrier
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = j * 8 + (lane >> 3), c8 = (lane & 7) * 8;
                const float* src = slot0 + row * 64 + (c8 ^ ((row & 4) << 3));
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
                unsigned h[8], md[8], lo[8];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    cno_split3(v0[i], h[i], md[i], lo[i]);
                    cno_split3(v1[i], h[4 + i], md[4 + i], lo[4 + i]);
                }
                u32x4 oh, om, ol;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    oh[q] = h[2 * q] | (h[2 * q + 1] << 16);
                    om[q] = md[2 * q] | (md[2 * q + 1] << 16);
                    ol[q] = lo[2 * q] | (lo[2 * q + 1] << 16);
                }
                const long m = m0 + tm * 32 + row;
                const int n = n0 + c8;
                if (m < a.M && n < a.nvalid) {                          // nvalid % 8 == 0 here: a run of 8 is inside or outside
                    uint16_t* dst = a.op + m * a.ldp + n;
                    const long pstride = a.M * (long)a.ldp;
                    *reinterpret_cast<u32x4*>(dst) = oh;
                    *reinterpret_cast<u32x4*>(dst + pstride) = om;
                    *reinterpret_cast<u32x4*>(dst + 2 * pstride) = ol;
                }
            }
            __builtin_amdgcn_wave_barrier();                            // (WN = 2: the next owned tile has its own slot)
        }
    }
}

extern "C" int rpb_cno_conv3x(const void* planes, const void* Wz, const float* sc, const float* sh, const float* res, float* out,
                              void* out_planes, long M, int N, int Ci, int nvalid, int act, int ldr, int ldo, int ldp, int Hc, int Wc,
                              int Dc, void* stream) {
    RPB_REQUIRE(planes && Wz && sc && sh && (out || out_planes) && M > 0 && M < (1L << 31), "cno_conv3x: bad arguments");
    RPB_REQUIRE(Ci > 0 && Ci % 64 == 0 && (N == 64 || N == 128) && nvalid >= 1 && nvalid <= N && (act == 0 || act == 1),
                "cno_conv3x: N=%d Ci=%d nvalid=%d act=%d unsupported (Ci %% 64, N = 64 or 128, 1 <= nvalid <= N, act 0 / 1)", N, Ci, nvalid, act);
    RPB_REQUIRE((uintptr_t)planes % 16 == 0 && (uintptr_t)Wz % 16 == 0, "cno_conv3x: planes and weights must be 16-byte aligned");
    RPB_REQUIRE(!out || ((uintptr_t)out % 4 == 0 && ldo >= nvalid), "cno_conv3x: ldo=%d < nvalid=%d", ldo, nvalid);
    RPB_REQUIRE(!res || ((uintptr_t)res % 4 == 0 && ldr >= nvalid), "cno_conv3x: ldr=%d < nvalid=%d", ldr, nvalid);
    RPB_REQUIRE(!out_planes || ((uintptr_t)out_planes % 16 == 0 && ldp % 8 == 0 && nvalid % 8 == 0 && ldp >= nvalid),
                "cno_conv3x: plane output needs a 16-byte aligned first column, ldp %% 8 == 0 and nvalid %% 8 == 0 (ldp=%d nvalid=%d)", ldp, nvalid);
    RPB_REQUIRE(Hc > 0 && Wc > 0 && Dc > 0 && M % ((long)Hc * Wc * Dc) == 0, "cno_conv3x: bad mesh");
    CnoArgs a{(const uint16_t*)planes, (const uint16_t*)Wz, sc, sh, res, out, (uint16_t*)out_planes, M, N, Ci, nvalid, act, ldr, ldo, ldp,
              Hc, Wc, Dc};
    const size_t lds = (size_t)2 * 24 * CN_ROWS * 16 + 9 * CN_ROWS + 16;
    const unsigned gx = (unsigned)(((M + CN_BM - 1) / CN_BM + 7) / 8 * 8);
    hipStream_t st = (hipStream_t)stream;
    (void)hipFuncSetAttribute((const void*)cno_conv3x_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipFuncSetAttribute((const void*)cno_conv3x_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (N == 64) {
        hipLaunchKernelGGL(cno_conv3x_kernel<1>, dim3(gx, 1), dim3(256), lds, st, a);
    } else {
        hipLaunchKernelGGL(cno_conv3x_kernel<2>, dim3(gx, 1), dim3(256), lds, st, a);
    }
    RPB_CHECK_LAUNCH("cno_conv3x");
}
