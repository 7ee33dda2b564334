// The main loop of the f16x2 3x3x3 convolution and the first half of the K-split reduction that follows it, as TEXT: this file is
// included inside the body of conv3x_f16x2_kernel<WN> (csrc/rpb_conv3h.hip) and cno_conv3x_f16x2_kernel<WN> (csrc/rpb_cno3h.hip), which
// differ in their epilogues only.  It is a fragment and not a function for the reason csrc/rpb_conv3x_loop.h gives for the bf16x3
// pair: as a forced-inline __device__ template the body is optimised on its own, without the kernel's launch bounds
// (profiles/conv3_fwd_unify.txt); included as text, conv3x_f16x2_kernel keeps its code instruction for instruction
// (profiles/cno_arith_probe.txt has the comparison).  The bf16x3 loop stays a text of its own: the same record has what one body for
// both plane schemes did to the <1> instance of this one.
//
// Expects  a template parameter WN (waves over co: 1, 2 or 4) and an argument object `a` with
//              P [2][M][Ci] fp16 planes, Wz (rpb_conv3x_wprep_f16x2 order), M, N, Ci, T, H, W;
//          dynamic LDS of 2 * 16 * CH_ROWS * 16 + 9 * CH_ROWS bytes (or the K-split slots if larger), 256 threads, grid.x a multiple
//          of 8 (CH_BM-token tiles).
// Leaves   KS = 4 / WN, lds4h, tid, lane, col, half, nw, kp, m0, n0 (workgroups with m0 >= a.M have returned);
//          f32x16 acc[4][2] -- wave (nw, kp)'s partial sums over its 16-channel chunks of the 128 token x 64 co tile (row tile tm, co
//          tile tn, MFMA D layout); red (the K-split slots in LDS) with the partials of the row tiles a wave does not own parked there
//          behind a barrier; and the macro CH_KSPLIT_SUM(tm), with which the owner (kp == tm % KS) completes acc[tm][*].
//          conv3x_f16x2_kernel keeps that sum written out in its epilogue, as it was; the macro is the same statements for the CNO
//          epilogue.  It is the one macro of this file that stays defined.
    constexpr int KS = 4 / WN;
    extern __shared__ u32x4 lds4h[];
    // two stage buffers of [2 planes][4 chunks][2 halves][CH_ROWS] x 16 B, then [9][CH_ROWS] row validity per (kt, kh)
    unsigned char* rv = reinterpret_cast<unsigned char*>(lds4h + 2 * 16 * CH_ROWS);
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nw = wave % WN, kp = wave / WN;
    // XCD-aware tile order (as conv3x_kernel)
    const unsigned chunk = gridDim.x >> 3;
    const long tile = (long)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    const long m0 = tile * CH_BM;
    if (m0 >= a.M) return;
    const int n0 = blockIdx.y * (64 * WN) + nw * 64;
    const int NT = a.N >> 5, NCC = a.Ci >> 4;
    const unsigned uT = a.T, uH = a.H, uW = a.W;

    for (int idx = tid; idx < 9 * CH_ROWS; idx += 256) {
        const int g = idx / CH_ROWS, j = idx - g * CH_ROWS;
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

    // software pipeline of conv3x_kernel: next stage's A loads spread over the current stage's tap steps, next tap step's B operands
    // requested before the current one's MFMAs, A operands of the next row tile read from LDS before the current tile's MFMAs
    constexpr int SPS = 4 / KS;                                        // my 16-channel chunks per stage
    const int nc64 = a.Ci >> 6;
    const uint16_t* wbase = a.Wz + ((long)(n0 >> 5) * 64 + lane) * 8;
    const long wplane = (long)NT * 512;                                // fp16 elements between the planes of one (tap, chunk)
    const long wchunk = 2 * wplane, wtap = (long)NCC * wchunk;
    auto bload = [&](const uint16_t* src, u32x4 (&b)[2][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn) b[tn][p] = *reinterpret_cast<const u32x4*>(src + p * wplane + tn * 512);
    };
    u32x4 bc[2][2], bn[2][2];
    const u32x4* As = lds4h;
    u32x4 ac[2], an[2];
    auto lda = [&](int s, int kw, int tm, u32x4 (&av)[2]) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p) av[p] = As[((p * 4 + s) * 2 + half) * CH_ROWS + tm * 32 + col + kw];
    };
    auto mfma6 = [&](int tm, int kw, u32x4 (&av)[2], const u32x4 (&b)[2][2]) __attribute__((always_inline)) {
        if ((kw == 0 && wlo[tm]) || (kw == 2 && whi[tm])) av[0] = av[1] = z4;
        // small terms first; the two co tiles alternate so consecutive MFMAs are independent
        acc[tm][0] = mfma32h(av[1], b[0][0], acc[tm][0]);
        acc[tm][1] = mfma32h(av[1], b[1][0], acc[tm][1]);
        acc[tm][0] = mfma32h(av[0], b[0][1], acc[tm][0]);
        acc[tm][1] = mfma32h(av[0], b[1][1], acc[tm][1]);
        acc[tm][0] = mfma32h(av[0], b[0][0], acc[tm][0]);
        acc[tm][1] = mfma32h(av[0], b[1][0], acc[tm][1]);
    };
    auto tap_step = [&](int s, int kw, bool more, const u32x4 (&b)[2][2]) __attribute__((always_inline)) {
        lda(s, kw, 1, an);
        __builtin_amdgcn_sched_barrier(0);
        mfma6(0, kw, ac, b);
        __builtin_amdgcn_sched_barrier(0);
        lda(s, kw, 2, ac);
        __builtin_amdgcn_sched_barrier(0);
        mfma6(1, kw, an, b);
        __builtin_amdgcn_sched_barrier(0);
        lda(s, kw, 3, an);
        __builtin_amdgcn_sched_barrier(0);
        mfma6(2, kw, ac, b);
        __builtin_amdgcn_sched_barrier(0);
        if (more) lda(kw == 2 ? s + KS : s, kw == 2 ? 0 : kw + 1, 0, ac);
        __builtin_amdgcn_sched_barrier(0);
        mfma6(3, kw, an, b);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto bsel = [&](auto pc) -> u32x4(&)[2][2] {
        if constexpr (decltype(pc)::value) return bn;
        else return bc;
    };
    // A staging registers: 9 x 16 B per thread (130 rows x 16 pieces of 16 B over 256 threads), named individually
    constexpr int NLD = (CH_ROWS * 16 + 255) / 256;
    static_assert(NLD == 9, "staging macros below are written for 9 loads per thread");
#define CH_FOR9(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#define CH_DECL(J) u32x4 sv##J = z4; bool ok##J = false;
    CH_FOR9(CH_DECL)
#define CH_LOAD(J)                                                                                            \
    if constexpr (J >= j0 && J < j1) {                                                                        \
        const int idx = tid + J * 256;                                                                        \
        const int row = idx >> 4, rem = idx & 15;                                                             \
        const int p = rem >> 3, sh = rem & 7; /* sh = 2 * chunk + half: 8 x 16 B = one 128 B line */          \
        ok##J = idx < CH_ROWS * 16 && rv[g * CH_ROWS + (row < CH_ROWS ? row : 0)];                            \
        const long off = ok##J ? (long)p * MC + (rowbase + row) * a.Ci + c * 64 + sh * 8 : 0;                 \
        sv##J = *reinterpret_cast<const u32x4*>(a.P + off);                                                  \
    }
#define CH_STORE(J)                                                                                           \
    {                                                                                                         \
        const int idx = tid + J * 256;                                                                        \
        const int row = idx >> 4, rem = idx & 15;                                                             \
        if (idx < CH_ROWS * 16) dst[rem * CH_ROWS + row] = ok##J ? sv##J : z4;                                \
    }
    auto stage_load = [&](int g, int c, auto j0c, auto j1c) __attribute__((always_inline)) {
        constexpr int j0 = decltype(j0c)::value, j1 = decltype(j1c)::value;
        const int kt = g / 3, kh = g - kt * 3;
        const long rowbase = m0 - 1 + ((long)(kt - 1) * a.H + (kh - 1)) * a.W;
        CH_FOR9(CH_LOAD)
    };
    auto stage_store = [&](u32x4* dst) __attribute__((always_inline)) { CH_FOR9(CH_STORE) };
    bload(wbase + (long)kp * wchunk, bc);                               // (g 0, c 0, s = kp, kw 0)
    stage_load(0, 0, IC<0>{}, IC<NLD>{});
    stage_store(lds4h);
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
            As = lds4h + buf * 16 * CH_ROWS;
            lda(kp, 0, 0, ac);
#define CH_SI_BLOCK(SI)                                                                                        \
    if constexpr (SI < SPS) {                                                                                  \
        const int s = kp + SI * KS;                                                                            \
        const uint16_t* w0 = wbase + (long)(g * 3) * wtap + (long)(c * 4 + s) * wchunk;                        \
        bload(w0 + wtap, bsel(IC<(SI * 3 + 1) & 1>{}));                                                        \
        if (more) stage_load(gn, cn, IC<(SI * 3 + 0) * NLD / NST>{}, IC<(SI * 3 + 1) * NLD / NST>{});          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        tap_step(s, 0, true, bsel(IC<(SI * 3 + 0) & 1>{}));                                                    \
        bload(w0 + 2 * wtap, bsel(IC<(SI * 3 + 2) & 1>{}));                                                    \
        if (more) stage_load(gn, cn, IC<(SI * 3 + 1) * NLD / NST>{}, IC<(SI * 3 + 2) * NLD / NST>{});          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        tap_step(s, 1, true, bsel(IC<(SI * 3 + 1) & 1>{}));                                                    \
        if (SI + 1 < SPS) bload(w0 + (long)KS * wchunk, bsel(IC<(SI * 3 + 3) & 1>{}));                         \
        else if (more) bload(wbase + (long)(gn * 3) * wtap + (long)(cn * 4 + kp) * wchunk, bsel(IC<(SI * 3 + 3) & 1>{}));  \
        if (more) stage_load(gn, cn, IC<(SI * 3 + 2) * NLD / NST>{}, IC<(SI * 3 + 3) * NLD / NST>{});          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        tap_step(s, 2, SI + 1 < SPS, bsel(IC<(SI * 3 + 2) & 1>{}));                                            \
    }
            CH_SI_BLOCK(0) CH_SI_BLOCK(1) CH_SI_BLOCK(2) CH_SI_BLOCK(3)
            if constexpr (NST & 1) {                                    // odd step count (N = 64): the next stage's first B set is in bn
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int p = 0; p < 2; ++p) bc[tn][p] = bn[tn][p];
            }
            if (more) stage_store(lds4h + (buf ^ 1) * 16 * CH_ROWS);
            __syncthreads();                                            // everyone is done with buf and has filled buf ^ 1
            buf ^= 1;
        }
    }
#undef CH_SI_BLOCK
#undef CH_STORE
#undef CH_LOAD
#undef CH_DECL
#undef CH_FOR9
    // ---- K-split partial sums through LDS in one round (as conv3x_kernel)
    float* red = reinterpret_cast<float*>(lds4h);                       // [WN][4 tiles][KS - 1 sources][2 col tiles][16 regs][64 lanes]
    if (KS > 1) {
        __syncthreads();
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
    // tile TM's parked partials added to its owner's accumulators, in the order of conv3x_f16x2_kernel's epilogue
#define CH_KSPLIT_SUM(TM)                                                                                      \
    if (KS > 1) {                                                                                              \
        _Pragma("unroll") for (int k2 = 0; k2 < KS - 1; ++k2) {                                                \
            const float* slot = red + ((nw * 4 + (TM)) * (KS - 1) + k2) * 2048;                                \
            _Pragma("unroll") for (int tn = 0; tn < 2; ++tn)                                                   \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[TM][tn][r] += slot[(tn * 16 + r) * 64 + lane]; \
        }                                                                                                      \
    }
