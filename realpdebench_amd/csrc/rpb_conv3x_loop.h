// The main loop of the bf16x3 3x3x3 convolution and the K-split reduction that follows it, as TEXT: this file is included inside the
// body of conv3x_kernel<WN> (csrc/rpb_conv3x.hip) and cno_conv3x_kernel<WN> (csrc/rpb_cno.hip), which differ in their epilogues only.
// It is a fragment and not a function on purpose: as a forced-inline __device__ template the body is optimised on its own, without
// the kernel's launch bounds, and every instance came out differently; included as text, every bf16x3 instance keeps its code
// (profiles/conv3_fwd_unify.txt, profiles/conv3x_loop_share.txt).  The two-fp16-plane kernels keep a text of their own,
// csrc/rpb_conv3h_loop.h: the same record has what one body for both plane schemes did to the f16x2 <1> instance.
//
// Expects  a template parameter WN (waves over co: 1, 2 or 4) and an argument object `a` with
//              P [3][M][Ci] bf16 planes, Wz (rpb_conv3x_wprep order), M, N, Ci, T, H, W;
//          dynamic LDS of 2 * 24 * CX_ROWS * 16 + 9 * CX_ROWS bytes, 256 threads, grid.x a multiple of 8 (CX_BM-token tiles).
// Leaves   KS = 4 / WN, lds4, tid, lane, col, half, nw, kp, m0, n0 (workgroups with m0 >= a.M have returned);
//          section 1: f32x16 acc[4][2] -- wave (nw, kp)'s partial sums over its 16-channel chunks of the 128 token x 64 co tile
//                     (row tile tm, co tile tn, MFMA D layout);
//          section 2: red (the K-split slots in LDS), the partials of the row tiles a wave does not own parked there behind a
//                     barrier, and the macro CX_KSPLIT_SUM(tm), with which the owner (kp == tm % KS) completes acc[tm][*]; it is
//                     the one macro of this file that stays defined.
// The layout overview is at the top of csrc/rpb_conv3x.hip.

// ====================================================================================== section 1: the main loop
    constexpr int KS = 4 / WN;
    extern __shared__ u32x4 lds4[];
    // two stage buffers of [3 planes][4 chunks][2 halves][CX_ROWS] x 16 B, then [9][CX_ROWS] row validity per (kt, kh)
    unsigned char* rv = reinterpret_cast<unsigned char*>(lds4 + 2 * 24 * CX_ROWS);
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nw = wave % WN, kp = wave / WN;
    // XCD-aware tile order: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so XCD x walks the
    // contiguous tile range [x * chunk, (x + 1) * chunk): the h +- 1 rows a tile stages are its neighbours' own rows and hit L2
    const unsigned chunk = gridDim.x >> 3;
    const long tile = (long)(blockIdx.x & 7) * chunk + (blockIdx.x >> 3);
    const long m0 = tile * CX_BM;
    if (m0 >= a.M) return;
    const int n0 = blockIdx.y * (64 * WN) + nw * 64;
    const int NT = a.N >> 5, NCC = a.Ci >> 4;
    const unsigned uT = a.T, uH = a.H, uW = a.W;

    for (int idx = tid; idx < 9 * CX_ROWS; idx += 256) {
        const int g = idx / CX_ROWS, j = idx - g * CX_ROWS;
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
        for (int p = 0; p < 3; ++p) av[p] = As[((p * 4 + s) * 2 + half) * CX_ROWS + tm * 32 + col + kw];
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
    constexpr int NLD = (CX_ROWS * 24 + 255) / 256;
    static_assert(NLD == 13, "staging macros below are written for 13 loads per thread");
#define CX_FOR13(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
#define CX_DECL(J) u32x4 sv##J = z4; bool ok##J = false;
    CX_FOR13(CX_DECL)
#define CX_LOAD(J)                                                                                            \
    if constexpr (J >= j0 && J < j1) {                                                                        \
        const int idx = tid + J * 256;                                                                        \
        const int row = idx / 24, rem = idx - row * 24;                                                       \
        const int p = rem >> 3, sh = rem & 7; /* sh = 2 * chunk + half: 8 x 16 B = one 128 B line */          \
        ok##J = idx < CX_ROWS * 24 && rv[g * CX_ROWS + (row < CX_ROWS ? row : 0)];                            \
        const long off = ok##J ? (long)p * MC + (rowbase + row) * a.Ci + c * 64 + sh * 8 : 0;                 \
        sv##J = *reinterpret_cast<const u32x4*>(a.P + off);                                                   \
    }
#define CX_STORE(J)                                                                                           \
    {                                                                                                         \
        const int idx = tid + J * 256;                                                                        \
        const int row = idx / 24, rem = idx - row * 24;                                                       \
        if (idx < CX_ROWS * 24) dst[rem * CX_ROWS + row] = ok##J ? sv##J : z4;                                \
    }
    // loads j0 <= j < j1 of the 13 a thread contributes to stage (g, c)
    auto stage_load = [&](int g, int c, auto j0c, auto j1c) __attribute__((always_inline)) {
        constexpr int j0 = decltype(j0c)::value, j1 = decltype(j1c)::value;
        const int kt = g / 3, kh = g - kt * 3;
        const long rowbase = m0 - 1 + ((long)(kt - 1) * a.H + (kh - 1)) * a.W;
        CX_FOR13(CX_LOAD)
    };
    auto stage_store = [&](u32x4* dst) __attribute__((always_inline)) { CX_FOR13(CX_STORE) };
    bload(wbase + (long)kp * wchunk, bc);                               // (g 0, c 0, s = kp, kw 0)
    stage_load(0, 0, IC<0>{}, IC<NLD>{});
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
            As = lds4 + buf * 24 * CX_ROWS;
            lda(kp, 0, 0, ac);
            // the next stage's A loads are spread over this stage's tap steps (13 MB at once from every CU of the chip in
            // lock-step is a burst that the in-order vmcnt of the next B operands would have to wait out)
#define CX_SI_BLOCK(SI)                                                                                        \
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
        /* the step after (s, kw 2): next chunk of this stage, else the next stage's first chunk */            \
        if (SI + 1 < SPS) bload(w0 + (long)KS * wchunk, bsel(IC<(SI * 3 + 3) & 1>{}));                         \
        else if (more) bload(wbase + (long)(gn * 3) * wtap + (long)(cn * 4 + kp) * wchunk, bsel(IC<(SI * 3 + 3) & 1>{})); \
        if (more) stage_load(gn, cn, IC<(SI * 3 + 2) * NLD / NST>{}, IC<(SI * 3 + 3) * NLD / NST>{});          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        tap_step(s, 2, SI + 1 < SPS, bsel(IC<(SI * 3 + 2) & 1>{}));                                            \
    }
            CX_SI_BLOCK(0) CX_SI_BLOCK(1) CX_SI_BLOCK(2) CX_SI_BLOCK(3)
            if constexpr (NST & 1) {                                    // odd step count (N = 64): the next stage's first B set is in bn
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                    for (int p = 0; p < 3; ++p) bc[tn][p] = bn[tn][p];
            }
            if (more) stage_store(lds4 + (buf ^ 1) * 24 * CX_ROWS);
            __syncthreads();                                            // everyone is done with buf and has filled buf ^ 1
            buf ^= 1;
        }
    }

    // ====================================================================================== section 2: the K-split reduction
    // K-split partial sums through LDS in ONE round: the KS waves of a column group own the four 32-token row tiles round-robin
    // (tile tm belongs to wave tm % KS); every wave parks its partials of the tiles it does not own, one barrier, every wave sums
    // and stores its own tiles.  (A first version let the kp == 0 waves reduce and store all four tiles, one tile and two
    // barriers at a time: measured 38 k of the 116 k cycles of a Ci = 64, N = 64 workgroup.)
    float* red = reinterpret_cast<float*>(lds4);                        // [WN][4 tiles][KS - 1 sources][2 col tiles][16 regs][64 lanes]
    if (KS > 1) {
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
    // tile TM's parked partials added to its owner's accumulators (the owner, kp == TM % KS, runs this before its epilogue).  A macro
    // and not a lambda: the lambda changed the register allocation of every instance.  The slot address is written as the owner's
    // first slot plus k2 slots, the form that leaves both kernels' code as it was (the CNO epilogue reuses that first slot).
#define CX_KSPLIT_SUM(TM)                                                                                      \
    if (KS > 1) {                                                                                              \
        _Pragma("unroll") for (int k2 = 0; k2 < KS - 1; ++k2) {                                                \
            const float* slot = red + ((nw * 4 + (TM)) * (KS - 1)) * 2048 + k2 * 2048;                         \
            _Pragma("unroll") for (int tn = 0; tn < 2; ++tn)                                                   \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[TM][tn][r] += slot[(tn * 16 + r) * 64 + lane]; \
        }                                                                                                      \
    }
#undef CX_SI_BLOCK
#undef CX_STORE
#undef CX_LOAD
#undef CX_DECL
#undef CX_FOR13
