// Token GEMM on the fp16 MFMA from two-plane operands for K above what fits resident:
//     out[m][n] = epilogue( sum_k A[m][k] * W[n][k] )   (nn.Linear layout)
// The large-K sibling of rpb_gemm3h.hip (the opt-in "f16x2" eval arithmetic, DESIGN.md sections 13.3 and 14): the same split8h planes, the
// same three products per k-step (mma3h: lo*hi, hi*lo, hi*hi, lo*lo <= 2^-22 of the product dropped), the same col_exp exponent rule and
// the SAME weight planes -- rpb_gemm3h_wprep's operand order and its device-side weight scale sc[0] = 2^-ew are used as they are.  What
// differs is everything that followed from "the whole 64-row x K tile is resident": the scale scheme, the tile and the epilogue set.
//
// Contract: A [M][lda] fp32 rows (may be a column range of a wider tensor), W [N][K] prepared once by rpb_gemm3h_wprep, out [M][ldo] (may
// be a column range); any M >= 1; K % 64 == 0, K > 512 (K <= 512 is rpb_gemm3h's; no upper limit: K is streamed in 64-column chunks);
// N % 256 == 0; lda >= K, ldo >= N, both % 4 == 0; epilogue = bias, act in {0 none, 1 GELU (gelu_f, the function rpb_gemm3x applies),
// 3 ReLU}, residual [M][ldo]; rowe = M ints of scratch the launch fills and reads.  rpb_gemm3hk_supported says so without launching;
// anything else is RPB_ERR_ARG.
//
// ACTIVATION SCALE: one exact power of two per token row from A ROW-EXPONENT PRE-PASS (the second of the two candidates).  A small kernel
// of the same launch wrapper reads A once (one wave per row, 16 B per lane), takes the EXACT maximum of the row's K values and writes
// e_row = col_exp<14>(max) -- max 2^e in [2^14, 2^15), capped at 62, 0 for an all-zero row -- to rowe on the device; no host read.  The
// GEMM scales a row by 2^e_row before the split and its accumulator row by 2^-e_row 2^-ew in the epilogue, so an all-zero row gives
// exactly epilogue(0).  The other candidate (an exponent per row and per resident K chunk, each chunk's accumulator rescaled into a
// running fp32 accumulator) needs the accumulators twice: 2 x 256 registers of a 512-register wave at the 256-row tile, and 2 x 128 at
// the 128-row tile, which would leave the CU to one workgroup where two measured faster (below); it was not built and its cost is
// not measured.  Cost of the pre-pass that was built, measured alone next to each GEMM (profiles/dpot_arith_probe.txt, "rowexp"): 0.02
// of the call at M = 16384, K = 1536 (0.019 of 0.974 ms), 0.07 at K = 6144 (0.073 of 1.033 ms: the 0.4 GB read), 0.06 at M = 1 M rows.
//
// TILE: operand bytes per MFMA.  One k-step (16 columns) of a BM x BN workgroup tile reads 64 (BM + BN) bytes beyond the CU (A as fp32,
// W as two fp16 planes: 4 bytes per element either way) and issues (BM / 32)(BN / 32) 3 MFMAs of 32 cycles on four SIMDs, so the CU
// asks for  (BM + BN) 64 / ((BM BN / 1024) 24)  =  2731 (BM + BN) / (BM BN) bytes per clock:
//     64 x 256 (rpb_gemm3h's rows)  53 B/clk/CU = 33 TB/s over 256 CUs at 2.4 GHz       128 x 256  32 B/clk/CU = 20 TB/s
//     128 x 128                     43 B/clk/CU = 26 TB/s                               256 x 256  21 B/clk/CU = 13 TB/s
// against 17-19 TB/s that the L2s deliver to all workgroups together and 8.6 TB/s from the Infinity Cache (MI355X figures).  Only the
// 256 x 256 tile leaves the MFMA, not the L2, as the limit on paper, and the six-product default kernel needs half of this per product,
// which is why its narrower tile is enough for it.  Hence: four waves as 2 x 2, a wave owns 32 TM rows x 128 columns (TM = 4: 16
// accumulator tiles = 256 registers), B operands straight from the operand-ordered planes one k-step ahead (the two row waves of a
// column pair read the same lines), A through LDS.  LDS: a 64-column chunk of the BM rows as two planes, [2 planes][8][BM + 2] x 16 B,
// double-buffered: 132 KB at BM = 256 of the CU's 160 KB -- one workgroup per CU, one wave per SIMD; per k-step a wave reads 8 x 1 KB
// of A from LDS for 48 MFMAs (1536 cycles): 21 B/clk/CU of the LDS's 128.
// MEASURED (profiles/dpot_gemm3hk_tile_probe.txt, each height forced for a whole run), the arithmetic is half the story: at 128 rows
// (TM = 2: 66 KB of LDS, 250 registers) TWO workgroups share a CU, one multiplies while the other waits at its barrier, splits or
// stores, and that is worth more than the L2 bytes wherever W stays in the Infinity Cache -- dpot_l FeedForward at M = 16384: 0.972 /
// 1.044 ms at 128 rows against 1.016 / 1.250 ms at 256 (default kernel 1.91 / 1.88 ms).  256 rows win only where W is streamed from
// HBM (out0 of dpot_l, 604 MB of planes: 4.66 against 4.82 ms at M = 4096).  The launcher therefore takes TM = 4 only for planes above
// half the Infinity Cache, TM = 2 where 128-row items keep three quarters of the CUs busy (192 items of K = 6144 on 256 CUs: 0.335 ms
// against 0.383 at 64 rows; 128 items of K = 1024: 0.081 against 0.061), else TM = 1.  With that rule (profiles/dpot_arith_probe.txt):
// 790-950 TFLOP/s of issued fp16 MFMA at the dpot_l shapes, 1.55x-2.6x the default kernel there and 1.11x-1.57x at dpot_s.
// Items (row tile, 256-column block) are dealt round-robin, column block fastest: the workgroups running together share few row tiles
// and few column blocks, so a chunk of either is fetched into an L2 once for several readers.
//
// Pipeline of one item: the next 64-column chunk of A is staged in four row groups, one per k-step of the current chunk -- requested
// into registers at the k-step's top, scaled, split and written to the other LDS buffer at its end; one barrier per chunk.  The epilogue is parked: a wave writes its accumulators
// to its quarter of the (then idle) A buffers in two halves and reads them back row-major, so that bias, residual and out move 16 bytes
// per lane (A, bias, residual and out are 16-byte aligned: leading dimensions % 4 and aligned base pointers).
//
// Fixed summation order, no atomics: two calls give the same bits.  Tail rows read row M - 1 and store nothing; nothing is written outside
// out[m][0..N) for m < M (rowe[0..M) aside).  Non-finite inputs are outside the contract, as for rpb_gemm3h.
#include "rpb_mma.h"

#define G3K_KC 64          // columns of a resident chunk
#define G3K_BN 256
#define G3K_KMIN 512      // rpb_gemm3h's G3H_KMAX: up to there the resident form owns the product

// ---------------------------------------------------------------------------------- row exponents: one wave per row
__global__ __launch_bounds__(256) void gemm3hk_rowexp_kernel(const float* __restrict__ A, int* __restrict__ rowe, long M, int K, int lda) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const f32x4* src = reinterpret_cast<const f32x4*>(A + row * lda);
    float m = 0.f;
    for (int c = lane; c < (K >> 2); c += 64) {
        const f32x4 v = src[c];
        m = fmaxf(m, fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))));
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if (lane == 0) rowe[row] = col_exp<14>(m);
}

// ---------------------------------------------------------------------------------- the GEMM
struct Gemm3hkArgs {
    const float* A;        // [M][lda] fp32
    const uint16_t* Wz;    // rpb_gemm3h_wprep's (hi, lo) planes of W[N][K] 2^ew
    const float* sc;       // sc[0] = 2^-ew
    const float* bias;     // [N] or null
    const float* residual; // [M][ldo] or null
    float* out;            // [M][ldo]
    const int* rowe;       // [M] row exponents (gemm3hk_rowexp_kernel)
    long M;
    int N, K, lda, ldo;
    int act;               // 0 none, 1 GELU, 3 ReLU
};

// TM: 32-row tiles per wave; the workgroup's four waves are 2 (rows) x 2 (columns), a wave owns 32 TM rows x 128 columns
template <int TM>
__global__ __launch_bounds__(256, TM <= 2 ? 2 : 1) void gemm3hk_kernel(Gemm3hkArgs a) {
    constexpr int TN = 4, BM = 64 * TM, RS = BM + 2, NJ = 2 * TM;      // RS: 16-byte units per 8-column group (the eight lanes of a row land in distinct banks)
    extern __shared__ u32x4 lds4[];                                    // [2 buffers][2 planes][8][RS] x 16 B, then BM row factors
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    float* const rowfac = reinterpret_cast<float*>(lds4 + 4 * 8 * RS);
    const int nks = a.K >> 4, nchunks = a.K / G3K_KC;
    const long ntiles = (a.M + BM - 1) / BM;
    const int NB = a.N / G3K_BN;
    const long nitems = ntiles * NB;
    const float wsc = a.sc[0];
    const int NT = a.N >> 5;
    const long wplane = (long)NT * 512, wstep = 2 * wplane;
    const int r0 = tid >> 3, sh = tid & 7;                             // staging: columns 8 sh .. + 8 of rows r0 + 32 j

    for (long item = blockIdx.x; item < nitems; item += gridDim.x) {
        const long m0 = (item / NB) * BM;
        const int n0 = (int)(item % NB) * G3K_BN + wc * (32 * TN);
        const uint16_t* const wbase = a.Wz + ((long)(n0 >> 5) * 64 + lane) * 8;
        // ---- this thread's rows: their scale, their source, the factor that undoes both scales
        const float* src[NJ];
        float rs[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const long row = m0 + r0 + 32 * j;
            const long rr = row < a.M ? row : a.M - 1;                 // tail: a valid row is read, nothing is stored
            const int ex = a.rowe[rr];
            rs[j] = pow2f(ex);
            src[j] = a.A + rr * a.lda + sh * 8;
            if (sh == 0) rowfac[r0 + 32 * j] = pow2f(-ex) * wsc;       // both >= 2^-62: the product is normal
        }
        // staging of a chunk in row groups of RPK rows: group q is requested at the top of k-step q of the chunk before and is scaled,
        // split and written to the other buffer at that k-step's end -- 16 registers in flight instead of the whole chunk's 64
        constexpr int RPK = NJ >= 4 ? NJ / 4 : 1, NQ = NJ / RPK;
        f32x4 sa[RPK], sb[RPK];
        auto group_load = [&](int kc, int q) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < RPK; ++i) {
                sa[i] = *reinterpret_cast<const f32x4*>(src[q * RPK + i] + kc * G3K_KC);
                sb[i] = *reinterpret_cast<const f32x4*>(src[q * RPK + i] + kc * G3K_KC + 4);
            }
        };
        auto group_store = [&](int buf, int q) __attribute__((always_inline)) {
            u32x4* const P0 = lds4 + buf * (16 * RS);
            u32x4* const P1 = P0 + 8 * RS;
#pragma unroll
            for (int i = 0; i < RPK; ++i) {
                const int j = q * RPK + i;
                float v[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    v[e] = sa[i][e] * rs[j];
                    v[4 + e] = sb[i][e] * rs[j];
                }
                bf16x8 h, l;
                split8h<false>(v, h, l);
                P0[sh * RS + r0 + 32 * j] = __builtin_bit_cast(u32x4, h);
                P1[sh * RS + r0 + 32 * j] = __builtin_bit_cast(u32x4, l);
            }
        };
        auto ldb_ = [&](int ksg, u32x4 (&bv)[TN][2]) __attribute__((always_inline)) {
            const uint16_t* s = wbase + (long)ksg * wstep;
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                for (int p = 0; p < 2; ++p) bv[tn][p] = *reinterpret_cast<const u32x4*>(s + p * wplane + tn * 512);
        };

        f32x16 acc[TM][TN];
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = zero16();
        u32x4 bc[TN][2], bn[TN][2];
        ldb_(0, bc);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            group_load(0, q);
            group_store(0, q);
        }
        __syncthreads();
        for (int kc = 0; kc < nchunks; ++kc) {
            const bool more = kc + 1 < nchunks;
            const u32x4* const P0 = lds4 + (kc & 1) * (16 * RS);
            const u32x4* const P1 = P0 + 8 * RS;
#pragma unroll
            for (int ks = 0; ks < G3K_KC / 16; ++ks) {
                const int ksg = kc * (G3K_KC / 16) + ks;
                // the next k-step's B operands and this k-step's row group of the next chunk are requested first and stay requested:
                // the scheduling barriers keep the loads from sinking to their uses (they did, and every MFMA group waited for memory)
                ldb_(ksg + 1 < nks ? ksg + 1 : ksg, bn);               // the last step requests its own operands again: in bounds, unused
                if (ks < NQ && more) group_load(kc + 1, ks);
                __builtin_amdgcn_sched_barrier(0);
                const int o = (2 * ks + half) * RS + wr * (32 * TM) + col;
                u32x4 ac[2] = {P0[o], P1[o]};
#pragma unroll
                for (int tm = 0; tm < TM; ++tm) {
                    u32x4 an[2] = {ac[0], ac[1]};
                    if (tm + 1 < TM) {
                        an[0] = P0[o + 32 * (tm + 1)];
                        an[1] = P1[o + 32 * (tm + 1)];
                    }
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = mma3h(ac, bc[tn], acc[tm][tn]);
                    ac[0] = an[0];
                    ac[1] = an[1];
                }
                __builtin_amdgcn_sched_barrier(0);
                if (ks < NQ && more) group_store((kc + 1) & 1, ks);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int p = 0; p < 2; ++p) bc[tn][p] = bn[tn][p];
            }
            __syncthreads();
        }
        // ---- parked epilogue: the A buffers are free after the last barrier; a wave parks half of its tile (32 TM rows x 64 columns) in
        //      its quarter of them and reads it back row-major, so that bias, residual and out move 16 bytes per lane in a LOOP -- run
        //      from the accumulators (one guarded 4-byte store per register, GELU inlined 256 times) the epilogue was 19000
        //      instructions, and the compiler kept the accumulators in scratch memory to index them
        float* const T = reinterpret_cast<float*>(lds4 + wave * (8 * RS));
        const int er = lane >> 4, ec = (lane & 15) * 4;
#pragma unroll
        for (int rd = 0; rd < 2; ++rd) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                    for (int r = 0; r < 16; ++r) T[(tm * 32 + mfma_row(lane, r)) * 64 + t2 * 32 + col] = acc[tm][2 * rd + t2][r];
            __syncthreads();
            const int n = n0 + rd * 64 + ec;
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (a.bias) bv = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll 2
            for (int i = 0; i < 8 * TM; ++i) {
                const int row = wr * (32 * TM) + 4 * i + er;           // of the workgroup's tile
                const long m = m0 + row;
                if (m < a.M) {
                    f32x4 v = *reinterpret_cast<const f32x4*>(T + (4 * i + er) * 64 + ec);
                    const float fq = rowfac[row];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float t = fmaf(v[e], fq, bv[e]);
                        if (a.act == 1) t = gelu_f(t);
                        else if (a.act == 3) t = fmaxf(t, 0.f);
                        v[e] = t;
                    }
                    const long o = m * a.ldo + n;
                    if (a.residual) v += *reinterpret_cast<const f32x4*>(a.residual + o);
                    *reinterpret_cast<f32x4*>(a.out + o) = v;
                }
            }
            __syncthreads();                                           // the parked tile, the row factors and both buffers are free again
        }
    }
}

template <int TM>
static int gemm3hk_launch(const Gemm3hkArgs& a, long nitems, hipStream_t st) {
    constexpr int RS = 64 * TM + 2;
    const size_t lds = (size_t)4 * 8 * RS * 16 + 64 * TM * sizeof(float);
    if (hipFuncSetAttribute((const void*)gemm3hk_kernel<TM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        RPB_FAIL(RPB_ERR_LAUNCH, "gemm3hk: %zu bytes of LDS refused", lds);
    const long cus = rpb_num_cus() < 1 ? 1 : rpb_num_cus(), cap = cus * (TM <= 2 ? 2 : 1);      // TM <= 2: two workgroups per CU (LDS, registers)
    const long gx = nitems < cap ? nitems : cap;
    hipLaunchKernelGGL((gemm3hk_kernel<TM>), dim3((unsigned)gx), dim3(256), lds, st, a);
    RPB_CHECK_LAUNCH("gemm3hk");
}

extern "C" int rpb_gemm3hk_supported(long M, int N, int K, int lda, int ldo) {
    return M >= 1 && K > G3K_KMIN && K % 64 == 0 && N > 0 && N % G3K_BN == 0 && lda % 4 == 0 && lda >= K && ldo % 4 == 0 && ldo >= N;
}

// the pre-pass on its own (rpb_gemm3hk runs it itself; exported so that its cost can be measured)
extern "C" int rpb_gemm3hk_rowexp(const float* A, int* rowe, long M, int K, int lda, void* stream) {
    RPB_REQUIRE(A && rowe && M > 0 && K > 0 && K % 4 == 0 && lda % 4 == 0 && lda >= K, "gemm3hk_rowexp: M=%ld K=%d lda=%d unsupported", M, K, lda);
    hipLaunchKernelGGL(gemm3hk_rowexp_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, A, rowe, M, K, lda);
    RPB_CHECK_LAUNCH("gemm3hk_rowexp");
}

extern "C" int rpb_gemm3hk(const float* A, const void* Wz, const float* sc, const float* bias, const float* residual, float* out, int* rowe,
                           long M, int N, int K, int lda, int ldo, int act, void* stream) {
    RPB_REQUIRE(A && Wz && sc && out && rowe && M > 0, "gemm3hk: bad arguments");
    RPB_REQUIRE(rpb_gemm3hk_supported(M, N, K, lda, ldo),
                "gemm3hk: N=%d K=%d lda=%d ldo=%d unsupported (K %% 64, K > 512; N a multiple of 256; leading dimensions %% 4)", N, K, lda, ldo);
    RPB_REQUIRE((((uintptr_t)A | (uintptr_t)bias | (uintptr_t)residual | (uintptr_t)out) & 15) == 0,
                "gemm3hk: A, bias, residual and out must be 16-byte aligned (they move 16 bytes per lane)");
    RPB_REQUIRE(act == 0 || act == 1 || act == 3,
                "gemm3hk: act=%d unsupported (0 none, 1 GELU, 3 ReLU; masks, dropout, pre_out / aux belong to training)", act);
    hipStream_t st = (hipStream_t)stream;
    const int rc = rpb_gemm3hk_rowexp(A, rowe, M, K, lda, stream);
    if (rc != RPB_OK) return rc;
    const Gemm3hkArgs a{A, (const uint16_t*)Wz, sc, bias, residual, out, rowe, M, N, K, lda, ldo, act};
    const long NB = N / G3K_BN, cus = rpb_num_cus();
    const long i4 = (M + 255) / 256 * NB, i2 = (M + 127) / 128 * NB, i1 = (M + 63) / 64 * NB;
    // instance (measured, profiles/dpot_arith_probe.txt): 128 rows at two workgroups per CU wherever it keeps three quarters of the CUs
    // busy; 256 rows only where W is re-read from HBM (planes larger than half the 256 MB Infinity Cache); 64 rows for what is left
    if (4L * N * K > (128L << 20) && i4 >= cus) return gemm3hk_launch<4>(a, i4, st);
    if (4 * i2 >= 3 * cus) return gemm3hk_launch<2>(a, i2, st);
    return gemm3hk_launch<1>(a, i1, st);
}
