// Token GEMM on the fp16 MFMA from two-plane operands:  out[m][n] = epilogue( sum_k A[m][k] * W[n][k] )   (nn.Linear layout)
// The opt-in "f16x2" eval arithmetic for the dense token products rpb_gemm3x runs on three bf16 planes: each
// operand is multiplied by an exact power of two and split into (hi, lo) fp16 planes, both rounded to nearest even (split8h of
// rpb_mma.h), and a product is accumulated in fp32 from three plane products, small terms first -- lo*hi, hi*lo, hi*hi (mma3h of
// rpb_mma.h); lo*lo (<= 2^-22 of the product) is dropped.  Half the matrix-pipe work of rpb_gemm3x for an fp32-grade result.
//
// Contract = rpb_gemm3x's, restricted to what an evaluation forward uses: A [M][lda] fp32 rows (may be a column range of a wider
// tensor), W [N][K] prepared once by rpb_gemm3h_wprep, out [M][ldo] (may be a column range); K % 64 == 0, 64 <= K <= 512; N = 64, 128
// or a multiple of 256; any M >= 1; lda, ldo % 4 == 0; epilogue = bias, act in {0 none, 3 ReLU}, residual.  No mask tensor, no dropout,
// no pre_out / aux: those belong to training, which this arithmetic never touches.
//
// Scales (fp16 has five exponent bits):
//   weights      ONE exponent ew per weight tensor by rpb_amax_exp's rule, max|W| 2^ew in [2^14, 2^15), capped at 62.  rpb_gemm3h_wprep
//                writes 2 N K fp16 in B-operand order and sc[0] = 2^-ew to device memory (sc[1] is its scratch word): no host read.
//   activations  ONE EXPONENT PER ROW, formed inside the GEMM launch.  Token rows are the MFMA rows here, so an A operand may carry a
//                scale per row and the row of the accumulator is rescaled once in the epilogue: out = acc * (2^-e_row 2^-ew) + bias --
//                the transpose of rpb_deeponet_h.hip's scale per point.  e_row comes from the EXACT maximum of the row's K values,
//                scaled into [2^14, 2^15), capped at 62; an all-zero row takes e = 0 (col_exp of rpb_mma.h).  A per-tensor scale would
//                not do: token rows of one tensor differ by many binades after the residual adds and a small row would lose its lo plane.
//
// How the row maximum is known before the row's first k-column is split: THE WHOLE 64-ROW x K TILE IS RESIDENT.  A thread holds 2 x K / 8
// fp32 values of two rows in registers (eight adjacent lanes share a row), so the maximum is a register reduction and three lane
// exchanges; the rows are then scaled, split and written to LDS as planes once ([2 planes][K / 8][64 rows + 2] x 16 B: 66 KB at K = 256,
// 132 KB at K = 512), and every column block of N is multiplied from the same planes -- the N = 768 Q|K|V product reads and splits A
// once, where rpb_gemm3x stages it once per 256 columns.  The other candidate (a maxima sweep over the next tile during the current
// tile's main loop, the staged reads hitting L2 afterwards) reads every A row twice and was not built, so its cost is not measured; this
// form adds no launch, no second pass over A and no host read.
//
// Organisation: persistent workgroups of four waves, tiles of 64 rows dealt round-robin; the NEXT tile's rows are requested into
// registers before the current tile's main loop and are split into LDS after its epilogue; B operands come from operand-ordered planes one
// k-step ahead; K <= 256 is built for two workgroups per CU (one splits / stores while the other multiplies), K <= 512 for one.  N = 64
// / 128 deal the four waves over 2 row halves x 2 column groups instead of splitting K, so every partial sum has one owner and a fixed
// order.  The epilogue runs from the accumulators: D register r of a lane is row mfma_row(lane, r), column lane & 31, so a store
// instruction writes two complete 128-byte row segments and the row factor is one LDS read per four registers; rpb_gemm3x's parked epilogue
// (wave-private LDS tiles, 16 B per lane) has no LDS left next to two resident tiles and was not measured against it.
// Measured on one MI355X against the default token GEMM on the same operands (tools/galerkin_probe.py, profiles/galerkin_arith_probe.txt;
// M = 2.6 M rows, K = 256, medians of 20 runs, two repeats, spread <= 0.010 ms): N = 768 with bias 6.358 -> 5.111 ms (1.244x; 605 TFLOP/s of
// issued fp16 MFMA = 0.39 of the sustained rate, 0.26 of 8 TB/s); N = 256 with bias + ReLU 2.064 -> 1.948 ms (1.060x); N = 256 with bias +
// residual 2.307 -> 4.696 ms -- SLOWER: the residual is read 4 bytes per lane inside the row guard, one dependent load-add-store chain per
// accumulator register; N = 128 plain 1.338 -> 1.691 ms -- SLOWER: 6 MFMAs per k-step for 2 LDS reads and 4 weight-operand loads.  The
// resident tile itself costs no extra pass over A; what two workgroups per CU against one, or the parked epilogue, would measure is open.
// GalerkinTransformer3d.set_arith("f16x2") therefore routes only its N = 768 and bias + ReLU products here.
//
// Fixed summation order, no atomics: two calls give the same bits.  Tail rows read row M - 1 and store nothing; nothing is written outside
// out[m][0..N) for m < M.  Non-finite inputs (A, W) are outside the contract: an exponent derived from Inf / NaN is meaningless and the
// output is then unspecified (finite or not), where rpb_gemm3x propagates them.
#include "rpb_mma.h"

extern "C" int rpb_amax_exp(const float* x, long M, int C, int ldx, int* e, void* stream);

#define G3H_BM 64
#define G3H_RS 66          // 16-byte units per 8-column group of a plane: 64 rows + 2 (the eight lanes of a row land in distinct banks)
#define G3H_KMAX 512

// ---------------------------------------------------------------------------------- weights in B-operand order
// W [N][K] fp32 -> Wz[K/16][2 planes][N/32][64 lanes][8] fp16 of W 2^ew, lane = (n & 31) + 32 * k-half, element e <-> k = 16 cc + 8 half + e;
// sc[1] holds rpb_amax_exp's exponent on entry, sc[0] receives 2^-ew
__global__ __launch_bounds__(256) void gemm3h_wprep_kernel(const float* __restrict__ W, uint16_t* __restrict__ Wz, float* sc, int N, int K) {
    const int NT = N >> 5, NCC = K >> 4;
    const long total = (long)NCC * NT * 64;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int ew = reinterpret_cast<const int*>(sc)[1];
    ew = ew > 62 ? 62 : ew;                                            // >= 14 - 127: 2^ew and 2^-ew are normal
    if (idx == 0) sc[0] = pow2f(-ew);
    if (idx >= total) return;
    const int lane = (int)(idx & 63);
    const long r = idx >> 6;
    const int nt = (int)(r % NT), cc = (int)(r / NT);
    const float* src = W + (long)(nt * 32 + (lane & 31)) * K + cc * 16 + (lane >> 5) * 8;
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
    const float s = pow2f(ew);
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        v[e] = v0[e] * s;
        v[4 + e] = v1[e] * s;
    }
    bf16x8 h, l;
    split8h<false>(v, h, l);
    const long dst = ((((long)cc * 2) * NT + nt) * 64 + lane) * 8;
    *reinterpret_cast<u32x4*>(Wz + dst) = __builtin_bit_cast(u32x4, h);
    *reinterpret_cast<u32x4*>(Wz + dst + (long)NT * 512) = __builtin_bit_cast(u32x4, l);
}

extern "C" int rpb_gemm3h_supported(long M, int N, int K, int lda, int ldo) {
    return M >= 1 && K >= 64 && K <= G3H_KMAX && K % 64 == 0 && (N == 64 || N == 128 || (N > 0 && N % 256 == 0)) && lda % 4 == 0 && lda >= K &&
           ldo % 4 == 0 && ldo >= N;
}

extern "C" int rpb_gemm3h_wprep(const float* W, void* Wz, float* sc, int N, int K, void* stream) {
    RPB_REQUIRE(W && Wz && sc && N > 0 && N % 32 == 0 && K > 0 && K % 16 == 0, "gemm3h_wprep: N=%d K=%d unsupported", N, K);
    const int rc = rpb_amax_exp(W, N, K, K, reinterpret_cast<int*>(sc) + 1, stream);
    if (rc != RPB_OK) return rc;
    const long total = (long)(K / 16) * (N / 32) * 64;
    hipLaunchKernelGGL(gemm3h_wprep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, W, (uint16_t*)Wz, sc, N, K);
    RPB_CHECK_LAUNCH("gemm3h_wprep");
}

// ---------------------------------------------------------------------------------- the GEMM
struct Gemm3hArgs {
    const float* A;        // [M][lda] fp32
    const uint16_t* Wz;    // operand-ordered (hi, lo) planes of W[N][K] 2^ew
    const float* sc;       // sc[0] = 2^-ew
    const float* bias;     // [N] or null
    const float* residual; // [M][ldo] or null
    float* out;            // [M][ldo]
    long M;
    int N, K, lda, ldo;
    int act;               // 0 none, 3 ReLU
};

// WR: row halves the four waves are dealt over (1: a wave owns 64 rows x 32 TN columns; 2: 32 rows); TN: 32-column tiles per wave;
// NS: 64-column stages a thread can hold (K <= 64 NS)
template <int WR, int TN, int NS>
__global__ __launch_bounds__(256, NS <= 4 ? 2 : 1) void gemm3h_kernel(Gemm3hArgs a) {
    constexpr int WC = 4 / WR, TM = 2 / WR, BN = WC * 32 * TN;
    extern __shared__ u32x4 lds4[];                                    // [2 planes][K / 8][G3H_RS] x 16 B, then 64 row factors
    const int tid = threadIdx.x, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WC, wc = wave % WC;
    const int nk8 = a.K >> 3, nks = a.K >> 4, nc64 = a.K >> 6;
    u32x4* const P0 = lds4;
    u32x4* const P1 = lds4 + nk8 * G3H_RS;
    float* const rowfac = reinterpret_cast<float*>(lds4 + 2 * nk8 * G3H_RS);
    const long ntiles = (a.M + G3H_BM - 1) / G3H_BM;
    long tile = blockIdx.x;
    if (tile >= ntiles) return;
    const float wsc = a.sc[0];
    const int NT = a.N >> 5;
    const long wplane = (long)NT * 512, wstep = 2 * wplane;

    // ---- A staging: a thread owns columns 64 c + 8 sh .. + 8 (c < K / 64) of rows r0 and r0 + 32; the eight lanes of a row are adjacent
    const int r0 = tid >> 3, sh = tid & 7;
    f32x4 sa[NS][2], sb[NS][2];
    auto tile_load = [&](long m0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long row = m0 + r0 + 32 * j;
            const float* src = a.A + (row < a.M ? row : a.M - 1) * a.lda + sh * 8;      // tail: a valid row is read, nothing is stored
#pragma unroll
            for (int c = 0; c < NS; ++c)
                if (c < nc64) {
                    sa[c][j] = *reinterpret_cast<const f32x4*>(src + c * 64);
                    sb[c][j] = *reinterpret_cast<const f32x4*>(src + c * 64 + 4);
                }
        }
    };
    // the exact row maximum -> the row's exponent; the scaled row as planes in LDS, the factor that undoes both scales next to them
    auto tile_store = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float m = 0.f;
#pragma unroll
            for (int c = 0; c < NS; ++c)
                if (c < nc64) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) m = fmaxf(m, fmaxf(fabsf(sa[c][j][e]), fabsf(sb[c][j][e])));
                }
            m = fmaxf(m, __shfl_xor(m, 1, 64));
            m = fmaxf(m, __shfl_xor(m, 2, 64));
            m = fmaxf(m, __shfl_xor(m, 4, 64));
            const int ex = col_exp<14>(m);
            const float s = pow2f(ex);
            const int row = r0 + 32 * j;
            if (sh == 0) rowfac[row] = pow2f(-ex) * wsc;               // both >= 2^-62: the product is normal
#pragma unroll
            for (int c = 0; c < NS; ++c)
                if (c < nc64) {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[e] = sa[c][j][e] * s;
                        v[4 + e] = sb[c][j][e] * s;
                    }
                    bf16x8 h, l;
                    split8h<false>(v, h, l);
                    P0[(c * 8 + sh) * G3H_RS + row] = __builtin_bit_cast(u32x4, h);
                    P1[(c * 8 + sh) * G3H_RS + row] = __builtin_bit_cast(u32x4, l);
                }
        }
    };

    // ---- operands of one k-step (16 columns): A from the resident planes, B from the operand-ordered weight planes
    const uint16_t* wbase = a.Wz;
    auto lda_ = [&](int ks, u32x4 (&av)[TM][2]) __attribute__((always_inline)) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            const int o = (2 * ks + half) * G3H_RS + (wr * TM + tm) * 32 + col;
            av[tm][0] = P0[o];
            av[tm][1] = P1[o];
        }
    };
    auto ldb_ = [&](int ks, u32x4 (&bv)[TN][2]) __attribute__((always_inline)) {
        const uint16_t* src = wbase + (long)ks * wstep;
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int p = 0; p < 2; ++p) bv[tn][p] = *reinterpret_cast<const u32x4*>(src + p * wplane + tn * 512);
    };

    tile_load(tile * G3H_BM);
    for (; tile < ntiles; tile += gridDim.x) {
        const long m0 = tile * G3H_BM;
        tile_store();
        __syncthreads();
        if (tile + gridDim.x < ntiles) tile_load((tile + gridDim.x) * G3H_BM);     // lands during the main loops below
        for (int nb = 0; nb < a.N / BN; ++nb) {
            const int n0 = nb * BN + wc * (32 * TN);
            wbase = a.Wz + ((long)(n0 >> 5) * 64 + lane) * 8;
            f32x16 acc[TM][TN];
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = zero16();
            u32x4 ac[TM][2], bc[TN][2], an[TM][2], bn[TN][2];
            lda_(0, ac);
            ldb_(0, bc);
            for (int ks = 0; ks < nks; ++ks) {
                const int kn = ks + 1 < nks ? ks + 1 : ks;             // the last step requests its own operands again: in bounds, unused
                lda_(kn, an);
                ldb_(kn, bn);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int tn = 0; tn < TN; ++tn) acc[tm][tn] = mma3h(ac[tm], bc[tn], acc[tm][tn]);
#pragma unroll
                for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                    for (int p = 0; p < 2; ++p) ac[tm][p] = an[tm][p];
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
#pragma unroll
                    for (int p = 0; p < 2; ++p) bc[tn][p] = bn[tn][p];
            }
            // ---- epilogue from the accumulators: register r of a lane = row mfma_row(lane, r), column lane & 31
            //      (offsets within the tile are 32-bit: 64 rows x ldo)
            float* const outT = a.out + m0 * a.ldo;
            const float* const resT = a.residual ? a.residual + m0 * a.ldo : nullptr;
            const int nrows = a.M - m0 < G3H_BM ? (int)(a.M - m0) : G3H_BM;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) {
                const int rb = (wr * TM + tm) * 32 + 4 * half;
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const int n = n0 + tn * 32 + col;
                    const float bv = a.bias ? a.bias[n] : 0.f;
                    const int o0 = rb * a.ldo + n;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x4 fq = *reinterpret_cast<const f32x4*>(rowfac + rb + 8 * q);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if (rb + 8 * q + e < nrows) {
                                const int o = o0 + (8 * q + e) * a.ldo;
                                float v = fmaf(acc[tm][tn][4 * q + e], fq[e], bv);
                                if (a.act == 3) v = fmaxf(v, 0.f);
                                if (resT) v += resT[o];
                                outT[o] = v;
                            }
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();                                               // the planes are free for the next tile
    }
}

template <int WR, int TN, int NS>
static int gemm3h_launch(const Gemm3hArgs& a, hipStream_t st) {
    const size_t lds = (size_t)2 * (a.K / 8) * G3H_RS * 16 + G3H_BM * sizeof(float);
    if (hipFuncSetAttribute((const void*)gemm3h_kernel<WR, TN, NS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        RPB_FAIL(RPB_ERR_LAUNCH, "gemm3h: %zu bytes of LDS refused", lds);
    long gx = (a.M + G3H_BM - 1) / G3H_BM;
    const long cap = (long)rpb_num_cus() * (NS <= 4 ? 2 : 1);
    if (gx > cap) gx = cap < 1 ? 1 : cap;
    hipLaunchKernelGGL((gemm3h_kernel<WR, TN, NS>), dim3((unsigned)gx), dim3(256), lds, st, a);
    RPB_CHECK_LAUNCH("gemm3h");
}

extern "C" int rpb_gemm3h(const float* A, const void* Wz, const float* sc, const float* bias, const float* residual, float* out, long M,
                          int N, int K, int lda, int ldo, int act, void* stream) {
    RPB_REQUIRE(A && Wz && sc && out && M > 0, "gemm3h: bad arguments");
    RPB_REQUIRE(rpb_gemm3h_supported(M, N, K, lda, ldo),
                "gemm3h: N=%d K=%d lda=%d ldo=%d unsupported (K %% 64, 64 <= K <= %d; N = 64, 128 or a multiple of 256; leading dimensions %% 4)",
                N, K, lda, ldo, G3H_KMAX);
    RPB_REQUIRE(act == 0 || act == 3, "gemm3h: act=%d unsupported (0 none, 3 ReLU; masks, dropout, pre_out / aux belong to training)", act);
    const Gemm3hArgs a{A, (const uint16_t*)Wz, sc, bias, residual, out, M, N, K, lda, ldo, act};
    hipStream_t st = (hipStream_t)stream;
    const bool small = K <= 256;
    if (N == 64) return small ? gemm3h_launch<2, 1, 4>(a, st) : gemm3h_launch<2, 1, 8>(a, st);
    if (N == 128) return small ? gemm3h_launch<2, 2, 4>(a, st) : gemm3h_launch<2, 2, 8>(a, st);
    return small ? gemm3h_launch<1, 2, 4>(a, st) : gemm3h_launch<1, 2, 8>(a, st);
}
