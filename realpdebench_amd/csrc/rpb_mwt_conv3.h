// The 3x3x3 convolution at 36 channels of MWT3d on v_mfma_f32_16x16x4_f32: ONE kernel text for the evaluation forward (rpb_mwt.hip), its
// training variant that also keeps z = ReLU(conv(x) + b), and the data gradient of the training step (rpb_mwt_train.hip), which is the
// same main loop on flipped, transposed taps with an empty epilogue.
//
// One wave = 64 consecutive cells = 4 column tiles of the instruction; rows = output channel (3 tiles, 36 of 48 used).
// Operand maps of the instruction: A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15], D register r = D[row = 4 (l >> 4) + r][col = l & 15].
// K = 27 taps x 36 input channels; inside a tap the k index of step j, lane group g = l >> 4 is input channel 9 g + j, so a lane reads 9
// consecutive floats of its neighbour cell per tap.  wp [27][9][3][64]: the A operand in lane order (rpb_mwt_conv3_wprep).
// The ReLU'd accumulator tile is the B operand of the second product as it stands: register r of row tile t on lane group g is hidden
// channel 16 t + 4 g + r, which is the k index that lop [3 t][4 r][3 u][64] pairs it with.
#pragma once
#include "rpb_common.h"

#define MWT_C 36       // c * k^2

typedef float mwt4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ mwt4 mwt_mfma(float a, float b, mwt4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

#define MWT_CONV_EVAL 0    // out (+)= Lo ReLU(conv(x) + cb) + lb
#define MWT_CONV_KEEP 1    // the same, and z [cell][36] = ReLU(conv(x) + cb)
#define MWT_CONV_PLAIN 2   // out (+)= conv(x): no bias, no ReLU, no Lo (cb, lop, lb, z unused)

template <int MODE>
__global__ __launch_bounds__(256) void mwt_conv3_k(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ cb,
                                                   const float* __restrict__ lop, const float* __restrict__ lb, float* __restrict__ out,
                                                   float* __restrict__ z, long ncell, int Nx, int Ny, int T, int accumulate) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane >> 4, cl = lane & 15;
    const long base = (blockIdx.x * 4L + wave) * 64;
    if (base >= ncell) return;                       // wave-uniform
    long cq[4];
    int cx[4], cy[4], ct[4];
    bool cv[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const long q = base + n * 16 + cl;
        cv[n] = q < ncell;
        cq[n] = cv[n] ? q : ncell - 1;
        long r = cq[n];
        ct[n] = (int)(r % T);
        r /= T;
        cy[n] = (int)(r % Ny);
        r /= Ny;
        cx[n] = (int)(r % Nx);
    }
    mwt4 acc[3][4];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[t][n] = mwt4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tap = 0; tap < 27; ++tap) {
        const int dx = tap / 9 - 1, dy = (tap / 3) % 3 - 1, dt = tap % 3 - 1;
        float bv[4][9];
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const bool ok = cv[n] && (unsigned)(cx[n] + dx) < (unsigned)Nx && (unsigned)(cy[n] + dy) < (unsigned)Ny &&
                            (unsigned)(ct[n] + dt) < (unsigned)T;
            // a neighbour inside the grid is inside the same sample; everything else reads cell 0 and is replaced by the zero pad
            const float* p = x + (ok ? (cq[n] + ((long)dx * Ny + dy) * T + dt) * MWT_C : 0L) + 9 * g;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const float v = p[j];
                bv[n][j] = ok ? v : 0.f;
            }
        }
        const float* wt = wp + (long)tap * 9 * 3 * 64 + lane;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            float a[3];
#pragma unroll
            for (int t = 0; t < 3; ++t) a[t] = wt[(j * 3 + t) * 64];
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[t][n] = mwt_mfma(a[t], bv[n][j], acc[t][n]);
        }
    }
    if constexpr (MODE == MWT_CONV_PLAIN) {          // the rows 16 t + 4 g + r of the accumulator leave as they are
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int o0 = 16 * t + 4 * g;
            if (o0 >= MWT_C) continue;               // rows 36..47 are padding
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                if (!cv[n]) continue;
                mwt4* dst = reinterpret_cast<mwt4*>(out + cq[n] * MWT_C + o0);
                mwt4 v = acc[t][n];
                if (accumulate) v += *dst;
                *dst = v;
            }
        }
        return;
    }
    // bias + ReLU on the rows 16 t + 4 g + r (cb is padded to 48 with zeros, so the pad rows stay 0)
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const mwt4 b4 = *reinterpret_cast<const mwt4*>(cb + 16 * t + 4 * g);
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[t][n][r] = fmaxf(acc[t][n][r] + b4[r], 0.f);
    }
    if constexpr (MODE == MWT_CONV_KEEP) {
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int o0 = 16 * t + 4 * g;
            if (o0 >= MWT_C) continue;
#pragma unroll
            for (int n = 0; n < 4; ++n)
                if (cv[n]) *reinterpret_cast<mwt4*>(z + cq[n] * MWT_C + o0) = acc[t][n];
        }
    }
    mwt4 o2[3][4];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
        for (int n = 0; n < 4; ++n) o2[u][n] = mwt4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const float a2 = lop[((t * 4 + r) * 3 + u) * 64 + lane];
#pragma unroll
                for (int n = 0; n < 4; ++n) o2[u][n] = mwt_mfma(a2, acc[t][n][r], o2[u][n]);
            }
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int o0 = 16 * u + 4 * g;
        if (o0 >= MWT_C) continue;                   // rows 36..47 are padding
        const mwt4 b4 = *reinterpret_cast<const mwt4*>(lb + o0);
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (!cv[n]) continue;
            mwt4* dst = reinterpret_cast<mwt4*>(out + cq[n] * MWT_C + o0);
            mwt4 v = o2[u][n] + b4;
            if (accumulate) v += *dst;
            *dst = v;
        }
    }
}

// last inverse stage of sparseKernelFT3d (c2r along T) + ReLU + Lo (+=): S [lines][K2 = 2 * kept T modes][36], GT [T][K2],
// loT [36 in][36 out], lb [36] -> out [lines * T][36]; KEEP: and rv [lines * T][36] = ReLU(v)
#define MWT_SO_CELLS 7
template <bool KEEP>
__global__ __launch_bounds__(MWT_SO_CELLS* MWT_C) void mwt_spec_out_k(const float* __restrict__ S, const float* __restrict__ GT,
                                                                      const float* __restrict__ loT, const float* __restrict__ lb,
                                                                      float* __restrict__ out, float* __restrict__ rv, long ncell, int T,
                                                                      int K2, int accumulate) {
    __shared__ float v[MWT_SO_CELLS][MWT_C];
    const int cl = threadIdx.x / MWT_C, c = threadIdx.x % MWT_C;
    const long q = blockIdx.x * (long)MWT_SO_CELLS + cl;
    const bool ok = q < ncell;
    float a = 0.f;
    if (ok) {
        const long line = q / T;
        const int t = (int)(q % T);
        for (int k = 0; k < K2; ++k) a = fmaf(GT[t * K2 + k], S[(line * K2 + k) * MWT_C + c], a);
    }
    v[cl][c] = fmaxf(a, 0.f);
    if constexpr (KEEP)
        if (ok) rv[q * MWT_C + c] = v[cl][c];
    __syncthreads();
    if (!ok) return;
    float acc = lb[c];
#pragma unroll
    for (int k = 0; k < MWT_C; ++k) acc = fmaf(v[cl][k], loT[k * MWT_C + c], acc);
    if (accumulate) acc += out[q * MWT_C + c];
    out[q * MWT_C + c] = acc;
}
