// MWT3d (multiwavelet operator) -- the kernels of the opt-in training step (MWT3d.enable_training()).
// The adjoints of the wavelet maps and of the truncated-DFT stages are the forward's own launches on transposed tables (rpb_mwt_decompose,
// rpb_mwt_reconstruct, rpb_mwt_axis); this file holds what the forward's fusion forces:
//   the two keep-variants of the fused forwards (the kernel texts of rpb_mwt_conv3.h with one more store),
//   lo_bwd      g_z = (g_out Lo) [z > 0] and the partials of dLo, dlb            (shared by A, B and C)
//   conv3_dgrad the main loop of rpb_mwt_conv3 on flipped, transposed taps, empty epilogue
//   conv3_wgrad dW[o][i][tap] = sum_cells g_z[cell][o] x[cell + tap][i], db, on v_mfma_f32_16x16x4_f32, K = cells, split-cell partials
//   modes_bwd   g_X = g_Y W^H per retained bin and dW[tab[bin]] += X^H-pairing of X and g_Y
//   head_bwd    recomputes ReLU(Lc0 x + b0); g_x and the partials of dLc0, dLc1 and both biases
//   lift_wgrad  the partials of dLk, db
// Activations are channels-last fp32 [B][Nx][Ny][T][36].  No kernel uses atomics and every sum has a fixed order: two backward passes give
// bit-equal gradients.  Partials are finished by rpb_reduce_partials (fp64).
#include "rpb_common.h"
#include "rpb_mwt_conv3.h"

#define MWT_HID 128
#define MWT_STREAM (static_cast<hipStream_t>(stream))

static inline unsigned mwtt_blocks(long n, long per) { return (unsigned)((n + per - 1) / per); }
static inline int mwtt_rows(long tiles, int cap) { return (int)(tiles < 1 ? 1 : (tiles < cap ? tiles : cap)); }

// ---------------------------------------------------------------------------------- lo_bwd
// gout, z, gz [ncell][36]; lo [36 out][36 in] (Linear.weight); part [gridDim.x][36 * 36 + 36] = (dLo[o][c] = sum gout[o] z[c] | dlb[o])
#define MWT_LO_TILE 64
#define MWT_LO_L (MWT_C * MWT_C + MWT_C)
__global__ __launch_bounds__(256) void mwt_lo_bwd_k(const float* __restrict__ gout, const float* __restrict__ z, const float* __restrict__ lo,
                                                    float* __restrict__ gz, float* __restrict__ part, long ncell) {
    __shared__ float sg[MWT_LO_TILE][MWT_C + 1], sz[MWT_LO_TILE][MWT_C + 1], sl[MWT_C * MWT_C];
    const int tid = threadIdx.x;
    for (int i = tid; i < MWT_C * MWT_C; i += 256) sl[i] = lo[i];
    float acc[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = 0.f;
    for (long q0 = blockIdx.x * (long)MWT_LO_TILE; q0 < ncell; q0 += gridDim.x * (long)MWT_LO_TILE) {     // block-uniform trip count
        for (int i = tid; i < MWT_LO_TILE * MWT_C; i += 256) {
            const int cell = i / MWT_C, c = i % MWT_C;
            const long q = q0 + cell;
            const bool ok = q < ncell;
            sg[cell][c] = ok ? gout[q * MWT_C + c] : 0.f;
            sz[cell][c] = ok ? z[q * MWT_C + c] : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < MWT_LO_TILE * MWT_C; i += 256) {
            const int cell = i / MWT_C, c = i % MWT_C;
            const long q = q0 + cell;
            if (q < ncell) {
                float s = 0.f;
#pragma unroll
                for (int o = 0; o < MWT_C; ++o) s = fmaf(sg[cell][o], sl[o * MWT_C + c], s);
                gz[q * MWT_C + c] = sz[cell][c] > 0.f ? s : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int e = tid + 256 * k;
            if (e < MWT_C * MWT_C) {
                const int o = e / MWT_C, c = e % MWT_C;
                float s = acc[k];
                for (int cell = 0; cell < MWT_LO_TILE; ++cell) s = fmaf(sg[cell][o], sz[cell][c], s);
                acc[k] = s;
            } else if (e < MWT_LO_L) {
                const int o = e - MWT_C * MWT_C;
                float s = acc[k];
                for (int cell = 0; cell < MWT_LO_TILE; ++cell) s += sg[cell][o];
                acc[k] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int e = tid + 256 * k;
        if (e < MWT_LO_L) part[(long)blockIdx.x * MWT_LO_L + e] = acc[k];
    }
}

// ---------------------------------------------------------------------------------- conv3_wgrad
// g, x [ncell][36] on the (Nx, Ny, T) mesh of every sample.  blockIdx.y = tap, blockIdx.x = split (cells [split * chunk, (split + 1) * chunk),
// chunk % 16 == 0).  One K step of the instruction = 4 consecutive cells: A[row = o][k] = g[cell k][o], B[k][col = i] = x[cell k + tap][i]
// (zero outside the sample); column 36 of the B operand is 1 on valid cells, so D[o][36] = db[o] (stored by tap 0 only).  The four waves
// of a block take K steps round-robin and are added in wave order through LDS.
// part [splits][36 * 36 * 27 + 36] in the layout of (Conv3d.weight [o][i][tap] | bias).
#define MWT_WG_L (MWT_C * MWT_C * 27 + MWT_C)
__global__ __launch_bounds__(256) void mwt_conv3_wgrad_k(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ part,
                                                         long ncell, long chunk, int Nx, int Ny, int T) {
    __shared__ float red[4][9][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int kk = lane >> 4, cl = lane & 15;
    const int tap = blockIdx.y;
    const int dx = tap / 9 - 1, dy = (tap / 3) % 3 - 1, dt = tap % 3 - 1;
    const long c0 = blockIdx.x * chunk;
    const long c1 = c0 + chunk < ncell ? c0 + chunk : ncell;
    mwt4 acc[3][3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int u = 0; u < 3; ++u) acc[t][u] = mwt4{0.f, 0.f, 0.f, 0.f};
    for (long q0 = c0 + wave * 4; q0 < c1; q0 += 16) {                 // wave-uniform
        const long q = q0 + kk;
        const bool valid = q < c1;
        const long qs = valid ? q : c0;                                // a safe cell to read
        long rr = qs;
        const int ct = (int)(rr % T);
        rr /= T;
        const int cy = (int)(rr % Ny);
        rr /= Ny;
        const int cx = (int)(rr % Nx);
        const bool ok = valid && (unsigned)(cx + dx) < (unsigned)Nx && (unsigned)(cy + dy) < (unsigned)Ny && (unsigned)(ct + dt) < (unsigned)T;
        const float* gp = g + qs * MWT_C;
        const float* xp = x + (ok ? qs + ((long)dx * Ny + dy) * T + dt : qs) * MWT_C;
        float a[3], b[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int ch = 16 * t + cl;
            const float ga = gp[ch < MWT_C ? ch : 0], xb = xp[ch < MWT_C ? ch : 0];
            a[t] = (valid && ch < MWT_C) ? ga : 0.f;
            b[t] = (ok && ch < MWT_C) ? xb : 0.f;
        }
        if (cl == 4) b[2] = valid ? 1.f : 0.f;                          // channel 36: the ones column
#pragma unroll
        for (int t = 0; t < 3; ++t)
#pragma unroll
            for (int u = 0; u < 3; ++u) acc[t][u] = mwt_mfma(a[t], b[u], acc[t][u]);
    }
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wave][t * 3 + u][r][lane] = acc[t][u][r];
    __syncthreads();
    float* dst = part + (long)blockIdx.x * MWT_WG_L;
    for (int e = threadIdx.x; e < 9 * 4 * 64; e += 256) {
        const int l = e & 63, r = (e >> 6) & 3, tile = e >> 8;
        const float s = ((red[0][tile][r][l] + red[1][tile][r][l]) + red[2][tile][r][l]) + red[3][tile][r][l];
        const int o = 16 * (tile / 3) + 4 * (l >> 4) + r, i = 16 * (tile % 3) + (l & 15);
        if (o < MWT_C && i < MWT_C) dst[(o * MWT_C + i) * 27 + tap] = s;
        if (o < MWT_C && i == MWT_C && tap == 0) dst[MWT_C * MWT_C * 27 + o] = s;
    }
}

// ---------------------------------------------------------------------------------- modes_bwd
// X, gY, gX [B][2 (re|im)][NB][36]; Wt, dWt [weight bins][36 in][36 out][2]; one block per retained bin.  tab is injective inside a level,
// so a weight bin has one writer per launch; dWt += (levels accumulate in launch order).
#define MWT_MB_CHUNK 8
__global__ __launch_bounds__(256) void mwt_modes_bwd_k(const float* __restrict__ X, const float* __restrict__ gY, const float* __restrict__ Wt,
                                                       const int* __restrict__ tab, float* __restrict__ gX, float* __restrict__ dWt, int B,
                                                       int NB) {
    __shared__ float sx[MWT_MB_CHUNK][2][MWT_C], sy[MWT_MB_CHUNK][2][MWT_C];
    const int tid = threadIdx.x, bin = blockIdx.x;
    const float* w = Wt + (long)tab[bin] * MWT_C * MWT_C * 2;
    float ar[6], ai[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) ar[k] = ai[k] = 0.f;
    for (int b0 = 0; b0 < B; b0 += MWT_MB_CHUNK) {
        const int nb = B - b0 < MWT_MB_CHUNK ? B - b0 : MWT_MB_CHUNK;
        for (int i = tid; i < MWT_MB_CHUNK * 2 * MWT_C; i += 256) {
            const int b = i / (2 * MWT_C), p = (i / MWT_C) & 1, c = i % MWT_C;
            const bool ok = b < nb;
            const long idx = ok ? ((((long)(b0 + b) * 2 + p) * NB + bin) * MWT_C + c) : 0L;
            const float xv = X[idx], yv = gY[idx];
            sx[b][p][c] = ok ? xv : 0.f;
            sy[b][p][c] = ok ? yv : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < nb * MWT_C; i += 256) {
            const int b = i / MWT_C, c = i % MWT_C;
            float gr = 0.f, gi = 0.f;
            for (int o = 0; o < MWT_C; ++o) {
                const float wr = w[(c * MWT_C + o) * 2], wi = w[(c * MWT_C + o) * 2 + 1];
                const float yr = sy[b][0][o], yi = sy[b][1][o];
                gr = fmaf(yr, wr, gr);
                gr = fmaf(yi, wi, gr);
                gi = fmaf(yi, wr, gi);
                gi = fmaf(-yr, wi, gi);
            }
            gX[(((long)(b0 + b) * 2 + 0) * NB + bin) * MWT_C + c] = gr;
            gX[(((long)(b0 + b) * 2 + 1) * NB + bin) * MWT_C + c] = gi;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int e = tid + 256 * k;
            if (e < MWT_C * MWT_C) {
                const int i = e / MWT_C, o = e % MWT_C;
                float sr = ar[k], si = ai[k];
#pragma unroll
                for (int b = 0; b < MWT_MB_CHUNK; ++b) {                // samples past nb are zeros
                    const float xa = sx[b][0][i], xb = sx[b][1][i], yr = sy[b][0][o], yi = sy[b][1][o];
                    sr = fmaf(xa, yr, sr);
                    sr = fmaf(xb, yi, sr);
                    si = fmaf(xa, yi, si);
                    si = fmaf(-xb, yr, si);
                }
                ar[k] = sr;
                ai[k] = si;
            }
        }
        __syncthreads();
    }
    float* dst = dWt + (long)tab[bin] * MWT_C * MWT_C * 2;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int e = tid + 256 * k;
        if (e < MWT_C * MWT_C) {
            dst[2 * e] += ar[k];
            dst[2 * e + 1] += ai[k];
        }
    }
}

// ---------------------------------------------------------------------------------- head_bwd
// x, gx [ncell][36]; gout [B][T r][Nx][Ny][Cout]; w0t [36][128]; w1 [dout = Cout r][128], dout <= 16.  Thread (h = tid & 127, half = tid >> 7)
// owns hidden unit h on every second cell of a 16-cell tile; each half is one partial row:
// part [2 gridDim.x][dout * 128 + dout + 128 * 36 + 128] = (dLc1 [dout][128] | db1 | dLc0 [128][36] | db0)
#define MWT_HB_CELLS 16
#define MWT_HB_DMAX 16
__global__ __launch_bounds__(256) void mwt_head_bwd_k(const float* __restrict__ x, const float* __restrict__ gout, const float* __restrict__ w0t,
                                                      const float* __restrict__ b0, const float* __restrict__ w1, float* __restrict__ gx,
                                                      float* __restrict__ part, long ncell, int Nx, int Ny, int T, int Cout, int r) {
    __shared__ float xin[MWT_HB_CELLS][MWT_C], gy[MWT_HB_CELLS][MWT_HB_DMAX];
    __shared__ float ghs[MWT_HB_CELLS][MWT_HID + 1];
    const int tid = threadIdx.x, h = tid & 127, half = tid >> 7;
    const int dout = Cout * r;
    float w0[MWT_C], w1r[MWT_HB_DMAX], a0[MWT_C], a1[MWT_HB_DMAX];
#pragma unroll
    for (int c = 0; c < MWT_C; ++c) {
        w0[c] = w0t[c * MWT_HID + h];
        a0[c] = 0.f;
    }
#pragma unroll
    for (int od = 0; od < MWT_HB_DMAX; ++od) {
        w1r[od] = od < dout ? w1[od * MWT_HID + h] : 0.f;
        a1[od] = 0.f;
    }
    const float bh = b0[h];
    float ab0 = 0.f, ab1 = 0.f;
    for (long g0 = blockIdx.x * (long)MWT_HB_CELLS; g0 < ncell; g0 += gridDim.x * (long)MWT_HB_CELLS) {   // block-uniform trip count
        for (int i = tid; i < MWT_HB_CELLS * MWT_C; i += 256) {
            const long q = g0 + i / MWT_C;
            xin[i / MWT_C][i % MWT_C] = q < ncell ? x[q * MWT_C + i % MWT_C] : 0.f;
        }
        {
            const int ci = tid >> 4, od = tid & 15;
            long q = g0 + ci;
            float v = 0.f;
            if (q < ncell && od < dout) {
                const int t = (int)(q % T);
                q /= T;
                const int y = (int)(q % Ny);
                q /= Ny;
                const int xx = (int)(q % Nx);
                const long bb = q / Nx;
                const int co = od / r, j = od % r;
                v = gout[(((bb * T * r + (long)t * r + j) * Nx + xx) * Ny + y) * Cout + co];
            }
            gy[ci][od] = v;
        }
        __syncthreads();
        for (int ci = half; ci < MWT_HB_CELLS; ci += 2) {
            float acc = bh;
#pragma unroll
            for (int c = 0; c < MWT_C; ++c) acc = fmaf(w0[c], xin[ci][c], acc);
            const float hv = fmaxf(acc, 0.f);
            float gh = 0.f;
#pragma unroll
            for (int od = 0; od < MWT_HB_DMAX; ++od) {
                const float gv = gy[ci][od];                           // zero past dout and past the last cell
                gh = fmaf(gv, w1r[od], gh);
                a1[od] = fmaf(gv, hv, a1[od]);
            }
            gh = hv > 0.f ? gh : 0.f;
            ghs[ci][h] = gh;
            ab0 += gh;
#pragma unroll
            for (int c = 0; c < MWT_C; ++c) a0[c] = fmaf(gh, xin[ci][c], a0[c]);
            if (h < MWT_HB_DMAX) ab1 += gy[ci][h];
        }
        __syncthreads();
        {
            const int ci = tid >> 4, l16 = tid & 15;
            const long q = g0 + ci;
            if (q < ncell)
                for (int c = l16; c < MWT_C; c += 16) {
                    float s = 0.f;
                    for (int k = 0; k < MWT_HID; ++k) s = fmaf(ghs[ci][k], w0t[c * MWT_HID + k], s);
                    gx[q * MWT_C + c] = s;
                }
        }
        __syncthreads();
    }
    const long L = (long)dout * MWT_HID + dout + MWT_HID * MWT_C + MWT_HID;
    float* p = part + (blockIdx.x * 2L + half) * L;
#pragma unroll
    for (int od = 0; od < MWT_HB_DMAX; ++od)
        if (od < dout) p[od * MWT_HID + h] = a1[od];
    if (h < dout) p[dout * MWT_HID + h] = ab1;
#pragma unroll
    for (int c = 0; c < MWT_C; ++c) p[dout * MWT_HID + dout + h * MWT_C + c] = a0[c];
    p[dout * MWT_HID + dout + MWT_HID * MWT_C + h] = ab0;
}

// ---------------------------------------------------------------------------------- lift_wgrad
// g [B][H][W][T][36], x [B][T][H][W][Cin], Cin <= 64; part [gridDim.x][36 * Cin + 36] = (dLk [36][Cin] | db)
#define MWT_LW_TILE 64
__global__ __launch_bounds__(256) void mwt_lift_wgrad_k(const float* __restrict__ g, const float* __restrict__ x, float* __restrict__ part,
                                                        long ncell, int T, int H, int W, int Cin) {
    __shared__ float sg[MWT_LW_TILE][MWT_C + 1], sx[MWT_LW_TILE][65];
    const int tid = threadIdx.x;
    const int NW = MWT_C * Cin, L = NW + MWT_C;
    float acc[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc[k] = 0.f;
    for (long q0 = blockIdx.x * (long)MWT_LW_TILE; q0 < ncell; q0 += gridDim.x * (long)MWT_LW_TILE) {     // block-uniform trip count
        for (int i = tid; i < MWT_LW_TILE * MWT_C; i += 256) {
            const long q = q0 + i / MWT_C;
            sg[i / MWT_C][i % MWT_C] = q < ncell ? g[q * MWT_C + i % MWT_C] : 0.f;
        }
        for (int i = tid; i < MWT_LW_TILE * Cin; i += 256) {
            const int cell = i / Cin, c = i % Cin;
            long q = q0 + cell;
            float v = 0.f;
            if (q < ncell) {
                const int t = (int)(q % T);
                q /= T;
                const int yw = (int)(q % W);
                q /= W;
                const int xh = (int)(q % H);
                const long bb = q / H;
                v = x[(((bb * T + t) * H + xh) * W + yw) * Cin + c];
            }
            sx[cell][c] = v;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const int e = tid + 256 * k;
            if (e < NW) {
                const int o = e / Cin, c = e % Cin;
                float s = acc[k];
                for (int cell = 0; cell < MWT_LW_TILE; ++cell) s = fmaf(sg[cell][o], sx[cell][c], s);
                acc[k] = s;
            } else if (e < L) {
                const int o = e - NW;
                float s = acc[k];
                for (int cell = 0; cell < MWT_LW_TILE; ++cell) s += sg[cell][o];
                acc[k] = s;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const int e = tid + 256 * k;
        if (e < L) part[(long)blockIdx.x * L + e] = acc[k];
    }
}

// ================================================================================== C ABI
extern "C" int rpb_mwt_conv3_keep(const float* x, const float* wp, const float* cb48, const float* lop, const float* lb, float* out, float* z,
                                  int B, int Nx, int Ny, int T, int accumulate, void* stream) {
    RPB_REQUIRE(x && wp && cb48 && lop && lb && out && z, "rpb_mwt_conv3_keep: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0, "rpb_mwt_conv3_keep: bad shape B=%d Nx=%d Ny=%d T=%d", B, Nx, Ny, T);
    RPB_REQUIRE(x != out && x != z && out != z, "rpb_mwt_conv3_keep: x, out and z must be three tensors");
    const long ncell = (long)B * Nx * Ny * T;
    hipLaunchKernelGGL(mwt_conv3_k<MWT_CONV_KEEP>, dim3(mwtt_blocks(ncell, 256)), dim3(256), 0, MWT_STREAM, x, wp, cb48, lop, lb, out, z,
                       ncell, Nx, Ny, T, accumulate);
    RPB_CHECK_LAUNCH("rpb_mwt_conv3_keep");
}

extern "C" int rpb_mwt_spec_out_keep(const float* S, const float* GT, const float* loT, const float* lb, float* out, float* rv, long lines,
                                     int T, int K2, int accumulate, void* stream) {
    RPB_REQUIRE(S && GT && loT && lb && out && rv, "rpb_mwt_spec_out_keep: null pointer");
    RPB_REQUIRE(lines > 0 && T > 0 && K2 > 0, "rpb_mwt_spec_out_keep: bad shape lines=%ld T=%d K2=%d", lines, T, K2);
    RPB_REQUIRE(out != rv, "rpb_mwt_spec_out_keep: out and rv must be two tensors");
    const long ncell = lines * T;
    hipLaunchKernelGGL(mwt_spec_out_k<true>, dim3(mwtt_blocks(ncell, MWT_SO_CELLS)), dim3(MWT_SO_CELLS * MWT_C), 0, MWT_STREAM, S, GT, loT, lb,
                       out, rv, ncell, T, K2, accumulate);
    RPB_CHECK_LAUNCH("rpb_mwt_spec_out_keep");
}

extern "C" int rpb_mwt_lo_bwd_rows(long ncell) { return mwtt_rows((ncell + MWT_LO_TILE - 1) / MWT_LO_TILE, 512); }

extern "C" int rpb_mwt_lo_bwd(const float* gout, const float* z, const float* lo, float* gz, float* part, long ncell, void* stream) {
    RPB_REQUIRE(gout && z && lo && gz && part, "rpb_mwt_lo_bwd: null pointer");
    RPB_REQUIRE(ncell > 0, "rpb_mwt_lo_bwd: ncell=%ld", ncell);
    RPB_REQUIRE(gz != gout && gz != z, "rpb_mwt_lo_bwd: gz must be its own tensor");
    hipLaunchKernelGGL(mwt_lo_bwd_k, dim3(rpb_mwt_lo_bwd_rows(ncell)), dim3(256), 0, MWT_STREAM, gout, z, lo, gz, part, ncell);
    RPB_CHECK_LAUNCH("rpb_mwt_lo_bwd");
}

extern "C" int rpb_mwt_conv3_dgrad(const float* g, const float* wpd, float* out, int B, int Nx, int Ny, int T, int accumulate, void* stream) {
    RPB_REQUIRE(g && wpd && out, "rpb_mwt_conv3_dgrad: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0, "rpb_mwt_conv3_dgrad: bad shape B=%d Nx=%d Ny=%d T=%d", B, Nx, Ny, T);
    RPB_REQUIRE(g != out, "rpb_mwt_conv3_dgrad: in-place convolution is not possible");
    const long ncell = (long)B * Nx * Ny * T;
    const float* none = nullptr;
    hipLaunchKernelGGL(mwt_conv3_k<MWT_CONV_PLAIN>, dim3(mwtt_blocks(ncell, 256)), dim3(256), 0, MWT_STREAM, g, wpd, none, none, none, out,
                       static_cast<float*>(nullptr), ncell, Nx, Ny, T, accumulate);
    RPB_CHECK_LAUNCH("rpb_mwt_conv3_dgrad");
}

static inline long mwt_wgrad_chunk(long ncell, int splits) { return ((ncell + splits - 1) / splits + 15) / 16 * 16; }

extern "C" int rpb_mwt_conv3_wgrad_splits(long ncell) {
    const int want = mwtt_rows(ncell / 1024, 64);                      // >= 1024 cells per split, at most 64 partial rows
    const long chunk = mwt_wgrad_chunk(ncell, want);
    return (int)((ncell + chunk - 1) / chunk);                         // no empty split
}

extern "C" int rpb_mwt_conv3_wgrad(const float* g, const float* x, float* part, int B, int Nx, int Ny, int T, void* stream) {
    RPB_REQUIRE(g && x && part, "rpb_mwt_conv3_wgrad: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0, "rpb_mwt_conv3_wgrad: bad shape B=%d Nx=%d Ny=%d T=%d", B, Nx, Ny, T);
    const long ncell = (long)B * Nx * Ny * T;
    const int want = mwtt_rows(ncell / 1024, 64);
    const long chunk = mwt_wgrad_chunk(ncell, want);
    const int splits = (int)((ncell + chunk - 1) / chunk);
    hipLaunchKernelGGL(mwt_conv3_wgrad_k, dim3(splits, 27), dim3(256), 0, MWT_STREAM, g, x, part, ncell, chunk, Nx, Ny, T);
    RPB_CHECK_LAUNCH("rpb_mwt_conv3_wgrad");
}

extern "C" int rpb_mwt_modes_bwd(const float* X, const float* gY, const float* Wt, const int* tab, float* gX, float* dWt, int B, int NB,
                                 void* stream) {
    RPB_REQUIRE(X && gY && Wt && tab && gX && dWt, "rpb_mwt_modes_bwd: null pointer");
    RPB_REQUIRE(B > 0 && NB > 0, "rpb_mwt_modes_bwd: bad shape B=%d NB=%d", B, NB);
    RPB_REQUIRE(gX != X && gX != gY, "rpb_mwt_modes_bwd: gX must be its own tensor");
    hipLaunchKernelGGL(mwt_modes_bwd_k, dim3(NB), dim3(256), 0, MWT_STREAM, X, gY, Wt, tab, gX, dWt, B, NB);
    RPB_CHECK_LAUNCH("rpb_mwt_modes_bwd");
}

extern "C" int rpb_mwt_head_bwd_rows(long ncell) { return 2 * mwtt_rows((ncell + MWT_HB_CELLS - 1) / MWT_HB_CELLS, 256); }

extern "C" int rpb_mwt_head_bwd(const float* x, const float* gout, const float* w0t, const float* b0, const float* w1, float* gx, float* part,
                                int B, int Nx, int Ny, int T, int Cout, int r, void* stream) {
    RPB_REQUIRE(x && gout && w0t && b0 && w1 && gx && part, "rpb_mwt_head_bwd: null pointer");
    RPB_REQUIRE(B > 0 && Nx > 0 && Ny > 0 && T > 0 && Cout > 0 && r > 0, "rpb_mwt_head_bwd: bad shape");
    RPB_REQUIRE(Cout * r <= MWT_HB_DMAX, "rpb_mwt_head_bwd: Cout * r = %d outputs per cell, at most %d are built", Cout * r, MWT_HB_DMAX);
    const long ncell = (long)B * Nx * Ny * T;
    hipLaunchKernelGGL(mwt_head_bwd_k, dim3(rpb_mwt_head_bwd_rows(ncell) / 2), dim3(256), 0, MWT_STREAM, x, gout, w0t, b0, w1, gx, part, ncell,
                       Nx, Ny, T, Cout, r);
    RPB_CHECK_LAUNCH("rpb_mwt_head_bwd");
}

extern "C" int rpb_mwt_lift_wgrad_rows(long ncell) { return mwtt_rows((ncell + MWT_LW_TILE - 1) / MWT_LW_TILE, 256); }

extern "C" int rpb_mwt_lift_wgrad(const float* g, const float* x, float* part, int B, int T, int H, int W, int Cin, void* stream) {
    RPB_REQUIRE(g && x && part, "rpb_mwt_lift_wgrad: null pointer");
    RPB_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && Cin > 0 && Cin <= 64, "rpb_mwt_lift_wgrad: bad shape B=%d T=%d H=%d W=%d Cin=%d", B, T, H, W,
                Cin);
    const long ncell = (long)B * T * H * W;
    hipLaunchKernelGGL(mwt_lift_wgrad_k, dim3(rpb_mwt_lift_wgrad_rows(ncell)), dim3(256), 0, MWT_STREAM, g, x, part, ncell, T, H, W, Cin);
    RPB_CHECK_LAUNCH("rpb_mwt_lift_wgrad");
}
