// WDNO (realpdebench/model/wdno.py): the wavelet and sampler kernels around the denoising U-Net.  All tensors are channels-last fp32.
//
//   rpb_wdno_dec   one level of the separable 3-D filter bank of ptwt.wavedec3(mode="zero", level=1): per axis (2L - 3) / 2 zeros on each
//                  side (one more on the right of an odd length), cross-correlation with the reversed decomposition filter at stride 2.
//                  x [B][r T][H][W][C] -> eight sub-bands per virtual channel cv = c r + sub (frame sub T + t of x), written as state
//                  columns col0 + 8 cv + s, s = 4 (T detail) + 2 (H detail) + (W detail), divided by the column's rescaler, zero outside
//                  the coefficient mesh.  A second mode writes no state: per-column partial maxima of |coefficient| in a fixed number of
//                  rows (find_rescaler).
//   rpb_wdno_rec   the inverse: state x rescaler through the transposed convolution at stride 2 with the reconstruction filters,
//                  (2L - 3) / 2 trimmed per side, cropped to [T][H][W], virtual channel c r + sub -> frame sub T + t, channel c.
//   rpb_wdno_step  the point-wise part of one sampling step in one pass over the state (modes below).
// One thread owns whole output elements: no atomics, fixed summation order, two calls are bit-equal.  No call synchronises with the host.
#include "rpb_common.h"

#define WD_ROWS 128                      // rows of partial maxima (rpb_wdno_dec_rows)

struct WdGeo {
    int B, T, H, W;                      // mesh of x (T: frames per virtual channel)
    int C, r;                            // channels of x, frames factor: x is [B][r T][H][W][C]
    int Tc, Hc, Wc;                      // coefficient mesh
    int Tp, Hp, Wp;                      // padded mesh of the state
    int ld, col0;                        // state row length, first column
};

// the eight coefficients of virtual channel cv at coefficient cell (tc, hc, wc); flo / fhi: the REVERSED decomposition filters
template <int L>
__device__ __forceinline__ void wd_coefs(const float* __restrict__ x, const float (&flo)[L], const float (&fhi)[L], const WdGeo& g, int b,
                                         int cv, int tc, int hc, int wc, float (&o)[8]) {
    constexpr int PAD = (2 * L - 3) / 2;
    const int c = cv / g.r, sub = cv - c * g.r;
    const float* xb = x + ((long)b * g.r + sub) * g.T * g.H * g.W * g.C + c;
#pragma unroll
    for (int s = 0; s < 8; ++s) o[s] = 0.f;
#pragma unroll
    for (int it = 0; it < L; ++it) {
        const int t = 2 * tc + it - PAD;
        if (t < 0 || t >= g.T) continue;
        float aa = 0.f, ad = 0.f, da = 0.f, dd = 0.f;
#pragma unroll
        for (int ih = 0; ih < L; ++ih) {
            const int h = 2 * hc + ih - PAD;
            if (h < 0 || h >= g.H) continue;
            const float* row = xb + ((long)t * g.H + h) * g.W * g.C;
            float sa = 0.f, sd = 0.f;
#pragma unroll
            for (int iw = 0; iw < L; ++iw) {
                const int w = 2 * wc + iw - PAD;
                if (w < 0 || w >= g.W) continue;
                const float v = row[(long)w * g.C];
                sa += flo[iw] * v;
                sd += fhi[iw] * v;
            }
            aa += flo[ih] * sa;
            ad += flo[ih] * sd;
            da += fhi[ih] * sa;
            dd += fhi[ih] * sd;
        }
        o[0] += flo[it] * aa;
        o[1] += flo[it] * ad;
        o[2] += flo[it] * da;
        o[3] += flo[it] * dd;
        o[4] += fhi[it] * aa;
        o[5] += fhi[it] * ad;
        o[6] += fhi[it] * da;
        o[7] += fhi[it] * dd;
    }
}

template <int L>
__device__ __forceinline__ void wd_filters(const float* __restrict__ filt, int lo_row, int hi_row, bool reversed, float (&flo)[L],
                                           float (&fhi)[L]) {
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const int j = reversed ? L - 1 - k : k;
        flo[k] = filt[lo_row * L + j];
        fhi[k] = filt[hi_row * L + j];
    }
}

// state mode: one thread = one (padded cell, virtual channel)
template <int L>
__global__ __launch_bounds__(256) void wdno_dec_kernel(const float* __restrict__ x, const float* __restrict__ filt,
                                                       const float* __restrict__ rescaler, float* __restrict__ state, WdGeo g) {
    float flo[L], fhi[L];
    wd_filters<L>(filt, 0, 1, true, flo, fhi);
    const int Cv = g.C * g.r;
    const long total = (long)g.B * g.Tp * g.Hp * g.Wp * Cv;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long cell = idx / Cv;
        const int cv = (int)(idx - cell * Cv);
        const int wc = (int)(cell % g.Wp);
        long q = cell / g.Wp;
        const int hc = (int)(q % g.Hp);
        q /= g.Hp;
        const int tc = (int)(q % g.Tp), b = (int)(q / g.Tp);
        float o[8];
        if (tc < g.Tc && hc < g.Hc && wc < g.Wc) {
            wd_coefs<L>(x, flo, fhi, g, b, cv, tc, hc, wc, o);
            const float* rs = rescaler + g.col0 + cv * 8;
#pragma unroll
            for (int s = 0; s < 8; ++s) o[s] = o[s] / rs[s];
        } else {
#pragma unroll
            for (int s = 0; s < 8; ++s) o[s] = 0.f;
        }
        float* dst = state + cell * g.ld + g.col0 + cv * 8;
        *reinterpret_cast<f32x4*>(dst) = f32x4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4*>(dst + 4) = f32x4{o[4], o[5], o[6], o[7]};
    }
}

// maximum mode: WD_ROWS workgroups, each walks its share of the coefficient cells; thread = (cell slot, virtual channel), Cv <= 256
template <int L>
__global__ __launch_bounds__(256) void wdno_dec_max_kernel(const float* __restrict__ x, const float* __restrict__ filt,
                                                           float* __restrict__ part, WdGeo g) {
    __shared__ float sm[256 * 8];
    float flo[L], fhi[L];
    wd_filters<L>(filt, 0, 1, true, flo, fhi);
    const int Cv = g.C * g.r, cpb = 256 / Cv;
    const int tid = threadIdx.x, cl = tid / Cv, cv = tid - cl * Cv;
    const long ncell = (long)g.B * g.Tc * g.Hc * g.Wc;
    float mx[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) mx[s] = 0.f;
    if (cl < cpb) {
        for (long cell = (long)blockIdx.x * cpb + cl; cell < ncell; cell += (long)gridDim.x * cpb) {
            const int wc = (int)(cell % g.Wc);
            long q = cell / g.Wc;
            const int hc = (int)(q % g.Hc);
            q /= g.Hc;
            const int tc = (int)(q % g.Tc), b = (int)(q / g.Tc);
            float o[8];
            wd_coefs<L>(x, flo, fhi, g, b, cv, tc, hc, wc, o);
#pragma unroll
            for (int s = 0; s < 8; ++s) mx[s] = fmaxf(mx[s], fabsf(o[s]));
        }
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) sm[tid * 8 + s] = mx[s];
    __syncthreads();
    for (int i = tid; i < Cv * 8; i += 256) {
        const int v = i >> 3, s = i & 7;
        float m = 0.f;
        for (int k = 0; k < cpb; ++k) m = fmaxf(m, sm[(k * Cv + v) * 8 + s]);
        part[(long)blockIdx.x * (Cv * 8) + i] = m;
    }
}

static int wd_geo(WdGeo& g, int B, int T, int H, int W, int C, int r, int L, int Tp, int Hp, int Wp, int ld, int col0) {
    RPB_REQUIRE(B > 0 && T > 0 && H > 0 && W > 0 && C > 0 && r > 0, "wdno: bad shape");
    RPB_REQUIRE(L == 2 || L == 6, "wdno: filter length %d unsupported (2: bior1.1, 6: bior1.3)", L);
    g = WdGeo{B, T, H, W, C, r, (T + L - 1) / 2, (H + L - 1) / 2, (W + L - 1) / 2, Tp, Hp, Wp, ld, col0};
    return RPB_OK;
}

extern "C" int rpb_wdno_dec_rows(void) { return WD_ROWS; }

extern "C" int rpb_wdno_dec(const float* x, const float* filt, const float* rescaler, float* state, float* part, int B, int T, int H, int W,
                            int C, int r, int L, int Tp, int Hp, int Wp, int ld, int col0, int mode, void* stream) {
    WdGeo g;
    if (int rc = wd_geo(g, B, T, H, W, C, r, L, Tp, Hp, Wp, ld, col0)) return rc;
    RPB_REQUIRE(x && filt, "wdno_dec: null operand");
    hipStream_t st = (hipStream_t)stream;
    if (mode == 1) {
        RPB_REQUIRE(part && C * r <= 256, "wdno_dec: the maximum mode takes up to 256 virtual channels, got %d", C * r);
        if (L == 2) hipLaunchKernelGGL(wdno_dec_max_kernel<2>, dim3(WD_ROWS), dim3(256), 0, st, x, filt, part, g);
        else hipLaunchKernelGGL(wdno_dec_max_kernel<6>, dim3(WD_ROWS), dim3(256), 0, st, x, filt, part, g);
        RPB_CHECK_LAUNCH("wdno_dec(max)");
    }
    RPB_REQUIRE(mode == 0 && state && rescaler, "wdno_dec: bad mode / null operand");
    RPB_REQUIRE(Tp >= g.Tc && Hp >= g.Hc && Wp >= g.Wc, "wdno_dec: padded mesh (%d,%d,%d) below the coefficient mesh (%d,%d,%d)", Tp, Hp,
                Wp, g.Tc, g.Hc, g.Wc);
    RPB_REQUIRE(ld % 4 == 0 && col0 % 4 == 0 && col0 >= 0 && col0 + 8 * C * r <= ld, "wdno_dec: columns [%d, %d) of %d", col0,
                col0 + 8 * C * r, ld);
    const long total = (long)B * Tp * Hp * Wp * C * r;
    long grid = (total + 255) / 256;
    const long cap = (long)rpb_num_cus() * 16;
    if (grid > cap) grid = cap;
    if (L == 2) hipLaunchKernelGGL(wdno_dec_kernel<2>, dim3((unsigned)grid), dim3(256), 0, st, x, filt, rescaler, state, g);
    else hipLaunchKernelGGL(wdno_dec_kernel<6>, dim3((unsigned)grid), dim3(256), 0, st, x, filt, rescaler, state, g);
    RPB_CHECK_LAUNCH("wdno_dec");
}

// ---------------------------------------------------------------------------------- reconstruction
// one thread = one output element (b, sub T + t, h, w, c); y[n] = sum_i coef[i] rec[n + PAD - 2 i] per axis
template <int L>
__global__ __launch_bounds__(256) void wdno_rec_kernel(const float* __restrict__ state, const float* __restrict__ filt,
                                                       const float* __restrict__ rescaler, float* __restrict__ out, WdGeo g) {
    constexpr int PAD = (2 * L - 3) / 2;
    float rlo[L], rhi[L];
    wd_filters<L>(filt, 2, 3, false, rlo, rhi);
    const long total = (long)g.B * g.r * g.T * g.H * g.W * g.C;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % g.C);
        long q = idx / g.C;
        const int w = (int)(q % g.W);
        q /= g.W;
        const int h = (int)(q % g.H);
        q /= g.H;
        const int to = (int)(q % (g.r * g.T)), b = (int)(q / (g.r * g.T));
        const int sub = to / g.T, t = to - sub * g.T;
        const int col = g.col0 + (c * g.r + sub) * 8;
        float rs[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) rs[s] = rescaler[col + s];
        float acc = 0.f;
#pragma unroll
        for (int jt = 0; jt < L / 2; ++jt) {
            const int kt = ((t + PAD) & 1) + 2 * jt, it = (t + PAD - kt) >> 1;
            if (it < 0 || it >= g.Tc) continue;
            float ha = 0.f, hd = 0.f;
#pragma unroll
            for (int jh = 0; jh < L / 2; ++jh) {
                const int kh = ((h + PAD) & 1) + 2 * jh, ih = (h + PAD - kh) >> 1;
                if (ih < 0 || ih >= g.Hc) continue;
                float w0 = 0.f, w1 = 0.f, w2 = 0.f, w3 = 0.f;
#pragma unroll
                for (int jw = 0; jw < L / 2; ++jw) {
                    const int kw = ((w + PAD) & 1) + 2 * jw, iw = (w + PAD - kw) >> 1;
                    if (iw < 0 || iw >= g.Wc) continue;
                    const float* src = state + ((((long)b * g.Tp + it) * g.Hp + ih) * g.Wp + iw) * g.ld + col;
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
                    const float lw = rlo[kw], hw = rhi[kw];
                    w0 += (v0[0] * rs[0]) * lw + (v0[1] * rs[1]) * hw;
                    w1 += (v0[2] * rs[2]) * lw + (v0[3] * rs[3]) * hw;
                    w2 += (v1[0] * rs[4]) * lw + (v1[1] * rs[5]) * hw;
                    w3 += (v1[2] * rs[6]) * lw + (v1[3] * rs[7]) * hw;
                }
                ha += w0 * rlo[kh] + w1 * rhi[kh];
                hd += w2 * rlo[kh] + w3 * rhi[kh];
            }
            acc += ha * rlo[kt] + hd * rhi[kt];
        }
        out[idx] = acc;
    }
}

extern "C" int rpb_wdno_rec(const float* state, const float* filt, const float* rescaler, float* out, int B, int T, int H, int W, int C,
                            int r, int L, int Tp, int Hp, int Wp, int ld, int col0, void* stream) {
    WdGeo g;
    if (int rc = wd_geo(g, B, T, H, W, C, r, L, Tp, Hp, Wp, ld, col0)) return rc;
    RPB_REQUIRE(state && filt && rescaler && out, "wdno_rec: null operand");
    RPB_REQUIRE(Tp >= g.Tc && Hp >= g.Hc && Wp >= g.Wc, "wdno_rec: padded mesh (%d,%d,%d) below the coefficient mesh (%d,%d,%d)", Tp, Hp,
                Wp, g.Tc, g.Hc, g.Wc);
    RPB_REQUIRE(ld % 4 == 0 && col0 % 4 == 0 && col0 >= 0 && col0 + 8 * C * r <= ld, "wdno_rec: columns [%d, %d) of %d", col0,
                col0 + 8 * C * r, ld);
    const long total = (long)B * r * T * H * W * C;
    long grid = (total + 255) / 256;
    const long cap = (long)rpb_num_cus() * 16;
    if (grid > cap) grid = cap;
    hipStream_t st = (hipStream_t)stream;
    if (L == 2) hipLaunchKernelGGL(wdno_rec_kernel<2>, dim3((unsigned)grid), dim3(256), 0, st, state, filt, rescaler, out, g);
    else hipLaunchKernelGGL(wdno_rec_kernel<6>, dim3((unsigned)grid), dim3(256), 0, st, state, filt, rescaler, out, g);
    RPB_CHECK_LAUNCH("wdno_rec");
}

// ---------------------------------------------------------------------------------- the sampling step
// modes (sc: five scalars of device memory, mode 3: two per sample)
//   0  DDIM step       x0 = clamp(a img - b eps, +-1); eps' = (a img - x0) / b; img' = sqrt(abar_next) x0 + c eps' + sigma noise
//                      sc = (a, b, sqrt(abar_next), c, sigma)
//   1  last DDIM step  img' = x0                                                  sc = (a, b, -, -, -)
//   2  ancestral step  img' = c1 x0 + c2 img + sd noise (noise == null: no noise) sc = (a, b, c1, c2, sd)
//   3  q_sample        out = sa[b] x + sb[b] noise, out2 = noise (the target)     sc = [B][2]; img = x, eps unused
//   4  start           img' = noise
// then, in every mode, the input condition (columns < Ccond come from cond; mode 3: out keeps x, out2 gets 0) and the pad condition (zero
// outside the coefficient mesh).  Products and sums are rounded one by one, in the reference's order (no contraction).
struct WdStep {
    const float *img, *eps, *cond, *noise, *sc;
    float *out, *out2;
    long cells;
    int Tp, Hp, Wp, Tc, Hc, Wc, Cs, Ccond, mode;
};

__global__ __launch_bounds__(256) void wdno_step_kernel(WdStep a) {
    const int c4n = a.Cs >> 2;
    const long total = a.cells * c4n;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f;
    if (a.mode != 3 && a.mode != 4) {
        s0 = a.sc[0];
        s1 = a.sc[1];
        s2 = a.sc[2];
        s3 = a.sc[3];
        s4 = a.sc[4];
    }
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long cell = idx / c4n;
        const int col = (int)(idx - cell * c4n) * 4;
        const int w = (int)(cell % a.Wp);
        long q = cell / a.Wp;
        const int h = (int)(q % a.Hp);
        q /= a.Hp;
        const int t = (int)(q % a.Tp);
        const long b = q / a.Tp;
        const long o = cell * a.Cs + col;
        f32x4 r = z, r2 = z;
        if (t < a.Tc && h < a.Hc && w < a.Wc) {
            if (col < a.Ccond) {
                r = a.mode == 3 ? *reinterpret_cast<const f32x4*>(a.img + o) : *reinterpret_cast<const f32x4*>(a.cond + cell * a.Ccond + col);
            } else if (a.mode == 4) {
                r = *reinterpret_cast<const f32x4*>(a.noise + o);
            } else if (a.mode == 3) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(a.img + o), n = *reinterpret_cast<const f32x4*>(a.noise + o);
                const float sa = a.sc[2 * b], sb = a.sc[2 * b + 1];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
                    const float u = sa * x[i], v = sb * n[i];
                    r[i] = u + v;
                }
                r2 = n;
            } else {
                const f32x4 x = *reinterpret_cast<const f32x4*>(a.img + o), e = *reinterpret_cast<const f32x4*>(a.eps + o);
                f32x4 n = z;
                if (a.mode != 1 && a.noise) n = *reinterpret_cast<const f32x4*>(a.noise + o);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
#pragma clang fp contract(off)
                    const float ax = s0 * x[i], be = s1 * e[i];
                    const float x0 = fminf(fmaxf(ax - be, -1.f), 1.f);
                    if (a.mode == 1) {
                        r[i] = x0;
                    } else if (a.mode == 0) {
                        const float e2 = (ax - x0) / s1;
                        const float p0 = x0 * s2, p1 = s3 * e2, p2 = s4 * n[i];
                        r[i] = (p0 + p1) + p2;
                    } else {
                        const float p0 = s2 * x0, p1 = s3 * x[i];
                        const float mean = p0 + p1;
                        r[i] = a.noise ? mean + s4 * n[i] : mean;
                    }
                }
            }
        }
        *reinterpret_cast<f32x4*>(a.out + o) = r;
        if (a.mode == 3) *reinterpret_cast<f32x4*>(a.out2 + o) = r2;
    }
}

extern "C" int rpb_wdno_step(const float* img, const float* eps, const float* cond, const float* noise, const float* sc, float* out,
                             float* out2, int B, int Tp, int Hp, int Wp, int Tc, int Hc, int Wc, int Cs, int Ccond, int mode,
                             void* stream) {
    RPB_REQUIRE(out && B > 0 && Tp > 0 && Hp > 0 && Wp > 0 && Tc <= Tp && Hc <= Hp && Wc <= Wp && Tc > 0 && Hc > 0 && Wc > 0,
                "wdno_step: bad mesh");
    RPB_REQUIRE(Cs > 0 && Cs % 4 == 0 && Ccond >= 0 && Ccond % 4 == 0 && Ccond <= Cs, "wdno_step: Cs=%d Ccond=%d (both %% 4)", Cs, Ccond);
    RPB_REQUIRE(mode >= 0 && mode <= 4, "wdno_step: mode %d", mode);
    if (mode <= 2) RPB_REQUIRE(img && eps && sc && (mode != 0 || noise) && (Ccond == 0 || cond), "wdno_step: null operand (mode %d)", mode);
    if (mode == 3) RPB_REQUIRE(img && noise && sc && out2, "wdno_step: null operand (q_sample)");
    if (mode == 4) RPB_REQUIRE(noise && (Ccond == 0 || cond), "wdno_step: null operand (start)");
    WdStep a{img, eps, cond, noise, sc, out, out2, (long)B * Tp * Hp * Wp, Tp, Hp, Wp, Tc, Hc, Wc, Cs, Ccond, mode};
    const long total = a.cells * (Cs / 4);
    long grid = (total + 255) / 256;
    const long cap = (long)rpb_num_cus() * 16;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(wdno_step_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    RPB_CHECK_LAUNCH("wdno_step");
}
