// The split-operand arithmetic of the bf16 / fp16 matrix pipe, defined ONCE: how an fp32 operand becomes bf16 (or fp16) planes, the MFMA
// wrappers the planes are multiplied with, and the 128-bit buffer accesses the operands arrive through.  Every kernel that runs on
// v_mfma_f32_{16x16x32,32x32x16}_{bf16,f16} includes this header; the primitives are __forceinline__ and are compiled under the flags of
// the including file (realpdebench_amd/build.py EXTRA).
//
//   three bf16 planes  x = hi + mid + lo EXACTLY (8 + 8 + 8 significand bits); a product is accumulated in fp32 from the six products
//                      hi*lo + lo*hi + mid*mid + hi*mid + mid*hi + hi*hi, each bf16 x bf16 product exact in fp32 -- fp32 grade, the default
//                      (rpb_split_pair, split8, mfma16 / mfma32b);
//   two fp16 planes    x = hi + lo to one fp32 unit in the last place (11 + 11 significand bits and the sign of lo), three products
//                      hi*lo + lo*hi + hi*hi, dropped term <= 2^-22 |a b| -- the grade of "3xTF32", the opt-in "f16x2" eval arithmetic
//                      (split8h, mfma16h / mfma32h).
//   the stored planes  of the 3x3x3 convolutions (rpb_split3, rpb_conv3x_wprep, rpb_split3t, the CNO plane outputs): bf16_rne / split3 /
//                      split3_store below round single values to nearest even in INTEGER arithmetic.  It is a separate primitive from
//                      rpb_split_pair_rne / split8_rne on purpose: the hardware conversion of those keeps a NaN a NaN where the integer form
//                      rounds its payload like any other bit pattern, and every producer of a plane buffer has to give the same bits
//                      (rpb_cno_conv3x promises the planes rpb_split3 would have written).  One definition enforces that.
// (Not here, because it only looks similar: split2h of rpb_conv3h.h -- scalar, scaled by ldexpf.)
#pragma once
#include "rpb_common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // native vector: selects stay in registers (HIP's uint4 struct did not)
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// a compile-time integer as a value: the argument through which a lambda of a hand-pipelined loop selects a NAMED register
template <int V>
struct IC {
    static constexpr int value = V;
};
// the token tile of the bf16x3 3x3x3 convolutions (csrc/rpb_conv3x_loop.h and the launchers of its two kernels): 128 output tokens and the
// rows of their w neighbours
#define CX_BM 128
#define CX_ROWS (CX_BM + 2)

// ---------------------------------------------------------------------------------- 128-bit (64-bit) buffer accesses
// AUX: the cache policy of the access (the aux operand of raw_buffer_load / _store: RPB_STREAM_AUX for a streamed tensor, 0 = default for
// one that is read again soon); every call site names its own.
template <int AUX>
__device__ __forceinline__ u32x4 ld16(rsrc_t r, int voff) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, AUX));
}
template <int AUX>
__device__ __forceinline__ f32x2 ld8(rsrc_t r, int voff) {
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, AUX));
}
template <int AUX>
__device__ __forceinline__ void st16(f32x4 v, rsrc_t r, int voff) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, 0, AUX);
}
// by VALUE: __builtin_bit_cast applied to a vector ELEMENT (v[1]) reads element 0 with hipcc 7.2 (it cost the b64 loads their second
// dword and the row swap its second result); a scalar copy first is safe
__device__ __forceinline__ float asf(unsigned u) { return __builtin_bit_cast(float, u); }

// ---------------------------------------------------------------------------------- the three-plane operand split
// bf16 STORAGE (BASELINE.json configs[4]): an operand that was stored as bf16 carries a rounding of 2^-9 of its value, and it is multiplied
// with the planes of an fp32 constant (conv / fc1 weights, DFT stage matrices).  The constant's third plane contributes 2^-16 of the product:
// 1 / 128 of the error the stored operand already has.  RPB_BF16_CONST_PLANES = 2 (default) drops that product -- two MFMAs per stored plane
// instead of three in every kernel of the bf16-storage forward; 3 keeps it (round 4).  fp32 storage is not touched.
#ifndef RPB_BF16_CONST_PLANES
#define RPB_BF16_CONST_PLANES 2
#endif

// x = hi + mid + lo EXACTLY with three bf16 numbers, two ways:
//   RPB_SPLIT_RNE = 0 (default)  truncation at every level (v_perm packs): mid < 2^-7 |x|, lo < 2^-15 |x|, so the three products the
//       six-product scheme drops (mid*lo, lo*mid, lo*lo) are 2^-24 |a b| typically (rms 2^-24.1) and reach 2^-21.3 in the worst case;
//   RPB_SPLIT_RNE = 1  round to nearest even at every level (gfx950: v_cvt_pk_bf16_f32 converts a pair): |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|,
//       still exact (the last residual has at most 8 significant bits), dropped terms <= 2^-24.2 |a b| worst case, 2^-27.5 rms
//       (tools/split_error.py).  Fewer instructions (4.5 against 5.5 per value) but NOT faster: the conversions and packed subtracts
//       issue at the packed rate -- measured (profiles/r06b_ab4_split_rne.txt, A/B twice on one box): train step 35.63 / 35.67 ms with the
//       truncating split, 36.04 / 36.09 with the rounding one (the wave-pair backward cell_mix 2.95 -> 3.05 ms), eval forward equal
//       (11.35 ms).  Every parity test passes either way; the build switch is for a caller that wants the tighter worst case for 1.1 %.
// The token GEMMs (rpb_gemm3x*.hip) call rpb_split_pair_rne directly: they round whatever the switch says, as the split3 passes of
// csrc/rpb_conv3x.hip -- memory-bound -- have since round 2.
#ifndef RPB_SPLIT_RNE
#define RPB_SPLIT_RNE 0
#endif
// (a, b) -> one dword per plane (a in the low half, b in the high half)
__device__ __forceinline__ void rpb_split_pair_trunc(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    const unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
    h = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
    const float ra = a - __builtin_bit_cast(float, ua & 0xffff0000u), rb = b - __builtin_bit_cast(float, ub & 0xffff0000u);
    const unsigned uc = __builtin_bit_cast(unsigned, ra), ud = __builtin_bit_cast(unsigned, rb);
    m = __builtin_amdgcn_perm(ud, uc, 0x07060302u);
    const float sa = ra - __builtin_bit_cast(float, uc & 0xffff0000u), sb = rb - __builtin_bit_cast(float, ud & 0xffff0000u);
    l = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, sb), __builtin_bit_cast(unsigned, sa), 0x07060302u);
}
__device__ __forceinline__ void rpb_split_pair_rne(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
    const f32x2 ab = {a, b};
    h = __builtin_bit_cast(unsigned, __builtin_convertvector(ab, bf16x2));                                             // v_cvt_pk_bf16_f32 (RNE)
    const f32x2 r = ab - f32x2{__builtin_bit_cast(float, h << 16), __builtin_bit_cast(float, h & 0xffff0000u)};        // exact
    m = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
    const f32x2 s = r - f32x2{__builtin_bit_cast(float, m << 16), __builtin_bit_cast(float, m & 0xffff0000u)};         // exact
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(s, bf16x2));                                              // exact: <= 8 significant bits
}
__device__ __forceinline__ void rpb_split_pair(float a, float b, unsigned& h, unsigned& m, unsigned& l) {
#if RPB_SPLIT_RNE
    rpb_split_pair_rne(a, b, h, m, l);
#else
    rpb_split_pair_trunc(a, b, h, m, l);
#endif
}
// (a, b) fp32 -> one dword of two truncated bf16 (a low half, b high half): the hi plane alone
__device__ __forceinline__ unsigned pack_hi(float a, float b) {
    return __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, b), __builtin_bit_cast(unsigned, a), 0x07060302u);
}
// 8 fp32 -> three bf16x8 planes (exact: hi + mid + lo == v)
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
    u32x4 uh, um, ul;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        unsigned ph, pm, pl;
        rpb_split_pair(v[2 * q], v[2 * q + 1], ph, pm, pl);
        uh[q] = ph;
        um[q] = pm;
        ul[q] = pl;
    }
    h = __builtin_bit_cast(bf16x8, uh);
    m = __builtin_bit_cast(bf16x8, um);
    l = __builtin_bit_cast(bf16x8, ul);
}
// the same with only the first `npairs` element pairs live (wave-uniform): the rest are zero planes at no vector cost
__device__ __forceinline__ void split8n(const float (&v)[8], int npairs, bf16x8& h, bf16x8& m, bf16x8& l) {
    u32x4 uh = {0u, 0u, 0u, 0u}, um = uh, ul = uh;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q >= npairs) break;
        const float a = v[2 * q], b = v[2 * q + 1];      // copied first: passed as v[..] the loads move and axg_kernel's registers are allocated differently
        unsigned ph, pm, pl;
        rpb_split_pair(a, b, ph, pm, pl);
        uh[q] = ph;
        um[q] = pm;
        ul[q] = pl;
    }
    h = __builtin_bit_cast(bf16x8, uh);
    m = __builtin_bit_cast(bf16x8, um);
    l = __builtin_bit_cast(bf16x8, ul);
}
// 8 fp32 as two f32x4 -> the planes as dwords, ALWAYS rounded to nearest (the token GEMMs)
__device__ __forceinline__ void split8_rne(f32x4 v0, f32x4 v1, u32x4& h, u32x4& m, u32x4& l) {
    unsigned hh[4], mm[4], ll[4];
    rpb_split_pair_rne(v0[0], v0[1], hh[0], mm[0], ll[0]);
    rpb_split_pair_rne(v0[2], v0[3], hh[1], mm[1], ll[1]);
    rpb_split_pair_rne(v1[0], v1[1], hh[2], mm[2], ll[2]);
    rpb_split_pair_rne(v1[2], v1[3], hh[3], mm[3], ll[3]);
    h = u32x4{hh[0], hh[1], hh[2], hh[3]};
    m = u32x4{mm[0], mm[1], mm[2], mm[3]};
    l = u32x4{ll[0], ll[1], ll[2], ll[3]};
}

// ---------------------------------------------------------------------------------- the stored planes (integer RNE)
// round-to-nearest-even bf16 of x (as the upper 16 bits of an fp32)
__device__ __forceinline__ unsigned bf16_rne(float x) {
    const unsigned u = __builtin_bit_cast(unsigned, x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
// round to nearest even at every level, hi + mid + lo == x exactly
__device__ __forceinline__ void split3(float x, unsigned& h, unsigned& m, unsigned& l) {
    h = bf16_rne(x);
    const float r1 = x - __builtin_bit_cast(float, h << 16);          // exact
    m = bf16_rne(r1);
    const float r2 = r1 - __builtin_bit_cast(float, m << 16);         // exact
    l = bf16_rne(r2);
}
// 8 consecutive channels of one token -> 16 B per plane at P + o, P + o + pstride, P + o + 2 pstride
__device__ __forceinline__ void split3_store(uint16_t* P, long o, long pstride, f32x4 v0, f32x4 v1) {
    unsigned h[8], md[8], lo[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        split3(v0[i], h[i], md[i], lo[i]);
        split3(v1[i], h[4 + i], md[4 + i], lo[4 + i]);
    }
    u32x4 oh, om, ol;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        oh[q] = h[2 * q] | (h[2 * q + 1] << 16);
        om[q] = md[2 * q] | (md[2 * q + 1] << 16);
        ol[q] = lo[2 * q] | (lo[2 * q + 1] << 16);
    }
    *reinterpret_cast<u32x4*>(P + o) = oh;
    *reinterpret_cast<u32x4*>(P + o + pstride) = om;
    *reinterpret_cast<u32x4*>(P + o + 2 * pstride) = ol;
}

// v_mfma_f32_16x16x32_bf16: A lane (m = l & 15, kg = l >> 4) holds k = 8 kg + e; D register r of lane (n, hg) is row 4 hg + r, column n
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// v_mfma_f32_32x32x16_bf16 ("b": the bf16 pipe -- mfma32(float, float, f32x16) of rpb_common.h is the fp32 one); V = bf16x8, or the same
// 16 bytes as u32x4
template <class V>
__device__ __forceinline__ f32x16 mfma32b(V a, V b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// ---------------------------------------------------------------------------------- the two-plane fp16 split ("f16x2")
// Both planes rounded to nearest even; half the matrix-pipe time of the three-plane form and 2.5 instead of 5.5 vector instructions per
// split value.  The planes travel in the bf16x8 containers of the default path (bit patterns only): plane slot 0 = hi, slot 1 = lo.  fp16's
// range is the caller's business (exact power-of-two scalings: CmxArgs::spec_exp, PH_H2W).
// FMAMIX: how the residual a - float(hi) (exact in fp32) is formed --
//   true   ONE v_fma_mix_f32 per value (f16 half * -1 + f32): 4 instead of 5 instructions per value pair; rpb_cmx.hip
//   false  left to the compiler, which converts both halves and subtracts packed (2 x v_cvt_f32_f16 + v_pk_add_f32); rpb_pjh.hip, where
//          the v_fma_mix_f32 form measured the head 1 % slower (profiles/r06b_ab.txt)
template <bool FMAMIX>
__device__ __forceinline__ void split8h(const float (&v)[8], bf16x8& h, bf16x8& l) {
    u32x4 uh, ul;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x2 ab = {v[2 * q], v[2 * q + 1]};
        const f16x2 hh = __builtin_convertvector(ab, f16x2);                       // v_cvt_pk_f16_f32 (RNE)
        uh[q] = __builtin_bit_cast(unsigned, hh);
        f32x2 r;
        if constexpr (FMAMIX) {
            float r0, r1;
            const unsigned hu = uh[q];
            const float a0 = ab[0], a1 = ab[1];
            asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r0) : "v"(hu), "v"(a0));
            asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r1) : "v"(hu), "v"(a1));
            r = f32x2{r0, r1};
        } else {
            r = ab - __builtin_convertvector(hh, f32x2);
        }
        const f16x2 ll = __builtin_convertvector(r, f16x2);
        ul[q] = __builtin_bit_cast(unsigned, ll);
    }
    h = __builtin_bit_cast(bf16x8, uh);
    l = __builtin_bit_cast(bf16x8, ul);
}
// v_mfma_f32_16x16x32_f16 / v_mfma_f32_32x32x16_f16 on planes in bf16x8 (or u32x4) containers
__device__ __forceinline__ f32x4 mfma16h(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
template <class V>
__device__ __forceinline__ f32x16 mfma32h(V a, V b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// the three products of one k-step from (hi, lo) operand pairs, small terms first: lo*hi, hi*lo, hi*hi (lo*lo <= 2^-22 of the product is
// dropped); a = the MFMA's A operand (rows of D), b = its B operand (columns of D).  rpb_deeponet_h.hip, rpb_gemm3h.hip
__device__ __forceinline__ f32x16 mma3h(const u32x4 (&a)[2], const u32x4 (&b)[2], f32x16 c) {
    c = mfma32h(a[1], b[0], c);
    c = mfma32h(a[0], b[1], c);
    c = mfma32h(a[0], b[0], c);
    return c;
}
// The power-of-two scale of one MFMA row / column of activations (a point of rpb_deeponet_h.hip, a token row of rpb_gemm3h.hip):
// e with m 2^e in [2^TOP, 2^(TOP + 1)) for a finite m > 0, capped at 62 so that 2^e and 2^-e stay normal fp32 numbers; 0 for m == 0
template <int TOP>
__device__ __forceinline__ int col_exp(float m) {
    const int e = TOP + 127 - (int)(__builtin_bit_cast(unsigned, m) >> 23);
    return m == 0.f ? 0 : (e > 62 ? 62 : e);
}
// 2^e as fp32, -126 <= e <= 127
__device__ __forceinline__ float pow2f(int e) { return asf((unsigned)(e + 127) << 23); }

// ---------------------------------------------------------------------------------- cross-lane
// x + y from the lane the DPP control names (the halving butterflies of the heads)
__device__ __forceinline__ float dpp_add(float x, float y, const int ctrl) {
    switch (ctrl) {
    case 0: return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), 0x140, 0xF, 0xF, true));   // row_mirror
    case 1: return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), 0x141, 0xF, 0xF, true));   // row_half_mirror
    case 2: return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    default: return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
    }
}
