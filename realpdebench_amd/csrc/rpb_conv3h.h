// What the two files of the "f16x2" 3x3x3 convolutions share at file scope: the tile constants and the scalar operand split of
// csrc/rpb_conv3h.hip (conv3x_f16x2_kernel, rpb_split2h, rpb_conv3x_wprep_f16x2) and csrc/rpb_cno3h.hip (cno_conv3x_f16x2_kernel,
// rpb_cno_pack_f16x2).  The main loop they share is a text fragment of its own, csrc/rpb_conv3h_loop.h.
#pragma once
#include "rpb_mma.h"

#define CH_BM 128
#define CH_ROWS (CH_BM + 2)

// x * 2^e -> (hi, lo) fp16 bit patterns, both RNE; non-finite values give a non-finite hi (and lo = NaN): they propagate
__device__ __forceinline__ void split2h(float x, int e, unsigned& h, unsigned& l) {
    const float v = ldexpf(x, e);                                       // exact (power of two, no overflow by the choice of e)
    const _Float16 hi = (_Float16)v;
    const _Float16 lo = (_Float16)(v - (float)hi);                      // v - hi exact in fp32
    h = __builtin_bit_cast(unsigned short, hi);
    l = __builtin_bit_cast(unsigned short, lo);
}
