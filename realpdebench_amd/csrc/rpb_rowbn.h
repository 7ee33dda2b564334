// What the row passes around batch-statistics BatchNorm share (rpb_rowbn.hip, rpb_deeponet_train.hip): the launch shape, the argument
// checks and the workgroup epilogue of the per-channel partial sums.
#pragma once
#include "rpb_mma.h"
#include <stdint.h>

#define ROWBN_THREADS 256

// C a power of two in [lo, hi]
static inline bool rowbn_chan_ok(int C, int lo, int hi) { return C >= lo && C <= hi && (C & (C - 1)) == 0; }
static inline bool rowbn_al16(const void* p) { return (uintptr_t)p % 16 == 0; }
// rows of every per-workgroup partial buffer = workgroups of the launches that write one (rpb_rowbn_rows)
static inline int rowbn_rows() { return rpb_num_cus() * 4; }
static inline unsigned rowbn_grid(long total) {
    long grid = (total + ROWBN_THREADS - 1) / ROWBN_THREADS;
    const long cap = (long)rpb_num_cus() * 16;
    return (unsigned)(grid > cap ? cap : (grid < 1 ? 1 : grid));
}

// A thread owns channels c0..c0+3 and sub-row `sub` of its workgroup's nsub = ROWBN_THREADS / (C / 4); s0 (and s1 with NS = 2) are its
// sums.  The nsub sub-rows are added in index order through LDS (red: nsub NS C doubles) -> part[blockIdx.x][NS C] = (s0 [C], s1 [C]).
template <int NS, typename OUT>
__device__ __forceinline__ void rowbn_block_sums(double* red, const double* s0, const double* s1, int C, int c0, int sub, int nsub, OUT* part) {
    double* mine = red + (long)sub * NS * C;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mine[c0 + i] = s0[i];
        if (NS == 2) mine[C + c0 + i] = s1[i];
    }
    __syncthreads();
    for (int n = threadIdx.x; n < NS * C; n += ROWBN_THREADS) {
        double s = 0.;
        for (int k = 0; k < nsub; ++k) s += red[(long)k * NS * C + n];
        part[(long)blockIdx.x * NS * C + n] = (OUT)s;
    }
}
