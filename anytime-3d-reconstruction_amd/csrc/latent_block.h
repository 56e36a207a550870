// What mm_latent.hip and prior_latent.hip share on the device side and in their argument checks: the workgroup's first argmin over
// latent_elem.h's (distance, index) pairs, and the pointer and size checks of the entries.
#pragma once
#include "common.h"
#include "latent_elem.h"

constexpr int VV_LE_WAVES = 4;           // waves of the 256-thread workgroup both stages launch

// The workgroup's minimum of (d, c) pairs in the order of vv_le_best_take; every thread gets the index.  red: [VV_LE_WAVES] pairs of LDS.
__device__ __forceinline__ int vv_le_block_argmin(VvLeBest s, VvLeBest *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(s.d, o, 64);
        const int oc = __shfl_xor(s.c, o, 64);
        vv_le_best_take(s, od, oc);
    }
    __syncthreads();                                   // a previous round's readers are done with red
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    VvLeBest r = vv_le_best_init();
#pragma unroll
    for (int w = 0; w < VV_LE_WAVES; ++w) vv_le_best_take(r, red[w].d, red[w].c);
    return vv_le_best_index(r);
}

inline bool vv_le_misaligned(const void *p, unsigned mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }
inline bool vv_le_dims_ok(int B, int L, int max_l) { return B >= 1 && L >= 1 && L <= max_l; }
