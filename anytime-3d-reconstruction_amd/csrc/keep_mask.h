// Bernoulli keep masks over a [batch, latent] latent from a counter-based generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw,
// "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the keep rule of the model classes' two masks -- the dropout mask of fit
// (Keras Dropout keeps where uniform >= rate) and the missing-latent mask of getEval (np.random.choice(2, n, p=[q, 1 - q]) is 1 where
// u >= q): keep = u >= p in both.  Plain C++ that compiles for the host and for the device alike (keep_mask.hip deals the blocks over
// threads and, through vv_keep_mask_host, runs the loop at the end of this file on the CPU), and without HIP (a plain C++ compiler).
//
// A mask is a pure function of (seed, offset, element): element e = b * latent + j takes word e & 3 of the Philox block with counter
// (blk_lo, blk_hi, offset_lo, offset_hi), blk = e >> 2, and key (seed_lo, seed_hi).  u = float(word >> 8) * 2^-24 is exact in float32
// and lies in [0, 1 - 2^-24]; keep = u >= rate ? 1.0f : 0.0f with the float32 rate.  Integer arithmetic and one exact conversion: the
// same bits on both sides.
//
// No inline assembly, no atomics, no memory besides the arguments.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VV_KM_HD __host__ __device__ inline
#else
#define VV_KM_HD inline
#endif

struct VvKmBlock {
    unsigned w[4];
};

VV_KM_HD unsigned vv_km_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * (unsigned long long)b) >> 32); }

// Philox4x32-10: counter c (four words), key (k0, k1)
VV_KM_HD VvKmBlock vv_km_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
    const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = vv_km_mulhi(M0, c0), lo0 = M0 * c0;
        const unsigned hi1 = vv_km_mulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    VvKmBlock o;
    o.w[0] = c0, o.w[1] = c1, o.w[2] = c2, o.w[3] = c3;
    return o;
}

// the four words of elements 4 * blk .. 4 * blk + 3
VV_KM_HD VvKmBlock vv_km_block(unsigned long long blk, unsigned long long seed, unsigned long long offset) {
    return vv_km_philox((unsigned)blk, (unsigned)(blk >> 32), (unsigned)offset, (unsigned)(offset >> 32), (unsigned)seed,
                        (unsigned)(seed >> 32));
}

VV_KM_HD float vv_km_uniform(unsigned word) { return (float)(word >> 8) * 5.9604644775390625e-08f; }     // 2^-24: both factors exact

VV_KM_HD float vv_km_keep(unsigned word, float rate) { return vv_km_uniform(word) >= rate ? 1.0f : 0.0f; }

// rate in [0, 1): a NaN fails both comparisons
VV_KM_HD bool vv_km_rate_ok(float rate) { return rate >= 0.0f && rate < 1.0f; }

// y = (x * keep) * scale, two float32 roundings (inverted dropout, forward on z and backward on dz alike)
VV_KM_HD float vv_km_mask_scale(float x, float keep, float scale) {
#pragma clang fp contract(off)
    const float t = x * keep;
    return t * scale;
}

// the whole mask on the CPU, in the device's block order
inline void vv_km_fill_all(float *keep, long long n, float rate, unsigned long long seed, unsigned long long offset) {
    for (long long blk = 0; 4 * blk < n; ++blk) {
        const VvKmBlock r = vv_km_block((unsigned long long)blk, seed, offset);
        for (int k = 0; k < 4 && 4 * blk + k < n; ++k) keep[4 * blk + k] = vv_km_keep(r.w[k], rate);
    }
}
