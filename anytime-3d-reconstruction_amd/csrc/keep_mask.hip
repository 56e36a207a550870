// Keep masks drawn on the device and inverted dropout on a float32 latent (include/voxvae.h: vv_keep_mask, vv_keep_mask_host,
// vv_mask_scale).  The arithmetic is csrc/keep_mask.h, shared with the host entry; here a thread takes one block of four elements:
// one Philox4x32-10 evaluation and one 16-byte store (vv_keep_mask), two 16-byte loads and one 16-byte store (vv_mask_scale).  The last
// block of a tensor whose element count is no multiple of four goes out element by element.  Plain C++: no inline assembly, no atomics.
#include "common.h"
#include "keep_mask.h"

namespace {

constexpr int KM_THREADS = 256;
// four floats at the alignment of one: the entries ask no more of their pointers than float alignment
typedef f32x4 km_f32x4 __attribute__((aligned(4)));

__global__ __launch_bounds__(KM_THREADS) void keep_mask_kernel(float *__restrict__ keep, long long n, float rate, unsigned long long seed,
                                                               unsigned long long offset) {
    const long long blk = (long long)blockIdx.x * KM_THREADS + threadIdx.x;
    const long long e = 4 * blk;
    if (e >= n) return;
    const VvKmBlock r = vv_km_block((unsigned long long)blk, seed, offset);
    if (e + 4 <= n) {
        km_f32x4 v;
        v[0] = vv_km_keep(r.w[0], rate), v[1] = vv_km_keep(r.w[1], rate), v[2] = vv_km_keep(r.w[2], rate), v[3] = vv_km_keep(r.w[3], rate);
        *reinterpret_cast<km_f32x4 *>(keep + e) = v;
    } else {
        for (int k = 0; k < 3; ++k)      // a tail holds one to three elements
            if (e + k < n) keep[e + k] = vv_km_keep(r.w[k], rate);
    }
}

__global__ __launch_bounds__(KM_THREADS) void mask_scale_kernel(const float *__restrict__ x, const float *__restrict__ keep, float scale,
                                                                float *__restrict__ y, long long n) {
    const long long e = 4 * ((long long)blockIdx.x * KM_THREADS + threadIdx.x);
    if (e >= n) return;
    if (e + 4 <= n) {
        const km_f32x4 a = *reinterpret_cast<const km_f32x4 *>(x + e), m = *reinterpret_cast<const km_f32x4 *>(keep + e);
        km_f32x4 v;
        for (int k = 0; k < 4; ++k) v[k] = vv_km_mask_scale(a[k], m[k], scale);
        *reinterpret_cast<km_f32x4 *>(y + e) = v;
    } else {
        for (int k = 0; k < 3; ++k)
            if (e + k < n) y[e + k] = vv_km_mask_scale(x[e + k], keep[e + k], scale);
    }
}

inline bool km_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) != 0; }

// -> the element count, or a negative status
inline long long km_count(int batch, int latent) {
    if (batch <= 0 || latent <= 0) return VV_ERR_SHAPE;
    const long long n = (long long)batch * latent;
    return n > 0x7FFFFFFFll ? (long long)VV_ERR_SHAPE : n;
}

inline long long km_mask_check(const float *keep, int batch, int latent, float rate) {
    if (!keep) return VV_ERR_NULL;
    const long long n = km_count(batch, latent);
    if (n < 0) return n;
    if (!vv_km_rate_ok(rate)) return VV_ERR_SHAPE;
    if (km_misaligned(keep)) return VV_ERR_ALIGN;
    return n;
}

inline unsigned km_grid(long long n) { return (unsigned)(((n + 3) / 4 + KM_THREADS - 1) / KM_THREADS); }

}  // namespace

VV_EXPORT int vv_keep_mask(float *keep, int batch, int latent, float rate, unsigned long long seed, unsigned long long offset,
                           void *hip_stream) {
    const long long n = km_mask_check(keep, batch, latent, rate);
    if (n < 0) return (int)n;
    VV_LAUNCH(keep_mask_kernel, dim3(km_grid(n)), dim3(KM_THREADS), 0, reinterpret_cast<hipStream_t>(hip_stream), keep, n, rate, seed, offset);
    return vv_launch_status();
}

VV_EXPORT int vv_keep_mask_host(float *keep, int batch, int latent, float rate, unsigned long long seed, unsigned long long offset) {
    const long long n = km_mask_check(keep, batch, latent, rate);
    if (n < 0) return (int)n;
    vv_km_fill_all(keep, n, rate, seed, offset);
    return VV_OK;
}

VV_EXPORT int vv_mask_scale(const float *x, const float *keep, float scale, float *y, int batch, int latent, void *hip_stream) {
    if (!x || !keep || !y) return VV_ERR_NULL;
    const long long n = km_count(batch, latent);
    if (n < 0) return (int)n;
    if (km_misaligned(x) || km_misaligned(keep) || km_misaligned(y)) return VV_ERR_ALIGN;
    VV_LAUNCH(mask_scale_kernel, dim3(km_grid(n)), dim3(KM_THREADS), 0, reinterpret_cast<hipStream_t>(hip_stream), x, keep, scale, y, n);
    return vv_launch_status();
}
