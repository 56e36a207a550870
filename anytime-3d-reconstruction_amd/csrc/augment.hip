// Pascal3D image batches built on the device (include/voxvae.h: vv_augment_images, vv_augment_draw and their host twins).  The arithmetic
// and every decision are csrc/augment.h (float64 for the warp and the cubic stage), shared with the host entries.
//
// vv_augment_images.  ONE launch for the batch: grid (output tiles, samples), a 256-thread workgroup per 16 x 16 output tile, per-sample
// sizes read from params.  An output pixel needs 4 x 4 warped levels, each made of 4 source reads, and neighbouring outputs share almost
// all of them, so a workgroup
//   1. works out its tile's footprint in the warped crop: rows clamp(i(first output row) - 1) .. clamp(i(last output row) + 2), columns
//      likewise (the tap index i of augment.h is monotone in the output index, so every clamped tap of the tile lies inside);
//   2. fills the footprint with warped levels, three channels packed in one 32-bit word, threads striding over it row-major;
//   3. after one barrier runs the cubic stage out of LDS, one output pixel (three floats) per thread.
// THE RULE for a footprint that does not fit: the footprint is about (15 * h / out_rows + 4) x (15 * w / out_cols + 4) words and the
// budget is AUG_LDS_WORDS = 12288 words (48 KiB: three workgroups per CU beside each other in the 160 KiB, and below the 64 KiB a kernel
// may take without opting in) -- crops up to about seven times the output in both directions.  The host fixes tile and budget per launch;
// the crop sizes are in device memory, so the comparison itself is made by each workgroup for its own tile (uniform inside the workgroup:
// every thread computes the same footprint): above the budget the workgroup takes the DIRECT form, each thread evaluating its pixel's 16
// warped levels itself, no LDS and no barrier.  Both forms call the same two functions of augment.h and give the same bits.
// A params row that augment.h refuses makes its workgroups return before anything is written (the host twin returns the status; a
// launch cannot).
//
// vv_augment_draw: a thread per sample, six Philox blocks, one 64-byte row.
// Plain C++: no inline assembly, no atomics, no workspace.  gfx950 only.
#include "common.h"
#include "augment.h"

namespace {

constexpr int AUG_TILE = 16;
constexpr int AUG_THREADS = AUG_TILE * AUG_TILE;
constexpr int AUG_LDS_WORDS = 12288;
constexpr int AUG_MAX_EXTENT = 0x7FFF;

struct AugLdsLevel {
    const unsigned *lds;
    int r0, c0, fh, fw;
    __device__ unsigned operator()(int r, int c) const {
        int rr = r - r0, cc = c - c0;
        rr = rr < 0 ? 0 : (rr >= fh ? fh - 1 : rr);                      // no-ops by the footprint's construction; they keep the read in the array
        cc = cc < 0 ? 0 : (cc >= fw ? fw - 1 : cc);
        return lds[rr * fw + cc];
    }
};

struct AugDirectLevel {
    const VvAugSample *a;
    __device__ unsigned operator()(int r, int c) const { return vv_aug_warp_level(*a, r, c); }
};

__global__ __launch_bounds__(AUG_THREADS) void augment_images_kernel(const unsigned char *__restrict__ images,
                                                                     const long long *__restrict__ image_meta, int n_images,
                                                                     const int *__restrict__ params, int out_rows, int out_cols,
                                                                     int tiles_x, float *__restrict__ out) {
    __shared__ unsigned levels[AUG_LDS_WORDS];
    const int b = blockIdx.y, tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    int p[VV_AUG_WORDS];
    for (int k = 0; k < VV_AUG_WORDS; ++k) p[k] = params[(size_t)b * VV_AUG_WORDS + k];
    VvAugSample a;
    if (vv_aug_sample(images, -1, image_meta, n_images, p, &a)) return;      // uniform: the whole workgroup leaves

    const double sy = vv_aug_scale(a.h, out_rows), sx = vv_aug_scale(a.w, out_cols);
    const int oy0 = tile_y * AUG_TILE, ox0 = tile_x * AUG_TILE;
    const int oy1 = min(oy0 + AUG_TILE, out_rows) - 1, ox1 = min(ox0 + AUG_TILE, out_cols) - 1;
    const int r0 = vv_aug_clamp(vv_aug_taps(oy0, sy).i - 1, a.h), r1 = vv_aug_clamp(vv_aug_taps(oy1, sy).i + 2, a.h);
    const int c0 = vv_aug_clamp(vv_aug_taps(ox0, sx).i - 1, a.w), c1 = vv_aug_clamp(vv_aug_taps(ox1, sx).i + 2, a.w);
    const int fh = r1 - r0 + 1, fw = c1 - c0 + 1;                            // >= 1: the tap index is monotone
    const bool in_lds = fh >= 1 && fw >= 1 && (long long)fh * fw <= AUG_LDS_WORDS;

    const int tid = threadIdx.x, oy = oy0 + tid / AUG_TILE, ox = ox0 + tid % AUG_TILE;
    const bool mine = oy < out_rows && ox < out_cols;
    float v[3];
    if (in_lds) {
        const int n = fh * fw;
        for (int i = tid; i < n; i += AUG_THREADS) {
            const int r = i / fw;
            levels[i] = vv_aug_warp_level(a, r0 + r, c0 + (i - r * fw));
        }
        __syncthreads();
        if (!mine) return;
        const AugLdsLevel level{levels, r0, c0, fh, fw};
        vv_aug_cubic_pixel(vv_aug_taps(oy, sy), vv_aug_taps(ox, sx), a.h, a.w, level, v);
    } else {
        if (!mine) return;
        const AugDirectLevel level{&a};
        vv_aug_cubic_pixel(vv_aug_taps(oy, sy), vv_aug_taps(ox, sx), a.h, a.w, level, v);
    }
    float *o = out + (((size_t)b * out_rows + oy) * out_cols + ox) * 3;
    o[0] = v[0], o[1] = v[1], o[2] = v[2];
}

__global__ __launch_bounds__(256) void augment_draw_kernel(const long long *__restrict__ image_meta, int n_images,
                                                           const int *__restrict__ image_index, const float *__restrict__ boxes, int batch,
                                                           int augmentation, unsigned long long seed, unsigned long long offset,
                                                           int *__restrict__ params) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    int p[VV_AUG_WORDS];
    (void)vv_aug_draw_one(image_meta, n_images, image_index, boxes, b, augmentation, seed, offset, p);
    for (int k = 0; k < VV_AUG_WORDS; ++k) params[(size_t)b * VV_AUG_WORDS + k] = p[k];
}

inline bool aug_misaligned(const void *p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

inline int aug_images_check(const void *images, const void *image_meta, int n_images, const void *params, int batch, int out_rows, int out_cols,
                            const void *out) {
    if (!images || !image_meta || !params || !out) return VV_ERR_NULL;
    if (n_images < 1 || batch < 1 || batch > 65535 || out_rows < 1 || out_cols < 1 || out_rows > AUG_MAX_EXTENT || out_cols > AUG_MAX_EXTENT)
        return VV_ERR_SHAPE;
    if (aug_misaligned(image_meta, 8) || aug_misaligned(params, 4) || aug_misaligned(out, 4)) return VV_ERR_ALIGN;
    return VV_OK;
}

inline int aug_draw_check(const void *image_meta, int n_images, const void *image_index, const void *boxes, int batch, const void *params) {
    if (!image_meta || !image_index || !boxes || !params) return VV_ERR_NULL;
    if (n_images < 1 || batch < 1 || batch > (1 << 24)) return VV_ERR_SHAPE;
    if (aug_misaligned(image_meta, 8) || aug_misaligned(image_index, 4) || aug_misaligned(boxes, 4) || aug_misaligned(params, 4)) return VV_ERR_ALIGN;
    return VV_OK;
}

}  // namespace

VV_EXPORT int vv_augment_images(const unsigned char *images, const long long *image_meta, int n_images, const int *params, int batch,
                                int out_rows, int out_cols, float *out, void *hip_stream) {
    const int rc = aug_images_check(images, image_meta, n_images, params, batch, out_rows, out_cols, out);
    if (rc != VV_OK) return rc;
    const int tiles_x = (out_cols + AUG_TILE - 1) / AUG_TILE, tiles_y = (out_rows + AUG_TILE - 1) / AUG_TILE;
    VV_LAUNCH(augment_images_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)batch), dim3(AUG_THREADS), 0,
              reinterpret_cast<hipStream_t>(hip_stream), images, image_meta, n_images, params, out_rows, out_cols, tiles_x, out);
    return vv_launch_status();
}

VV_EXPORT int vv_augment_images_host(const unsigned char *images, const long long *image_meta, int n_images, const int *params, int batch,
                                     int out_rows, int out_cols, float *out) {
    const int rc = aug_images_check(images, image_meta, n_images, params, batch, out_rows, out_cols, out);
    if (rc != VV_OK) return rc;
    return vv_aug_images_all(images, -1, image_meta, n_images, params, batch, out_rows, out_cols, out) ? VV_ERR_SHAPE : VV_OK;
}

// The admissibility of params rows alone, on the host (what vv_augment_images_host checks before it writes): image_meta and params are
// host pointers.
VV_EXPORT int vv_augment_check_host(const long long *image_meta, int n_images, const int *params, int batch) {
    if (!image_meta || !params) return VV_ERR_NULL;
    if (n_images < 1 || batch < 1) return VV_ERR_SHAPE;
    if (aug_misaligned(image_meta, 8) || aug_misaligned(params, 4)) return VV_ERR_ALIGN;
    return vv_aug_check_all(nullptr, -1, image_meta, n_images, params, batch) ? VV_ERR_SHAPE : VV_OK;
}

VV_EXPORT int vv_augment_draw(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                              int augmentation, unsigned long long seed, unsigned long long offset, int *params, void *hip_stream) {
    const int rc = aug_draw_check(image_meta, n_images, image_index, boxes, batch, params);
    if (rc != VV_OK) return rc;
    VV_LAUNCH(augment_draw_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), image_meta,
              n_images, image_index, boxes, batch, augmentation ? 1 : 0, seed, offset, params);
    return vv_launch_status();
}

VV_EXPORT int vv_augment_draw_host(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                                   int augmentation, unsigned long long seed, unsigned long long offset, int *params) {
    const int rc = aug_draw_check(image_meta, n_images, image_index, boxes, batch, params);
    if (rc != VV_OK) return rc;
    return vv_aug_draw_all(image_meta, n_images, image_index, boxes, batch, augmentation ? 1 : 0, seed, offset, params) ? VV_ERR_SHAPE : VV_OK;
}
