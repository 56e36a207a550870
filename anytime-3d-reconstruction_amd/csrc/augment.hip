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
// vv_augment_draw: a thread per sample, six Philox blocks, one 64-byte row.  vv_augment_draw_ex: the same thread also writes the sample's
// 16-byte colour row (augment.h: blur and hue/saturation, out of the same six blocks).
//
// vv_augment_images_ex.  TWO launches.  The first is the colour pre-pass (augment_colour_kernel): for every sample whose colour row has a
// flag set it writes the finished source level (blur -> invert -> add -> hue/saturation) of each crop pixel, three channels packed in
// a word, into the sample's slab of the workspace (sample b owns words b * max_rows * max_cols ..., row stride w).  The second is the
// kernel above with one change: a flagged sample's source read comes out of its slab, every other sample's from the image as before.
// The blur is a neighbourhood operation, so the pre-pass is a kernel of its own: grid (32 x 32 tiles of a max_rows x max_cols crop,
// samples), 256 threads.  The grid only says how many workgroups a sample gets: each sample's workgroups walk that sample's OWN
// ceil(h / 32) * ceil(w / 32) tiles in a strided loop, because a crop is admitted on h * w <= max_rows * max_cols alone and may be
// taller or wider than that rectangle (100 x 10 in slabs of 10 x 100): every word that the second launch reads has been written.
// A workgroup without a tile returns, and so do all workgroups of a sample with flags 0.  Per tile a workgroup
//   1. has thread k work out the unnormalised weight u_k (vv_aug_blur_tap), every thread sum them left to right, thread k divide;
//   2. stages the tile plus a halo of r raw levels on every side as packed words in LDS, mirror already applied (56 x 56 words);
//   3. runs axis 0 into a float64 LDS array (3 x 32 x 56), threads along a row so that neighbouring lanes read neighbouring words;
//   4. runs axis 1 out of it, four pixels per thread, then invert / add / hue-saturation and one packed store per pixel.
// 12544 + 43008 + 1032 bytes of LDS: below the 64 KiB a kernel may take without opting in, two workgroups per CU.
// THE RULE for a radius that the staging does not hold: r = (int)(4 sigma + 0.5) <= COL_MAX_R = 12 (sigma < 3.125: every sigma that is
// drawn) takes the staged form; a larger r (sigma up to 16: r <= 64) takes the DIRECT form, each thread summing the (2r + 1)^2 taps of
// its pixels from the image (vv_aug_blur_direct) -- the same products and sums in the same order, hence the same bits.  r is a property
// of the sample, so the choice is uniform inside a workgroup.  The direct form is a slow path ((2r + 1)^2 image reads per pixel, up to
// 16641), reachable through injected tables only and not measured.  r == 0 (no blur flag, or a sigma under 0.125) skips 1 .. 3.
// A row that augment.h refuses -- its params row, its colour row, or a flagged crop of more than max_rows * max_cols pixels -- makes
// its workgroups return in BOTH launches before anything is written.  The workspace is written before it is read (only flagged
// samples' slabs are read, and the pre-pass has written every word that the second launch reads), and nothing depends on its size
// beyond the minimum.
// Plain C++: no inline assembly, no atomics; no workspace besides the slabs of the _ex entry.  gfx950 only.
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
    VvAugSlabSource source;
    __device__ unsigned operator()(int r, int c) const { return vv_aug_warp_level(*a, r, c, source); }
};

// EX: the second launch of vv_augment_images_ex (colour and slabs are read); without it the three arguments are unused
template <bool EX>
__global__ __launch_bounds__(AUG_THREADS) void augment_images_kernel(const unsigned char *__restrict__ images,
                                                                     const long long *__restrict__ image_meta, int n_images,
                                                                     const int *__restrict__ params, int out_rows, int out_cols,
                                                                     int tiles_x, float *__restrict__ out, const int *__restrict__ colour,
                                                                     const unsigned *__restrict__ slabs, long long slab_words) {
    __shared__ unsigned levels[AUG_LDS_WORDS];
    const int b = blockIdx.y, tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
    int p[VV_AUG_WORDS];
    for (int k = 0; k < VV_AUG_WORDS; ++k) p[k] = params[(size_t)b * VV_AUG_WORDS + k];
    VvAugSample a;
    if (vv_aug_sample(images, -1, image_meta, n_images, p, &a)) return;      // uniform: the whole workgroup leaves
    VvAugSlabSource source{nullptr};
    if (EX) {
        int cw[VV_AUG_COLOUR_WORDS];
        for (int k = 0; k < VV_AUG_COLOUR_WORDS; ++k) cw[k] = colour[(size_t)b * VV_AUG_COLOUR_WORDS + k];
        VvAugColour c;
        if (vv_aug_colour(cw, &c)) return;
        if (c.flags) {
            if ((long long)a.h * a.w > slab_words) return;
            source.slab = slabs + (size_t)b * (size_t)slab_words;
        }
    }

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
            levels[i] = vv_aug_warp_level(a, r0 + r, c0 + (i - r * fw), source);
        }
        __syncthreads();
        if (!mine) return;
        const AugLdsLevel level{levels, r0, c0, fh, fw};
        vv_aug_cubic_pixel(vv_aug_taps(oy, sy), vv_aug_taps(ox, sx), a.h, a.w, level, v);
    } else {
        if (!mine) return;
        const AugDirectLevel level{&a, source};
        vv_aug_cubic_pixel(vv_aug_taps(oy, sy), vv_aug_taps(ox, sx), a.h, a.w, level, v);
    }
    float *o = out + (((size_t)b * out_rows + oy) * out_cols + ox) * 3;
    o[0] = v[0], o[1] = v[1], o[2] = v[2];
}

// ---------------------------------------------------------------------------------------------------------------- the colour pre-pass
constexpr int COL_TILE = 32;
constexpr int COL_THREADS = 256;
constexpr int COL_MAX_R = 12;                                                // the halo that the staging holds
constexpr int COL_SPAN = COL_TILE + 2 * COL_MAX_R;                           // 56

struct AugRaw {
    const VvAugSample *a;
    __device__ unsigned operator()(int y, int x) const { return vv_aug_raw(*a, y, x); }
};

__global__ __launch_bounds__(COL_THREADS) void augment_colour_kernel(const unsigned char *__restrict__ images,
                                                                     const long long *__restrict__ image_meta, int n_images,
                                                                     const int *__restrict__ params, const int *__restrict__ colour,
                                                                     unsigned *__restrict__ slabs, long long slab_words) {
#pragma clang fp contract(off)
    __shared__ unsigned raw[COL_SPAN * COL_SPAN];
    __shared__ double tmp[3 * COL_TILE * COL_SPAN];
    __shared__ double wts[2 * VV_AUG_BLUR_MAX_R + 1];
    const int b = blockIdx.y;
    int cw[VV_AUG_COLOUR_WORDS];
    for (int k = 0; k < VV_AUG_COLOUR_WORDS; ++k) cw[k] = colour[(size_t)b * VV_AUG_COLOUR_WORDS + k];
    VvAugColour c;
    if (vv_aug_colour(cw, &c) || !c.flags) return;                           // uniform, like every return below
    int p[VV_AUG_WORDS];
    for (int k = 0; k < VV_AUG_WORDS; ++k) p[k] = params[(size_t)b * VV_AUG_WORDS + k];
    VvAugSample a;
    if (vv_aug_sample(images, -1, image_meta, n_images, p, &a)) return;
    if ((long long)a.h * a.w > slab_words) return;
    // The sample's OWN tiles, dealt over the grid's workgroups in a strided loop: the grid is sized from max_rows x max_cols, and a crop
    // is admitted on h * w alone, so it may be taller or wider than that rectangle (100 x 10 in slabs of 10 x 100).
    const int tiles_x = (a.w + COL_TILE - 1) / COL_TILE, n_tiles = tiles_x * ((a.h + COL_TILE - 1) / COL_TILE);      // <= 2^20
    if ((int)blockIdx.x >= n_tiles) return;
    unsigned *slab = slabs + (size_t)b * (size_t)slab_words;
    const int tid = threadIdx.x, r = c.r;                                    // r <= VV_AUG_BLUR_MAX_R: vv_aug_colour holds sigma to 16

    if (r == 0) {
        for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
            const int y0 = (tile / tiles_x) * COL_TILE, x0 = (tile % tiles_x) * COL_TILE;
            for (int i = tid; i < COL_TILE * COL_TILE; i += COL_THREADS) {
                const int y = y0 + i / COL_TILE, x = x0 + i % COL_TILE;
                if (y < a.h && x < a.w) slab[(size_t)y * a.w + x] = vv_aug_finish(a, c, vv_aug_raw(a, y, x));
            }
        }
        return;
    }
    const int n = 2 * r + 1;                                                 // <= 129 < COL_THREADS
    if (tid < n) wts[tid] = vv_aug_blur_tap(tid - r, c.sigma);
    __syncthreads();
    double sum = wts[0];
    for (int i = 1; i < n; ++i) sum = sum + wts[i];
    __syncthreads();
    if (tid < n) wts[tid] = wts[tid] / sum;

    // tile is uniform in the workgroup, so every barrier below is reached by all threads or by none.  Between two tiles no further
    // barrier is needed: raw is rewritten only after the barrier that follows its last read, and tmp only after the next staging's.
    for (int tile = (int)blockIdx.x; tile < n_tiles; tile += (int)gridDim.x) {
        const int y0 = (tile / tiles_x) * COL_TILE, x0 = (tile % tiles_x) * COL_TILE;
        if (r <= COL_MAX_R) {
            const int span = COL_TILE + 2 * r;                                   // <= COL_SPAN
            for (int i = tid; i < span * span; i += COL_THREADS) {
                const int yy = i / span, xx = i - yy * span;
                raw[yy * COL_SPAN + xx] = vv_aug_raw(a, vv_aug_mirror(y0 - r + yy, a.h), vv_aug_mirror(x0 - r + xx, a.w));
            }
            __syncthreads();
            for (int i = tid; i < COL_TILE * span; i += COL_THREADS) {          // axis 0: t(y0 + yy, column x0 - r + xx)
                const int yy = i / span, xx = i - yy * span;
                double t[3] = {0.0, 0.0, 0.0};
                for (int k = 0; k < n; ++k) {
                    const unsigned px = raw[(yy + k) * COL_SPAN + xx];
                    const double wk = wts[k];
                    for (int ch = 0; ch < 3; ++ch) {
                        const double m = wk * (double)((px >> (8 * ch)) & 255u);
                        t[ch] = k == 0 ? m : t[ch] + m;
                    }
                }
                for (int ch = 0; ch < 3; ++ch) tmp[(ch * COL_TILE + yy) * COL_SPAN + xx] = t[ch];
            }
            __syncthreads();
            for (int i = tid; i < COL_TILE * COL_TILE; i += COL_THREADS) {      // axis 1
                const int yy = i / COL_TILE, xx = i % COL_TILE;
                const int y = y0 + yy, x = x0 + xx;
                if (y >= a.h || x >= a.w) continue;
                double v[3] = {0.0, 0.0, 0.0};
                for (int k = 0; k < n; ++k) {
                    const double wk = wts[k];
                    for (int ch = 0; ch < 3; ++ch) {
                        const double m = wk * tmp[(ch * COL_TILE + yy) * COL_SPAN + xx + k];
                        v[ch] = k == 0 ? m : v[ch] + m;
                    }
                }
                slab[(size_t)y * a.w + x] = vv_aug_finish(a, c, vv_aug_pack_levels(v));
            }
        } else {
            __syncthreads();
            const AugRaw src{&a};
            for (int i = tid; i < COL_TILE * COL_TILE; i += COL_THREADS) {
                const int y = y0 + i / COL_TILE, x = x0 + i % COL_TILE;
                if (y < a.h && x < a.w) slab[(size_t)y * a.w + x] = vv_aug_finish(a, c, vv_aug_blur_direct(a.h, a.w, r, wts, y, x, src));
            }
        }
    }
}

__global__ __launch_bounds__(256) void augment_draw_kernel(const long long *__restrict__ image_meta, int n_images,
                                                           const int *__restrict__ image_index, const float *__restrict__ boxes, int batch,
                                                           int augmentation, unsigned long long seed, unsigned long long offset,
                                                           int *__restrict__ params, int *__restrict__ colour) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    int p[VV_AUG_WORDS], c[VV_AUG_COLOUR_WORDS];
    (void)vv_aug_draw_pair(image_meta, n_images, image_index, boxes, b, augmentation, seed, offset, p, c);
    for (int k = 0; k < VV_AUG_WORDS; ++k) params[(size_t)b * VV_AUG_WORDS + k] = p[k];
    if (colour)
        for (int k = 0; k < VV_AUG_COLOUR_WORDS; ++k) colour[(size_t)b * VV_AUG_COLOUR_WORDS + k] = c[k];
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

inline int aug_images_ex_check(const void *images, const void *image_meta, int n_images, const void *params, int batch, int out_rows,
                               int out_cols, const void *out, const void *colour, const void *workspace, size_t workspace_bytes, int max_rows,
                               int max_cols) {
    const int rc = aug_images_check(images, image_meta, n_images, params, batch, out_rows, out_cols, out);
    if (rc != VV_OK) return rc;
    if (!workspace) return VV_ERR_NULL;
    if (max_rows < 1 || max_cols < 1 || max_rows > AUG_MAX_EXTENT || max_cols > AUG_MAX_EXTENT) return VV_ERR_SHAPE;
    if (aug_misaligned(colour, 4) || aug_misaligned(workspace, 4)) return VV_ERR_ALIGN;
    if (workspace_bytes < (size_t)max_rows * (size_t)max_cols * (size_t)batch * sizeof(unsigned)) return VV_ERR_WORKSPACE;
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
    VV_LAUNCH(augment_images_kernel<false>, dim3((unsigned)(tiles_x * tiles_y), (unsigned)batch), dim3(AUG_THREADS), 0,
              reinterpret_cast<hipStream_t>(hip_stream), images, image_meta, n_images, params, out_rows, out_cols, tiles_x, out,
              static_cast<const int *>(nullptr), static_cast<const unsigned *>(nullptr), 0ll);
    return vv_launch_status();
}

VV_EXPORT size_t vv_augment_colour_workspace_bytes(int max_rows, int max_cols, int batch) {
    if (max_rows < 1 || max_cols < 1 || batch < 1 || max_rows > AUG_MAX_EXTENT || max_cols > AUG_MAX_EXTENT) return 0;
    return (size_t)max_rows * (size_t)max_cols * (size_t)batch * sizeof(unsigned);
}

VV_EXPORT int vv_augment_images_ex(const unsigned char *images, const long long *image_meta, int n_images, const int *params, int batch,
                                   int out_rows, int out_cols, float *out, const int *colour, void *workspace, size_t workspace_bytes,
                                   int max_rows, int max_cols, void *hip_stream) {
    if (!colour) return vv_augment_images(images, image_meta, n_images, params, batch, out_rows, out_cols, out, hip_stream);
    const int rc = aug_images_ex_check(images, image_meta, n_images, params, batch, out_rows, out_cols, out, colour, workspace,
                                       workspace_bytes, max_rows, max_cols);
    if (rc != VV_OK) return rc;
    const long long slab_words = (long long)max_rows * max_cols;
    const hipStream_t stream = reinterpret_cast<hipStream_t>(hip_stream);
    const int ctx = (max_cols + COL_TILE - 1) / COL_TILE, cty = (max_rows + COL_TILE - 1) / COL_TILE;
    VV_LAUNCH(augment_colour_kernel, dim3((unsigned)(ctx * cty), (unsigned)batch), dim3(COL_THREADS), 0, stream, images, image_meta, n_images,
              params, colour, static_cast<unsigned *>(workspace), slab_words);
    const int rc1 = vv_launch_status();
    if (rc1 != VV_OK) return rc1;
    const int tiles_x = (out_cols + AUG_TILE - 1) / AUG_TILE, tiles_y = (out_rows + AUG_TILE - 1) / AUG_TILE;
    VV_LAUNCH(augment_images_kernel<true>, dim3((unsigned)(tiles_x * tiles_y), (unsigned)batch), dim3(AUG_THREADS), 0, stream, images,
              image_meta, n_images, params, out_rows, out_cols, tiles_x, out, colour, static_cast<const unsigned *>(workspace), slab_words);
    return vv_launch_status();
}

VV_EXPORT int vv_augment_images_ex_host(const unsigned char *images, const long long *image_meta, int n_images, const int *params, int batch,
                                        int out_rows, int out_cols, float *out, const int *colour, void *workspace, size_t workspace_bytes,
                                        int max_rows, int max_cols) {
    if (!colour) return vv_augment_images_host(images, image_meta, n_images, params, batch, out_rows, out_cols, out);
    const int rc = aug_images_ex_check(images, image_meta, n_images, params, batch, out_rows, out_cols, out, colour, workspace,
                                       workspace_bytes, max_rows, max_cols);
    if (rc != VV_OK) return rc;
    return vv_aug_images_all_ex(images, -1, image_meta, n_images, params, colour, static_cast<unsigned *>(workspace),
                                (long long)max_rows * max_cols, batch, out_rows, out_cols, out)
               ? VV_ERR_SHAPE
               : VV_OK;
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
              n_images, image_index, boxes, batch, augmentation ? 1 : 0, seed, offset, params, static_cast<int *>(nullptr));
    return vv_launch_status();
}

VV_EXPORT int vv_augment_draw_ex(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                                 int augmentation, unsigned long long seed, unsigned long long offset, int *params, int *colour,
                                 void *hip_stream) {
    const int rc = aug_draw_check(image_meta, n_images, image_index, boxes, batch, params);
    if (rc != VV_OK) return rc;
    if (!colour) return VV_ERR_NULL;
    if (aug_misaligned(colour, 4)) return VV_ERR_ALIGN;
    VV_LAUNCH(augment_draw_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), image_meta,
              n_images, image_index, boxes, batch, augmentation ? 1 : 0, seed, offset, params, colour);
    return vv_launch_status();
}

VV_EXPORT int vv_augment_draw_ex_host(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                                      int augmentation, unsigned long long seed, unsigned long long offset, int *params, int *colour) {
    const int rc = aug_draw_check(image_meta, n_images, image_index, boxes, batch, params);
    if (rc != VV_OK) return rc;
    if (!colour) return VV_ERR_NULL;
    if (aug_misaligned(colour, 4)) return VV_ERR_ALIGN;
    return vv_aug_draw_all_ex(image_meta, n_images, image_index, boxes, batch, augmentation ? 1 : 0, seed, offset, params, colour) ? VV_ERR_SHAPE
                                                                                                                                   : VV_OK;
}

VV_EXPORT int vv_augment_draw_host(const long long *image_meta, int n_images, const int *image_index, const float *boxes, int batch,
                                   int augmentation, unsigned long long seed, unsigned long long offset, int *params) {
    const int rc = aug_draw_check(image_meta, n_images, image_index, boxes, batch, params);
    if (rc != VV_OK) return rc;
    return vv_aug_draw_all(image_meta, n_images, image_index, boxes, batch, augmentation ? 1 : 0, seed, offset, params) ? VV_ERR_SHAPE : VV_OK;
}
