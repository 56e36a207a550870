// The optimiser tail of the data-parallel 3D autoencoder (src/module/AE3D.py): Keras Adam with the kernel regulariser's gradient
// folded in and its loss value left behind by the same pass, and the step's six scalars in one small launch.
#include "common.h"

// vv_adam_step_multi's record plus the chunk's coefficient (voxvae.h has the layout); one workgroup per chunk.
struct AdamL2Chunk { float *p; const float *g; float *m; float *v; long n; float coef; float pad; };
static_assert(sizeof(AdamL2Chunk) == 48, "the table is built on the host as six 8-byte words per record");

// Same arithmetic as adam_multi_kernel (train.hip) on g_eff = fma(coef, w, g); a chunk with coef == 0 takes g itself, so that it gives
// that kernel's bits.  sum w^2 of the weights as read: each thread over its <= 64 strided elements in index order, the 64 lanes of a wave by
// the xor butterfly, the four wave sums as (s0 + s1) + (s2 + s3).  Nothing depends on timing: the same state gives the same bits.
__global__ __launch_bounds__(256) void adam_multi_l2_kernel(const AdamL2Chunk *__restrict__ table, float lr_t, float b1, float b2, float eps,
                                                            float *__restrict__ sumsq_partial) {
    __shared__ float red[4];
    const AdamL2Chunk c = table[blockIdx.x];
    if (c.coef == 0.f) {
        for (long i = threadIdx.x; i < c.n; i += 256) {
            const float gi = c.g[i];
            const float mi = b1 * c.m[i] + (1.f - b1) * gi;
            const float vi = b2 * c.v[i] + (1.f - b2) * gi * gi;
            c.m[i] = mi; c.v[i] = vi;
            c.p[i] -= lr_t * mi / (sqrtf(vi) + eps);
        }
        if (threadIdx.x == 0) sumsq_partial[blockIdx.x] = 0.f;
        return;
    }
    float s = 0.f;
    for (long i = threadIdx.x; i < c.n; i += 256) {
        const float w = c.p[i];
        const float gi = fmaf(c.coef, w, c.g[i]);
        s = fmaf(w, w, s);
        const float mi = b1 * c.m[i] + (1.f - b1) * gi;
        const float vi = b2 * c.v[i] + (1.f - b2) * gi * gi;
        c.m[i] = mi; c.v[i] = vi;
        c.p[i] = w - lr_t * mi / (sqrtf(vi) + eps);
    }
    s = vv_wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sumsq_partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// One wave.  Every sum in double: lane l adds elements l, l + 64, ... in index order, lane 0 then adds the 64 lane sums in lane order.
// (The counts are integers below 2^53 and add exactly; bce and the partials lose nothing a float32 result could show.)
__global__ __launch_bounds__(64) void ae3d_step_scalars_kernel(const float *__restrict__ stats, int batch, const float *__restrict__ sumsq_partial,
                                                               int nchunks, float l2, float inv_gb, float *__restrict__ out6) {
    __shared__ double red[5][64];
    const int lane = threadIdx.x;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = lane; i < nchunks; i += 64) a[0] += (double)sumsq_partial[i];
    for (int b = lane; b < batch; b += 64) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[1 + k] += (double)stats[4 * (long)b + k];
    }
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k][lane] = a[k];
    __syncthreads();
    if (lane == 0) {
        double t[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            t[k] = 0.0;
            for (int l = 0; l < 64; ++l) t[k] += red[k][l];
        }
        const float reg = (float)((double)l2 * t[0]), pred = (float)(t[1] * (double)inv_gb);
        out6[0] = reg;
        out6[1] = pred;
        out6[2] = reg + pred;
        out6[3] = (float)(t[2] * (double)inv_gb);
        out6[4] = (float)(t[3] * (double)inv_gb);
        out6[5] = (float)(t[4] * (double)inv_gb);
    }
}

VV_EXPORT int vv_adam_step_multi_l2(const void *chunk_table, int nchunks, float lr_t, float beta1, float beta2, float epsilon,
                                    float *sumsq_partial, void *hip_stream) {
    if (!chunk_table || !sumsq_partial) return VV_ERR_NULL;
    if (nchunks <= 0) return VV_ERR_SHAPE;
    VV_LAUNCH(adam_multi_l2_kernel, dim3(nchunks), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream),
              reinterpret_cast<const AdamL2Chunk *>(chunk_table), lr_t, beta1, beta2, epsilon, sumsq_partial);
    return vv_launch_status();
}

VV_EXPORT int vv_ae3d_step_scalars(const float *stats, int batch, const float *sumsq_partial, int nchunks, float l2, float inv_global_batch,
                                   float *out6, void *hip_stream) {
    if (!stats || !out6 || (!sumsq_partial && nchunks > 0)) return VV_ERR_NULL;
    if (batch <= 0 || nchunks < 0) return VV_ERR_SHAPE;
    VV_LAUNCH(ae3d_step_scalars_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(hip_stream), stats, batch, sumsq_partial, nchunks,
              l2, inv_global_batch, out6);
    return vv_launch_status();
}
