// What the training step (reference nolbo.py:1411-1447 `fit`) needs besides the layer kernels, BatchNorm (bn.hip) and the weight
// gradients (wgrad.hip, wgrad_phase.hip): the adjoints of the two "layer as a dense panel" packings and a float32 transpose, the
// BCE and reparameterisation / KL backward, Keras Adam (one tensor per launch, or every tensor through a chunk table) and the
// column sum of a float32 or bf16 matrix (Dense bias gradient).  All element-wise or small reductions in float32.  gfx950.
#include "common.h"

namespace {

// Adjoints of the two "layer as a dense panel" packings (vv_pack_conv_k4s1_meanpool / vv_pack_convT_k4s1_dense).
__global__ void unpack_meanpool_grad_kernel(const float *__restrict__ dpanel, float *__restrict__ dw, int side, int cin, int cout) {
    // dw[t][ci][co] = (1/S^3) sum_{(i,o) : i - o + 1 = t per axis} dpanel[co][i*cin + ci]
    const int S3 = side * side * side;
    const long total = (long)64 * cin * cout;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int co = (int)(idx % cout), ci = (int)((idx / cout) % cin), t = (int)(idx / ((long)cout * cin));
        const int td = t >> 4, th = (t >> 2) & 3, tw = t & 3;
        float s = 0.f;
        for (int od = 0; od < side; ++od) {
            const int id = od + td - 1;
            if ((unsigned)id >= (unsigned)side) continue;
            for (int oh = 0; oh < side; ++oh) {
                const int ih = oh + th - 1;
                if ((unsigned)ih >= (unsigned)side) continue;
                for (int ow = 0; ow < side; ++ow) {
                    const int iw = ow + tw - 1;
                    if ((unsigned)iw >= (unsigned)side) continue;
                    s += dpanel[(size_t)co * S3 * cin + (size_t)((id * side + ih) * side + iw) * cin + ci];
                }
            }
        }
        dw[idx] = s / (float)S3;
    }
}

// The same through a 64 x 64 LDS tile (cin % 64 == 0, cout % 64 == 0): block (tap t, 64 ci, 64 co) sums the valid (i, o) pairs with
// 16-byte reads along ci (a dpanel row is contiguous in k = i * cin + ci) and writes dw rows contiguous in co.
__global__ __launch_bounds__(256) void unpack_meanpool_grad_tiled_kernel(const float *__restrict__ dpanel, float *__restrict__ dw, int side, int cin, int cout) {
    __shared__ float tile[64][65];
    const int S3 = side * side * side, tid = threadIdx.x;
    const int nci = cin >> 6;
    const int t = blockIdx.x / nci, ci0 = (blockIdx.x % nci) * 64, co0 = blockIdx.y * 64;
    const int td = t >> 4, th = (t >> 2) & 3, tw = t & 3;
    const int c4 = tid & 15, r = tid >> 4;                 // ci quad, co row (16 per pass)
    f32x4 s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int od = 0; od < side; ++od) {
        const int id = od + td - 1;
        if ((unsigned)id >= (unsigned)side) continue;
        for (int oh = 0; oh < side; ++oh) {
            const int ih = oh + th - 1;
            if ((unsigned)ih >= (unsigned)side) continue;
            for (int ow = 0; ow < side; ++ow) {
                const int iw = ow + tw - 1;
                if ((unsigned)iw >= (unsigned)side) continue;
                const float *src = dpanel + (size_t)co0 * S3 * cin + (size_t)((id * side + ih) * side + iw) * cin + ci0 + 4 * c4;
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] += *reinterpret_cast<const f32x4 *>(src + (size_t)(r + 16 * j) * S3 * cin);
            }
        }
    }
    const float inv = 1.0f / (float)S3;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) tile[4 * c4 + e][r + 16 * j] = s[j][e] * inv;      // [ci][co]
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int cil = r + 16 * j;
        *reinterpret_cast<f32x4 *>(dw + ((size_t)t * cin + ci0 + cil) * cout + co0 + 4 * c4) =
            f32x4{tile[cil][4 * c4], tile[cil][4 * c4 + 1], tile[cil][4 * c4 + 2], tile[cil][4 * c4 + 3]};
    }
}

__global__ void unpack_convT_dense_grad_kernel(const float *__restrict__ dpanel, float *__restrict__ dw, int side, int cin, int cout) {
    // dw[t][co][ci] = sum_{(o,j) : o - j + 1 = t per axis} dpanel[(o,co)][(j,ci)]
    const int S3 = side * side * side, K = S3 * cin;
    const long total = (long)64 * cin * cout;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int ci = (int)(idx % cin), co = (int)((idx / cin) % cout), t = (int)(idx / ((long)cout * cin));
        const int td = t >> 4, th = (t >> 2) & 3, tw = t & 3;
        float s = 0.f;
        for (int jd = 0; jd < side; ++jd) {
            const int od = jd + td - 1;
            if ((unsigned)od >= (unsigned)side) continue;
            for (int jh = 0; jh < side; ++jh) {
                const int oh = jh + th - 1;
                if ((unsigned)oh >= (unsigned)side) continue;
                for (int jw = 0; jw < side; ++jw) {
                    const int ow = jw + tw - 1;
                    if ((unsigned)ow >= (unsigned)side) continue;
                    const int o = (od * side + oh) * side + ow, j = (jd * side + jh) * side + jw;
                    s += dpanel[((size_t)o * cout + co) * K + (size_t)j * cin + ci];
                }
            }
        }
        dw[idx] = s;
    }
}

__global__ void transpose_kernel(const float *__restrict__ in, float *__restrict__ out, int rows, int cols) {
    __shared__ float tile[32][33];
    const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int r = by + j, c = bx + threadIdx.x;
        tile[j][threadIdx.x] = (r < rows && c < cols) ? in[(size_t)r * cols + c] : 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.y; j < 32; j += 8) {
        const int r = bx + j, c = by + threadIdx.x;   // out is [cols][rows]
        if (r < cols && c < rows) out[(size_t)r * rows + c] = tile[threadIdx.x][j];
    }
}

// ------------------------------------------------------------------------------------------------ losses backward
// d(mean_b bce_b)/dlogit: bce = -(g y log q + (1-g)(1-y) log(1-q)), q = clip(sigmoid(l), eps, 1-eps); the clip passes
// the gradient only inside [eps, 1-eps] (tf.clip_by_value).  function.py:73-82, nolbo.py:1432-1433.
__global__ void bce_bwd_kernel(const float *__restrict__ probs, const float *__restrict__ target, float *__restrict__ dlogit,
                               long n, float gamma, float epsilon, float inv_batch) {
    const float hi = 1.0f - epsilon;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float p = probs[i], y = target[i];
        float g = 0.f;
        if (p >= epsilon && p <= hi) g = (-gamma * y * (1.f - p) + (1.f - gamma) * (1.f - y) * p) * inv_batch;
        dlogit[i] = g;
    }
}

// Backward of slice | clip | sampling | dropout | mean_b KL  (nolbo.py:1417-1436; function.py:35-38, 84-98)
__global__ void reparam_kl_bwd_kernel(const float *__restrict__ enc_out, const float *__restrict__ eps, const float *__restrict__ dz,
                                      const float *__restrict__ drop_mask, float drop_scale, float *__restrict__ d_enc_out,
                                      int B, int L, float inv_batch) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * L) return;
    const int b = i / L, j = i % L;
    const float mu = enc_out[(size_t)b * 2 * L + j], raw = enc_out[(size_t)b * 2 * L + L + j];
    const float lv = fminf(fmaxf(raw, -10.f), 10.f);
    float g = dz[i];
    if (drop_mask) g *= drop_mask[i] * drop_scale;
    const float e = expf(lv);
    d_enc_out[(size_t)b * 2 * L + j] = g + mu * inv_batch;
    const float dlv = g * (0.5f * sqrtf(e) * eps[i]) + 0.5f * (e - 1.f) * inv_batch;
    d_enc_out[(size_t)b * 2 * L + L + j] = (raw >= -10.f && raw <= 10.f) ? dlv : 0.f;
}

// Keras Adam (beta1, beta2, epsilon 1e-7; lr_t = lr*sqrt(1-b2^t)/(1-b1^t)):  nolbo.py:1402, 1441
__global__ void adam_kernel(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                            long n, float lr_t, float b1, float b2, float eps) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float gi = g[i];
        const float mi = b1 * m[i] + (1.f - b1) * gi;
        const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi; v[i] = vi;
        p[i] -= lr_t * mi / (sqrtf(vi) + eps);
    }
}

// All variables in ONE launch: the caller supplies a device table of chunks (pointers already offset, <= 16384 elements
// each); one workgroup per chunk.  Same arithmetic as adam_kernel.
struct AdamChunk { float *p; const float *g; float *m; float *v; long n; };
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamChunk *__restrict__ table, float lr_t, float b1, float b2, float eps) {
    const AdamChunk c = table[blockIdx.x];
    for (long i = threadIdx.x; i < c.n; i += 256) {
        const float gi = c.g[i];
        const float mi = b1 * c.m[i] + (1.f - b1) * gi;
        const float vi = b2 * c.v[i] + (1.f - b2) * gi * gi;
        c.m[i] = mi; c.v[i] = vi;
        c.p[i] -= lr_t * mi / (sqrtf(vi) + eps);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const T *__restrict__ x, float *__restrict__ out, long R, int C) {
    // out[c] = sum_r x[r][c] (Dense bias gradient; R = batch): 32 columns x 8 row slices per workgroup, slice sums added in order
    __shared__ float red[8][32];
    const int cl = threadIdx.x & 31, sl = threadIdx.x >> 5, c = blockIdx.x * 32 + cl;
    float s = 0.f;
    if (c < C) {
        long r = sl;
        for (; r + 24 < R; r += 32) {
            const float v0 = (float)x[r * C + c], v1 = (float)x[(r + 8) * C + c], v2 = (float)x[(r + 16) * C + c], v3 = (float)x[(r + 24) * C + c];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; r < R; r += 8) s += (float)x[r * C + c];
    }
    red[sl][cl] = s;
    __syncthreads();
    if (sl == 0 && c < C) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += red[k][cl];
        out[c] = t;
    }
}

}  // namespace

VV_EXPORT int vv_unpack_meanpool_grad(const float *dpanel, float *dw, int side, int cin, int cout, void *stream) {
    if (!dpanel || !dw) return VV_ERR_NULL;
    if (side <= 0 || cin <= 0 || cout <= 0) return VV_ERR_SHAPE;
    if (cin % 64 == 0 && cout % 64 == 0 && side > 0 && vv_aligned16(dpanel) && vv_aligned16(dw)) {
        VV_LAUNCH(unpack_meanpool_grad_tiled_kernel, dim3(64 * (cin / 64), cout / 64), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dpanel, dw,
                  side, cin, cout);
        return vv_launch_status();
    }
    VV_LAUNCH(unpack_meanpool_grad_kernel, dim3(vv_grid_1d((long)64 * cin * cout, 16384)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
              dpanel, dw, side, cin, cout);
    return vv_launch_status();
}

VV_EXPORT int vv_unpack_convT_dense_grad(const float *dpanel, float *dw, int side, int cin, int cout, void *stream) {
    if (!dpanel || !dw) return VV_ERR_NULL;
    if (side <= 0 || cin <= 0 || cout <= 0) return VV_ERR_SHAPE;
    VV_LAUNCH(unpack_convT_dense_grad_kernel, dim3(vv_grid_1d((long)64 * cin * cout, 16384)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
              dpanel, dw, side, cin, cout);
    return vv_launch_status();
}

VV_EXPORT int vv_transpose_f32(const float *in, float *out, int rows, int cols, void *stream) {
    if (!in || !out) return VV_ERR_NULL;
    if (rows <= 0 || cols <= 0) return VV_ERR_SHAPE;
    VV_LAUNCH(transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(32, 8), 0, reinterpret_cast<hipStream_t>(stream), in, out, rows, cols);
    return vv_launch_status();
}

VV_EXPORT int vv_bce_bwd(const float *probs, const float *target, float *dlogit, int batch, long voxels, float gamma, float epsilon,
                         float inv_batch, void *stream) {
    if (!probs || !target || !dlogit) return VV_ERR_NULL;
    if (batch <= 0 || voxels <= 0) return VV_ERR_SHAPE;
    const long n = (long)batch * voxels;
    VV_LAUNCH(bce_bwd_kernel, dim3(vv_grid_1d(n, 16384)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), probs, target, dlogit, n, gamma,
              epsilon, inv_batch);
    return vv_launch_status();
}

VV_EXPORT int vv_reparam_kl_bwd(const float *enc_out, const float *eps, const float *dz, const float *drop_mask, float drop_scale,
                                float *d_enc_out, int batch, int latent, float inv_batch, void *stream) {
    if (!enc_out || !eps || !dz || !d_enc_out) return VV_ERR_NULL;
    if (batch <= 0 || latent <= 0) return VV_ERR_SHAPE;
    VV_LAUNCH(reparam_kl_bwd_kernel, dim3((batch * latent + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), enc_out,
              eps, dz, drop_mask, drop_scale, d_enc_out, batch, latent, inv_batch);
    return vv_launch_status();
}

VV_EXPORT int vv_adam_step(float *param, const float *grad, float *m, float *v, long n, float lr_t, float beta1, float beta2,
                           float epsilon, void *stream) {
    if (!param || !grad || !m || !v) return VV_ERR_NULL;
    if (n <= 0) return VV_ERR_SHAPE;
    VV_LAUNCH(adam_kernel, dim3(vv_grid_1d(n, 16384)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), param, grad, m, v, n, lr_t, beta1,
              beta2, epsilon);
    return vv_launch_status();
}

VV_EXPORT int vv_adam_step_multi(const void *chunk_table, int nchunks, float lr_t, float beta1, float beta2, float epsilon, void *stream) {
    if (!chunk_table) return VV_ERR_NULL;
    if (nchunks <= 0) return VV_ERR_SHAPE;
    VV_LAUNCH(adam_multi_kernel, dim3(nchunks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
              reinterpret_cast<const AdamChunk *>(chunk_table), lr_t, beta1, beta2, epsilon);
    return vv_launch_status();
}

VV_EXPORT int vv_colsum(const void *x, float *out, long rows, int cols, int dtype, void *stream) {
    if (!x || !out) return VV_ERR_NULL;
    if (!vv_dtype_in<float, __bf16>(dtype)) return VV_ERR_DTYPE;
    if (rows <= 0 || cols <= 0) return VV_ERR_SHAPE;
    vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        VV_LAUNCH(colsum_kernel<T>, dim3((cols + 31) / 32), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const T *>(x), out, rows, cols);
    });
    return vv_launch_status();
}
