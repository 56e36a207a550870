// 2D convolution of the image encoder (Darknet19 + head2D, src/net_core/darknet.py): Conv2D k in {1, 3}, stride 1, SAME, no bias ->
// folded BatchNormalization -> activation, as a channels-last implicit GEMM on MFMA, and the 2x2 SAME max-pool between the stages.
//
//   y[b,r,c,co] = act(scale[co] * sum_{tr,tc,ci} x[b, r+tr-p, c+tc-p, ci] * w[tr,tc,ci,co] + shift[co]),  p = k / 2
//
// GEMM rows m = (b R + r) C + c (M = B R C), K = k k Cin in chunks of 32 elements, N = Cout.  conv2d_plan.h holds the index arithmetic.
//
//   tile      : 64 rows x 64 channels per 256-thread workgroup, 4 waves as 2 x 2, one 32 x 32 accumulator each.  The weights are the
//               MFMA's first operand, so a lane holds 4 x 4 consecutive channels of ONE row: channels-last stores need no transpose.
//   operands  : VV_BF16 on v_mfma_f32_32x32x16_bf16 (two per chunk), VV_F32 on v_mfma_f32_32x32x2_f32 (sixteen per chunk; a lane's
//               16-byte fragment feeds four of them -- the order of k inside a chunk is the same for both operands, which is all a
//               sum needs).  f32 accumulation in both.
//   staging   : compiler-scheduled 16-byte global loads of chunk i + 1 into registers while chunk i is multiplied, then into the other
//               of two LDS buffers: one barrier per chunk.  LDS rows are one chunk (64 B bf16, 128 B f32), their 16-byte slots XORed
//               with row bits so that the 16 lanes of a ds_read_b128 phase hit 16 different bank groups.  cin = 32 is one tap per
//               chunk like every other width.  No inline assembly, no buffer descriptors: a padded tap or a row past M is a zero
//               written by its own predicate (per (row, tap): the address of such a tap is usually a valid one).
//   small M   : split-K over gridDim.z into float32 slabs [share][M][Cout], summed share 0, 1, 2, ... by conv2d_splitk_epilogue.
//               No atomics: two runs give the same bits.
//   stride 2  : Darknet53Conv(strides=2) (darknet.py:11-31), ZeroPadding2D(((1,0),(1,0))) + 'valid' k3 s2: the same kernel with the GEMM
//               rows on the floor(R/2) x floor(C/2) output grid and taps at (2 ro + tr - 1, 2 co + tc - 1) of the input (STRIDE).
//   residual  : Darknet53Residual's `inputs + x` (darknet.py:33-38) is the epilogue's last step, y = act(scale acc + shift) + residual in
//               float32 before the one rounding (RES), in the GEMM kernel's epilogue and in the split-K epilogue alike: no add launch.
//   cin = 3   : the float32 image, K = 27 of one 32-chunk.  A direct kernel (one thread per output, fmaf in k order) with the image
//               rounded to the operand type as it is read: 0.15 G MAC of 9 for a 416 x 416 frame.
#include "common.h"
#include "conv2d_plan.h"

namespace {

template <typename T> struct C2T;
template <> struct C2T<__bf16> { enum { SLOTS = 4, EPS = 8, SHIFT = 2 }; };     // 16-byte slots per LDS row, elements per slot, row bits skipped by the key
template <> struct C2T<float> { enum { SLOTS = 8, EPS = 4, SHIFT = 1 }; };

// byte offset of 16-byte slot `slot` of row `row`: rows with equal (row * rowbytes) mod 256 get different slots
template <int SLOTS, int SHIFT>
__device__ __forceinline__ int c2_swz(int row, int slot) {
    return row * (SLOTS * 16) + ((slot ^ ((row >> SHIFT) & (SLOTS - 1))) << 4);
}

// darknet.py:87-88 LeakyReLU(alpha), ELU(1), ReLU; alpha is the caller's (0.1 in Darknet; the 3D layers' 0.3 is not assumed here)
__device__ __forceinline__ float c2_act(float v, int act, float alpha) {
    switch (act) {
        case VV_ACT_ELU: return v > 0.f ? v : expm1f(v);
        case VV_ACT_RELU: return v > 0.f ? v : 0.f;
        case VV_ACT_LRELU: return v > 0.f ? v : alpha * v;
        default: return v;
    }
}
__device__ __forceinline__ float c2_bn_act(float v, const float *scale, const float *shift, int ch, int act, float alpha) {
    return c2_act(fmaf(v, scale ? scale[ch] : 1.f, shift ? shift[ch] : 0.f), act, alpha);
}

__device__ __forceinline__ void c2_mma_chunk(const char *As, const char *Bs, int arow, int brow, int h, f32x16 &acc, __bf16) {
#pragma unroll
    for (int step = 0; step < 2; ++step) {
        const uint4 a = *reinterpret_cast<const uint4 *>(As + c2_swz<4, 2>(arow, step * 2 + h));
        const uint4 b = *reinterpret_cast<const uint4 *>(Bs + c2_swz<4, 2>(brow, step * 2 + h));
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&b), *reinterpret_cast<const bf16x8 *>(&a), acc, 0, 0, 0);
    }
}
__device__ __forceinline__ void c2_mma_chunk(const char *As, const char *Bs, int arow, int brow, int h, f32x16 &acc, float) {
#pragma unroll
    for (int step = 0; step < 4; ++step) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(As + c2_swz<8, 1>(arow, step * 2 + h));
        const f32x4 b = *reinterpret_cast<const f32x4 *>(Bs + c2_swz<8, 1>(brow, step * 2 + h));
#pragma unroll
        for (int t = 0; t < 4; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b[t], a[t], acc, 0, 0, 0);
    }
}

// SPLIT: share blockIdx.z of K goes out raw as slabs[share][M][cout]; otherwise the epilogue runs here.
// STRIDE 2 (vv_conv2d_ex_fwd): the GEMM rows run over the Ro x Co output grid and a row's taps start at input pixel (2 ro, 2 co); R x C
// stays the INPUT grid, which is what the tap predicate and the tap offset are about.  RES: y = act(...) + residual[m][ch], added in
// float32 behind the activation (Darknet53Residual, darknet.py:33-38); with SPLIT the add is the split-K epilogue's.
template <typename T, typename OT, bool SPLIT, int STRIDE = 1, bool RES = false>
__global__ __launch_bounds__(256) void conv2d_mfma_kernel(const T *__restrict__ x, const T *__restrict__ w, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, OT *__restrict__ y, float *__restrict__ slabs, int M,
                                                          int R, int C, int cin, int cout, int npad, int ksize, int kchunks, int act,
                                                          float alpha, const T *__restrict__ residual, int Ro, int Co) {
    constexpr int SLOTS = C2T<T>::SLOTS, EPS = C2T<T>::EPS, SHIFT = C2T<T>::SHIFT;
    constexpr int PASSES = SLOTS * C2_BM / 256;                 // 16-byte loads per thread, operand and chunk
    constexpr int TILE_BYTES = C2_BM * SLOTS * 16;
    __shared__ __attribute__((aligned(16))) char As[2][TILE_BYTES];
    __shared__ __attribute__((aligned(16))) char Bs[2][TILE_BYTES];

    const int tid = threadIdx.x, m0 = blockIdx.x * C2_BM, n0 = blockIdx.y * C2_BN;
    int k0 = 0, k1 = kchunks;
    if (SPLIT) c2_split_range(kchunks, (int)gridDim.z, (int)blockIdx.z, &k0, &k1);

    // this thread's rows of the two tiles, split once
    int lrow[PASSES], lslot[PASSES], pr[PASSES], pc[PASSES];
    long pix[PASSES];
    bool live[PASSES];
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int idx = tid + p * 256;
        lrow[p] = idx / SLOTS;
        lslot[p] = idx % SLOTS;
        const long m = (long)m0 + lrow[p];
        live[p] = m < M;
        if constexpr (STRIDE == 1) {
            const C2Row rc = c2_row(live[p] ? m : 0, R, C);
            pr[p] = rc.r;
            pc[p] = rc.c;
            pix[p] = live[p] ? m : 0;
        } else {
            const C2Row rc = c2_row(live[p] ? m : 0, Ro, Co);
            pr[p] = rc.r;
            pc[p] = rc.c;
            pix[p] = c2_ex_tap_pixel(rc.b, rc.r, rc.c, ksize / 2, ksize / 2, ksize, STRIDE, R, C);      // the centre tap: offset 0
        }
    }
    uint4 ra[PASSES], rb[PASSES];
    auto fetch = [&](int kc) {
        const int kk = kc * C2_KC, tap = kk / cin, ci0 = kk - tap * cin, tr = tap / ksize, tc = tap - tr * ksize;
        const int off = c2_tap_offset(tr, tc, ksize, C);
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            ra[p] = uint4{0u, 0u, 0u, 0u};
            bool in;
            if constexpr (STRIDE == 1) in = c2_tap_valid(pr[p], pc[p], tr, tc, ksize, R, C);
            else in = c2_ex_tap_valid(pr[p], pc[p], tr, tc, ksize, STRIDE, R, C);
            if (live[p] && in)
                ra[p] = *reinterpret_cast<const uint4 *>(x + ((pix[p] + off) * cin + ci0 + lslot[p] * EPS));
            rb[p] = *reinterpret_cast<const uint4 *>(w + (((long)kc * npad + n0 + lrow[p]) * C2_KC + lslot[p] * EPS));
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int o = c2_swz<SLOTS, SHIFT>(lrow[p], lslot[p]);
            *reinterpret_cast<uint4 *>(As[buf] + o) = ra[p];
            *reinterpret_cast<uint4 *>(Bs[buf] + o) = rb[p];
        }
    };

    const int wave = tid >> 6, lane = tid & 63, wm = wave & 1, wn = wave >> 1, r32 = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;

    fetch(k0);
    stash(0);
    __syncthreads();
    for (int kc = k0; kc < k1; ++kc) {
        const int buf = (kc - k0) & 1;
        if (kc + 1 < k1) fetch(kc + 1);
        c2_mma_chunk(As[buf], Bs[buf], wm * 32 + r32, wn * 32 + r32, h, acc, T{});
        if (kc + 1 < k1) stash(buf ^ 1);
        __syncthreads();
    }

    // D[channel][row]: the lane is the row, register i the channel (i & 3) + 8 (i >> 2) + 4 h of the wave's 32
    const long m = (long)m0 + wm * 32 + r32;
    if (m >= M) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int ch0 = n0 + wn * 32 + 8 * g + 4 * h;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ch = ch0 + e;
            if (ch >= cout) continue;
            const float v = acc[4 * g + e];
            if (SPLIT) slabs[((long)blockIdx.z * M + m) * cout + ch] = v;
            else if (RES) vv_store(y, (size_t)(m * cout + ch), c2_bn_act(v, scale, shift, ch, act, alpha) + vv_load_f32(residual, (size_t)(m * cout + ch)));
            else vv_store(y, (size_t)(m * cout + ch), c2_bn_act(v, scale, shift, ch, act, alpha));
        }
    }
}

// y = act(scale * (slab 0 + slab 1 + ...) + shift): the shares in index order, whatever order they were computed in
// RT: the residual's type (the operand type of the convolution); RES as in the GEMM kernel
template <typename OT, typename RT = OT, bool RES = false>
__global__ __launch_bounds__(256) void conv2d_splitk_epilogue(const float *__restrict__ slabs, const float *__restrict__ scale,
                                                              const float *__restrict__ shift, OT *__restrict__ y, long total, int cout, int splits,
                                                              int act, float alpha, const RT *__restrict__ residual) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        float v = slabs[i];
        for (int s = 1; s < splits; ++s) v += slabs[(long)s * total + i];
        v = c2_bn_act(v, scale, shift, (int)(i % cout), act, alpha);
        if (RES) v += vv_load_f32(residual, (size_t)i);
        vv_store(y, (size_t)i, v);
    }
}

// cin = 3: x is the float32 image; T is the operand type the image is rounded to and the packed weights are stored in
template <typename T, typename OT, bool RES = false>
__global__ __launch_bounds__(256) void conv2d_image_kernel(const float *__restrict__ x, const T *__restrict__ w, const float *__restrict__ scale,
                                                           const float *__restrict__ shift, OT *__restrict__ y, long total, int R, int C, int cout,
                                                           int ksize, int act, float alpha, const T *__restrict__ residual) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / cout;
        const int co = (int)(i - m * cout);
        const C2Row rc = c2_row(m, R, C);
        const T *wr = w + (long)co * C2_KC;
        float acc = 0.f;
        for (int tr = 0; tr < ksize; ++tr)
            for (int tc = 0; tc < ksize; ++tc) {
                if (!c2_tap_valid(rc.r, rc.c, tr, tc, ksize, R, C)) continue;
                const float *px = x + (m + c2_tap_offset(tr, tc, ksize, C)) * 3;
                const T *wt = wr + (tr * ksize + tc) * 3;
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) acc = fmaf(static_cast<float>(static_cast<T>(px[ci])), static_cast<float>(wt[ci]), acc);
            }
        float v = c2_bn_act(acc, scale, shift, co, act, alpha);
        if (RES) v += vv_load_f32(residual, (size_t)i);
        vv_store(y, (size_t)i, v);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void conv2d_pack_kernel(const float *__restrict__ wk, T *__restrict__ packed, long total, int K, int cout, int npad) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int kin = (int)(i % C2_KC);
        const long rest = i / C2_KC;
        const int n = (int)(rest % npad);
        const long k = (rest / npad) * C2_KC + kin;
        packed[i] = static_cast<T>((k < K && n < cout) ? wk[k * cout + n] : 0.f);
    }
}

// MaxPool2D(2, 2, 'same') (darknet.py:100-124): output (ceil(R/2), ceil(C/2)); for an odd size the last window is one wide
template <typename T>
__global__ __launch_bounds__(256) void maxpool2d_same_kernel(const T *__restrict__ x, T *__restrict__ y, long total, int R, int C, int ch) {
    const int Ro = (R + 1) / 2, Co = (C + 1) / 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % ch);
        long rest = i / ch;
        const int co = (int)(rest % Co);
        rest /= Co;
        const int ro = (int)(rest % Ro);
        const long b = rest / Ro;
        const int r0 = 2 * ro, c0 = 2 * co;
        const T *base = x + ((b * R + r0) * C + c0) * ch + c;
        float v = vv_load_f32(base, 0);
        if (c0 + 1 < C) v = fmaxf(v, vv_load_f32(base, (size_t)ch));
        if (r0 + 1 < R) {
            v = fmaxf(v, vv_load_f32(base, (size_t)C * ch));
            if (c0 + 1 < C) v = fmaxf(v, vv_load_f32(base, (size_t)(C + 1) * ch));
        }
        vv_store(y, (size_t)i, v);
    }
}

// MaxPool2D(2, 1, 'same') (darknet.py:77, Darknet53Tiny's last pool): the input's grid; the window is clipped at the last row / column
template <typename T>
__global__ __launch_bounds__(256) void maxpool2d_s1_same_kernel(const T *__restrict__ x, T *__restrict__ y, long total, int R, int C, int ch) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long m = i / ch;
        const int c = (int)(i - m * ch);
        const C2Row rc = c2_row(m, R, C);
        const int r1 = c2_pool1_last(rc.r, R), c1 = c2_pool1_last(rc.c, C);
        const T *img = x + (long)rc.b * R * C * ch + c;
        float v = vv_load_f32(img, ((size_t)rc.r * C + rc.c) * ch);
        v = fmaxf(v, vv_load_f32(img, ((size_t)rc.r * C + c1) * ch));
        v = fmaxf(v, vv_load_f32(img, ((size_t)r1 * C + rc.c) * ch));
        v = fmaxf(v, vv_load_f32(img, ((size_t)r1 * C + c1) * ch));
        vv_store(y, (size_t)i, v);
    }
}

bool c2_dtype_ok(int dt) { return vv_dtype_in<float, __bf16>(dt); }
long c2_forced_splits() { return vv_hook_int(vv_hook("VV_C2_SPLITS"), 0); }

// M, Ro, Co: the OUTPUT's rows and grid (= the input's at stride 1); R, C the input grid
template <typename T, typename OT, int STRIDE, bool RES>
int c2_launch(const void *x, const void *w, const float *scale, const float *shift, const void *residual, void *y, int M, int R, int C, int Ro, int Co,
              int cin, int cout, int ksize, int act, float alpha, int splits, void *ws, hipStream_t st) {
    const long total = (long)M * cout;
    if (cin == 3) {
        VV_LAUNCH((conv2d_image_kernel<T, OT, RES>), dim3(vv_grid_1d(total)), dim3(256), 0, st, (const float *)x, (const T *)w, scale, shift, (OT *)y,
                  total, R, C, cout, ksize, act, alpha, (const T *)residual);
        return vv_launch_status();
    }
    const int kchunks = c2_kchunks(ksize, cin), npad = c2_npad(cout);
    const dim3 grid((M + C2_BM - 1) / C2_BM, npad / C2_BN, splits);
    if (splits == 1) {
        VV_LAUNCH((conv2d_mfma_kernel<T, OT, false, STRIDE, RES>), grid, dim3(256), 0, st, (const T *)x, (const T *)w, scale, shift, (OT *)y,
                  (float *)nullptr, M, R, C, cin, cout, npad, ksize, kchunks, act, alpha, (const T *)residual, Ro, Co);
        return vv_launch_status();
    }
    VV_LAUNCH((conv2d_mfma_kernel<T, OT, true, STRIDE, false>), grid, dim3(256), 0, st, (const T *)x, (const T *)w, scale, shift, (OT *)nullptr,
              (float *)ws, M, R, C, cin, cout, npad, ksize, kchunks, act, alpha, (const T *)nullptr, Ro, Co);
    if (const int s = vv_launch_status()) return s;
    VV_LAUNCH((conv2d_splitk_epilogue<OT, T, RES>), dim3(vv_grid_1d(total)), dim3(256), 0, st, (const float *)ws, scale, shift, (OT *)y, total, cout,
              splits, act, alpha, (const T *)residual);
    return vv_launch_status();
}

// the one body of vv_conv2d_fwd (stride 1, no residual) and vv_conv2d_ex_fwd: every refusal is decided here, before any launch
int c2_forward(const void *x, const void *w_packed, const float *scale, const float *shift, const void *residual, void *y, int batch, int rows,
               int cols, int cin, int cout, int ksize, int stride, int act, float alpha, int dtype, int out_dtype, void *workspace,
               size_t workspace_bytes, void *hip_stream) {
    if (!x || !w_packed || !y) return VV_ERR_NULL;
    if (!c2_ex_shape_ok(ksize, stride, cin, cout) || !c2_ex_extent_ok(batch, rows, cols, stride, cin, cout)) return VV_ERR_SHAPE;
    if (!c2_dtype_ok(dtype) || !c2_dtype_ok(out_dtype)) return VV_ERR_DTYPE;
    if (act < VV_ACT_NONE || act > VV_ACT_LRELU) return VV_ERR_SHAPE;
    if (!vv_aligned16(x) || !vv_aligned16(w_packed) || !vv_aligned16(y) || !vv_aligned16(residual)) return VV_ERR_ALIGN;
    const int Ro = c2_out_extent(rows, stride), Co = c2_out_extent(cols, stride), M = batch * Ro * Co;
    const int splits = c2_splits(M, ksize, cin, cout, c2_forced_splits());
    const size_t need = splits > 1 ? (size_t)splits * M * cout * sizeof(float) : 0;
    if (need && (!workspace || workspace_bytes < need)) return VV_ERR_WORKSPACE;
    if (need && !vv_aligned16(workspace)) return VV_ERR_ALIGN;
    const hipStream_t st = (hipStream_t)hip_stream;
    int status = VV_ERR_DTYPE;
    vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
        vv_with_dtype<float, __bf16>(out_dtype, [&](auto ot) {
            const auto go = [&](auto stride_c, auto res_c) {
                status = c2_launch<typename decltype(t)::type, typename decltype(ot)::type, decltype(stride_c)::value, decltype(res_c)::value>(
                    x, w_packed, scale, shift, residual, y, M, rows, cols, Ro, Co, cin, cout, ksize, act, alpha, splits, workspace, st);
            };
            using S1 = std::integral_constant<int, 1>;
            using S2 = std::integral_constant<int, 2>;
            if (stride == 2 && residual) go(S2{}, std::true_type{});
            else if (stride == 2) go(S2{}, std::false_type{});
            else if (residual) go(S1{}, std::true_type{});
            else go(S1{}, std::false_type{});
        });
    });
    return status;
}

}  // namespace

VV_EXPORT size_t vv_conv2d_packed_bytes(int ksize, int cin, int cout, int dtype) {
    if (!c2_shape_ok(ksize, cin, cout) || !c2_dtype_ok(dtype)) return 0;
    return c2_packed_elems(ksize, cin, cout) * vv_dtype_size(dtype);
}

VV_EXPORT int vv_conv2d_supported(int ksize, int cin, int cout, int dtype, int out_dtype) {
    return c2_shape_ok(ksize, cin, cout) && c2_dtype_ok(dtype) && c2_dtype_ok(out_dtype) ? 1 : 0;
}

VV_EXPORT int vv_conv2d_splits(int batch, int rows, int cols, int ksize, int cin, int cout) {
    if (!c2_shape_ok(ksize, cin, cout) || !c2_extent_ok(batch, rows, cols, cin, cout)) return 0;
    return c2_splits((long)batch * rows * cols, ksize, cin, cout, c2_forced_splits());
}

VV_EXPORT size_t vv_conv2d_workspace_bytes(int batch, int rows, int cols, int ksize, int cin, int cout, int dtype) {
    const int splits = vv_conv2d_splits(batch, rows, cols, ksize, cin, cout);
    if (splits <= 1 || !c2_dtype_ok(dtype)) return 0;
    return (size_t)splits * batch * rows * cols * cout * sizeof(float);
}

VV_EXPORT int vv_pack_conv2d(const float *w_keras, void *packed, int ksize, int cin, int cout, int dtype, void *hip_stream) {
    if (!w_keras || !packed) return VV_ERR_NULL;
    if (!c2_shape_ok(ksize, cin, cout)) return VV_ERR_SHAPE;
    if (!c2_dtype_ok(dtype)) return VV_ERR_DTYPE;
    if (!vv_aligned16(packed)) return VV_ERR_ALIGN;
    const long total = (long)c2_packed_elems(ksize, cin, cout);
    const hipStream_t st = (hipStream_t)hip_stream;
    vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        VV_LAUNCH(conv2d_pack_kernel<T>, dim3(vv_grid_1d(total)), dim3(256), 0, st, w_keras, (T *)packed, total, ksize * ksize * cin, cout, c2_npad(cout));
    });
    return vv_launch_status();
}

VV_EXPORT int vv_conv2d_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, void *y, int batch, int rows, int cols,
                            int cin, int cout, int ksize, int act, float alpha, int dtype, int out_dtype, void *workspace, size_t workspace_bytes,
                            void *hip_stream) {
    return c2_forward(x, w_packed, scale, shift, nullptr, y, batch, rows, cols, cin, cout, ksize, 1, act, alpha, dtype, out_dtype, workspace,
                      workspace_bytes, hip_stream);
}

VV_EXPORT int vv_conv2d_ex_supported(int ksize, int stride, int cin, int cout, int dtype, int out_dtype) {
    return c2_ex_shape_ok(ksize, stride, cin, cout) && c2_dtype_ok(dtype) && c2_dtype_ok(out_dtype) ? 1 : 0;
}

VV_EXPORT int vv_conv2d_ex_splits(int batch, int rows, int cols, int ksize, int stride, int cin, int cout) {
    if (!c2_ex_shape_ok(ksize, stride, cin, cout) || !c2_ex_extent_ok(batch, rows, cols, stride, cin, cout)) return 0;
    return c2_splits((long)batch * c2_out_extent(rows, stride) * c2_out_extent(cols, stride), ksize, cin, cout, c2_forced_splits());
}

VV_EXPORT size_t vv_conv2d_ex_workspace_bytes(int batch, int rows, int cols, int ksize, int stride, int cin, int cout, int dtype) {
    const int splits = vv_conv2d_ex_splits(batch, rows, cols, ksize, stride, cin, cout);
    if (splits <= 1 || !c2_dtype_ok(dtype)) return 0;
    return (size_t)splits * batch * c2_out_extent(rows, stride) * c2_out_extent(cols, stride) * cout * sizeof(float);
}

VV_EXPORT int vv_conv2d_ex_fwd(const void *x, const void *w_packed, const float *scale, const float *shift, const void *residual, void *y, int batch,
                               int rows, int cols, int cin, int cout, int ksize, int stride, int act, float alpha, int dtype, int out_dtype,
                               void *workspace, size_t workspace_bytes, void *hip_stream) {
    return c2_forward(x, w_packed, scale, shift, residual, y, batch, rows, cols, cin, cout, ksize, stride, act, alpha, dtype, out_dtype, workspace,
                      workspace_bytes, hip_stream);
}

VV_EXPORT int vv_maxpool2d_same_fwd(const void *x, void *y, int batch, int rows, int cols, int channels, int dtype, void *hip_stream) {
    if (!x || !y) return VV_ERR_NULL;
    if (channels < 1 || !c2_extent_ok(batch, rows, cols, channels, channels)) return VV_ERR_SHAPE;
    const long total = (long)batch * ((rows + 1) / 2) * ((cols + 1) / 2) * channels;
    const hipStream_t st = (hipStream_t)hip_stream;
    const bool ok = vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        VV_LAUNCH(maxpool2d_same_kernel<T>, dim3(vv_grid_1d(total)), dim3(256), 0, st, (const T *)x, (T *)y, total, rows, cols, channels);
    });
    return ok ? vv_launch_status() : VV_ERR_DTYPE;
}

VV_EXPORT int vv_maxpool2d_s1_same_fwd(const void *x, void *y, int batch, int rows, int cols, int channels, int dtype, void *hip_stream) {
    if (!x || !y) return VV_ERR_NULL;
    if (channels < 1 || !c2_extent_ok(batch, rows, cols, channels, channels)) return VV_ERR_SHAPE;
    const long total = (long)batch * rows * cols * channels;
    const hipStream_t st = (hipStream_t)hip_stream;
    const bool ok = vv_with_dtype<float, __bf16>(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        VV_LAUNCH(maxpool2d_s1_same_kernel<T>, dim3(vv_grid_1d(total)), dim3(256), 0, st, (const T *)x, (T *)y, total, rows, cols, channels);
    });
    return ok ? vv_launch_status() : VV_ERR_DTYPE;
}
