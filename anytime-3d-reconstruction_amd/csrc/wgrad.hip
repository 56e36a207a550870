// Weight gradients of the training step as reduction-over-rows GEMMs, dW[m][n] = sum_r A[r][m] * G[r][n] (r = samples x positions),
// float32 result.  Two kernels, each over a dense A (Dense kernels, pooled / panel layers) or over the 64-tap rows of a stride-2 k4
// layer gathered from its source grid (several channels, or one float32 channel):
//   wgrad_kernel       float32 or bf16 operands widened to float32, exact-f32 MFMA 32x32x2, 64 x 64|128 tiles
//   wgrad_bf16_kernel  bf16 operands, MFMA 32x32x16 bf16, 128 x 128 tiles staged by LDS-DMA (a single 64 x 64 tile for N <= 64 on one channel)
// Both split the reduction into per-split float32 slabs in the workspace, summed in split order by one of two reduce kernels
// (deterministic).  The phase form of the stride-2 layers is wgrad_phase.hip.  Which form runs and how it is split is decided in
// wgrad_plan.h, once; the entries at the end of this file validate, ask it, fill the argument block and launch.  gfx950.
#include "wgrad.h"

static_assert(WG_DT_F32 == VV_F32 && WG_DT_BF16 == VV_BF16, "wgrad_plan.h restates the dtype codes");

namespace {

// 4 consecutive elements of a float32 or bf16 tensor as float4 (element index 4*i4 .. +3), and the store back.
template <typename T>
__device__ __forceinline__ f32x4 ld4(const T *p, long i4) {
    if constexpr (sizeof(T) == 4) {
        return reinterpret_cast<const f32x4 *>(p)[i4];
    } else {
        const bf16x4 v = reinterpret_cast<const bf16x4 *>(p)[i4];
        return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
}
template <typename T>
__device__ __forceinline__ void st4(T *p, long i4, f32x4 v) {
    if constexpr (sizeof(T) == 4) {
        reinterpret_cast<f32x4 *>(p)[i4] = v;
    } else {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = static_cast<__bf16>(v[e]);
        reinterpret_cast<bf16x4 *>(p)[i4] = o;
    }
}
// runtime-typed variant for the weight-gradient staging (dtype flag in the argument block)
__device__ __forceinline__ f32x4 ld4_rt(const void *p, long elem, int is_bf16) {
    return is_bf16 ? ld4(reinterpret_cast<const __bf16 *>(p) + elem, 0) : ld4(reinterpret_cast<const float *>(p) + elem, 0);
}

// ------------------------------------------------------------------------------------------------ weight gradients
// dW[m][n] = sum_r A[r][m] * G[r][n]   (reduction over rows r = samples x positions), exact-f32 MFMA 32x32x2.
//   AMODE 0: A[r][m] dense, row pitch lda                                  (Dense kernels, pooled / panel layers)
//   AMODE 1: A[r][(t,ci)] = src[b, 2o-1+t, ci] (zero in the SAME padding), r = (b,o) over the HALF-size grid: the
//            weight gradient of a stride-2 Conv3D (src = layer input, G = dL/d(conv out)) -> Keras [t][ci][co];
//            with src = dL/d(out) and G = layer input it is the weight gradient of a stride-2 Conv3DTranspose
//            -> Keras [t][co][ci].
//   AMODE 2: as 1 with one source channel (m = tap): first conv / last transposed conv.
// Tile 64 (m) x BN (n), 4 waves (2x2), reduction chunks of 32 rows staged in LDS as [r][m] / [r][n] (the f32 MFMA
// wants lane = m, k = row: rows of the chunk ARE k, no transposition needed).  grid.y splits the reduction; slabs are
// summed in split order by wgrad_reduce_kernel (deterministic).
struct WgradArgs {
    const void *A;      // float32 or bf16 (a_bf16)
    const void *G;      // float32 or bf16 (g_bf16)
    float *slabs;       // [splits][M][N]
    long R;             // reduction rows
    int M, N;
    int lda;            // AMODE 0 row pitch (elements)
    int din_log2, cin;  // AMODE 1/2: source grid side (log2) and channels
    int rows_per_split;
    int a_bf16, g_bf16;
};

template <int AMODE, int BN>
__global__ __launch_bounds__(256) void wgrad_kernel(const WgradArgs a) {
    constexpr int BM = 64, BR = 32, TN = BN / 64;
    __shared__ __attribute__((aligned(16))) float As[BR][BM + 4];
    __shared__ __attribute__((aligned(16))) float Gs[BR][BN + 4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = (a.N + BN - 1) / BN;
    const int tile_n = blockIdx.x % ntn, tile_m = blockIdx.x / ntn;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const long r_begin = (long)blockIdx.y * a.rows_per_split;
    const long r_end = r_begin + a.rows_per_split < a.R ? r_begin + a.rows_per_split : a.R;
    const int li = a.din_log2, n = 1 << li, lo = li - 1, omsk = (1 << lo) - 1;

    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[j][q] = 0.f;

    // staging roles: A chunk = 32 rows x 64 floats = 512 float4 slots -> 2 per thread; G chunk = 32 x BN -> BN/32 per thread
    const int fr = lane & 31, fh = lane >> 5;
    for (long rc = r_begin; rc < r_end; rc += BR) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int slot = tid + 256 * it, rr = slot >> 4, c4 = slot & 15;
            const long r = rc + rr;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r < r_end) {
                if (AMODE == 0) {
                    const int m = m0 + c4 * 4;
                    if (m < a.M) v = ld4_rt(a.A, r * a.lda + m, a.a_bf16);
                } else {
                    const int ow = (int)(r & omsk), oh = (int)((r >> lo) & omsk), od = (int)((r >> (2 * lo)) & omsk);
                    const long b = r >> (3 * lo);
                    if (AMODE == 1) {
                        const int m = m0 + c4 * 4, t = m / a.cin, ci = m % a.cin;   // cin % 64 == 0: a tile stays inside one tap
                        const int id = 2 * od - 1 + (t >> 4), ih = 2 * oh - 1 + ((t >> 2) & 3), iw = 2 * ow - 1 + (t & 3);
                        if (m < a.M && (unsigned)id < (unsigned)n && (unsigned)ih < (unsigned)n && (unsigned)iw < (unsigned)n)
                            v = ld4_rt(a.A, ((((b << li) + id << li) + ih << li) + iw) * a.cin + ci, a.a_bf16);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int t = c4 * 4 + e;
                            const int id = 2 * od - 1 + (t >> 4), ih = 2 * oh - 1 + ((t >> 2) & 3), iw = 2 * ow - 1 + (t & 3);
                            if ((unsigned)id < (unsigned)n && (unsigned)ih < (unsigned)n && (unsigned)iw < (unsigned)n)
                                v[e] = reinterpret_cast<const float *>(a.A)[(((b << li) + id << li) + ih << li) + iw];   // cin = 1 sources are float32 grids
                        }
                    }
                }
            }
            *reinterpret_cast<f32x4 *>(&As[rr][c4 * 4]) = v;
        }
#pragma unroll
        for (int it = 0; it < BN / 32; ++it) {
            const int slot = tid + 256 * it, rr = slot / (BN / 4), c4 = slot % (BN / 4);
            const long r = rc + rr;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            const int nn = n0 + c4 * 4;
            if (r < r_end && nn < a.N) v = ld4_rt(a.G, r * a.N + nn, a.g_bf16);
            *reinterpret_cast<f32x4 *>(&Gs[rr][c4 * 4]) = v;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < BR; k += 2) {
            const float av = As[k + fh][wm * 32 + fr];
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float gv = Gs[k + fh][wn * (BN / 2) + j * 32 + fr];
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, gv, acc[j], 0, 0, 0);   // D[m][n]: lane = n, regs walk m
            }
        }
        __syncthreads();
    }
    float *slab = a.slabs + (size_t)blockIdx.y * a.M * a.N;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int nn = n0 + wn * (BN / 2) + j * 32 + fr;
        if (nn >= a.N) continue;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int m = m0 + wm * 32 + (q & 3) + 8 * (q >> 2) + 4 * fh;
            if (m < a.M) slab[(size_t)m * a.N + nn] = acc[j][q];
        }
    }
}

// ---- bf16 weight gradients on v_mfma_f32_32x32x16_bf16.  Both operands of dW = A^T G are k-strided (k = the row index
// r): the LDS tiles stay row-major as staged, [column block of 32][row][32 bf16] (64-byte rows, so the 32 lanes of a
// half cover 256 B exactly once), and the MFMA fragments are read with the hardware transpose ds_read_b64_tr_b16:
// lane 4q+p of a 16-lane group supplies row q / columns 4p..4p+3 of a 4 x 16 block and receives column (lane & 15) of
// the 4 rows -- two reads give the 8 consecutive k of a lane.  128 x 128 tile per 256-thread workgroup (2 x 2 waves of
// 64 x 64), 64-row chunks staged by LDS-DMA into a 2-deep ring (zeros for padded taps / rows past R through the
// buffer range check), split over the reduction into slabs summed in fixed order by wgrad_reduce_kernel.
struct WgradBArgs {
    const void *A, *G;
    float *slabs;
    long R;
    int M, N, lda, din_log2, cin, rows_per_split;
    unsigned a_bytes, g_bytes;
};

template <int AMODE, bool ONE = false>      // 0: A[r][m] dense (pitch lda); 1: A[r][(t,ci)] = src[b, 2o-1+t, ci], cin % 64 == 0;
                          // 2: A[r][t] = src[b, 2o-1+t] of a single-channel float32 grid (M = 64), built in registers
__global__ __launch_bounds__(256, ONE ? 4 : 2) void wgrad_bf16_kernel(const WgradBArgs a) {
    constexpr int BM = 128, BN = 128, BR = 64, OPB = BR * 128 * 2;        // one operand chunk: 16 KiB
    // ONE (AMODE 2 with N <= 64, chosen at launch): a single 64 x 64 output tile.  Only column blocks 0, 1 of either operand exist, so a
    // stage is 16 KiB (A | G, 8 KiB each) instead of 32, the whole ring 32 KiB, and FOUR workgroups fit a CU: the kernel waits for one
    // chunk at a time (vmcnt(0) + barrier per 64 rows), so what it achieves is set by the chunks in flight per CU.
    constexpr int STG = ONE ? 16384 : 2 * OPB, GOFF = ONE ? 8192 : OPB;
    extern __shared__ __attribute__((aligned(16))) char smem[];           // [2 stages][A | G]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int ntn = (a.N + BN - 1) / BN;
    const int tile_n = blockIdx.x % ntn, tile_m = blockIdx.x / ntn;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const long r_begin = (long)blockIdx.y * a.rows_per_split;
    const long r_end = r_begin + a.rows_per_split < a.R ? r_begin + a.rows_per_split : a.R;
    const int li = a.din_log2, n = 1 << li, lo = li - 1, omsk = (1 << lo) - 1;
    constexpr bool one_tile = ONE;                          // single-channel layer, one 64 x 64 output tile: K split over the waves (below)
    const u32x4 rsa = vv_make_rsrc(a.A, a.a_bytes), rsg = vv_make_rsrc(a.G, a.g_bytes);
    const unsigned lds0 = (unsigned)(unsigned long long)(lptr_t)smem;

    // staging: piece = (column block cb, 16-row group rg): 16 rows x 64 B; 16 pieces per operand, 4 per wave each
    const int prow = lane >> 2, pch = lane & 3;
    auto stage = [&](long rc, int st) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int piece = wave * 4 + i, cb = piece >> 2, rg = piece & 3;
            if (one_tile && cb >= 2) continue;             // single-channel layers with <= 64 channels: column blocks 2, 3 are never read
            const long r = rc + rg * 16 + prow;
            const int mcol = m0 + cb * 32, ncol = n0 + cb * 32;
            unsigned va = 0xFFFFFFF0u, vg = 0xFFFFFFF0u;
            if (r < r_end) {
                if (mcol < a.M) {
                    if (AMODE == 0) {
                        va = (unsigned)((r * a.lda + mcol + pch * 8) * 2);
                    } else {
                        const int ow = (int)(r & omsk), oh = (int)((r >> lo) & omsk), od = (int)((r >> (2 * lo)) & omsk);
                        const long b = r >> (3 * lo);
                        const int t = mcol / a.cin, ci = mcol - t * a.cin;
                        const int id = 2 * od - 1 + (t >> 4), ih = 2 * oh - 1 + ((t >> 2) & 3), iw = 2 * ow - 1 + (t & 3);
                        if ((unsigned)id < (unsigned)n && (unsigned)ih < (unsigned)n && (unsigned)iw < (unsigned)n)
                            va = (unsigned)((((((b << li) + id << li) + ih << li) + iw) * a.cin + ci + pch * 8) * 2);
                    }
                }
                if (ncol < a.N) vg = (unsigned)((r * a.N + ncol + pch * 8) * 2);
            }
            const unsigned dst = lds0 + st * STG + cb * 4096 + rg * 1024;
            if (AMODE != 2) vv_dma16(rsa, va, dst);
            vv_dma16(rsg, vg, dst + GOFF);
        }
    };
    // AMODE 2: thread = (chunk row tid >> 2, tap plane td = tid & 3) owns 16 taps (th, tw) = 32 bytes of the row.  The
    // occupancy is loaded one chunk ahead (four 16-byte loads of the 4-voxel run 2 ow - 1 .. 2 ow + 2, read at a shifted
    // base on the two grid edges so that no load leaves the row), converted and written after the MFMAs of the chunk.
    const float *srcf = reinterpret_cast<const float *>(a.A);
    f32x4 xr[4];
    int xsh = 0;
    auto load_x = [&](long rc) {
        const long r = rc + (tid >> 2);
        const int td = tid & 3;
        const int ow = (int)(r & omsk), oh = (int)((r >> lo) & omsk), od = (int)((r >> (2 * lo)) & omsk);
        const long b = r >> (3 * lo);
        const int id = 2 * od - 1 + td, iw0 = 2 * ow - 1;
        xsh = iw0 < 0 ? 1 : (iw0 + 3 >= n ? -1 : 0);
#pragma unroll
        for (int th = 0; th < 4; ++th) {
            const int ih = 2 * oh - 1 + th;
            const bool ok = r < r_end && (unsigned)id < (unsigned)n && (unsigned)ih < (unsigned)n;
            xr[th] = ok ? *reinterpret_cast<const f32x4 *>(srcf + ((((b << li) + id << li) + ih) << li) + iw0 + xsh) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_x = [&](int st) {
        const int row = tid >> 2, td = tid & 3;
        bf16x8 o[2];
#pragma unroll
        for (int th = 0; th < 4; ++th) {
            const f32x4 l = xr[th];
            const f32x4 v = xsh == 0 ? l : (xsh > 0 ? f32x4{0.f, l[0], l[1], l[2]} : f32x4{l[1], l[2], l[3], 0.f});
#pragma unroll
            for (int e = 0; e < 4; ++e) o[th >> 1][(th & 1) * 4 + e] = static_cast<__bf16>(v[e]);
        }
        char *dst = smem + st * STG + (td >> 1) * 4096 + row * 64 + (td & 1) * 32;
        *reinterpret_cast<bf16x8 *>(dst) = o[0];
        *reinterpret_cast<bf16x8 *>(dst + 16) = o[1];
    };
    if (AMODE == 2 && !ONE) {                              // taps 64..127 of the 128-wide tile do not exist: column blocks 2, 3 stay zero
        const bf16x8 z = {};
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<bf16x8 *>(smem + (tid >> 7) * (2 * OPB) + 8192 + ((tid & 127) * 4 + q) * 16) = z;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

    // transposed-read address of this lane inside a column block, for k-step 0: row 8 fh + q, columns 16 (g & 1) + 4p
    const int g4 = lane >> 4, q4 = (lane & 15) >> 2, p4 = lane & 3;
    const unsigned troff = ((g4 >> 1) * 8 + q4) * 64 + ((g4 & 1) * 16 + p4 * 4) * 2;
    long rc = r_begin;
    int st = 0;
    if (rc < r_end) {
        if (AMODE == 2) { load_x(rc); store_x(0); }
        stage(rc, 0);
    }
    for (; rc < r_end; rc += BR, st ^= 1) {
        vv_wait_vm<0>();
        __syncthreads();                                     // chunk landed for everyone; previous chunk's reads are done
        const bool more = rc + BR < r_end;
        if (more) {
            if (AMODE == 2) load_x(rc + BR);
            stage(rc + BR, st ^ 1);
        }
        const unsigned sa = lds0 + st * STG, sg = sa + GOFF;
        if (one_tile) {
            // M = 64, N <= 64: ONE 64 x 64 tile.  The generic mapping (2 x 2 waves of 64 x 64 on a 128 x 128 tile) left three of the
            // four waves multiplying zeros and the fourth one waiting for sixteen serialised fragment reads per chunk; here the
            // four waves split the chunk's K (one 16-row k-step each), issue their eight transposed reads together, and their
            // accumulators meet through LDS after the last chunk (in wave order: deterministic).
            const unsigned ka = sa + wave * 1024 + troff, kg = sg + wave * 1024 + troff;
            u32x2 r0, r1, r2, r3, r4, r5, r6, r7;
            asm volatile("ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %8 offset:256\n\t"
                         "ds_read_b64_tr_b16 %2, %8 offset:4096\n\tds_read_b64_tr_b16 %3, %8 offset:4352\n\t"
                         "ds_read_b64_tr_b16 %4, %9\n\tds_read_b64_tr_b16 %5, %9 offset:256\n\t"
                         "ds_read_b64_tr_b16 %6, %9 offset:4096\n\tds_read_b64_tr_b16 %7, %9 offset:4352\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7) : "v"(ka), "v"(kg) : "memory");
            const u32x4 a0 = {r0[0], r0[1], r1[0], r1[1]}, a1 = {r2[0], r2[1], r3[0], r3[1]};
            const u32x4 g0 = {r4[0], r4[1], r5[0], r5[1]}, g1 = {r6[0], r6[1], r7[0], r7[1]};
            const bf16x8 fa[2] = {*reinterpret_cast<const bf16x8 *>(&a0), *reinterpret_cast<const bf16x8 *>(&a1)};
            const bf16x8 fg[2] = {*reinterpret_cast<const bf16x8 *>(&g0), *reinterpret_cast<const bf16x8 *>(&g1)};
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fg[j], acc[i][j], 0, 0, 0);   // D[m][n]
        } else
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            // the eight transposed reads of a k-step are issued together and waited for once (one wait per fragment serialised
            // eight LDS round trips per k-step)
            const unsigned ka = sa + wm * 8192 + ks * 1024 + troff, kg = sg + wn * 8192 + ks * 1024 + troff;
            u32x2 r0, r1, r2, r3, r4, r5, r6, r7;
            asm volatile("ds_read_b64_tr_b16 %0, %8\n\tds_read_b64_tr_b16 %1, %8 offset:256\n\t"
                         "ds_read_b64_tr_b16 %2, %8 offset:4096\n\tds_read_b64_tr_b16 %3, %8 offset:4352\n\t"
                         "ds_read_b64_tr_b16 %4, %9\n\tds_read_b64_tr_b16 %5, %9 offset:256\n\t"
                         "ds_read_b64_tr_b16 %6, %9 offset:4096\n\tds_read_b64_tr_b16 %7, %9 offset:4352\n\ts_waitcnt lgkmcnt(0)"
                         : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3), "=&v"(r4), "=&v"(r5), "=&v"(r6), "=&v"(r7) : "v"(ka), "v"(kg) : "memory");
            const u32x4 a0 = {r0[0], r0[1], r1[0], r1[1]}, a1 = {r2[0], r2[1], r3[0], r3[1]};
            const u32x4 g0 = {r4[0], r4[1], r5[0], r5[1]}, g1 = {r6[0], r6[1], r7[0], r7[1]};
            const bf16x8 fa[2] = {*reinterpret_cast<const bf16x8 *>(&a0), *reinterpret_cast<const bf16x8 *>(&a1)};
            const bf16x8 fg[2] = {*reinterpret_cast<const bf16x8 *>(&g0), *reinterpret_cast<const bf16x8 *>(&g1)};
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fg[j], acc[i][j], 0, 0, 0);   // D[m][n]
        }
        if (AMODE == 2 && more) store_x(st ^ 1);
    }
    const int fr = lane & 31, fh = lane >> 5;
    float *slab = a.slabs + (size_t)blockIdx.y * a.M * a.N;
    if (one_tile) {
        // the four waves' accumulators meet in the 32 KiB of the ring: waves 0, 1 store, waves 2, 3 add on top (same lane -> same
        // element), then every thread adds the two halves: (w0 + w2) + (w1 + w3), a fixed order
        float *red = reinterpret_cast<float *>(smem) + (wave & 1) * 4096;
        __syncthreads();                                     // every wave is done with the stages
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            if ((wave >> 1) == pass) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            float *e = red + (i * 32 + (q & 3) + 8 * (q >> 2) + 4 * fh) * 64 + j * 32 + fr;
                            *e = pass == 0 ? acc[i][j][q] : *e + acc[i][j][q];
                        }
            }
            __syncthreads();
        }
        const float *r0 = reinterpret_cast<const float *>(smem);
        for (int idx = tid; idx < 4096; idx += 256) {
            const int m = idx >> 6, nn = idx & 63;
            if (nn < a.N) slab[(size_t)m * a.N + nn] = r0[idx] + r0[4096 + idx];
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int nn = n0 + (wn * 2 + j) * 32 + fr;
            if (nn >= a.N) continue;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = m0 + (wm * 2 + i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * fh;
                if (m < a.M) slab[(size_t)m * a.N + nn] = acc[i][j][q];
            }
        }
}

__global__ void wgrad_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ out, long n, int splits, float alpha,
                                    int accumulate) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float s = 0.f;
        int k = 0;
        for (; k + 4 <= splits; k += 4) {       // four loads in flight, added in split order
            const float v0 = slabs[(size_t)k * n + i], v1 = slabs[(size_t)(k + 1) * n + i], v2 = slabs[(size_t)(k + 2) * n + i],
                        v3 = slabs[(size_t)(k + 3) * n + i];
            s += v0; s += v1; s += v2; s += v3;
        }
        for (; k < splits; ++k) s += slabs[(size_t)k * n + i];
        out[i] = accumulate ? out[i] + alpha * s : alpha * s;
    }
}

// Few outputs, many slabs (the single-channel layers: 4096 outputs x 256 splits): 64 outputs x 4 slices of the split
// list per workgroup; the 4 slice sums are added in slice order.
__global__ __launch_bounds__(256) void wgrad_reduce_sliced_kernel(const float *__restrict__ slabs, float *__restrict__ out, long n,
                                                                  int splits, float alpha, int accumulate) {
    __shared__ float red[4][64];
    const int ol = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + ol;
    const int per = (splits + 3) / 4, k0 = sl * per, k1 = k0 + per < splits ? k0 + per : splits;
    float s = 0.f;
    if (i < n) {
        int k = k0;
        for (; k + 8 <= k1; k += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = slabs[(size_t)(k + u) * n + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; k < k1; ++k) s += slabs[(size_t)k * n + i];
    }
    red[sl][ol] = s;
    __syncthreads();
    if (sl == 0 && i < n) {
        const float t = ((red[0][ol] + red[1][ol]) + red[2][ol]) + red[3][ol];
        out[i] = accumulate ? out[i] + alpha * t : alpha * t;
    }
}

}  // namespace

void vv_wgrad_reduce_launch(const float *slabs, float *out, long n, int splits, float alpha, int accumulate, hipStream_t st) {
    if (wgrad_reduce_sliced(splits, n))
        VV_LAUNCH(wgrad_reduce_sliced_kernel, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, st, slabs, out, n, splits, alpha, accumulate);
    else
        VV_LAUNCH(wgrad_reduce_kernel, dim3(vv_grid_1d(n, 16384)), dim3(256), 0, st, slabs, out, n, splits, alpha, accumulate);
}

namespace {

template <int AMODE>
int launch_wgrad(const WgradArgs &a, const WgradPlan &p, float *out, float alpha, int accumulate, hipStream_t st) {
    const int tiles = ((a.M + 63) / 64) * ((a.N + p.bn - 1) / p.bn);
    if (p.bn == 128) VV_LAUNCH((wgrad_kernel<AMODE, 128>), dim3(tiles, p.splits), dim3(256), 0, st, a);
    else VV_LAUNCH((wgrad_kernel<AMODE, 64>), dim3(tiles, p.splits), dim3(256), 0, st, a);
    const long n = (long)a.M * a.N;
    vv_wgrad_reduce_launch(a.slabs, out, n, p.splits, alpha, accumulate, st);
    return vv_launch_status();
}

template <int AMODE>
int launch_wgrad_bf16(const WgradBArgs &a_in, const WgradPlan &p, float *out, hipStream_t st) {
    WgradBArgs a = a_in;
    if (p.splits == 1) a.slabs = out;              // one share: its "slab" IS the result (the reduce pass was a 33 MB copy on the 256 <-> 512 layers)
    const int tiles = ((a.M + 127) / 128) * ((a.N + 127) / 128);
    vv_allow_lds<&wgrad_bf16_kernel<AMODE>>(65536);
    if (AMODE == 2 && wgrad_grid_one_tile(a.N)) VV_LAUNCH((wgrad_bf16_kernel<2, true>), dim3(tiles, p.splits), dim3(256), 32768, st, a);
    else VV_LAUNCH((wgrad_bf16_kernel<AMODE>), dim3(tiles, p.splits), dim3(256), 65536, st, a);
    const long n = (long)a.M * a.N;
    if (p.splits > 1) vv_wgrad_reduce_launch(a.slabs, out, n, p.splits, 1.f, 0, st);
    return vv_launch_status();
}

// The two kernel-form overrides of the hooks build, read here and nowhere else.
struct WgradHooks { bool f32_only, no_phase; };
WgradHooks wgrad_hooks() { return {vv_hook("VV_WGRAD_F32") != nullptr, vv_hook("VV_NO_WGRAD_PHASE") != nullptr}; }

}  // namespace

VV_EXPORT size_t vv_wgrad_workspace_bytes(long rows, int m, int n) { return wgrad_workspace_bytes(rows, m, n); }

VV_EXPORT int vv_wgrad_dense(const void *a, const void *g, float *dw, long rows, int m, int n, int lda, int a_dtype, int g_dtype,
                             void *workspace, size_t workspace_bytes, void *stream) {
    if (!a || !g || !dw) return VV_ERR_NULL;
    if (!vv_dtype_in<float, __bf16>(a_dtype) || !vv_dtype_in<float, __bf16>(g_dtype)) return VV_ERR_DTYPE;
    if (rows <= 0 || m <= 0 || n <= 0 || m % 4 || n % 4 || lda % 4) return VV_ERR_SHAPE;
    if (!workspace || workspace_bytes < vv_wgrad_workspace_bytes(rows, m, n)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *slabs = reinterpret_cast<float *>(workspace);
    const WgradRoute r = wgrad_dense_route(rows, m, n, lda, a_dtype, g_dtype, vv_aligned16(a), vv_aligned16(g), wgrad_hooks().f32_only);
    switch (r.form) {
    case WG_BF16_DENSE: {
        WgradBArgs wb{a, g, slabs, rows, m, n, lda, 0, 0, r.plan.rps, (unsigned)((size_t)rows * lda * 2), (unsigned)((size_t)rows * n * 2)};
        return launch_wgrad_bf16<0>(wb, r.plan, dw, st);
    }
    case WG_F32: {
        WgradArgs w{a, g, slabs, rows, m, n, lda, 0, 0, r.plan.rps, a_dtype == VV_BF16, g_dtype == VV_BF16};
        return launch_wgrad<0>(w, r.plan, dw, 1.f, 0, st);
    }
    default: return VV_ERR_SHAPE;       // no other form is a dense route
    }
}

VV_EXPORT int vv_wgrad_conv_k4s2(const void *src, const void *g, float *dw, int batch, int side, int cin, int cout, int src_dtype,
                                 int g_dtype, void *workspace, size_t workspace_bytes, void *stream) {
    if (!src || !g || !dw) return VV_ERR_NULL;
    if (!vv_dtype_in<float, __bf16>(src_dtype) || !vv_dtype_in<float, __bf16>(g_dtype)) return VV_ERR_DTYPE;
    if (!wgrad_conv_src_dtype_ok(cin, src_dtype)) return VV_ERR_DTYPE;
    if (batch <= 0 || side < 2 || !vv_is_pow2(side) || cout % 4 || (cin != 1 && cin % 64)) return VV_ERR_SHAPE;
    const int o = side / 2;
    const long rows = (long)batch * o * o * o;
    const int m = 64 * cin;
    if (!workspace || workspace_bytes < vv_wgrad_workspace_bytes(rows, m, cout)) return VV_ERR_WORKSPACE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    float *slabs = reinterpret_cast<float *>(workspace);
    const WgradHooks h = wgrad_hooks();
    const WgradRoute r = wgrad_conv_route(batch, side, cin, cout, src_dtype, g_dtype, vv_aligned16(src), vv_aligned16(g), h.f32_only, h.no_phase);
    const unsigned g_bytes = (unsigned)((size_t)rows * cout * 2);            // the bf16 forms' buffer ranges (the route checked that they fit)
    const unsigned src_bytes = (unsigned)((size_t)batch * side * side * side * cin * 2);
    switch (r.form) {
    case WG_PHASE:
        vv_wgrad_phase_launch(src, g, slabs, batch, side, cin, cout, r.plan, st);
        vv_wgrad_reduce_launch(slabs, dw, (long)m * cout, r.plan.splits, 1.f, 0, st);
        return vv_launch_status();
    case WG_BF16_TAPS: {
        WgradBArgs wb{src, g, slabs, rows, m, cout, 0, vv_log2(side), cin, r.plan.rps, src_bytes, g_bytes};
        return launch_wgrad_bf16<1>(wb, r.plan, dw, st);
    }
    case WG_BF16_GRID: {
        // single input channel: the 64-tap rows are built from the float32 grid inside the bf16 kernel's staging
        WgradBArgs wb{src, g, slabs, rows, 64, cout, 0, vv_log2(side), 1, r.plan.rps, 0u, g_bytes};
        return launch_wgrad_bf16<2>(wb, r.plan, dw, st);
    }
    case WG_F32: {
        WgradArgs w{src, g, slabs, rows, m, cout, 0, vv_log2(side), cin, r.plan.rps, src_dtype == VV_BF16, g_dtype == VV_BF16};
        return cin == 1 ? launch_wgrad<2>(w, r.plan, dw, 1.f, 0, st) : launch_wgrad<1>(w, r.plan, dw, 1.f, 0, st);
    }
    default: return VV_ERR_SHAPE;       // no other form is a stride-2 route
    }
}
