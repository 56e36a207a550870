// The first encoder layer (gfx950):
//   first_conv : Conv3D k4 s2 SAME with ONE input channel (float32 occupancy grid) -> 64 channels, folded BN + activation, bf16 or
//                e4m3fn output (autoencoder3D.py:54-61); gather, plane and chained-plane forms, chosen by vv_first_conv_bf16_launch
#include "common.h"

namespace {

__device__ float vv_zero_word = 0.f;

// first_conv (bf16): Conv3D k4 s2 SAME with ONE input channel -- a [rows x 64 taps] x [64 x 64] product per 128-row
// tile with the taps gathered from the float32 occupancy grid.  The layer is latency-bound (one K chunk per tile: gather
// -> LDS -> 8 MFMAs -> store, PMC: 68 % of wave time parked on vmcnt), so each workgroup walks several tiles and issues
// the NEXT tile's 32 gathers per thread before it multiplies and stores the current one.
__global__ __launch_bounds__(256) void first_conv_bf16_kernel(const float *__restrict__ x, const __bf16 *__restrict__ wp,
                                                              const float *__restrict__ scale, const float *__restrict__ shift,
                                                              __bf16 *__restrict__ y, int batch, int din_log2, int act) {
    constexpr int COUT = 64, EPITCH = COUT * 2 + 16;
    __shared__ __attribute__((aligned(16))) char Bs[64 * 128];         // [co][64 taps] bf16, slot-swizzled
    __shared__ __attribute__((aligned(16))) char As[128 * 128];        // [row][64 taps] bf16, slot-swizzled
    __shared__ __attribute__((aligned(16))) char Es[128 * EPITCH];     // output tile [row][64 co] bf16
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = din_log2, lo = li - 1, n = 1 << li, omsk = (1 << lo) - 1;
    const long M = (long)batch << (3 * lo);
    const int ntiles = (int)((M + 127) >> 7);
    const int pos = tid & 7, r0 = tid >> 3;
    const int gchunk = pos ^ ((r0 >> 1) & 7);

    for (int i = tid; i < 64 * 8; i += 256) {            // weights: 64 rows x 8 slots, once per workgroup
        const int row = i >> 3, slot = i & 7;
        *reinterpret_cast<uint4 *>(Bs + vv_swz_off(row, slot)) = *reinterpret_cast<const uint4 *>(wp + row * 64 + slot * 8);
    }

    // The gather only ISSUES loads (invalid taps read a zero word through a selected address, so nothing consumes the
    // values here); conversion to bf16 happens when the tile is written to LDS, one loop iteration later.
    float raw[4][8];
    auto gather = [&](int tile) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long m = (long)tile * 128 + r0 + 32 * i;
            const int ow = (int)(m & omsk), oh = (int)((m >> lo) & omsk), od = (int)((m >> (2 * lo)) & omsk);
            const long b = m >> (3 * lo);
            const int d0 = 2 * od - 1, h0 = 2 * oh - 1, w0 = 2 * ow - 1;
#pragma unroll
            for (int r = 0; r < 2; ++r) {                 // slot = taps (td, th0 + r, tw 0..3): one run of 4 voxels along w
                const int td = gchunk >> 1, th = ((gchunk & 1) << 1) + r;
                const bool ok = m < M && (unsigned)(d0 + td) < (unsigned)n && (unsigned)(h0 + th) < (unsigned)n;
                const float *xr = x + ((((((b << li) + d0 + td) << li) + h0 + th) << li) + w0);
                const float *p0 = (ok && w0 >= 0) ? xr : &vv_zero_word, *p1 = ok ? xr + 1 : &vv_zero_word;
                const float *p2 = ok ? xr + 2 : &vv_zero_word, *p3 = (ok && w0 + 3 < n) ? xr + 3 : &vv_zero_word;
                raw[i][4 * r + 0] = *p0; raw[i][4 * r + 1] = *p1; raw[i][4 * r + 2] = *p2; raw[i][4 * r + 3] = *p3;
            }
        }
    };

    const int fr = lane & 31, fh = lane >> 5;
    int tile = blockIdx.x;
    if (tile < ntiles) gather(tile);
    for (; tile < ntiles; tile += gridDim.x) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bf16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = static_cast<__bf16>(raw[i][e]);
            *reinterpret_cast<bf16x8 *>(As + (r0 + 32 * i) * 128 + pos * 16) = v;
        }
        __syncthreads();
        if (tile + (int)gridDim.x < ntiles) gather(tile + gridDim.x);    // in flight during the MFMAs and the stores below

        f32x16 acc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const uint4 fb = *reinterpret_cast<const uint4 *>(Bs + vv_swz_off(wn * 32 + fr, ks * 2 + fh));
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const uint4 fa = *reinterpret_cast<const uint4 *>(As + vv_swz_off(wm * 64 + i * 32 + fr, ks * 2 + fh));
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&fb),
                                                                 *reinterpret_cast<const bf16x8 *>(&fa), acc[i], 0, 0, 0);   // D[co][row]
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = wn * 32 + 8 * g + 4 * fh;
            f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
            if (scale) sc = *reinterpret_cast<const f32x4 *>(scale + c);
            if (shift) sh = *reinterpret_cast<const f32x4 *>(shift + c);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                bf16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[i][4 * g + e] * sc[e] + sh[e];
                    if (act == VV_ACT_ELU) t = t > 0.f ? t : __expf(t) - 1.f;
                    else if (act == VV_ACT_RELU) t = fmaxf(t, 0.f);
                    else if (act == VV_ACT_LRELU) t = t > 0.f ? t : 0.3f * t;
                    o[e] = static_cast<__bf16>(t);
                }
                *reinterpret_cast<bf16x4 *>(Es + (wm * 64 + i * 32 + fr) * EPITCH + c * 2) = o;
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, rl = idx >> 3, c = idx & 7;
            const long m = (long)tile * 128 + rl;
            if (m < M) *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(y) + m * (COUT * 2) + c * 16) =
                           *reinterpret_cast<const uint4 *>(Es + rl * EPITCH + c * 16);
        }
    }
}

// first_conv, plane form (bf16, 32 <= D <= 256): one work item = 256 outputs of ONE output plane (all D/2 columns x
// 512/D rows) x 64 channels.  Its input is 4 consecutive occupancy planes (2 od - 1 .. 2 od + 2), full-width rows: a
// single contiguous stream of float4 loads per item (the gather form above re-reads every voxel 8x as scattered dwords).
// The planes are kept in LDS as bf16 with a one-voxel left pad, S[c + 1] = x[c], so that dword j of a row holds
// (x[2j-1], x[2j]): the 4 taps tw = 0..3 of output column ow are dwords ow, ow+1 -- the MFMA B fragment of a lane
// (k = 16 td + 8 fh + j  <->  th = 2 fh + (j>>2), tw = j&3) is two 8-byte LDS reads, and no im2col tile is ever written.
// Weights (64 x 64 taps) live in registers as A fragments for the whole persistent loop; the next item's planes are in
// flight (registers) while the current item multiplies, transposes through LDS and stores its contiguous 32 KiB.
template <int NI, bool OUT8>       // OUT8: store e4m3fn (64-byte rows) for an fp8 second layer instead of bf16
__global__ __launch_bounds__(256, 3) void first_conv_plane_kernel(const float *__restrict__ x, const __bf16 *__restrict__ wp,
                                                               const float *__restrict__ scale, const float *__restrict__ shift,
                                                               void *__restrict__ y, int batch, int din_log2, int act, int items_per_wg) {
    constexpr int COUT = 64, EPITCH = COUT * 2;            // output rows are 8 chunks of 16 B, chunk ^ (row & 7); fp8: 4 chunks, chunk ^ (row & 3)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = din_log2, D = 1 << li, lo = li - 1, OW = 1 << lo;
    const int loh = 8 - lo, OH = 1 << loh;                 // output rows per item
    const int R = 2 * OH + 2, PD = (D >> 1) + 2, PP = R * PD;   // tile rows per plane, dwords per row / per plane
    // bf16 output: the tile is double buffered and the outputs go from registers to memory (v_permlane32_swap pairs, 16-byte
    // stores), so an item costs ONE barrier (tile published) -- the stage transpose, its barrier and its 32 KiB are the fp8
    // output form's only (OUT8: [256][EPITCH] stage in place of the second tile buffer)
    unsigned *tile0 = reinterpret_cast<unsigned *>(smem);  // [4][R][PD] dwords of bf16 pairs
    const int tile_bytes = (4 * PP * 4 + 15) & ~15;
    char *stage = smem + tile_bytes;                       // OUT8 only
    float *ss = reinterpret_cast<float *>(smem + tile_bytes + (OUT8 ? 256 * EPITCH : tile_bytes));   // folded BN: scale[64], shift[64]
    uint4 *wl = reinterpret_cast<uint4 *>(ss + 128);       // weights as A fragments [ks][nt][lane]
    if (tid < 64) ss[tid] = scale ? scale[tid] : 1.f;
    else if (tid < 128) ss[tid] = shift ? shift[tid - 64] : 0.f;
    const int hblocks = OW >> loh;                         // items per output plane
    const long nitems = (long)batch * OW * hblocks;

    // ---- per-thread load slots (the same for every item): slot s = tid + 256 i -> (plane, tile row, float4 column)
    const int qpr = D >> 2, lq = li - 2;                   // float4 per row
    const int nslots = 4 * R * qpr;
    int sp[NI], srr[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int s = tid + 256 * i, row = s >> lq;        // row = plane * R + rr
        sp[i] = s < nslots ? row / R : -1;
        srr[i] = row - (s < nslots ? row / R : 0) * R;
    }
    const int m4 = tid & (qpr - 1);                        // float4 column (256 % qpr == 0)

    // ---- weights as A fragments: [ks][nt], lane (co = nt*32 + lane&31, k = ks*16 + 8*(lane>>5) + j)
    const int fr = lane & 31, fh = lane >> 5;
    for (int i = wave; i < 8; i += 4)                      // i = ks*2 + nt
        wl[i * 64 + lane] = *reinterpret_cast<const uint4 *>(wp + ((i & 1) * 32 + fr) * 64 + (i >> 1) * 16 + 8 * fh);

    float4 raw[NI];
    auto fetch = [&](long item) {
        const int hb = (int)(item % hblocks);
        const long t = item / hblocks;
        const int od = (int)(t & (OW - 1));
        const long b = t >> lo;
        const int d0 = 2 * od - 1, h0 = 2 * hb * OH - 1;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int id = d0 + sp[i], ih = h0 + srr[i];
            const bool ok = sp[i] >= 0 && (unsigned)id < (unsigned)D && (unsigned)ih < (unsigned)D;
            raw[i] = ok ? *reinterpret_cast<const float4 *>(x + ((((b << li) + id) << li) + ih << li) + 4 * m4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto pack2 = [](float a, float b) -> unsigned {
        const __bf16 ha = static_cast<__bf16>(a), hb = static_cast<__bf16>(b);
        return (unsigned)__builtin_bit_cast(unsigned short, ha) | ((unsigned)__builtin_bit_cast(unsigned short, hb) << 16);
    };

    const long item0 = (long)blockIdx.x * items_per_wg;
    const long item_end = item0 + items_per_wg < nitems ? item0 + items_per_wg : nitems;
    if (item0 < item_end) fetch(item0);
    auto run = [&](auto act_c) {
    constexpr int ACT = decltype(act_c)::value;
    int buf = 0;
    for (long item = item0; item < item_end; ++item) {
        unsigned *tile = OUT8 ? tile0 : tile0 + buf * (tile_bytes >> 2);
        buf ^= 1;
        // ---- planes -> LDS (bf16 pairs, left pad)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            float left = __shfl_up(raw[i].w, 1);
            if (m4 == 0) left = 0.f;
            if (sp[i] >= 0) {
                unsigned *dst = tile + (sp[i] * R + srr[i]) * PD + 2 * m4;
                *reinterpret_cast<uint2 *>(dst) = make_uint2(pack2(left, raw[i].x), pack2(raw[i].y, raw[i].z));
                if (m4 == qpr - 1) dst[2] = pack2(raw[i].w, 0.f);
            }
        }
        __syncthreads();
        if (item + 1 < item_end) fetch(item + 1);

        // one 32-output row tile at a time (2 x 16 accumulator registers live): 8 MFMAs, then its epilogue
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x16 acc[2];                                  // [nt]
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;
            const int o = (wave * 2 + mt) * 32 + fr, ohl = o >> lo, ow = o & (OW - 1);
            const unsigned *t0 = tile + (2 * ohl + 2 * fh) * PD + ow;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const unsigned *t1 = t0 + ks * PP;
                const uint4 xf = make_uint4(t1[0], t1[1], t1[PD], t1[PD + 1]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const uint4 wf = wl[(ks * 2 + nt) * 64 + lane];
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&wf),
                                                                      *reinterpret_cast<const bf16x8 *>(&xf), acc[nt], 0, 0, 0);
                }
            }
            if constexpr (!OUT8) {
                // folded BN + activation; lanes fr / fr + 32 hold channels 8g + 0..3 / 8g + 4..7 of output o: swapping the upper
                // half of quad 2j with the lower half of quad 2j + 1 gives every lane 8 consecutive channels (guide T21)
                char *yo = reinterpret_cast<char *>(y) + item * (256 * COUT * 2) + o * (COUT * 2) + fh * 16;
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    u32x2 oq[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int c = nt * 32 + 8 * g + 4 * fh;
                        const f32x4 sc = *reinterpret_cast<const f32x4 *>(ss + c), sh = *reinterpret_cast<const f32x4 *>(ss + 64 + c);
                        f32x4 tv = f32x4{acc[nt][4 * g], acc[nt][4 * g + 1], acc[nt][4 * g + 2], acc[nt][4 * g + 3]};
                        tv = vv_bn_act4<ACT>(tv, sc, sh);
                        bf16x4 ov;
#pragma unroll
                        for (int e = 0; e < 4; ++e) ov[e] = static_cast<__bf16>(tv[e]);
                        oq[g] = *reinterpret_cast<const u32x2 *>(&ov);
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        auto rx = __builtin_amdgcn_permlane32_swap(oq[2 * j][0], oq[2 * j + 1][0], false, false);
                        auto ry = __builtin_amdgcn_permlane32_swap(oq[2 * j][1], oq[2 * j + 1][1], false, false);
                        *reinterpret_cast<u32x4 *>(yo + nt * 64 + j * 32) = u32x4{rx[0], ry[0], rx[1], ry[1]};
                    }
                }
            } else
            // folded BN + activation, transpose through LDS
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = nt * 32 + 8 * g + 4 * fh;
                    const f32x4 sc = *reinterpret_cast<const f32x4 *>(ss + c), sh = *reinterpret_cast<const f32x4 *>(ss + 64 + c);
                    f32x4 tv = f32x4{acc[nt][4 * g], acc[nt][4 * g + 1], acc[nt][4 * g + 2], acc[nt][4 * g + 3]};
                    tv = vv_bn_act4<ACT>(tv, sc, sh);
                    if constexpr (OUT8) {                  // e4m3fn for an fp8 second layer: 64-byte rows
                        *reinterpret_cast<unsigned *>(stage + o * EPITCH + ((((c >> 4) ^ o) & 3) << 4) + (c & 12)) = vv_pack_fp8x4(tv);
                    } else {
                        bf16x4 ov;
#pragma unroll
                        for (int e = 0; e < 4; ++e) ov[e] = static_cast<__bf16>(tv[e]);
                        *reinterpret_cast<bf16x4 *>(stage + o * EPITCH + ((((c >> 3) ^ o) & 7) << 4) + (c & 4) * 2) = ov;
                    }
                }
        }
        if constexpr (OUT8) {
            __syncthreads();
            char *yo = reinterpret_cast<char *>(y) + item * (256 * COUT);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = tid + 256 * i, rl = idx >> 2, c = idx & 3;
                *reinterpret_cast<uint4 *>(yo + (size_t)idx * 16) = *reinterpret_cast<const uint4 *>(stage + rl * EPITCH + (((c ^ rl) & 3) << 4));
            }
        }
    }
    };
    VV_WITH_ACT(act, run);
}

// first_conv, chained plane form (D = 32 or 64, bf16 or e4m3fn output, at least two consecutive items per workgroup).  One item =
// 256 outputs x 64 channels of ONE output plane od (D = 32: the whole 16 x 16 plane; D = 64: 8 of its 32 rows) from input planes
// 2 od - 1 .. 2 od + 2; the next output plane of the same sample (and row block) needs 2 od + 1 .. 2 od + 4: half of what is
// already in LDS.  The plane form above loads all four planes for every item (16 planes per four-item workgroup, every input plane
// fetched twice chip-wide); here the items are ordered with od fastest, the tile is a ring of four HALF tiles (two planes each), an
// item takes its first half from its predecessor's second one and only the two new planes travel (10 planes per four-item
// workgroup): 37 % fewer load instructions, conversions and LDS writes, 12 instead of 20 prefetch registers -- which is what lets
// FOUR workgroups per CU fit in 128 VGPRs without scratch (the plane form had drifted to 134 = three per CU under a launcher that
// still dealt the items for four: a 1.33-round grid).  Loads go through a buffer descriptor: a slot in the SAME padding (plane -1 / D,
// rows -1 / D) or past the slot list reads offset 0xFFFFFFF0 and comes back as zeros, no exec-masked branch per load.  The e4m3fn
// output goes from registers to memory as well (two v_permlane32_swap per 32 channels give a lane 16 consecutive channels = one
// 16-byte store): no 32 KiB transpose stage, no second barrier, four workgroups per CU instead of three.
// Ring safety with ONE barrier per item: item j reads halves (A_j, B_j); the halves written at the top of item j + 1 are the next one
// or two ring positions, never A_j or B_j (four positions), and nobody is behind item j (everyone passed barrier j + 1's predecessor).
template <int LI, bool OUT8>
__global__ __launch_bounds__(256, 4) void first_conv_chain_kernel(const float *__restrict__ x, const __bf16 *__restrict__ wp,
                                                                  const float *__restrict__ scale, const float *__restrict__ shift,
                                                                  void *__restrict__ y, int batch, int act, int items_per_wg) {
    constexpr int COUT = 64, D = 1 << LI, LO = LI - 1, OW = 1 << LO, OH = 256 / OW, LHB = LO - (8 - LO);   // hblocks = OW / OH = 2^LHB
    constexpr int R = 2 * OH + 2, PD = OW + 2, PP = R * PD, HALF = 2 * PP;   // tile rows per plane, dwords per row / plane / half tile
    constexpr int QPR = D / 4, LQ = LI - 2;                // float4 per input row
    constexpr int NIH = (2 * R * QPR + 255) / 256;         // float4 slots per thread and half (544 / 576 -> 3)
    constexpr int ROW = COUT * (OUT8 ? 1 : 2);             // bytes per output voxel
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned *ring = reinterpret_cast<unsigned *>(smem);   // [4 halves][2 planes][R][PD] dwords of bf16 pairs (left pad: dword j = (x[2j-1], x[2j]))
    float *ss = reinterpret_cast<float *>(smem + 4 * HALF * 4);
    uint4 *wl = reinterpret_cast<uint4 *>(ss + 128);       // weights as A fragments [ks][nt][lane]
    if (tid < 64) ss[tid] = scale ? scale[tid] : 1.f;
    else if (tid < 128) ss[tid] = shift ? shift[tid - 64] : 0.f;
    const long nitems = ((long)batch << LO) << LHB;

    const int m4 = tid & (QPR - 1);                        // float4 column of every slot of this thread
    int loff[NIH], pl[NIH], rr[NIH];                       // dword offset inside a half (-1: no slot); plane of the half (-4 D: none); tile row
    unsigned soff[NIH];                                    // byte offset from (first plane of the half, first tile row, column 0)
#pragma unroll
    for (int i = 0; i < NIH; ++i) {
        const int s = tid + 256 * i, row = s >> LQ, p = row >= R ? 1 : 0;
        const bool slot = s < 2 * R * QPR;
        rr[i] = row - p * R;
        loff[i] = slot ? (p * R + rr[i]) * PD + 2 * m4 : -1;
        pl[i] = slot ? p : -4 * D;
        soff[i] = (unsigned)((((p << LI) + rr[i]) << LI) + 4 * m4) * 4u;
    }
    const int fr = lane & 31, fh = lane >> 5;
    for (int i = wave; i < 8; i += 4)                      // i = ks*2 + nt
        wl[i * 64 + lane] = *reinterpret_cast<const uint4 *>(wp + ((i & 1) * 32 + fr) * 64 + (i >> 1) * 16 + 8 * fh);

    const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(x), 0, (int)(((unsigned)batch << (3 * LI)) * 4u), 0x00020000);
    // item -> (sample, row block, output plane), od fastest
    auto decode = [&](long item, int &b, int &hb, int &od) {
        od = (int)(item & (OW - 1));
        hb = (int)(item >> LO) & ((1 << LHB) - 1);
        b = (int)(item >> (LO + LHB));
    };
    auto load_half = [&](int b, int hb, int d, f32x4 (&r)[NIH]) {   // planes d, d + 1 of sample b, tile rows of row block hb
        const int h0 = 2 * hb * OH - 1;
        const unsigned base = (unsigned)(((((b << LI) + d) << LI) + h0) << LI) * 4u;     // wraps below zero for d / h0 = -1; valid slots land back in range
#pragma unroll
        for (int i = 0; i < NIH; ++i) {
            const bool ok = (unsigned)(d + pl[i]) < (unsigned)D && (unsigned)(h0 + rr[i]) < (unsigned)D;
            // (whole-vector bit cast: __builtin_bit_cast(float, v[k]) on a vector ELEMENT reads element 0 for every k with this compiler)
            r[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsx, (int)(ok ? base + soff[i] : 0xFFFFFFF0u), 0, 0));
        }
    };
    auto pack2 = [](float a, float b) -> unsigned {
        const __bf16 ha = static_cast<__bf16>(a), hb = static_cast<__bf16>(b);
        return (unsigned)__builtin_bit_cast(unsigned short, ha) | ((unsigned)__builtin_bit_cast(unsigned short, hb) << 16);
    };
    auto write_half = [&](int h, const f32x4 (&r)[NIH]) {
        unsigned *half = ring + h * HALF;
#pragma unroll
        for (int i = 0; i < NIH; ++i) {
            float left = __shfl_up(r[i][3], 1);
            if (m4 == 0) left = 0.f;
            if (loff[i] >= 0) {
                unsigned *dst = half + loff[i];
                *reinterpret_cast<uint2 *>(dst) = make_uint2(pack2(left, r[i][0]), pack2(r[i][1], r[i][2]));
                if (m4 == QPR - 1) dst[2] = pack2(r[i][3], 0.f);
            }
        }
    };

    const long item0 = (long)blockIdx.x * items_per_wg;
    const long item_end = item0 + items_per_wg < nitems ? item0 + items_per_wg : nitems;
    f32x4 raw[NIH];                                        // the second half (planes 2 od + 1, 2 od + 2) of the item about to run
    if (item0 < item_end) {
        int b, hb, od;
        decode(item0, b, hb, od);
        load_half(b, hb, 2 * od + 1, raw);
    }
    auto run = [&](auto act_c) {
    constexpr int ACT = decltype(act_c)::value;
    int nxt = 0, hA = 0, hB = 0;
    for (long item = item0; item < item_end; ++item) {
        int b, hb, od;
        decode(item, b, hb, od);
        if (item == item0 || od == 0) {                    // no predecessor in this workgroup / for this row block: planes 2 od - 1, 2 od as well
            f32x4 ra[NIH];
            load_half(b, hb, 2 * od - 1, ra);
            write_half(nxt, ra);
            hA = nxt;
            nxt = (nxt + 1) & 3;
        } else hA = hB;
        write_half(nxt, raw);
        hB = nxt;
        nxt = (nxt + 1) & 3;
        __syncthreads();
        if (item + 1 < item_end) {
            int nb, nhb, nod;
            decode(item + 1, nb, nhb, nod);
            load_half(nb, nhb, 2 * nod + 1, raw);
        }
        const unsigned *tA = ring + hA * HALF, *tB = ring + hB * HALF;
        const long oitem = ((((long)b << LO) + od) << LHB) + hb;      // the output is (sample, plane, row block) major
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x16 acc[2];                                  // [nt]
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[c][e] = 0.f;
            const int o = (wave * 2 + mt) * 32 + fr, ohl = o >> LO, ow = o & (OW - 1);
            const int ti = (2 * ohl + 2 * fh) * PD + ow;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const unsigned *t1 = (ks < 2 ? tA + ks * PP : tB + (ks - 2) * PP) + ti;
                const uint4 xf = make_uint4(t1[0], t1[1], t1[PD], t1[PD + 1]);
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const uint4 wf = wl[(ks * 2 + nt) * 64 + lane];
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8 *>(&wf),
                                                                      *reinterpret_cast<const bf16x8 *>(&xf), acc[nt], 0, 0, 0);
                }
            }
            // folded BN + activation; lanes fr / fr + 32 hold channels 8g + 0..3 / 8g + 4..7 of output o
            char *yo = reinterpret_cast<char *>(y) + oitem * (256 * ROW) + o * ROW;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                u32x2 oq[4];
                unsigned o8[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = nt * 32 + 8 * g + 4 * fh;
                    const f32x4 sc = *reinterpret_cast<const f32x4 *>(ss + c), sh = *reinterpret_cast<const f32x4 *>(ss + 64 + c);
                    f32x4 tv = f32x4{acc[nt][4 * g], acc[nt][4 * g + 1], acc[nt][4 * g + 2], acc[nt][4 * g + 3]};
                    tv = vv_bn_act4<ACT>(tv, sc, sh);
                    if constexpr (OUT8) o8[g] = vv_pack_fp8x4(tv);
                    else {
                        bf16x4 ov;
#pragma unroll
                        for (int e = 0; e < 4; ++e) ov[e] = static_cast<__bf16>(tv[e]);
                        oq[g] = *reinterpret_cast<const u32x2 *>(&ov);
                    }
                }
                if constexpr (OUT8) {
                    // dword g of lane half fh = channels 8g + 4fh .. + 3.  swap(g + 2, g): the upper half of dword g + 2 goes to the lower
                    // lanes' dword g and back -- lower lanes end with (g + 2: fh 0, fh 1) = 8 consecutive channels of group g + 2, upper
                    // lanes with those of group g: lane half 0 stores channels 16 .. 31, lane half 1 channels 0 .. 15 of this 32-block
                    auto r0 = __builtin_amdgcn_permlane32_swap(o8[2], o8[0], false, false);
                    auto r1 = __builtin_amdgcn_permlane32_swap(o8[3], o8[1], false, false);
                    *reinterpret_cast<u32x4 *>(yo + nt * 32 + (1 - fh) * 16) = u32x4{r0[0], r0[1], r1[0], r1[1]};
                } else {
                    // swapping the upper half of quad 2j with the lower half of quad 2j + 1 gives every lane 8 consecutive channels (guide T21)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        auto rx = __builtin_amdgcn_permlane32_swap(oq[2 * j][0], oq[2 * j + 1][0], false, false);
                        auto ry = __builtin_amdgcn_permlane32_swap(oq[2 * j][1], oq[2 * j + 1][1], false, false);
                        *reinterpret_cast<u32x4 *>(yo + fh * 16 + nt * 64 + j * 32) = u32x4{rx[0], ry[0], rx[1], ry[1]};
                    }
                }
            }
        }
    }
    };
    VV_WITH_ACT(act, run);
}

}  // namespace

// bf16 fast path of vv_conv3d_first_fwd (igemm.hip dispatches here): w_packed = vv_pack_conv_k4(cin = 1) = [64][64] bf16.
int vv_first_conv_bf16_launch(const float *x, const void *w_packed, const float *scale, const float *shift, void *y, int batch,
                              int side, int act, void *stream, int out_fp8) {
    const int li = vv_log2(side);
    if (out_fp8 && !(side >= 32 && side <= 256)) return VV_ERR_DTYPE;      // only the plane-form kernel stores e4m3fn
    if (side >= 32 && side <= 256 && (out_fp8 || !vv_hook("VV_FIRSTCONV_GATHER"))) {
        const int ow = side / 2, oh = 256 / ow, r = 2 * oh + 2, pd = side / 2 + 2;
        const long nitems = (long)batch * ow * (ow / oh);
        const size_t tile_b = ((size_t)4 * r * pd * 4 + 15) & ~(size_t)15;
        const size_t lds = tile_b + (out_fp8 ? (size_t)256 * (64 * 2) : tile_b) + 128 * sizeof(float) + 8 * 64 * 16;
        const int nslots = 4 * r * (side / 4), ni = (nslots + 255) / 256;
        static const long envwg = vv_hook_int(vv_hook("VV_FIRSTCONV_WGS"), 0);
        // D = 32 / 64 and batches that give every workgroup a chain of >= 2 consecutive output planes: the chained kernel, FOUR persistent
        // workgroups per CU (D = 32, batch 256: 4,096 items = 1,024 x 4); its input offsets are 32-bit (< 2 GiB of input per launch)
        const bool nochain = vv_hook("VV_FIRSTCONV_NOCHAIN") != nullptr;      // test hook: the plane form at every batch
        if ((side == 32 || side == 64) && !nochain && (size_t)batch * side * side * side * sizeof(float) < 0x7FFFFFFFull) {
            const long maxwg4 = envwg > 0 ? envwg : 256 * 4;
            const int ipw4 = (int)((nitems + maxwg4 - 1) / maxwg4);
            if (ipw4 >= 2) {
                const size_t lds4 = (size_t)4 * 2 * r * pd * 4 + 128 * sizeof(float) + 8 * 64 * 16;
                const dim3 g4((unsigned)((nitems + ipw4 - 1) / ipw4));
                hipStream_t st4 = reinterpret_cast<hipStream_t>(stream);
                const __bf16 *wb4 = reinterpret_cast<const __bf16 *>(w_packed);
                if (side == 32) {
                    if (out_fp8) VV_LAUNCH((first_conv_chain_kernel<5, true>), g4, dim3(256), lds4, st4, x, wb4, scale, shift, y, batch, act, ipw4);
                    else VV_LAUNCH((first_conv_chain_kernel<5, false>), g4, dim3(256), lds4, st4, x, wb4, scale, shift, y, batch, act, ipw4);
                } else {
                    if (out_fp8) VV_LAUNCH((first_conv_chain_kernel<6, true>), g4, dim3(256), lds4, st4, x, wb4, scale, shift, y, batch, act, ipw4);
                    else VV_LAUNCH((first_conv_chain_kernel<6, false>), g4, dim3(256), lds4, st4, x, wb4, scale, shift, y, batch, act, ipw4);
                }
                return vv_launch_status();
            }
        }
        // persistent workgroups of the plane form: what fits a CU at once = 3 (134-168 VGPRs; the bf16-output form at D = 32 once fitted 4)
        const long maxwg = envwg > 0 ? envwg : 256 * 3;
        const int ipw = (int)((nitems + maxwg - 1) / maxwg);
        const int grid = (int)((nitems + ipw - 1) / ipw);
        hipStream_t st = reinterpret_cast<hipStream_t>(stream);
        const __bf16 *wb = reinterpret_cast<const __bf16 *>(w_packed);
        if (ni <= 5) {
            if (out_fp8) VV_LAUNCH((first_conv_plane_kernel<5, true>), dim3(grid), dim3(256), lds, st, x, wb, scale, shift, y, batch, li, act, ipw);
            else VV_LAUNCH((first_conv_plane_kernel<5, false>), dim3(grid), dim3(256), lds, st, x, wb, scale, shift, y, batch, li, act, ipw);
        } else {
            if (out_fp8) VV_LAUNCH((first_conv_plane_kernel<6, true>), dim3(grid), dim3(256), lds, st, x, wb, scale, shift, y, batch, li, act, ipw);
            else VV_LAUNCH((first_conv_plane_kernel<6, false>), dim3(grid), dim3(256), lds, st, x, wb, scale, shift, y, batch, li, act, ipw);
        }
        return vv_launch_status();
    }
    const long M = (long)batch << (3 * (li - 1));
    const int ntiles = (int)((M + 127) / 128);
    const int grid = ntiles < 2048 ? ntiles : 2048;
    VV_LAUNCH(first_conv_bf16_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
              reinterpret_cast<const __bf16 *>(w_packed), scale, shift, reinterpret_cast<__bf16 *>(y), batch, li, act);
    return vv_launch_status();
}
