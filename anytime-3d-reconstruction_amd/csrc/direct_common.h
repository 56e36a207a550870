// Scaffolding shared by the direct stride-2 convolution kernels (conv_direct.hip: conv_direct_kernel, conv_direct16_kernel,
// conv_direct16h_kernel; conv_direct_fp8.hip: conv_direct_fp8_kernel).  All four work on a 4 x 8 x 8 box of outputs per workgroup and
// end the same way: folded BN + activation into an LDS stage of 256 output rows, then 16-byte stores of whole channel rows.  What
// lives here is the part that is the same expression in every one of them -- the box decode, the epilogue fills and the staged store.
// MFMA macros, fragment sets, tap loops, producers (issue_x / issue_w), the BN fetch and the wait counts stay in the kernels.
#pragma once
#include "common.h"

// Output box of this workgroup: sample b, first output cell (od0, oh0, ow0); nh = channel half (HALVES only, else 0).
struct VvDirectBox { int b, od0, oh0, ow0, nh; };

// XCD-aware order: consecutive boxes (same sample) run on one XCD and share its L2.  `no` = output side.  HALVES: the two channel
// halves of a box come first (they read the same tiles), then the boxes of a sample.
template <bool HALVES = false>
__device__ __forceinline__ VvDirectBox vv_direct_box(int no) {
    const int nwg = gridDim.x;
    int blk = (nwg & 7) == 0 ? (int)(blockIdx.x & 7) * (nwg >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    VvDirectBox o;
    o.nh = 0;
    if (HALVES) { o.nh = blk & 1; blk >>= 1; }
    const int bxw = no >> 3, bxh = no >> 3, bxd = no >> 2;
    const int bw = blk % bxw; blk /= bxw;
    const int bh = blk % bxh; blk /= bxh;
    const int bd = blk % bxd;
    o.b = blk / bxd;
    o.od0 = bd * 4; o.oh0 = bh * 8; o.ow0 = bw * 8;
    return o;
}

// One activated quad v (4 consecutive channels from c) into its stage row: e4m3fn at byte c, or bf16 at byte 2 c (inside the fills).
#define VV_DIRECT_PUT4(dst, c, v)                                                                          \
    do {                                                                                                   \
        if (FP8) {                                                                                         \
            *reinterpret_cast<unsigned *>(dst + c) = vv_pack_fp8x4(v);                                     \
        } else {                                                                                           \
            bf16x4 o;                                                                                      \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = static_cast<__bf16>(v[e]);                \
            *reinterpret_cast<bf16x4 *>(dst + c * 2) = o;                                                  \
        }                                                                                                  \
    } while (0)

// The two epilogue fills: fill(activation constant, fp8-output constant) applies folded BN + activation to the accumulators and
// packs them into the stage.  They are macros that expand to the lambda INSIDE the kernel and name its locals (acc, scv, shv = the
// BN quads fetched by the kernel, stage, wm and the lane's fragment coordinates) for the same reason VV_WITH_ACT is a macro
// (common.h): as functions or functors taking the accumulators by reference they change the register allocation of the tap loops
// in front of them (and the VGPR count of conv_direct16h_kernel), as lambdas in the kernel body they do not.  PITCH = stage row
// pitch, C0 = first channel of the wave inside the stage row.
//
// 16x16x32 forms (conv_direct16_kernel, conv_direct16h_kernel): acc[cot][ct], lane (r, kq) = channels C0 + 16 cot + 4 kq .. + 3 of
// stage row wm * 64 + 16 ct + r; scv[cot] / shv[cot].
#define VV_DIRECT_FILL16(PITCH, C0)                                                                        \
    [&](auto act_c, auto fp8_c) {                                                                          \
        constexpr int ACT = decltype(act_c)::value;                                                        \
        constexpr bool FP8 = decltype(fp8_c)::value;                                                       \
        _Pragma("unroll") for (int ct = 0; ct < 4; ++ct)                                                   \
            _Pragma("unroll") for (int cot = 0; cot < 4; ++cot) {                                          \
                const int c = (C0) + cot * 16 + 4 * kq;                                                    \
                const f32x4 sc = scv[cot], sh = shv[cot];                                                  \
                const f32x4 v = vv_bn_act4<ACT>(acc[cot][ct], sc, sh);                                     \
                char *dst = stage + (wm * 64 + ct * 16 + r) * (PITCH);                                     \
                VV_DIRECT_PUT4(dst, c, v);                                                                 \
            }                                                                                              \
    }
// 32x32 forms (conv_direct_kernel, conv_direct_fp8_kernel): acc[nt][mt][4 g + e], lane (fr, fh) = channel C0 + 32 nt + 8 g + 4 fh + e
// of stage row wm * 64 + 32 mt + fr; scv[nt][g] / shv[nt][g].  NOT vv_bn_act4: these two kernels spell the epilogue per element --
// `acc * sc + sh` left to the compiler's contraction, compare + select on __expf -- where vv_bn_act4 fixes an explicit fma and the
// packed max + (exp2 - 1) form.  The values may well agree, but nothing pins that, and the outputs of these kernels must not move by
// a bit: the spelling stays, in one copy.
#define VV_DIRECT_FILL32(PITCH, C0)                                                                        \
    [&](auto act_c, auto fp8_c) {                                                                          \
        constexpr int ACT = decltype(act_c)::value;                                                        \
        constexpr bool FP8 = decltype(fp8_c)::value;                                                       \
        _Pragma("unroll") for (int mt = 0; mt < 2; ++mt)                                                   \
            _Pragma("unroll") for (int nt = 0; nt < 2; ++nt)                                               \
                _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                            \
                    const int c = (C0) + nt * 32 + 8 * g + 4 * fh;                                         \
                    const f32x4 sc = scv[nt][g], sh = shv[nt][g];                                          \
                    f32x4 v;                                                                               \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                        \
                        float t = acc[nt][mt][4 * g + e] * sc[e] + sh[e];                                  \
                        if (ACT == VV_ACT_ELU) { const float em = __expf(fminf(t, 0.f)) - 1.f; t = t > 0.f ? t : em; } \
                        else if (ACT == VV_ACT_RELU) t = fmaxf(t, 0.f);                                    \
                        else if (ACT == VV_ACT_LRELU) t = t > 0.f ? t : 0.3f * t;                          \
                        v[e] = t;                                                                          \
                    }                                                                                      \
                    char *dst = stage + (wm * 64 + mt * 32 + fr) * (PITCH);                                \
                    VV_DIRECT_PUT4(dst, c, v);                                                             \
                }                                                                                          \
    }

// The staged box leaves as 16-byte pieces of whole channel rows (the 256 outputs of a box are contiguous in y when the output side is
// 8).  THREADS per workgroup; stage rows of PITCH bytes holding STAGE_CH channels, which are channels nh * STAGE_CH .. of y's Y_CH.
// out_fp8: the layer hands its output to an fp8 consumer (e4m3fn, 1 byte per channel) instead of bf16.
template <int THREADS, int PITCH, int STAGE_CH, int Y_CH>
__device__ __forceinline__ void vv_direct_store_box(const char *stage, void *y, const VvDirectBox &box, int lo, int tid, int out_fp8) {
    const int es = out_fp8 ? 1 : 2;
    const int cpr = STAGE_CH * es / 16;               // 16-byte chunks per stage row
    for (int id = tid; id < 256 * cpr; id += THREADS) {
        const int r = id / cpr, cc = id % cpr;
        const int od = box.od0 + (r >> 6), oh = box.oh0 + ((r >> 3) & 7), ow = box.ow0 + (r & 7);
        const size_t vox = ((((((size_t)box.b << lo) + od) << lo) + oh) << lo) + ow;
        *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(y) + vox * (Y_CH * es) + box.nh * STAGE_CH * es + cc * 16) =
            *reinterpret_cast<const uint4 *>(stage + r * PITCH + cc * 16);
    }
}
