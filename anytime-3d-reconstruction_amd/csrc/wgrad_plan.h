// Which kernel a weight gradient runs on and how its reduction is split, stated once for vv_wgrad_dense, vv_wgrad_conv_k4s2 and
// vv_wgrad_workspace_bytes (wgrad.hip, wgrad_phase.hip).  Plain C++: it also compiles without a GPU compiler
// (tests/wgrad_plan_main.cpp prints the routes, tests/test_wgrad_plan_host.py compares them with the restatement the GPU tests use).
#pragma once
#include <stddef.h>

enum { WG_DT_F32 = 0, WG_DT_BF16 = 1 };        // = VV_F32, VV_BF16 of voxvae.h (asserted in wgrad.hip)

// The kernel forms, in the entries' order of preference.
enum WgradForm {
    WG_PHASE,          // wgrad_phase_kernel<LS>: stride-2 layer, taps split by parity
    WG_BF16_TAPS,      // wgrad_bf16_kernel<1>: stride-2 layer, 64-tap rows by LDS-DMA
    WG_BF16_GRID,      // wgrad_bf16_kernel<2> (<2, true> when N <= 64): one source channel, rows built from the float32 grid
    WG_BF16_DENSE,     // wgrad_bf16_kernel<0>
    WG_F32,            // wgrad_kernel<0 | 1 | 2, BN>: any operand types, widened to float32
    WG_FORMS
};
enum WgradReduce { WG_REDUCE_NONE, WG_REDUCE_PLAIN, WG_REDUCE_SLICED };

// splits slabs [M][N] of float32; rps = reduction rows per split (WG_PHASE: boxes of 128 rows per split); bn = tile width in N
struct WgradPlan { int bn, splits, rps; size_t ws; };

// float32 kernel: 64 x bn tiles, 32-row chunks
inline WgradPlan wgrad_plan(long R, int M, int N) {
    WgradPlan p;
    p.bn = (N % 128 == 0) ? 128 : 64;
    const long tiles = (long)((M + 63) / 64) * ((N + p.bn - 1) / p.bn);
    long chunks = (R + 31) / 32;
    long splits = 1;
    while (tiles * splits < 1024 && splits * 2 <= chunks && splits < 256) splits *= 2;
    p.rps = (int)(((chunks + splits - 1) / splits) * 32);
    p.splits = (int)((R + p.rps - 1) / p.rps);
    p.ws = (size_t)p.splits * M * N * sizeof(float);
    return p;
}

// bf16 kernel: 128 x 128 tiles, 64-row chunks
inline WgradPlan wgrad_plan_bf16(long R, int M, int N) {
    WgradPlan p;
    p.bn = 128;
    const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
    long chunks = (R + 63) / 64;
    long splits = 1;
    // one or two tiles (the single-channel layers, M = N = 64): the kernel is a latency-bound stream over the rows, so
    // four workgroups per CU's worth of splits instead of two
    const long want = tiles <= 2 ? 1024 : 512;
    while (tiles * splits < want && splits * 2 <= chunks && splits < want) splits *= 2;
    p.rps = (int)(((chunks + splits - 1) / splits) * 64);
    p.splits = (int)((R + p.rps - 1) / p.rps);
    p.ws = (size_t)p.splits * M * N * sizeof(float);
    return p;
}

// phase kernel: boxes of 128 rows, workgroup kinds = 8 parities x (cin / 64) x (cout / 128); slabs [64 cin][cout].  The plan depends on
// the row count and the channel blocks only; without whole channel blocks there is no plan (no slabs).
inline WgradPlan wg_phase_plan(long rows, int cin, int cout) {
    WgradPlan p = {128, 0, 0, 0};
    if (cin <= 0 || cout <= 0 || cin % 64 || cout % 128) return p;
    const int nboxes = (int)((rows + 127) / 128);
    const int kinds = 8 * (cin / 64) * (cout / 128);
    int splits = 1;
    while (kinds * splits * 2 <= 256 && splits * 2 <= nboxes) splits *= 2;     // one workgroup per CU (LDS-bound occupancy)
    p.rps = (nboxes + splits - 1) / splits;
    p.splits = (nboxes + p.rps - 1) / p.rps;
    p.ws = (size_t)p.splits * 64 * cin * cout * sizeof(float);
    return p;
}

// THE list: the plan of every form for `rows` reduction rows and an [m][n] result (m = 64 cin, n = cout for the stride-2 layers).
inline WgradPlan wgrad_form_plan(int form, long rows, int m, int n) {
    switch (form) {
    case WG_PHASE: return m % 4096 == 0 ? wg_phase_plan(rows, m / 64, n) : WgradPlan{128, 0, 0, 0};
    case WG_BF16_TAPS:
    case WG_BF16_GRID:
    case WG_BF16_DENSE: return wgrad_plan_bf16(rows, m, n);
    default: return wgrad_plan(rows, m, n);
    }
}

// The caller of an entry need not know which kernel runs: the largest slab set of any form.
inline size_t wgrad_workspace_bytes(long rows, int m, int n) {
    size_t ws = 0;
    for (int form = 0; form < WG_FORMS; ++form) {
        const size_t w = wgrad_form_plan(form, rows, m, n).ws;
        if (w > ws) ws = w;
    }
    return ws;
}

// WG_BF16_GRID with at most 64 output channels is a single 64 x 64 tile: wgrad_bf16_kernel<2, true>.
inline bool wgrad_grid_one_tile(int n) { return n <= 64; }

// Sum of the slabs: few outputs and many slabs -> wgrad_reduce_sliced_kernel, else wgrad_reduce_kernel; a bf16 reduction-GEMM kernel with
// one split writes dw itself.
inline bool wgrad_reduce_sliced(int splits, long n) { return splits >= 16 && n <= 65536; }
inline WgradReduce wgrad_reduce_kind(int form, int splits, long n) {
    const bool bf16_gemm = form == WG_BF16_TAPS || form == WG_BF16_GRID || form == WG_BF16_DENSE;
    if (bf16_gemm && splits == 1) return WG_REDUCE_NONE;
    return wgrad_reduce_sliced(splits, n) ? WG_REDUCE_SLICED : WG_REDUCE_PLAIN;
}

struct WgradRoute { WgradForm form; WgradPlan plan; WgradReduce reduce; };
inline WgradRoute wgrad_route_of(WgradForm form, long rows, int m, int n) {
    WgradRoute r;
    r.form = form;
    r.plan = wgrad_form_plan(form, rows, m, n);
    r.reduce = wgrad_reduce_kind(form, r.plan.splits, (long)m * n);
    return r;
}

// The bf16 kernels address either operand through a 32-bit buffer offset: `elems` bf16 elements must end below the out-of-range marker.
inline bool wgrad_bf16_span_ok(size_t elems) { return elems * 2 < 0xFFFFFFF0ull; }

// vv_wgrad_dense on validated arguments.  a_aligned / g_aligned: the operand starts on a 16-byte boundary; f32_only: VV_WGRAD_F32 is set.
inline WgradRoute wgrad_dense_route(long rows, int m, int n, int lda, int a_dtype, int g_dtype, bool a_aligned, bool g_aligned,
                                    bool f32_only) {
    const bool bf16 = a_dtype == WG_DT_BF16 && g_dtype == WG_DT_BF16 && !f32_only && m % 32 == 0 && n % 32 == 0 && lda % 8 == 0 &&
                      wgrad_bf16_span_ok((size_t)rows * lda) && wgrad_bf16_span_ok((size_t)rows * n) && a_aligned && g_aligned;
    return wgrad_route_of(bf16 ? WG_BF16_DENSE : WG_F32, rows, m, n);
}

// Single-channel sources are float32 grids in every form (vv_wgrad_conv_k4s2 refuses anything else with VV_ERR_DTYPE).
inline bool wgrad_conv_src_dtype_ok(int cin, int src_dtype) { return cin != 1 || src_dtype == WG_DT_F32; }

// vv_wgrad_conv_k4s2 on validated arguments (side a power of two >= 2, cin == 1 or cin % 64 == 0, cout % 4 == 0).  no_phase:
// VV_NO_WGRAD_PHASE is set.
inline WgradRoute wgrad_conv_route(int batch, int side, int cin, int cout, int src_dtype, int g_dtype, bool src_aligned, bool g_aligned,
                                   bool f32_only, bool no_phase) {
    const int S = side / 2;
    const long rows = (long)batch * S * S * S;
    const int m = 64 * cin;
    const size_t src_elems = (size_t)batch * side * side * side * cin;
    const bool g_ok = g_dtype == WG_DT_BF16 && !f32_only && wgrad_bf16_span_ok((size_t)rows * cout) && g_aligned;
    const bool both_ok = cin != 1 && src_dtype == WG_DT_BF16 && g_ok && cin % 64 == 0 && wgrad_bf16_span_ok(src_elems) && src_aligned;
    WgradForm form = WG_F32;
    // rows >= 128 * 8: tiny problems stay on the reduction-GEMM form, which splits finer
    if (both_ok && !no_phase && (S == 4 || S == 8 || S == 16) && cout % 128 == 0 && rows >= 128 * 8)
        form = WG_PHASE;
    else if (both_ok && m % 32 == 0 && cout % 32 == 0)
        form = WG_BF16_TAPS;
    else if (cin == 1 && side >= 4 && src_dtype == WG_DT_F32 && g_ok && cout % 32 == 0)
        form = WG_BF16_GRID;
    return wgrad_route_of(form, rows, m, cout);
}
