// Index arithmetic of the 2D convolution (conv2d.hip), stated once for the device and the host: tile sizes, the padded extents of the
// packed weight image, the row -> (image, row, column) split, per-(row, tap) validity and the split-K schedule.  Plain C++: it also
// compiles without a GPU compiler (tests/conv2d_plan_main.cpp runs it under the host sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define C2_HD __host__ __device__
#else
#define C2_HD
#endif

// A 256-thread workgroup owns C2_BM GEMM rows x C2_BN output channels and walks K in chunks of C2_KC elements.  cin % 32 == 0 puts
// every chunk inside ONE tap, so validity is decided once per (row, chunk).
enum { C2_BM = 64, C2_BN = 64, C2_KC = 32, C2_MAX_SPLITS = 32, C2_MIN_CHUNKS = 4, C2_TARGET_WGS = 512, C2_FULL_WGS = 256 };

C2_HD inline int c2_kchunks(int ksize, int cin) { return (ksize * ksize * cin + C2_KC - 1) / C2_KC; }
C2_HD inline int c2_npad(int cout) { return (cout + C2_BN - 1) / C2_BN * C2_BN; }
C2_HD inline bool c2_shape_ok(int ksize, int cin, int cout) {
    return (ksize == 1 || ksize == 3) && cout >= 1 && (cin == 3 || (cin >= 32 && cin % 32 == 0));
}
// elements of the packed image: [kchunks][npad][C2_KC], k = (tr * ksize + tc) * cin + ci, zero where k or the channel is padding
C2_HD inline size_t c2_packed_elems(int ksize, int cin, int cout) { return (size_t)c2_kchunks(ksize, cin) * c2_npad(cout) * C2_KC; }

// GEMM row m = (b * R + r) * C + c.  R and C are arbitrary, so this is a division, done once per row and kept.
struct C2Row { int b, r, c; };
C2_HD inline C2Row c2_row(long m, int R, int C) {
    C2Row o;
    const long rc = (long)R * C;
    o.b = (int)(m / rc);
    const int rem = (int)(m - (long)o.b * rc);
    o.r = rem / C;
    o.c = rem - o.r * C;
    return o;
}
// Tap (tr, tc) of a row at (r, c): inside the image or not.  The ADDRESS of an outside tap is usually a valid one (column -1 is the
// previous row's last pixel, row -1 of image b the last row of image b - 1), so only this predicate may decide.
C2_HD inline bool c2_tap_valid(int r, int c, int tr, int tc, int ksize, int R, int C) {
    const int p = ksize / 2, rr = r + tr - p, cc = c + tc - p;
    return rr >= 0 && rr < R && cc >= 0 && cc < C;
}
// pixel-index offset of a valid tap relative to its row's own pixel
C2_HD inline int c2_tap_offset(int tr, int tc, int ksize, int C) { return (tr - ksize / 2) * C + (tc - ksize / 2); }

// The strided form (vv_conv2d_ex_fwd): GEMM rows run over the OUTPUT grid, Ro x Co = c2_out_extent of the input's R x C.  Stride 2 is
// ZeroPadding2D(((1, 0), (1, 0))) + a 'valid' k3 s2 convolution: output (ro, co) reads input (2 ro + tr - 1, 2 co + tc - 1), so only row
// and column -1 are padding and, for an odd size, the last input row / column is never read.  Stride 1 is the 'same' form above.
C2_HD inline int c2_out_extent(int n, int stride) { return stride == 2 ? n / 2 : n; }
C2_HD inline bool c2_ex_shape_ok(int ksize, int stride, int cin, int cout) {
    if (!c2_shape_ok(ksize, cin, cout)) return false;
    return stride == 1 || (stride == 2 && ksize == 3 && cin != 3);
}
// Tap (tr, tc) of the output at (ro, co): inside the R x C input or not.  As above the address of an outside tap is usually a valid one
// (row -1 of image b is the last row of image b - 1), so only this predicate may decide.
C2_HD inline bool c2_ex_tap_valid(int ro, int co, int tr, int tc, int ksize, int stride, int R, int C) {
    const int p = ksize / 2, rr = ro * stride + tr - p, cc = co * stride + tc - p;
    return rr >= 0 && rr < R && cc >= 0 && cc < C;
}
// pixel index, in the [B,R,C] input, of a valid tap of output (b, ro, co)
C2_HD inline long c2_ex_tap_pixel(int b, int ro, int co, int tr, int tc, int ksize, int stride, int R, int C) {
    return ((long)b * R + ro * stride) * C + co * stride + c2_tap_offset(tr, tc, ksize, C);
}
// MaxPool2D(2, 1, 'same') reads (r .. min(r + 1, R - 1), c .. min(c + 1, C - 1)): padding only at the end
C2_HD inline int c2_pool1_last(int i, int n) { return i + 1 < n ? i + 1 : n - 1; }
// every tensor of the strided form within 2^31 - 1 elements: the input with cin, the output grid with cout
C2_HD inline bool c2_ex_extent_ok(long batch, long rows, long cols, int stride, int cin, int cout);

// Split-K: how many shares K is cut into so that a small M still fills 256 CUs.  1 = the direct form (epilogue in the GEMM kernel).
// `forced` > 0 (test hook) overrides the choice, clamped to what the K extent admits.
inline int c2_splits(long M, int ksize, int cin, int cout, long forced) {
    const int kchunks = c2_kchunks(ksize, cin);
    if (cin == 3) return 1;
    long s;
    if (forced > 0) {
        s = forced;
    } else {
        const long tiles = ((M + C2_BM - 1) / C2_BM) * ((cout + C2_BN - 1) / C2_BN);
        if (tiles >= C2_FULL_WGS) return 1;
        s = (C2_TARGET_WGS + tiles - 1) / tiles;
        if (s > kchunks / C2_MIN_CHUNKS) s = kchunks / C2_MIN_CHUNKS;
    }
    if (s > C2_MAX_SPLITS) s = C2_MAX_SPLITS;
    if (s > kchunks) s = kchunks;
    return s < 1 ? 1 : (int)s;
}
// chunks [k0, k1) of share s: the first kchunks % splits shares take one more; every share is non-empty for splits <= kchunks
C2_HD inline void c2_split_range(int kchunks, int splits, int s, int *k0, int *k1) {
    const int base = kchunks / splits, rem = kchunks % splits;
    *k0 = s * base + (s < rem ? s : rem);
    *k1 = *k0 + base + (s < rem ? 1 : 0);
}
// what an entry may address: every tensor at most 2^31 - 1 elements
C2_HD inline bool c2_extent_ok(long batch, long rows, long cols, int cin, int cout) {
    if (batch < 1 || rows < 1 || cols < 1) return false;
    const long lim = 0x7FFFFFFFl;
    if (rows > lim / cols) return false;
    const long rc = rows * cols;
    if (batch > lim / rc) return false;
    const long M = batch * rc;
    const long widest = cin > cout ? cin : cout;
    return M <= lim / widest;
}
C2_HD inline bool c2_ex_extent_ok(long batch, long rows, long cols, int stride, int cin, int cout) {
    if (stride != 2) return c2_extent_ok(batch, rows, cols, cin, cout);
    return rows >= 2 && cols >= 2 && c2_extent_ok(batch, rows, cols, cin, cin) && c2_extent_ok(batch, rows / 2, cols / 2, cout, cout);
}
