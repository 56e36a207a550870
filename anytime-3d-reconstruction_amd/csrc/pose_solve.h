// A detection's pose in the world: the arithmetic of the reference's getObjectInRealWorld / getTranslation (src/visualizer/visualizer.py
// :237-308, :79-146) for ONE detection, as plain C++ that compiles for the host and for the device alike (object_pose.hip runs it in a
// kernel and, through vv_object_pose_host, in a loop on the CPU).  float64 throughout: the four constraint rows mix entries of ~1e3 with
// entries of ~1e-3 and the null vector is read off the SMALLEST singular value.  No inline assembly, no atomics, no memory besides the
// arguments.
//
// Floating-point contraction is switched OFF in every function below, so that the host build (no FMA on a plain x86-64 target) and the
// device build (v_fma_f64) round every product and sum alike: the acceptance tests, the argmax and the int() truncation then decide the
// same way on both sides.
//
// The solver: ONE-SIDED (Hestenes) Jacobi on the columns of the 4x4 constraint matrix A itself -- pairs of columns are rotated until
// they are orthogonal, V collects the rotations, the column of A V with the smallest norm names the right singular vector of the
// smallest singular value.  It never forms A^T A, so the condition number is not squared.  VV_POSE_SWEEPS cyclic sweeps of the six
// pairs; a pair whose cosine is already below 2^-50 is left alone, which is what makes a converged matrix a fixed point (a further
// sweep changes no bit; tests/test_pose_host.py checks that on the fixture set through the `sweeps` argument).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#define VV_POSE_HD __host__ __device__ inline

constexpr int VV_POSE_SWEEPS = 6;      // the fixture set is bit-converged after 4 (3 leave 7e-9 m); two in reserve
constexpr int VV_POSE_CANDIDATES = 128;

// proj / proj_inv row-major 4x4; the image size in pixels.  Travels by value as a kernel argument.
struct VvPoseCamera {
    double P[16], Pinv[16], col, row;
};

struct VvPoseFit {
    int ok;          // 0: rejected
    double iou, t[3];
};

// One detection's result.  candidate: the winning k, -1 when every candidate was rejected (X = 0), -2 when the detection never reached
// the fit (the "too close" pre-filter, or a NaN among its inputs).
struct VvPoseObject {
    int keep, candidate;
    double iou, X[3];
    float pose[16], size[3], proj[16];
    int box2d[4];
};

// Corner tables of :85-88 in units of (dx, dy, dz): entry list * 2 + element holds three bits, bit a set = +d_a.
constexpr unsigned VV_POSE_XMIN = 0u | (4u << 3) | (2u << 6) | (6u << 9);   // (-,-,-) (-,-,+) | (-,+,-) (-,+,+)
constexpr unsigned VV_POSE_XMAX = 3u | (7u << 3) | (5u << 6) | (1u << 9);   // (+,+,-) (+,+,+) | (+,-,+) (+,-,-)
constexpr unsigned VV_POSE_YMIN = 4u | (5u << 3) | (6u << 6) | (7u << 9);   // (-,-,+) (+,-,+) | (-,+,+) (+,+,+)
constexpr unsigned VV_POSE_YMAX = 2u | (3u << 3) | (0u << 6) | (1u << 9);   // (-,+,-) (+,+,-) | (-,-,-) (+,-,-)

// Rows 0 .. 2 of proj [I | R d; 0 0 0 1] for the corner `idx` of a table (matmul3x1, then the last column of matmul4x4: the first
// three columns are those of proj).
VV_POSE_HD void vv_pose_corner_rows(unsigned table, int idx, const double *P, const double *R, double dx, double dy, double dz, double B[3][4]) {
#pragma clang fp contract(off)
    const unsigned c = (table >> (3 * idx)) & 7u;
    const double d0 = (c & 1u) ? dx : -dx, d1 = (c & 2u) ? dy : -dy, d2 = (c & 4u) ? dz : -dz;
    const double v0 = R[0] * d0 + R[1] * d1 + R[2] * d2;
    const double v1 = R[3] * d0 + R[4] * d1 + R[5] * d2;
    const double v2 = R[6] * d0 + R[7] * d1 + R[8] * d2;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        B[r][0] = P[r * 4], B[r][1] = P[r * 4 + 1], B[r][2] = P[r * 4 + 2];
        B[r][3] = P[r * 4] * v0 + P[r * 4 + 1] * v1 + P[r * 4 + 2] * v2 + P[r * 4 + 3];
    }
}

// One rotation of columns p < q of A (and of V): after it the two columns of A are orthogonal.
template <int p, int q>
VV_POSE_HD void vv_pose_rotate(double A[4][4], double V[4][4]) {
#pragma clang fp contract(off)
    double alpha = 0.0, beta = 0.0, gamma = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        alpha += A[r][p] * A[r][p];
        beta += A[r][q] * A[r][q];
        gamma += A[r][p] * A[r][q];
    }
    const double tol2 = 0x1p-100;                                      // (2^-50)^2
    if (!(gamma * gamma > tol2 * (alpha * beta))) return;               // orthogonal to working precision (or a zero / NaN column)
    const double zeta = (beta - alpha) / (2.0 * gamma);
    const double t = (zeta < 0.0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double ap = A[r][p], aq = A[r][q];
        A[r][p] = c * ap - s * aq;
        A[r][q] = s * ap + c * aq;
        const double vp = V[r][p], vq = V[r][q];
        V[r][p] = c * vp - s * vq;
        V[r][q] = s * vp + c * vq;
    }
}

// The right singular vector of the smallest singular value of A (destroyed), up to its sign.
VV_POSE_HD void vv_pose_null_vector(double A[4][4], int sweeps, double t[4]) {
#pragma clang fp contract(off)
    double V[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
    for (int s = 0; s < sweeps; ++s) {
        vv_pose_rotate<0, 1>(A, V);
        vv_pose_rotate<0, 2>(A, V);
        vv_pose_rotate<0, 3>(A, V);
        vv_pose_rotate<1, 2>(A, V);
        vv_pose_rotate<1, 3>(A, V);
        vv_pose_rotate<2, 3>(A, V);
    }
    double best = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const double n = A[0][c] * A[0][c] + A[1][c] * A[1][c] + A[2][c] * A[2][c] + A[3][c] * A[3][c];
        if (c == 0 || n < best) {
            best = n;
#pragma unroll
            for (int r = 0; r < 4; ++r) t[r] = V[r][c];
        }
    }
}

VV_POSE_HD double vv_pose_dot4(const double *b, const double *t) {
#pragma clang fp contract(off)
    return b[0] * t[0] + b[1] * t[1] + b[2] * t[2] + b[3] * t[3];
}

// Candidate k of the reference's loop nest in execution order (:89-119): k = ((((pairx * 2 + pairy) * 2 + a) * 2 + b) * 2 + c) * 2 + d
// with pairx 0 .. 3 the x-side pairing, pairy 0 .. 1 the y-side pairing, a / b / c / d the element of the xmin / ymin / xmax / ymax set.
// box2d = (x_min, y_min, x_max, y_max) in pixels, (w, h, l) as getTranslation names them (dx = w / 2, dy = l / 2, dz = h / 2).
VV_POSE_HD VvPoseFit vv_pose_candidate(int k, const double *P, const double *R, const double *box2d, double w, double h, double l,
                                       int sweeps = VV_POSE_SWEEPS) {
#pragma clang fp contract(off)
    VvPoseFit f;
    f.ok = 0, f.iou = -1.0, f.t[0] = f.t[1] = f.t[2] = 0.0;
    const double x_min = box2d[0], y_min = box2d[1], x_max = box2d[2], y_max = box2d[3];
    const double dx = w / 2.0, dy = l / 2.0, dz = h / 2.0;
    const int pairx = (k >> 5) & 3, pairy = (k >> 4) & 1, a = (k >> 3) & 1, b = (k >> 2) & 1, c = (k >> 1) & 1, d = k & 1;
    const int lx = pairx & 1;
    const unsigned xmin_table = pairx < 2 ? VV_POSE_XMIN : VV_POSE_XMAX, xmax_table = pairx < 2 ? VV_POSE_XMAX : VV_POSE_XMIN;
    double B0[3][4], B1[3][4], B2[3][4], B3[3][4];
    vv_pose_corner_rows(xmin_table, lx * 2 + a, P, R, dx, dy, dz, B0);
    vv_pose_corner_rows(VV_POSE_YMIN, pairy * 2 + b, P, R, dx, dy, dz, B1);
    vv_pose_corner_rows(xmax_table, lx * 2 + c, P, R, dx, dy, dz, B2);
    vv_pose_corner_rows(VV_POSE_YMAX, pairy * 2 + d, P, R, dx, dy, dz, B3);
    double A[4][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        A[0][e] = B0[0][e] - x_min * B0[2][e];
        A[1][e] = B1[1][e] - y_min * B1[2][e];
        A[2][e] = B2[0][e] - x_max * B2[2][e];
        A[3][e] = B3[1][e] - y_max * B3[2][e];
    }
    double t[4];
    vv_pose_null_vector(A, sweeps, t);
    if (!(t[3] * t[2] > 0.0)) return f;
    const double t3 = t[3];
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = t[e] / t3;
    const double x_min_pred = vv_pose_dot4(B0[0], t) / vv_pose_dot4(B0[2], t);
    const double y_min_pred = vv_pose_dot4(B1[1], t) / vv_pose_dot4(B1[2], t);
    const double x_max_pred = vv_pose_dot4(B2[0], t) / vv_pose_dot4(B2[2], t);
    const double y_max_pred = vv_pose_dot4(B3[1], t) / vv_pose_dot4(B3[2], t);
    if (!(x_min_pred < x_max_pred && y_min_pred < y_max_pred)) return f;
    const double pred_area = (x_max_pred - x_min_pred) * (y_max_pred - y_min_pred);
    const double gt_area = (x_max - x_min) * (y_max - y_min);
    const double x_min_inter = x_min_pred > x_min ? x_min_pred : x_min, x_max_inter = x_max_pred < x_max ? x_max_pred : x_max;
    const double y_min_inter = y_min_pred > y_min ? y_min_pred : y_min, y_max_inter = y_max_pred < y_max ? y_max_pred : y_max;
    const double inter_area = (x_max_inter - x_min_inter) * (y_max_inter - y_min_inter);      // unclamped, as written at :140
    const double iou = inter_area / (pred_area + gt_area - inter_area);
    if (!(iou < 1.0)) return f;
    f.ok = 1, f.iou = iou, f.t[0] = t[0], f.t[1] = t[1], f.t[2] = t[2];
    return f;
}

// (iou, k) of one candidate against the running best, which starts as (-1, -1): the reference keeps the first candidate of the largest
// IoU (`iou_max < iou` is strict and starts at -1), so an IoU of -1 or less never wins and an equal IoU goes to the lower k.
VV_POSE_HD bool vv_pose_better(double iou, int k, double best_iou, int best_k) {
    return iou > best_iou || (iou == best_iou && best_k >= 0 && k >= 0 && k < best_k);
}

// getRay (:148-155; its print is dropped): the unit ray through pixel (px, py).
VV_POSE_HD void vv_pose_ray(const double *Q, double px, double py, double ray[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r) ray[r] = Q[r * 4] * px + Q[r * 4 + 1] * py + Q[r * 4 + 2] * 1.0 + Q[r * 4 + 3] * 1.0;
    const double nrm = sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) ray[r] = ray[r] / nrm;
}

// getRayRotation (:157-168): the ray as a rotation about x, then about y.
VV_POSE_HD void vv_pose_ray_rotation(const double ray[3], double Rr[9]) {
#pragma clang fp contract(off)
    const double nrm = sqrt(ray[0] * ray[0] + ray[1] * ray[1] + ray[2] * ray[2]);
    const double rx = ray[0] / nrm, ry = ray[1] / nrm, rz = ray[2] / nrm;
    const double cy = sqrt(ry * ry + rz * rz), cx = rz / sqrt(ry * ry + rz * rz), sx = -ry / sqrt(ry * ry + rz * rz), sy = rx;
    Rr[0] = cy, Rr[1] = 0.0, Rr[2] = sy;
    Rr[3] = sx * sy, Rr[4] = cx, Rr[5] = -sx * cy;
    Rr[6] = -cx * sy, Rr[7] = sx, Rr[8] = cx * cy;
}

// get3DbboxProjection (:191-205) with ITS (w, h, l): half extents (w / 2, l / 2, h / 2) along the object's axes, [2][2][2][2] in
// (i, j, k, xy) order, index 0 of i / j / k = +, index 1 = -.
VV_POSE_HD void vv_pose_box_projection(const double *P, const double *R, const double *X, double w, double h, double l, double out[16]) {
#pragma clang fp contract(off)
    const double hx = w / 2.0, hy = l / 2.0, hz = h / 2.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const double d0 = (c & 4) ? -hx : hx, d1 = (c & 2) ? -hy : hy, d2 = (c & 1) ? -hz : hz;
        const double x0 = (R[0] * d0 + R[1] * d1 + R[2] * d2) + X[0], x1 = (R[3] * d0 + R[4] * d1 + R[5] * d2) + X[1],
                     x2 = (R[6] * d0 + R[7] * d1 + R[8] * d2) + X[2];
        const double u = P[0] * x0 + P[1] * x1 + P[2] * x2 + P[3] * 1.0, v = P[4] * x0 + P[5] * x1 + P[6] * x2 + P[7] * 1.0,
                     z = P[8] * x0 + P[9] * x1 + P[10] * x2 + P[11] * 1.0;
        out[c * 2] = u / z, out[c * 2 + 1] = v / z;
    }
}

// getTranslation (:79-146) as a plain loop over the candidates -> the winning k (-1: none, X = 0).
VV_POSE_HD int vv_pose_fit(const double *P, const double *R, const double *box, double w, double h, double l, int sweeps, double *iou,
                           double X[3]) {
    int best = -1;
    *iou = -1.0, X[0] = X[1] = X[2] = 0.0;
    for (int k = 0; k < VV_POSE_CANDIDATES; ++k) {
        const VvPoseFit f = vv_pose_candidate(k, P, R, box, w, h, l, sweeps);
        if (f.ok && vv_pose_better(f.iou, k, *iou, best)) best = k, *iou = f.iou, X[0] = f.t[0], X[1] = f.t[1], X[2] = f.t[2];
    }
    return best;
}

// What precedes the fit (:247-280).  -> false when the detection never reaches it.  box[4] = the pixel box, R[9] the rotation with the
// ray correction applied.
VV_POSE_HD bool vv_pose_prepare(const float *b2, const float *b3, const float *sn, const float *cs, const VvPoseCamera &cam, double box[4],
                                double R[9]) {
#pragma clang fp contract(off)
    for (int e = 0; e < 5; ++e)
        if (b2[e] != b2[e]) return false;
    for (int e = 0; e < 3; ++e)
        if (b3[e] != b3[e] || sn[e] != sn[e] || cs[e] != cs[e]) return false;
    double b2x1 = b2[0], b2y1 = b2[1], b2x2 = b2[2], b2y2 = b2[3];
    if (!(b2x1 > 1e-1 && b2x2 < 1.0 - 1e-1 && b2y2 < 1.0 - 1e-1)) return false;           // avoid too close obj
    b2x1 = b2x1 * cam.col, b2y1 = b2y1 * cam.row, b2x2 = b2x2 * cam.col, b2y2 = b2y2 * cam.row;
    box[0] = b2x1, box[1] = b2y1, box[2] = b2x2, box[3] = b2y2;
    const double sinA = sn[0], sinI = sn[2], cosA = cs[0], cosI = cs[2];
    // the -5 degree elevation correction: cos / sin of beta = -5 / 180 * pi, as numpy gives them
    const double cb = 0.9961946980917455, sb = -0.08715574274765817;
    const double sinE = (double)sn[1] * cb - (double)cs[1] * sb, cosE = (double)cs[1] * cb + (double)sn[1] * sb;
    // RA * RE * RI
    const double r11 = -sinA * sinE * sinI + cosA * cosI, r12 = -sinA * cosE, r13 = sinA * sinE * cosI + sinI * cosA;
    const double r21 = sinA * cosI + sinE * sinI * cosA, r22 = cosA * cosE, r23 = sinA * sinI - sinE * cosA * cosI;
    const double r31 = -sinI * cosE, r32 = sinE, r33 = cosE * cosI;
    // pascal -> kitti: a quarter turn about x
    const double Ro[9] = {r11, r12, r13, -r31, -r32, -r33, r21, r22, r23};
    // the ray through the box centre and its rotation
    double ray[3], Rr[9];
    vv_pose_ray(cam.Pinv, (b2x2 + b2x1) / 2.0, (b2y2 + b2y1) / 2.0, ray);
    vv_pose_ray_rotation(ray, Rr);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = Rr[i * 3] * Ro[j] + Rr[i * 3 + 1] * Ro[3 + j] + Rr[i * 3 + 2] * Ro[6 + j];
    return true;
}

VV_POSE_HD int vv_pose_int(double v) {          // Python's int(): toward zero; saturated, so that the cast is defined for every input
    return v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (-2147483647 - 1) : (int)v);
}

// What follows the fit (:286-300): the 4x4 pose, the eight projected corners, the post-filter, the truncated pixel box, the size row.
VV_POSE_HD void vv_pose_finish(const float *b3, const VvPoseCamera &cam, const double box[4], const double R[9], VvPoseObject &o) {
#pragma clang fp contract(off)
    const double *X = o.X, *P = cam.P;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o.pose[r * 4] = (float)R[r * 3], o.pose[r * 4 + 1] = (float)R[r * 3 + 1], o.pose[r * 4 + 2] = (float)R[r * 3 + 2];
        o.pose[r * 4 + 3] = (float)X[r];
    }
    o.pose[12] = 0.f, o.pose[13] = 0.f, o.pose[14] = 0.f, o.pose[15] = 1.f;
    double uv[16];
    vv_pose_box_projection(P, R, X, (double)b3[1], (double)b3[0], (double)b3[2], uv);      // called with (b3h, b3w, b3l), as the reference does
#pragma unroll
    for (int e = 0; e < 16; ++e) o.proj[e] = (float)uv[e];
    o.keep = X[2] > 1e-1 ? 1 : 0;               // not the trivial solution, not too close to the image plane
#pragma unroll
    for (int e = 0; e < 4; ++e) o.box2d[e] = vv_pose_int(box[e]);
    o.size[0] = b3[1], o.size[1] = b3[2], o.size[2] = b3[0];       // [b3h, b3l, b3w]
}

// Everything for one detection, the candidates in a plain loop (the host entry; the kernel deals the candidates over a wave instead).
VV_POSE_HD void vv_pose_object(const float *b2, const float *b3, const float *sn, const float *cs, const VvPoseCamera &cam, int sweeps,
                               VvPoseObject &o) {
    o.keep = 0, o.candidate = -2, o.iou = -1.0, o.X[0] = o.X[1] = o.X[2] = 0.0;
    double box[4], R[9];
    if (!vv_pose_prepare(b2, b3, sn, cs, cam, box, R)) return;
    o.candidate = vv_pose_fit(cam.P, R, box, (double)b3[0], (double)b3[1], (double)b3[2], sweeps, &o.iou, o.X);
    vv_pose_finish(b3, cam, box, R, o);
}
