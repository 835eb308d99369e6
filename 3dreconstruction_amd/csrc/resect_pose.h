// Camera resection (include/sfmcore.h, "Camera resection"), the
// arithmetic written once for the device kernel (resect.hip) and the serial
// host twin (resect.cpp, sfm_resect_host): the real roots of a quartic, the
// P3P minimal solver, the error of a correspondence under a model, the
// a-contrario NFA term, and the refit's normal-equation terms, 6x6 solve and
// pose update.  A model is Rt[12]: R row-major, then t, with P = R X + t.
// Only + - * / and sqrt (frexp / ldexp inside acransac.h's cube root and
// log10): no libm transcendental call, so host and device differ by rounding
// only (track.h's depth_rcp, and the order of the refit's sums).  The
// including file sets `#pragma clang fp contract(off)` first.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "acransac.h"
#include "track.h"
#include "tri_point.h"

namespace sfm {
namespace {

constexpr int kP3PSample = 3;       // P3P: MINIMUM_SAMPLES
constexpr int kP3PMaxModels = 4;    // MAX_MODELS
constexpr int kQuarticNewton = 2;   // Newton steps on each quartic root
constexpr int kDistanceNewton = 2;  // Newton steps on each solution's three distances
constexpr int kExpTerms = 12;       // terms of the series of sin(t)/t and (1 - cos t)/t^2

__host__ __device__ inline double resect_inf() { return __builtin_inf(); }

// Real roots of x^4 + p3 x^3 + p2 x^2 + p1 x + p0 into r[0..3] (any order):
// Ferrari's factorisation into two quadratics through the largest real root
// of the resolvent cubic (acransac.h's solve_cubic), each root polished by
// kQuarticNewton Newton steps on the quartic itself.
__host__ __device__ inline int quartic_real_roots(double p3, double p2, double p1, double p0, double* r) {
    const double h = p3 / 4.0, h2 = h * h;   // x = y - h: y^4 + P y^2 + Q y + R
    const double P = p2 - 6.0 * h2;
    const double Q = p1 - 2.0 * p2 * h + 8.0 * h2 * h;
    const double R = p0 - p1 * h + p2 * h2 - 3.0 * h2 * h2;
    int n = 0;
    if (Q == 0.0) {   // biquadratic
        const double disc = P * P - 4.0 * R;
        if (!(disc >= 0.0)) return 0;
        const double sd = sqrt(disc);
        const double z0 = (-P + sd) / 2.0, z1 = (-P - sd) / 2.0;
        if (z0 >= 0.0) { const double y = sqrt(z0); r[n++] = y - h; r[n++] = -y - h; }
        if (z1 >= 0.0) { const double y = sqrt(z1); r[n++] = y - h; r[n++] = -y - h; }
    } else {
        // (y^2 + P/2 + m)^2 = 2m (y - Q / 4m)^2 at a root m > 0 of
        // m^3 + P m^2 + (P^2/4 - R) m - Q^2/8
        const double C[4] = {-(Q * Q) / 8.0, P * P / 4.0 - R, P, 1.0};
        double cr[3] = {0.0, 0.0, 0.0};
        const int nc = solve_cubic(C, cr);
        double m = cr[0];
        if (nc == 3) {
            m = cr[1] > m ? cr[1] : m;
            m = cr[2] > m ? cr[2] : m;
        }
        if (nc == 0 || !(m > 0.0)) return 0;
        const double s = sqrt(2.0 * m), g = Q / (2.0 * s), c = P / 2.0 + m;
        const double d0 = s * s - 4.0 * (c + g);   // y^2 - s y + (c + g)
        if (d0 >= 0.0) { const double sd = sqrt(d0); r[n++] = (s + sd) / 2.0 - h; r[n++] = (s - sd) / 2.0 - h; }
        const double d1 = s * s - 4.0 * (c - g);   // y^2 + s y + (c - g)
        if (d1 >= 0.0) { const double sd = sqrt(d1); r[n++] = (-s + sd) / 2.0 - h; r[n++] = (-s - sd) / 2.0 - h; }
    }
    for (int i = 0; i < n; ++i) {
        double x = r[i];
        for (int it = 0; it < kQuarticNewton; ++it) {
            const double f = (((x + p3) * x + p2) * x + p1) * x + p0;
            const double df = ((4.0 * x + 3.0 * p3) * x + 2.0 * p2) * x + p1;
            const double xn = x - f / df;
            if (track_finite(xn)) x = xn;
        }
        r[i] = x;
    }
    return n;
}

// P3P: the poses that map the three world points X[3i..] onto the unit
// bearings b[3i..].  Grunert's formulation: with the distances s2 = u s1,
// s3 = v s1, the difference of two of the three cosine laws is linear in u,
// u = N(v) / D(v), and the third becomes a quartic in v, built here by
// multiplying the small polynomials out; each real root gives (s1, s2, s3),
// polished by kDistanceNewton Newton steps on the three cosine laws; kept when
// all three are positive.  The pose then is the closed-form alignment of the
// two triangles' orthonormal frames, t from their centroids.  Returns the
// number of models written to Rt[12 * i]; roots[4] is workspace.  0 for a
// collinear or repeated sample (sin of the angle at X1 <= 1e-10) and for a
// vanishing leading coefficient.
__host__ __device__ inline int p3p_solve(const double* b, const double* X, double* Rt, double* roots) {
    double d12[3], d13[3], d23[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        d12[j] = X[3 + j] - X[j];
        d13[j] = X[6 + j] - X[j];
        d23[j] = X[6 + j] - X[3 + j];
    }
    const double C2 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
    const double B2 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
    const double A2 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
    const double nx[3] = {d12[1] * d13[2] - d12[2] * d13[1], d12[2] * d13[0] - d12[0] * d13[2],
                          d12[0] * d13[1] - d12[1] * d13[0]};
    const double nx2 = nx[0] * nx[0] + nx[1] * nx[1] + nx[2] * nx[2];
    if (!(nx2 > 1e-20 * (C2 * B2))) return 0;
    const double ca = b[3] * b[6] + b[4] * b[7] + b[5] * b[8];   // cos(b2, b3)
    const double cb = b[0] * b[6] + b[1] * b[7] + b[2] * b[8];   // cos(b1, b3)
    const double cg = b[0] * b[3] + b[1] * b[4] + b[2] * b[5];   // cos(b1, b2)
    const double k1 = (A2 - C2) / B2, k2 = C2 / B2;
    // Q(v) = 1 - 2 cb v + v^2, N = k1 Q - v^2 + 1, D = 2 (cg - ca v)
    const double q0 = 1.0, q1 = -2.0 * cb, q2 = 1.0;
    const double n0 = k1 + 1.0, n1 = -2.0 * cb * k1, n2 = k1 - 1.0;
    const double e0 = 2.0 * cg, e1 = -2.0 * ca;
    const double dd0 = e0 * e0, dd1 = 2.0 * e0 * e1, dd2 = e1 * e1;                       // D^2
    const double nn0 = n0 * n0, nn1 = 2.0 * n0 * n1, nn2 = n1 * n1 + 2.0 * n0 * n2, nn3 = 2.0 * n1 * n2,
                 nn4 = n2 * n2;                                                            // N^2
    const double nd0 = n0 * e0, nd1 = n0 * e1 + n1 * e0, nd2 = n1 * e1 + n2 * e0, nd3 = n2 * e1;   // N D
    const double qd0 = q0 * dd0, qd1 = q0 * dd1 + q1 * dd0, qd2 = q0 * dd2 + q1 * dd1 + q2 * dd0,
                 qd3 = q1 * dd2 + q2 * dd1, qd4 = q2 * dd2;                                // Q D^2
    // D^2 + N^2 - 2 cg N D - k2 Q D^2 = 0
    const double c0 = dd0 + nn0 - 2.0 * cg * nd0 - k2 * qd0;
    const double c1 = dd1 + nn1 - 2.0 * cg * nd1 - k2 * qd1;
    const double c2 = dd2 + nn2 - 2.0 * cg * nd2 - k2 * qd2;
    const double c3 = nn3 - 2.0 * cg * nd3 - k2 * qd3;
    const double c4 = nn4 - k2 * qd4;
    if (!(fabs(c4) > 0.0)) return 0;
    const int nr = quartic_real_roots(c3 / c4, c2 / c4, c1 / c4, c0 / c4, roots);
    // the world triangle's frame and centroid
    const double lc = sqrt(C2), ln = sqrt(nx2);
    const double w1[3] = {d12[0] / lc, d12[1] / lc, d12[2] / lc};
    const double w3[3] = {nx[0] / ln, nx[1] / ln, nx[2] / ln};
    const double w2[3] = {w3[1] * w1[2] - w3[2] * w1[1], w3[2] * w1[0] - w3[0] * w1[2], w3[0] * w1[1] - w3[1] * w1[0]};
    const double Xc[3] = {(X[0] + X[3] + X[6]) / 3.0, (X[1] + X[4] + X[7]) / 3.0, (X[2] + X[5] + X[8]) / 3.0};
    int nm = 0;
    for (int i = 0; i < nr; ++i) {
        const double v = roots[i];
        const double Qv = (v - 2.0 * cb) * v + 1.0;
        const double u = ((n2 * v + n1) * v + n0) / (e1 * v + e0);
        double s1 = sqrt(B2 / Qv), s2 = u * s1, s3 = v * s1;
        for (int it = 0; it < kDistanceNewton; ++it) {
            const double f1 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - A2;
            const double f2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - B2;
            const double f3 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - C2;
            // J = [0 a12 a13; a21 0 a23; a31 a32 0]
            const double a12 = 2.0 * (s2 - s3 * ca), a13 = 2.0 * (s3 - s2 * ca);
            const double a21 = 2.0 * (s1 - s3 * cb), a23 = 2.0 * (s3 - s1 * cb);
            const double a31 = 2.0 * (s1 - s2 * cg), a32 = 2.0 * (s2 - s1 * cg);
            const double det = a12 * a23 * a31 + a13 * a21 * a32;
            const double x1 = (a12 * a23 * f3 + a13 * a32 * f2 - f1 * a23 * a32) / det;   // Cramer
            const double x2 = (f1 * a23 * a31 + a13 * (a21 * f3 - f2 * a31)) / det;
            const double x3 = (f1 * a21 * a32 - a12 * (a21 * f3 - f2 * a31)) / det;
            const double t1 = s1 - x1, t2 = s2 - x2, t3 = s3 - x3;
            if (track_finite(t1) && track_finite(t2) && track_finite(t3)) { s1 = t1; s2 = t2; s3 = t3; }
        }
        if (!(s1 > 0.0 && s2 > 0.0 && s3 > 0.0)) continue;
        if (!(track_finite(s1) && track_finite(s2) && track_finite(s3))) continue;
        const double P1[3] = {s1 * b[0], s1 * b[1], s1 * b[2]}, P2[3] = {s2 * b[3], s2 * b[4], s2 * b[5]},
                     P3[3] = {s3 * b[6], s3 * b[7], s3 * b[8]};
        const double g12[3] = {P2[0] - P1[0], P2[1] - P1[1], P2[2] - P1[2]};
        const double g13[3] = {P3[0] - P1[0], P3[1] - P1[1], P3[2] - P1[2]};
        const double gn[3] = {g12[1] * g13[2] - g12[2] * g13[1], g12[2] * g13[0] - g12[0] * g13[2],
                              g12[0] * g13[1] - g12[1] * g13[0]};
        const double l1 = sqrt(g12[0] * g12[0] + g12[1] * g12[1] + g12[2] * g12[2]);
        const double l3 = sqrt(gn[0] * gn[0] + gn[1] * gn[1] + gn[2] * gn[2]);
        if (!(l1 > 0.0 && l3 > 0.0)) continue;
        const double f1[3] = {g12[0] / l1, g12[1] / l1, g12[2] / l1};
        const double f3[3] = {gn[0] / l3, gn[1] / l3, gn[2] / l3};
        const double f2[3] = {f3[1] * f1[2] - f3[2] * f1[1], f3[2] * f1[0] - f3[0] * f1[2],
                              f3[0] * f1[1] - f3[1] * f1[0]};
        double* M = Rt + 12 * nm;
        bool fin = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                M[3 * r + c] = f1[r] * w1[c] + f2[r] * w2[c] + f3[r] * w3[c];
                fin = fin && track_finite(M[3 * r + c]);
            }
        }
        const double Pc[3] = {(P1[0] + P2[0] + P3[0]) / 3.0, (P1[1] + P2[1] + P3[1]) / 3.0,
                              (P1[2] + P2[2] + P3[2]) / 3.0};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            M[9 + r] = Pc[r] - (M[3 * r] * Xc[0] + M[3 * r + 1] * Xc[1] + M[3 * r + 2] * Xc[2]);
            fin = fin && track_finite(M[9 + r]);
        }
        if (fin) ++nm;
    }
    return nm;
}

// P = R X + t, and R X
__host__ __device__ inline void resect_transform(const double* Rt, const double* X, double (&RX)[3], double (&P)[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        RX[r] = Rt[3 * r] * X[0] + Rt[3 * r + 1] * X[1] + Rt[3 * r + 2] * X[2];
        P[r] = RX[r] + Rt[9 + r];
    }
}

template <int CM>
__host__ __device__ inline bool resect_front(const double (&P)[3]) {
    return CM == SFM_CAM_SNAVELY ? P[2] < 0.0 : P[2] > 0.0;
}

// The error of a correspondence under a model: the squared pixel norm of the
// camera model's residual (track.h's pixel_residual) at P = R X + t; +inf when
// it is not finite or the point is not in front of the camera.
template <int CM>
__host__ __device__ inline double resect_error(const double* Rt, const double* in, const double* X, double u0,
                                               double u1) {
    double RX[3], P[3], r0, r1;
    resect_transform(Rt, X, RX, P);
    pixel_residual<CM>(in, P, u0, u1, r0, r1);
    const double e = r0 * r0 + r1 * r1;
    if (!resect_front<CM>(P) || !track_finite(r0) || !track_finite(r1) || !track_finite(e)) return resect_inf();
    return e;
}

// NFA of the k smallest errors, the k-th being e (point-to-point: mult_error 1)
__host__ __device__ inline double resect_nfa(double loge0, double logalpha0, double e, int64_t k, float logc_n,
                                             float logc_k) {
    const double logalpha = logalpha0 + det_log10(e + 1.1920928955078125e-07);
    return loge0 + logalpha * (double)(k - kP3PSample) + (double)logc_n + (double)logc_k;
}

// One correspondence's terms of the refit's normal equations at the model Rt,
// for the update R <- exp[d]x R, t += d_t: S[0..20] += the upper triangle of
// J'J (row-major), S[21..26] -= J'r, J the analytic 2 x 6 Jacobian of the
// camera model's residual.  False (nothing added) when the point is not in
// front of the camera or the residual is not finite.
template <int CM>
__host__ __device__ inline bool resect_normal_terms(const double* Rt, const double* in, const double* X, double u0,
                                                    double u1, double (&S)[27]) {
    double RX[3], P[3], r0, r1;
    resect_transform(Rt, X, RX, P);
    if (!resect_front<CM>(P)) return false;
    pixel_residual<CM>(in, P, u0, u1, r0, r1);
    if (!track_finite(r0) || !track_finite(r1)) return false;
    const double iz = depth_rcp(P[2]);
    // pixel = (f0 g x + .., f1 g y + ..) of (x, y) = sg (P0, P1) / P2, g = g(x^2 + y^2)
    double sg = 1.0, g = 1.0, gp = 0.0, f0 = in[0], f1 = in[0];
    if constexpr (CM == SFM_CAM_SNAVELY) sg = -1.0;
    if constexpr (CM == SFM_CAM_PINHOLE) f1 = in[1];
    const double x = sg * P[0] * iz, y = sg * P[1] * iz;
    const double r2 = x * x + y * y;
    if constexpr (CM == SFM_CAM_RADIAL3) {
        g = 1.0 + in[3] * r2 + in[4] * (r2 * r2) + in[5] * (r2 * r2 * r2);
        gp = in[3] + 2.0 * in[4] * r2 + 3.0 * in[5] * (r2 * r2);
    } else if constexpr (CM == SFM_CAM_SNAVELY) {
        g = 1.0 + r2 * (in[1] + in[2] * r2);
        gp = in[1] + 2.0 * in[2] * r2;
    }
    const double a = g + 2.0 * x * x * gp, bb = 2.0 * x * y * gp, c = g + 2.0 * y * y * gp;
    // d(pixel)/dP, with dx/dP = (sg iz, 0, -x iz), dy/dP = (0, sg iz, -y iz)
    const double JP[2][3] = {{f0 * a * sg * iz, f0 * bb * sg * iz, -f0 * (a * x + bb * y) * iz},
                             {f1 * bb * sg * iz, f1 * c * sg * iz, -f1 * (bb * x + c * y) * iz}};
    double J[2][6];
#pragma unroll
    for (int i = 0; i < 2; ++i) {   // dP/dd = -[R X]x, dP/dt = I
        J[i][0] = JP[i][2] * RX[1] - JP[i][1] * RX[2];
        J[i][1] = JP[i][0] * RX[2] - JP[i][2] * RX[0];
        J[i][2] = JP[i][1] * RX[0] - JP[i][0] * RX[1];
        J[i][3] = JP[i][0];
        J[i][4] = JP[i][1];
        J[i][5] = JP[i][2];
    }
    int e = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int q = p; q < 6; ++q) S[e++] += J[0][p] * J[0][q] + J[1][p] * J[1][q];
#pragma unroll
    for (int p = 0; p < 6; ++p) S[21 + p] -= J[0][p] * r0 + J[1][p] * r1;
    return true;
}

// d of H d = g from the sums S (H's upper triangle, then g): elimination with
// partial pivoting on [H | g] in the workspace H[42].  False: singular (a
// pivot that is zero or not finite) or a d that is not finite.
__host__ __device__ inline bool resect_solve6(const double* S, double* H, double* d) {
    int e = 0;
    for (int p = 0; p < 6; ++p)
        for (int q = p; q < 6; ++q) {
            H[7 * p + q] = S[e];
            H[7 * q + p] = S[e];
            ++e;
        }
    for (int p = 0; p < 6; ++p) H[7 * p + 6] = S[21 + p];
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(H[7 * r + c]) > fabs(H[7 * piv + c])) piv = r;
        const double pv = H[7 * piv + c];
        if (!(fabs(pv) > 0.0) || !track_finite(pv)) return false;
        if (piv != c)
            for (int k = 0; k < 7; ++k) {
                const double t = H[7 * c + k];
                H[7 * c + k] = H[7 * piv + k];
                H[7 * piv + k] = t;
            }
        for (int r = c + 1; r < 6; ++r) {
            const double f = H[7 * r + c] / H[7 * c + c];
            for (int k = c; k < 7; ++k) H[7 * r + k] = H[7 * r + k] - f * H[7 * c + k];
        }
    }
    for (int c = 5; c >= 0; --c) {
        double s = H[7 * c + 6];
        for (int k = c + 1; k < 6; ++k) s = s - H[7 * c + k] * d[k];
        d[c] = s / H[7 * c + c];
        if (!track_finite(d[c])) return false;
    }
    return true;
}

// R <- exp[d]x R, t += d_t.  exp[d]x = (1 - B t2) I + A [d]x + B d d', with
// A = sin(t)/t and B = (1 - cos t)/t^2 from kExpTerms terms of their series in
// t2 = |d|^2 (exact to rounding for the steps a refit takes).  False, Rt
// untouched: a rotation step above 1 rad.
__host__ __device__ inline bool resect_apply(double* Rt, const double* d) {
    const double t2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    if (!(t2 <= 1.0)) return false;
    double A = 1.0, B = 1.0;
    for (int k = kExpTerms; k >= 1; --k) {
        A = 1.0 - t2 / (double)((2 * k) * (2 * k + 1)) * A;
        B = 1.0 - t2 / (double)((2 * k + 1) * (2 * k + 2)) * B;
    }
    B = 0.5 * B;
    const double dg = 1.0 - B * t2;
    const double E[9] = {dg + B * d[0] * d[0],        B * d[0] * d[1] - A * d[2],  B * d[0] * d[2] + A * d[1],
                         B * d[1] * d[0] + A * d[2],  dg + B * d[1] * d[1],        B * d[1] * d[2] - A * d[0],
                         B * d[2] * d[0] - A * d[1],  B * d[2] * d[1] + A * d[0],  dg + B * d[2] * d[2]};
    double Rn[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rn[3 * r + c] = E[3 * r] * Rt[c] + E[3 * r + 1] * Rt[3 + c] + E[3 * r + 2] * Rt[6 + c];
    for (int a = 0; a < 9; ++a) Rt[a] = Rn[a];
    for (int a = 0; a < 3; ++a) Rt[9 + a] = Rt[9 + a] + d[3 + a];
    return true;
}

}  // namespace
}  // namespace sfm
