// Device pieces of the post-BA wash (ba_wash.hip) that the track
// triangulation (tri.hip) uses as well, one definition for both: the
// unweighted residual of an observation and the widest angle between the
// rays of a lane group.
#pragma once
#include "ba_device.h"

namespace sfm {
namespace {

// P = R X + t and the unweighted residual (r0, r1): linearize()'s projection
// (ba_device.h) without the loss and the Jacobians, formula for formula, so
// this is the residual the solver squares.
template <int CM>
__device__ __forceinline__ void wash_project(const CamPre& cp, const double* in, const double* X, double u0,
                                             double u1, double (&P)[3], double& r0, double& r1) {
    const double* u = cp.u;
    const double cr0 = u[1] * X[2] - u[2] * X[1], cr1 = u[2] * X[0] - u[0] * X[2],
                 cr2 = u[0] * X[1] - u[1] * X[0];
    if (cp.small != 0.0) {
        P[0] = X[0] + cr0; P[1] = X[1] + cr1; P[2] = X[2] + cr2;
    } else {
        const double tmp = (u[0] * X[0] + u[1] * X[1] + u[2] * X[2]) * cp.omc;
        P[0] = X[0] * cp.c + cr0 * cp.s + u[0] * tmp;
        P[1] = X[1] * cp.c + cr1 * cp.s + u[1] * tmp;
        P[2] = X[2] * cp.c + cr2 * cp.s + u[2] * tmp;
    }
    P[0] += cp.t[0]; P[1] += cp.t[1]; P[2] += cp.t[2];
    const double iz = rcp_nr(P[2]);
    if constexpr (CM == SFM_CAM_RADIAL3) {
        const double xu = P[0] * iz, yu = P[1] * iz;
        const double r2 = xu * xu + yu * yu, r4 = r2 * r2, r6 = r4 * r2;
        const double rc = 1.0 + in[3] * r2 + in[4] * r4 + in[5] * r6;
        r0 = in[1] + in[0] * (xu * rc) - u0;
        r1 = in[2] + in[0] * (yu * rc) - u1;
    } else if constexpr (CM == SFM_CAM_SNAVELY) {
        const double xp = -P[0] * iz, yp = -P[1] * iz;
        const double r2 = xp * xp + yp * yp;
        const double d = 1.0 + r2 * (in[1] + in[2] * r2);
        r0 = in[0] * d * xp - u0;
        r1 = in[0] * d * yp - u1;
    } else {
        const double x = P[0] * iz, y = P[1] * iz;
        r0 = in[0] * x + in[2] - u0;
        r1 = in[1] * y + in[3] - u1;
    }
}

// The widest pair so far as (|a x b|, a.b): the angle is atan2(s, c).
struct Widest {
    double s, c;
};
// angle(s1, c1) > angle(s2, c2), both in [0, pi]: the sign of sin(t1 - t2);
// opposite against parallel rays (both sines 0) by the cosine
__device__ __forceinline__ bool wider(double s1, double c1, double s2, double c2) {
    const double det = s1 * c2 - c1 * s2;
    return det > 0.0 || (det == 0.0 && c1 < c2);
}

// This lane's ray a against the ray b of lanes (g + r) % W of its W-lane group,
// r = r_begin .. r_end.  Every lane of the wave calls it (shuffles).
template <int W>
__device__ __forceinline__ void pair_rounds(int g, const double (&a)[3], bool a_ok, const double (&b)[3], bool b_ok,
                                            int r_begin, int r_end, Widest& best) {
#pragma unroll 2
    for (int r = r_begin; r <= r_end; ++r) {
        const int src = (g + r) & (W - 1);
        const double b0 = __shfl(b[0], src, W), b1 = __shfl(b[1], src, W), b2 = __shfl(b[2], src, W);
        const int ok = __shfl((int)b_ok, src, W);
        if (a_ok && ok) {
            double c0, c1, c2;
            {
                // no contraction: the cross product of a ray with itself (two
                // observations in one image) is exactly zero
#pragma clang fp contract(off)
                c0 = a[1] * b2 - a[2] * b1;
                c1 = a[2] * b0 - a[0] * b2;
                c2 = a[0] * b1 - a[1] * b0;
            }
            const double sn = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
            const double cs = a[0] * b0 + a[1] * b1 + a[2] * b2;
            if (wider(sn, cs, best.s, best.c)) best = Widest{sn, cs};
        }
    }
}

// the widest pair of a W-lane group, in every lane of it
template <int W>
__device__ __forceinline__ void group_widest(Widest& best) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) {
        const double os = __shfl_xor(best.s, o, W), oc = __shfl_xor(best.c, o, W);
        if (wider(os, oc, best.s, best.c)) best = Widest{os, oc};
    }
}

__device__ __forceinline__ double widest_deg(const Widest& w) {
    return atan2(w.s, w.c) * (180.0 / 3.14159265358979323846);
}

}  // namespace
}  // namespace sfm
