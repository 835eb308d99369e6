// Device helpers shared by the bundle-adjustment kernels for CDNA4 (gfx950),
// fp64 throughout: ba_gram.hip, ba_schur.hip, ba_reduce.hip, ba_step.hip
// (and track.h, which restates linearize()'s projection without Jacobians).
// (ba_bcr.hip keeps its own rsqrt_nr / clampd / stamp and does not include this.)
//
// Reference: src/adjuster/BundleAdjuster.h — ReprojectCost :33-69 (pinhole,
// ceres::AngleAxisRotatePoint), HuberLoss(4) :109, ceres::Solve with
// SPARSE_SCHUR (point blocks eliminated) :125-126, 167-174; residual models
// SnavelyReprojectionError.h:16-54 and OpenMVG PINHOLE_CAMERA_RADIAL3
// (sparseBuilder.cpp:1292-1299) through the CM template parameter.
//
// One LM iteration on device (ba_gram.hip: campre, image_gram;
// ba_schur.hip: schur, zpoint; ba_reduce.hip: reduce; ba_step.hip: the rest):
//   campre      per-camera rotation terms (sin/cos once per camera, not per obs)
//   image_gram  per image (WGs): U = J_F' J_F over its observations (pose 6 |
//               intrinsics 4 or 6), b = J_F' f, cost 1/2 sum rho   [after an
//               accepted step only]
//   schur       chunk points, per chunk (one wave): observations -> corrected,
//               Jacobi-scaled Jacobians (VALU) -> per point V + D^2, Cholesky
//               L, w = L^-1 g -> Z = W L^-T into an LDS panel -> the chunk tile
//               -Z Z' (and -Z w) on the fp64 MFMA (v_mfma_f64_16x16x4_f64),
//               lower 16x16 tiles only
//   zpoint      general points, per point (one wave): the same elimination,
//               Z rows to a global buffer (product terms, preduce_*)
//   reduce      static gather plan: tiles + image blocks (+ products) -> RCS
//   solve       band + arrow: block cyclic reduction (ba_bcr.hip; solve_kernel
//               is the one-workgroup fallback); dense: blocked Cholesky
//   cand/step   candidate cameras; per point back-substitution y_E =
//               L^-T (w - Z' y_F), model cost change, candidate cost
//   finalize    fixed-order reduction of per-block partials (deterministic)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "ba_cand.h"
#include "ba_kernels.h"
#include "common.h"

// Inter-workgroup hand-offs in these files use the counter form of
// cdna_hip_programming.md Guideline 16: payloads stored and loaded with
// agent-scope relaxed atomics (sc1: written through / read past the CU's L1),
// drained with s_waitcnt vmcnt(0) (on gfx9 the vector memory counter also
// counts stores), then a relaxed agent-scope ticket or flag -- no release or
// acquire fence.  That is a property of the gfx950 ISA and its cache
// policy, not of the HIP memory model, so the device code refuses to build
// for any other target.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "counter-form hand-offs (sc1 payloads + vmcnt drain + relaxed ticket) are written for gfx950 only"
#endif

namespace sfm {
namespace {

typedef double v4d __attribute__((ext_vector_type(4)));

// doubles per intrinsics block of a residual model (RADIAL3: f, ppx, ppy, k1-k3)
template <int CM>
constexpr int kIW = CM == SFM_CAM_RADIAL3 ? 6 : 4;

// 1/d: hardware estimate + two Newton steps
__device__ __forceinline__ double rcp_nr(double d) {
    double y = __builtin_amdgcn_rcp(d);
#pragma unroll
    for (int it = 0; it < 2; ++it) y = fma(y, fma(-d, y, 1.0), y);
    return y;
}

// 1/sqrt(d): hardware estimate + two Newton steps (full fp64 accuracy)
__device__ __forceinline__ double rsqrt_nr(double d) {
    double y = __builtin_amdgcn_rsq(d);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double hy = 0.5 * d * y;
        y = fma(y, fma(-hy, y, 0.5), y);
    }
    return y;
}

__device__ __forceinline__ double clampd(double v, double lo, double hi) {
    return fmin(fmax(v, lo), hi);
}

// LM damping of a point-block diagonal entry: D^2 = clamp(diag) / radius.
// Ceres forms D = sqrt(clamp(diag) / radius) and adds D * D (the oracle does
// the same); the square of the rounded square root differs from its argument
// by about an ulp, and dropping the sqrt takes three dependent sqrt sequences
// off the point factorisation's critical path (Schur 0.347 -> 0.335 ms at
// C4).  Every point kernel (Schur, step, general points) uses this formula,
// so the elimination and the back substitution see the same V + D^2.  The
// camera columns keep Ceres's form (formed once per RCS, not per point).
__device__ __forceinline__ double point_d2(const DevProblem& P, double diag, double inv_radius) {
    return clampd(diag, P.min_diag, P.max_diag) * inv_radius;
}

// residual + loss-corrected Jacobian of one observation
// (BundleAdjuster.h:40-65 model; ceres Corrector with rho'' <= 0: r and J
// scaled by sqrt(rho'))
template <int IW>
struct LinW {
    double f[2];
    double Jc[2][6];
    double Ji[2][IW];
    double Jx[2][3];
    double half_rho;
    bool ok;
};
using Lin = LinW<4>;
template <int CM>
using LinT = LinW<kIW<CM>>;

template <int CM, bool JC, bool JI, bool JX>
__device__ __forceinline__ void linearize(const CamPre& cp, const double* in, const double* X, double u0,
                                          double u1, double huber_a, LinT<CM>& L) {
    double P[3];
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
    // one reciprocal for the projection and its Jacobian (x = P0/P2 to about
    // 1 ulp): v_rcp + two Newton steps, a shorter dependent chain than the
    // IEEE division sequence (C4 +0.6 % LM iterations/s)
    const double iz = rcp_nr(P[2]);
    double r0, r1;
    // unscaled dr/dP (2x3) and dr/d(intrinsics) (2 x kIW) of the model
    double A[2][3], Ji[2][kIW<CM>];
    if constexpr (CM == SFM_CAM_RADIAL3) {
        // OpenMVG ResidualErrorFunctor_Pinhole_Intrinsic_Radial_K3: (x, y) = P/P2,
        // c = 1 + k1 r2 + k2 r2^2 + k3 r2^3, r = pp + f c (x, y) - obs;
        // dr/dP = f [c I + D (x, y)(x, y)'] dp/dP with D = 2 (k1 + 2 k2 r2 + 3 k3 r2^2),
        // dp/dP = 1/P2 [1 0 -x; 0 1 -y]
        const double xu = P[0] * iz, yu = P[1] * iz;
        const double r2 = xu * xu + yu * yu, r4 = r2 * r2, r6 = r4 * r2;
        const double rc = 1.0 + in[3] * r2 + in[4] * r4 + in[5] * r6;
        r0 = in[1] + in[0] * (xu * rc) - u0;
        r1 = in[2] + in[0] * (yu * rc) - u1;
        if (JC || JI || JX) {
            const double dd = 2.0 * (in[3] + 2.0 * in[4] * r2 + 3.0 * in[5] * r4);
            const double b01 = in[0] * dd * xu * yu;
            const double B[2][2] = {{in[0] * (rc + dd * xu * xu), b01}, {b01, in[0] * (rc + dd * yu * yu)}};
            const double pu[2] = {xu, yu};
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                A[r][0] = iz * B[r][0];
                A[r][1] = iz * B[r][1];
                A[r][2] = -iz * (B[r][0] * xu + B[r][1] * yu);
                Ji[r][0] = pu[r] * rc;
                Ji[r][1] = r == 0 ? 1.0 : 0.0;
                Ji[r][2] = r == 1 ? 1.0 : 0.0;
                Ji[r][3] = in[0] * pu[r] * r2;
                Ji[r][4] = in[0] * pu[r] * r4;
                Ji[r][5] = in[0] * pu[r] * r6;
            }
        }
    } else if constexpr (CM == SFM_CAM_SNAVELY) {
        // SnavelyReprojectionError.h:31-47: p = -P/P2, d = 1 + r2 (l1 + l2 r2),
        // r = f d p - obs; dr/dP = f [d I + 2 (l1 + 2 l2 r2) p p'] dp/dP with
        // dp/dP = -1/P2 [1 0 xp; 0 1 yp]
        const double xp = -P[0] * iz, yp = -P[1] * iz;
        const double r2 = xp * xp + yp * yp;
        const double d = 1.0 + r2 * (in[1] + in[2] * r2);
        r0 = in[0] * d * xp - u0;
        r1 = in[0] * d * yp - u1;
        if (JC || JI || JX) {
            const double dd2 = 2.0 * (in[1] + 2.0 * in[2] * r2);
            const double b01 = in[0] * dd2 * xp * yp;
            const double B[2][2] = {{in[0] * (d + dd2 * xp * xp), b01}, {b01, in[0] * (d + dd2 * yp * yp)}};
            const double pp[2] = {xp, yp};
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                A[r][0] = -iz * B[r][0];
                A[r][1] = -iz * B[r][1];
                A[r][2] = -iz * (B[r][0] * xp + B[r][1] * yp);
                Ji[r][0] = d * pp[r];
                Ji[r][1] = in[0] * r2 * pp[r];
                Ji[r][2] = in[0] * r2 * r2 * pp[r];
                Ji[r][3] = 0.0;
            }
        }
    } else {
        const double x = P[0] * iz, y = P[1] * iz;
        r0 = in[0] * x + in[2] - u0;
        r1 = in[1] * y + in[3] - u1;
        A[0][0] = in[0] * iz; A[0][1] = 0.0; A[0][2] = -in[0] * x * iz;
        A[1][0] = 0.0; A[1][1] = in[1] * iz; A[1][2] = -in[1] * y * iz;
        Ji[0][0] = x; Ji[0][1] = 0.0; Ji[0][2] = 1.0; Ji[0][3] = 0.0;
        Ji[1][0] = 0.0; Ji[1][1] = y; Ji[1][2] = 0.0; Ji[1][3] = 1.0;
    }
    L.ok = isfinite(r0) && isfinite(r1);
    const double sq = r0 * r0 + r1 * r1;
    double rho0, sr = 1.0;   // Huber: rho' = 1 (inlier) needs no square root
    if (huber_a > 0.0 && sq > huber_a * huber_a) {
        const double rr = sqrt(sq);
        rho0 = 2.0 * huber_a * rr - huber_a * huber_a;
        sr = sqrt(fmax(DBL_MIN, huber_a / rr));
    } else {
        rho0 = sq;
    }
    L.half_rho = 0.5 * rho0;
    L.f[0] = r0 * sr; L.f[1] = r1 * sr;
    if (JC || JI || JX) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) A[r][k] *= sr;
        if (JI) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int k = 0; k < kIW<CM>; ++k) L.Ji[r][k] = Ji[r][k] * sr;
        }
        // dP/dX = R; dP/dw = -Al [X]x Ar with Al = R (Rodrigues) or I (small
        // angle), so the left factor A Al is J_X itself or A.
        double Jx[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < 3; ++j)
                Jx[r][j] = A[r][0] * cp.R[j] + A[r][1] * cp.R[3 + j] + A[r][2] * cp.R[6 + j];
        if (JX) {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 3; ++j) L.Jx[r][j] = Jx[r][j];
        }
        if (JC) {
            double N[9];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                N[0 + j] = -X[2] * cp.Ar[3 + j] + X[1] * cp.Ar[6 + j];
                N[3 + j] = X[2] * cp.Ar[0 + j] - X[0] * cp.Ar[6 + j];
                N[6 + j] = -X[1] * cp.Ar[0 + j] + X[0] * cp.Ar[3 + j];
            }
            const bool small = cp.small != 0.0;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                double B[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) B[k] = small ? A[r][k] : Jx[r][k];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    L.Jc[r][j] = -(B[0] * N[j] + B[1] * N[3 + j] + B[2] * N[6 + j]);
                    L.Jc[r][3 + j] = A[r][j];
                }
            }
        }
    }
}

// Global-address-space agent-scope accesses for values handed between
// workgroups of one launch (sc1: written through / read past this CU's L1;
// cdna_hip_programming.md Guideline 16, counter form)
typedef __attribute__((address_space(1))) unsigned gu32_t;
typedef __attribute__((address_space(1))) double gf64_t;
__device__ __forceinline__ void st_wt64(double* p, double v) {
    __hip_atomic_store((gf64_t*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_wt64(const double* p) {
    return __hip_atomic_load((gf64_t*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// block reduction helpers (256 threads, fixed order => deterministic)
template <int N>
__device__ __forceinline__ void wave_sum(double (&v)[N]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += __shfl_xor(v[k], o);
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ unsigned long long stamp() {
    unsigned long long t;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}

// wave-local LDS exchange: every lane's writes visible to the wave
// (LDS-only fences: the exchange is through LDS, so the fences need not
// order, or wait for, the wave's global accesses -- e.g. a prefetch in flight)
__device__ __forceinline__ void wsync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// staged camera t is optimised (has F columns); constant images are not
__device__ __forceinline__ bool crow_valid(const ChunkDesc& cd, int t) { return cd.cam_col[t] >= 0; }

// The 3x3 point block of the elimination (schur_kernel, zbatch_kernel,
// zpoint_kernel): V = V00 V10 V11 V20 V21 V22, damped with point_d2 as in the
// back substitution (step_kernel, step_general_kernel: sqrt and divisions, on
// purpose a different form).
// L^-1 (lower) of the damped block V + D^2 = L L', from reciprocal square
// roots; V is damped in place
struct PointInv { double i00, i10, i11, i20, i21, i22; };
__device__ __forceinline__ PointInv point_factor(const DevProblem& P, double (&V)[6], double inv_radius) {
    const int di[3] = {0, 2, 5};
#pragma unroll
    for (int a = 0; a < 3; ++a) V[di[a]] += point_d2(P, V[di[a]], inv_radius);
    const double i00 = rsqrt_nr(V[0]);
    const double l10 = V[1] * i00, l20 = V[3] * i00;
    const double i11 = rsqrt_nr(V[2] - l10 * l10);
    const double l21 = (V[4] - l20 * l10) * i11;
    const double i22 = rsqrt_nr(V[5] - l20 * l20 - l21 * l21);
    const double i10 = -l10 * i00 * i11, i21 = -l21 * i11 * i22;
    const double i20 = -(l20 * i00 + l21 * i10) * i22;
    return PointInv{i00, i10, i11, i20, i21, i22};
}

// gradient / norm bookkeeping of a point at x, added to xn2 = |x|^2 and
// gmx = max |g| (b = g_E in scaled columns)
__device__ __forceinline__ void point_norms(const double (&b)[3], const double (&sE)[3], const double (&Xp)[3],
                                            double& xn2, double& gmx) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double g = b[a] * rcp_nr(sE[a]);
        xn2 += Xp[a] * Xp[a];
        gmx = fmax(gmx, fabs(Xp[a] - (Xp[a] - g)));
    }
}

}  // namespace

// the residual model is a template parameter of every kernel that linearises
// (chunk tiles carry the model's intrinsics width: 4, RADIAL3 6)
#define SFM_BY_MODEL_ALL(P, CALL)                              \
    do {                                                       \
        if ((P).cam_model == SFM_CAM_RADIAL3) {                \
            constexpr int CM = SFM_CAM_RADIAL3;                \
            CALL;                                              \
        } else if ((P).cam_model == SFM_CAM_SNAVELY) {         \
            constexpr int CM = SFM_CAM_SNAVELY;                \
            CALL;                                              \
        } else {                                               \
            constexpr int CM = SFM_CAM_PINHOLE;                \
            CALL;                                              \
        }                                                      \
    } while (0)

// a run-time flag as a compile-time tag (as ba_step's lanes-per-point tag)
template <class F>
void by_flag(bool v, F&& fn) {
    if (v) fn(std::true_type{});
    else fn(std::false_type{});
}

}  // namespace sfm
