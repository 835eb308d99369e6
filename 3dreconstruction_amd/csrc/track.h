// What the post-BA wash (ba_wash.hip) and the track triangulation (tri.hip,
// tri.cpp) have in common, one definition each: the kernel input and its
// upload from a caller-order problem, the reject codes, the projection
// without Jacobians, the depth / residual verdict of an observation, and the
// point pass (survivors, the widest angle between two surviving rays, the
// point's verdict, the observations' keep flags).
//
// The first half is host-visible and builds with a plain host compiler (the
// stand-alone host triangulator, tests/cpp/triangulate_test.cpp); the device
// half needs hipcc.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ba_types.h"
#if defined(__HIPCC__)
#include "ba_device.h"
#endif

namespace sfm {

// reject code of an observation at a point; the wash gives the first three
enum : uint8_t { kObsKeep = 0, kObsDepth = 1, kObsResidual = 2, kObsBad = 3, kObsNoPoint = 4 };

// lanes per point of the short form of the per-point passes (a point of up to
// this many observations shares its wave with 64 / kTrackGroup - 1 others);
// longer points take a whole wave each, in rounds of 64 observations
constexpr int kTrackGroup = 16;

// What the kernels read: observations grouped by point in "kernel order" (the
// caller's, or a plan's shard order) and the parameters.  The triangulation
// leaves X and the maps null.
struct TrackInput {
    int32_t n_pt = 0, n_obs = 0, cam_model = 0, iw = 4;
    const int32_t* pt_off = nullptr;    // [n_pt + 1]
    const int32_t* obs_img = nullptr;   // [n_obs]
    const double* obs_uv = nullptr;     // [2 * n_obs]
    const int32_t* img_intr = nullptr;  // [n_img]
    const CamPre* cp = nullptr;         // [n_img]
    const double* intr = nullptr;       // [iw * n_intr]
    const double* X = nullptr;          // [3 * n_pt], kernel order
    // kernel order -> caller order (null: the identity)
    const int32_t* pt_map = nullptr;    // [n_pt]
    const int32_t* obs_map = nullptr;   // [n_obs]
};

// the rule of an observation: residual above max_residual_px (> 0), depth
struct ObsRule {
    double max_residual_px;
    int32_t cheirality;
};
// the rule of a point: survivors below min_track, widest angle below min_angle_deg (> 0)
struct PointRule {
    double min_angle_deg;
    int32_t min_track;
};

namespace {

#if !defined(__HIPCC__)   // a plain host compiler
using std::fabs;
using std::sqrt;
#endif

// finite: neither NaN nor an infinity (one definition for host and device)
__host__ __device__ inline bool track_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// 1 / depth: the one operation host and device do differently (the solver's
// rcp_nr on the device, a division on the host), so the two agree to
// rounding, not bit for bit.  A file that defines SFM_DEPTH_RCP_DIVIDES before
// including this one divides on the device too (resect.hip: the errors of a
// minimal sample's own correspondences are rounding noise, and their order
// feeds the next samples, so there the two paths must round alike).
__host__ __device__ inline double depth_rcp(double z) {
#if defined(__HIP_DEVICE_COMPILE__) && !defined(SFM_DEPTH_RCP_DIVIDES)
    return rcp_nr(z);
#else
    return 1.0 / z;
#endif
}

// P = R X + t and the unweighted residual (r0, r1) of camera model CM: the
// projection of linearize() (ba_device.h) without the loss and the Jacobians,
// formula for formula, so this is the residual the solver squares.
// linearize() is the one other copy in csrc/: its projection is fused with
// the Jacobians it feeds, and that kernel code is measured and pinned bit for
// bit, so it does not call this.
// The part from P on: the model's pixel at the camera-frame point P, minus the
// observation.  One definition for project_residual below and the camera
// resection's error and refit (resect_pose.h), which has P from a rotation
// matrix and no CamPre.
template <int CM>
__host__ __device__ inline void pixel_residual(const double* in, const double (&P)[3], double u0, double u1,
                                               double& r0, double& r1) {
    const double iz = depth_rcp(P[2]);
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

template <int CM>
__host__ __device__ inline void project_residual(const CamPre& cp, const double* in, const double* X, double u0,
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
    pixel_residual<CM>(in, P, u0, u1, r0, r1);
}

// The reject code of an observation from what project_residual gave: depth
// first (not finite, or behind the camera under the cheirality rule), then
// the residual rule.
template <int CM>
__host__ __device__ inline uint8_t obs_verdict(const ObsRule& R, const double (&P)[3], double r0, double r1) {
    const bool front = CM == SFM_CAM_SNAVELY ? P[2] < 0.0 : P[2] > 0.0;
    if (!(track_finite(r0) && track_finite(r1)) || (R.cheirality != 0 && !front)) return kObsDepth;
    if (R.max_residual_px > 0.0 && sqrt(r0 * r0 + r1 * r1) > R.max_residual_px) return kObsResidual;
    return kObsKeep;
}

// Both for an observation (u0, u1) of the point X, as the triangulation asks:
// its reject code and residual.  The rule is obs_verdict's, restated here and
// not called: which product of the Snavely model's r2 = xp xp + yp yp the
// compiler contracts into the fma depends on what surrounds the inlined
// projection.  With the verdict in a function of its own the triangulation's
// kernels fuse the other one, with it nested like this the wash's observation
// pass does (one ulp of r2, some 1e-14 px in one residual of a thousand), and
// both are pinned to their bits.
template <int CM>
__host__ __device__ inline uint8_t judge_obs(const CamPre& cp, const double* in, const double* X, double u0,
                                             double u1, const ObsRule& R, double& r0, double& r1) {
    double P[3];
    project_residual<CM>(cp, in, X, u0, u1, P, r0, r1);
    const bool front = CM == SFM_CAM_SNAVELY ? P[2] < 0.0 : P[2] > 0.0;
    if (!(track_finite(r0) && track_finite(r1)) || (R.cheirality != 0 && !front)) return kObsDepth;
    if (R.max_residual_px > 0.0 && sqrt(r0 * r0 + r1 * r1) > R.max_residual_px) return kObsResidual;
    return kObsKeep;
}

}  // namespace
}  // namespace sfm

#if defined(__HIPCC__)
namespace sfm {

// A caller-order problem at (extr, intr, X; X may be null) on the device: the
// uploads on stream s and the TrackInput over them.  in.cp is allocated, not
// filled: the caller launches ba_campre(extr.p, n_img, cp.p, s), inside
// whatever it times.
struct TrackUpload {
    HostVec<int32_t> off_h;   // (lives until the upload is done)
    DBuf<int32_t> off, img, img_intr;
    DBuf<double> uv, extr, intr, X;
    DBuf<CamPre> cp;
    TrackInput in;
    TrackUpload(const sfm_ba_problem& P, const double* h_extr, const double* h_intr, const double* h_X,
                hipStream_t s) {
        const int iw = sfm_ba_intr_width(P.camera_model);
        const size_t np = (size_t)P.n_pt, no = (size_t)P.n_obs, ni = (size_t)P.n_img;
        off_h.resize(np + 1);
        for (size_t p = 0; p <= np; ++p) off_h[p] = (int32_t)P.pt_offsets[p];
        off.alloc(np + 1); off.upload(off_h.data(), np + 1, s);
        img.alloc(no); img.upload(P.obs_img, no, s);
        uv.alloc(2 * no); uv.upload(P.obs_uv, 2 * no, s);
        img_intr.alloc(ni); img_intr.upload(P.img_intr, ni, s);
        extr.alloc(6 * ni); extr.upload(h_extr, 6 * ni, s);
        intr.alloc((size_t)iw * P.n_intr); intr.upload(h_intr, (size_t)iw * P.n_intr, s);
        if (h_X) {
            X.alloc(3 * np); X.upload(h_X, 3 * np, s);
        }
        cp.alloc(ni);
        in.n_pt = (int32_t)np; in.n_obs = (int32_t)no;
        in.cam_model = P.camera_model; in.iw = iw;
        in.pt_off = off.p; in.obs_img = img.p; in.obs_uv = uv.p; in.img_intr = img_intr.p;
        in.cp = cp.p; in.intr = intr.p; in.X = X.p;
    }
};

namespace {

// 0 kept, 1 short, 2 angle: the first rule that applies
__device__ __forceinline__ int point_rule(const PointRule& R, int survivors, double deg) {
    if (survivors < R.min_track) return 1;
    if (R.min_angle_deg > 0.0 && deg < R.min_angle_deg) return 2;
    return 0;
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

// the per-point passes' launch shape: four waves, 64 / kTrackGroup points each
constexpr int kPtThreads = 256;
constexpr int kPtPerWave = 64 / kTrackGroup;
inline unsigned point_grid(int64_t n_pt) {
    const int per_block = (kPtThreads / 64) * kPtPerWave;
    return (unsigned)((n_pt + per_block - 1) / per_block);
}

// The point pass over the observations' reject codes and rays (both in kernel
// order): the survivors (code kObsKeep) of each point, the widest angle
// between two of their rays and the point's verdict; an observation is kept
// when it survives and its point's verdict is 0.  A point of <= kTrackGroup
// observations takes a lane group, a longer one a whole wave, all pairs in
// rounds of 64; the widest pair is chosen by comparing (|a x b|, a.b) tuples,
// one atan2 per point.  The Policy supplies what differs between callers:
//   kCounts                    its counters, and slot(t): where counter t goes in counts[]
//   verdict(k, survivors, deg) of point k (0: kept)
//   point(in, k, v, deg, c)    one lane per point: its outputs and counters
//   obs(in, s, keep, c)        one lane per observation: its output and counter
// The counters are integer sums per workgroup (LDS) added with integer
// atomics: the same numbers every run.
template <class Policy>
__global__ __launch_bounds__(kPtThreads) void track_point_kernel(TrackInput in, Policy pol,
                                                                 const uint8_t* __restrict__ code,
                                                                 const double* __restrict__ ray,
                                                                 unsigned long long* __restrict__ counts) {
    constexpr int NC = Policy::kCounts;
    __shared__ unsigned cnt[NC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < NC) cnt[tid] = 0;
    __syncthreads();
    const int64_t kw = ((int64_t)blockIdx.x * (kPtThreads / 64) + wave) * kPtPerWave;   // the wave's first point
    unsigned c[NC] = {};
    {
        const int grp = lane / kTrackGroup, g = lane % kTrackGroup;
        const int64_t k = kw + grp;
        const bool has = k < in.n_pt;
        const int32_t o0 = has ? in.pt_off[k] : 0;
        const int32_t n = has ? in.pt_off[k + 1] - o0 : 0;
        if (!__any(n > kTrackGroup)) {
            // ---- a lane group per point ----
            const bool mine = g < n;
            const int64_t s = (int64_t)o0 + g;
            const bool ok = mine && code[s] == kObsKeep;
            double a[3] = {0.0, 0.0, 0.0};
            if (ok) {
#pragma unroll
                for (int j = 0; j < 3; ++j) a[j] = ray[3 * s + j];
            }
            Widest best{0.0, 1.0};
            pair_rounds<kTrackGroup>(g, a, ok, a, ok, 1, kTrackGroup / 2, best);
            group_widest<kTrackGroup>(best);
            const unsigned long long m = __ballot(ok);
            const int survivors = __popcll((m >> (grp * kTrackGroup)) & ((1ull << kTrackGroup) - 1));
            const double deg = widest_deg(best);
            const int v = has ? pol.verdict(k, survivors, deg) : 1;
            if (has && g == 0) pol.point(in, k, v, deg, c);
            if (mine) pol.obs(in, s, v == 0 && ok, c);
        } else {
            // ---- a wave per point, pairs in rounds of 64 ----
            for (int q = 0; q < kPtPerWave; ++q) {
                const int64_t kq = kw + q;
                if (kq >= in.n_pt) break;   // (wave-uniform)
                const int32_t q0 = in.pt_off[kq];
                const int32_t nq = in.pt_off[kq + 1] - q0;
                const int nt = (nq + 63) / 64;
                Widest best{0.0, 1.0};
                int survivors = 0;
                for (int ti = 0; ti < nt; ++ti) {
                    const int i = ti * 64 + lane;
                    const bool a_ok = i < nq && code[(int64_t)q0 + i] == kObsKeep;
                    double a[3] = {0.0, 0.0, 0.0};
                    if (a_ok) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) a[j] = ray[3 * ((int64_t)q0 + i) + j];
                    }
                    survivors += __popcll(__ballot(a_ok));
                    pair_rounds<64>(lane, a, a_ok, a, a_ok, 1, 32, best);
                    for (int tj = ti + 1; tj < nt; ++tj) {
                        const int jn = tj * 64 + lane;
                        const bool b_ok = jn < nq && code[(int64_t)q0 + jn] == kObsKeep;
                        double b[3] = {0.0, 0.0, 0.0};
                        if (b_ok) {
#pragma unroll
                            for (int j = 0; j < 3; ++j) b[j] = ray[3 * ((int64_t)q0 + jn) + j];
                        }
                        pair_rounds<64>(lane, a, a_ok, b, b_ok, 0, 63, best);
                    }
                }
                group_widest<64>(best);
                const double deg = widest_deg(best);
                const int v = pol.verdict(kq, survivors, deg);
                if (lane == 0) pol.point(in, kq, v, deg, c);
                for (int i = lane; i < nq; i += 64) {
                    const int64_t s = (int64_t)q0 + i;
                    pol.obs(in, s, v == 0 && code[s] == kObsKeep, c);
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < NC; ++t) {
        unsigned v = c[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0 && v) atomicAdd(&cnt[t], v);
    }
    __syncthreads();
    if (tid < NC && cnt[tid]) atomicAdd(&counts[Policy::slot(tid)], (unsigned long long)cnt[tid]);
}

template <class Policy>
void track_point_pass(const TrackInput& in, const Policy& pol, const uint8_t* code, const double* ray,
                      unsigned long long* counts, hipStream_t s) {
    hipLaunchKernelGGL(track_point_kernel<Policy>, dim3(point_grid(in.n_pt)), dim3(kPtThreads), 0, s, in, pol, code,
                       ray, counts);
    SFM_HIP(hipGetLastError());
}

}  // namespace
}  // namespace sfm
#endif
