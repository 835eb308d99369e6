// N-view track triangulation for CDNA4 (gfx950), fp64: OpenMVG's
// ComputeStructureFromKnownPoses step (TriangulateNViewAlgebraic, and a
// deterministic stand-in for its robust track triangulation), restated;
// semantics in include/sfmcore.h, the per-track algorithm in tri_point.h.
//
//   obs pass    one lane per observation: the unit bearing b of the pixel (20
//               undistortion iterations for the radial models), the 10 unique
//               entries of C'C, C = (I - b b')[R|t], the world ray R' b and the
//               bad flag.  Streaming: reads image 4 B + pixel 16 B, writes
//               80 B + 24 B + 1 B per observation.
//   solve pass  a point of <= kTrackGroup observations takes a lane group (64 /
//               kTrackGroup points per wave), a longer one a whole wave, and
//               runs tri_solve_track (tri_point.h) over its lanes: LINEAR one
//               4x4 Jacobi of the summed Grams; ROBUST a lane per two-view
//               hypothesis, the best score by a total order through shuffles,
//               then the N-view refit over its inliers.  Last, a lane per
//               observation: residual and reject code at the final X.
//   point pass  track_point_kernel (track.h) with the TriPoint policy below,
//               over those codes and the measured rays: survivors, the widest
//               angle between two of them, the status; X = NaN and keep_obs =
//               0 for a point that is not OK.
//
// The staged Grams and rays live in a global scratch at every track length
// (a point's 104 B per observation are read back by its own lane group right
// after the obs pass wrote them: L2 hits at the sizes of interest), so one
// code path serves any length the problem format allows.  All sums run in a
// fixed order and the counters are integer atomics: two runs give the same
// bits.
#include "tri.h"
#include "tri_point.h"

namespace sfm {
namespace {

constexpr int kObsThreads = 256;

template <int CM>
__global__ __launch_bounds__(kObsThreads) void tri_obs_kernel(TrackInput in, double* __restrict__ gram,
                                                              double* __restrict__ ray, uint8_t* __restrict__ badf,
                                                              unsigned long long* __restrict__ counts) {
    const int64_t s = (int64_t)blockIdx.x * kObsThreads + threadIdx.x;
    bool bad = false;
    if (s < in.n_obs) {
        const int32_t img = in.obs_img[s];
        const CamPre& cp = in.cp[img];
        const double* ib = in.intr + (int64_t)in.iw * in.img_intr[img];
        const double2 uv = reinterpret_cast<const double2*>(in.obs_uv)[s];
        double b[3], G[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, d[3] = {0, 0, 0};
        bad = !tri_bearing<CM>(ib, uv.x, uv.y, b);
        if (!bad) {
            tri_gram(cp, b, G);
            tri_world_ray(cp, b, d);
        }
#pragma unroll
        for (int e = 0; e < 10; ++e) gram[10 * s + e] = G[e];
#pragma unroll
        for (int j = 0; j < 3; ++j) ray[3 * s + j] = d[j];
        badf[s] = bad;
    }
    const unsigned long long mb = __ballot(bad);
    if ((threadIdx.x & 63) == 0 && mb) atomicAdd(&counts[kTcObsBad], (unsigned long long)__popcll(mb));
}

template <int W, class T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, W);
    return v;
}

// tri_solve_track's lanes: the W lanes of a wave that share a point
template <int W_>
struct GroupLanes {
    static constexpr int W = W_;
    int g;   // the lane within the group
    template <class T>
    __device__ T sum(T v) const { return group_sum<W>(v); }
    __device__ void best(TriScore& best, double (&bX)[3]) const {
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1) {
            TriScore ot{__shfl_xor(best.cnt, o, W), __shfl_xor(best.ssq, o, W), __shfl_xor(best.h, o, W)};
            const double x0 = __shfl_xor(bX[0], o, W), x1 = __shfl_xor(bX[1], o, W), x2 = __shfl_xor(bX[2], o, W);
            if (tri_better(ot, best)) {
                best = ot;
                bX[0] = x0; bX[1] = x1; bX[2] = x2;
            }
        }
    }
};

struct SolveOpts {
    ObsRule rule;
    int32_t max_hyp;
};

// One point (first observation o0, n of them) by the W lanes of a group: every
// lane of the wave calls it; a group without a point has n = 0.
template <int CM, bool ROBUST, int W>
__device__ __forceinline__ void solve_point(const TrackInput& in, const SolveOpts& O, bool has, int64_t k, int32_t o0,
                                            int32_t n, int g, const double* __restrict__ gram,
                                            const uint8_t* __restrict__ badf, uint8_t* __restrict__ code, double* __restrict__ Xs,
                                            uint8_t* __restrict__ solved, double2* __restrict__ residual,
                                            unsigned (&c)[2]) {
    auto good = [&](int32_t i) { return badf[(int64_t)o0 + i] == 0; };
    auto add_gram = [&](double (&G)[10], int32_t i) {
        const double* gp = gram + 10 * ((int64_t)o0 + i);
#pragma unroll
        for (int e = 0; e < 10; ++e) G[e] += gp[e];
    };
    auto judge = [&](int32_t i, const double (&X)[3], double& r0, double& r1) {
        const int64_t s = (int64_t)o0 + i;
        const int32_t img = in.obs_img[s];
        const double2 uv = reinterpret_cast<const double2*>(in.obs_uv)[s];
        return judge_obs<CM>(in.cp[img], in.intr + (int64_t)in.iw * in.img_intr[img], X, uv.x, uv.y, O.rule, r0, r1);
    };
    auto img_of = [&](int32_t i) { return good(i) ? in.obs_img[(int64_t)o0 + i] : -1; };
    auto out = [&](int32_t i, uint8_t cd, double r0, double r1) {
        c[0] += cd == kObsDepth;
        c[1] += cd == kObsResidual;
        residual[(int64_t)o0 + i] = make_double2(r0, r1);
        code[(int64_t)o0 + i] = cd;
    };
    double X[3];
    const uint8_t fin = tri_solve_track<ROBUST>(GroupLanes<W>{g}, n, O.max_hyp, good, add_gram, judge, img_of, out, X);
    if (has && g == 0) {
        const double nan = __builtin_nan("");
#pragma unroll
        for (int j = 0; j < 3; ++j) Xs[3 * k + j] = fin == kTriSolved ? X[j] : nan;
        solved[k] = fin;
    }
}

template <int CM, bool ROBUST>
__global__ __launch_bounds__(kPtThreads) void tri_solve_kernel(TrackInput in, SolveOpts O,
                                                               const double* __restrict__ gram,
                                                               const uint8_t* __restrict__ badf,
                                                               uint8_t* __restrict__ code, double* __restrict__ Xs, uint8_t* __restrict__ solved,
                                                               double2* __restrict__ residual,
                                                               unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t kw = ((int64_t)blockIdx.x * (kPtThreads / 64) + wave) * kPtPerWave;   // the wave's first point
    unsigned c[2] = {0, 0};
    const int grp = lane / kTrackGroup, g = lane % kTrackGroup;
    const int64_t k = kw + grp;
    const bool has = k < in.n_pt;
    const int32_t o0 = has ? in.pt_off[k] : 0;
    const int32_t n = has ? in.pt_off[k + 1] - o0 : 0;
    if (!__any(n > kTrackGroup)) {
        solve_point<CM, ROBUST, kTrackGroup>(in, O, has, k, o0, n, g, gram, badf, code, Xs, solved, residual, c);
    } else {
        for (int q = 0; q < kPtPerWave; ++q) {
            const int64_t kq = kw + q;
            if (kq >= in.n_pt) break;   // (wave-uniform)
            const int32_t q0 = in.pt_off[kq];
            solve_point<CM, ROBUST, 64>(in, O, true, kq, q0, in.pt_off[kq + 1] - q0, lane, gram, badf, code, Xs,
                                        solved, residual, c);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const unsigned v = group_sum<64>(c[t]);
        if (lane == 0 && v) atomicAdd(&counts[t == 0 ? kTcObsDepth : kTcObsResidual], (unsigned long long)v);
    }
}

// The triangulation's side of the point pass (track.h), over the codes of the
// solve pass and the measured rays: the verdict is an SFM_TRI_* status, what
// the solve left first, then the point rule; status and keep_obs go out in
// the caller's order, and X = NaN for a point that is not OK.
static_assert(SFM_TRI_OK == 0 && SFM_TRI_SHORT == 1 && SFM_TRI_ANGLE == 2, "point_rule's verdicts are the statuses");
struct TriPoint {
    static constexpr int kCounts = 5;   // ok, short, angle, infinite, observations kept
    __device__ static int slot(int t) {
        const int s[kCounts] = {kTcPtOk, kTcPtShort, kTcPtAngle, kTcPtInfinite, kTcObsKept};
        return s[t];
    }
    PointRule rule;
    const uint8_t* __restrict__ solved;
    double* __restrict__ X;
    uint8_t* __restrict__ status;
    uint8_t* __restrict__ keep_obs;
    __device__ int verdict(int64_t k, int survivors, double deg) const {
        const uint8_t fin = solved[k];
        if (fin == kTriNoSolve) return SFM_TRI_SHORT;
        if (fin == kTriInfinite) return SFM_TRI_INFINITE;
        return point_rule(rule, survivors, deg);
    }
    __device__ void point(const TrackInput&, int64_t k, int v, double, unsigned (&c)[kCounts]) const {
        status[k] = (uint8_t)v;
        if (v != SFM_TRI_OK) {
            const double nan = __builtin_nan("");
#pragma unroll
            for (int j = 0; j < 3; ++j) X[3 * k + j] = nan;
        }
        c[0] += v == SFM_TRI_OK; c[1] += v == SFM_TRI_SHORT; c[2] += v == SFM_TRI_ANGLE; c[3] += v == SFM_TRI_INFINITE;
    }
    __device__ void obs(const TrackInput&, int64_t s, bool keep, unsigned (&c)[kCounts]) const {
        keep_obs[s] = keep;
        c[4] += keep;
    }
};

}  // namespace

void TriBuffers::alloc(int64_t n_pt_, int64_t n_obs_) {
    n_pt = n_pt_;
    n_obs = n_obs_;
    X.alloc(3 * (size_t)n_pt);
    status.alloc((size_t)n_pt);
    keep_obs.alloc((size_t)n_obs);
    residual.alloc(2 * (size_t)n_obs);
    gram.alloc(10 * (size_t)n_obs);
    ray.alloc(3 * (size_t)n_obs);
    bad.alloc((size_t)n_obs);
    code.alloc((size_t)n_obs);
    solved.alloc((size_t)n_pt);
    counts.alloc(kTcCount);
}

void tri_eval(const TrackInput& in, const sfm_tri_opts& o, TriBuffers& b, hipStream_t s) {
    SFM_REQUIRE(b.n_pt == in.n_pt && b.n_obs == in.n_obs, SFM_ERR_INVALID_ARG, "internal: triangulation buffers of another size");
    b.counts.zero(s);
    if (in.n_obs > 0) {
        const unsigned grid = (unsigned)(((int64_t)in.n_obs + kObsThreads - 1) / kObsThreads);
        SFM_BY_MODEL_ALL(in, hipLaunchKernelGGL(tri_obs_kernel<CM>, dim3(grid), dim3(kObsThreads), 0, s, in, b.gram.p,
                                                b.ray.p, b.bad.p, b.counts.p));
        SFM_HIP(hipGetLastError());
    }
    if (in.n_pt > 0) {
        const unsigned grid = point_grid(in.n_pt);
        const SolveOpts O{ObsRule{o.max_residual_px, o.cheirality}, o.max_hypotheses};
        by_flag(o.method == SFM_TRI_ROBUST, [&](auto robust) {
            SFM_BY_MODEL_ALL(in, hipLaunchKernelGGL((tri_solve_kernel<CM, decltype(robust)::value>), dim3(grid),
                                                    dim3(kPtThreads), 0, s, in, O, b.gram.p, b.bad.p, b.code.p, b.X.p,
                                                    b.solved.p, reinterpret_cast<double2*>(b.residual.p),
                                                    b.counts.p));
        });
        SFM_HIP(hipGetLastError());
        track_point_pass(in, TriPoint{PointRule{o.min_angle_deg, o.min_track_len}, b.solved.p, b.X.p, b.status.p,
                                      b.keep_obs.p},
                         b.code.p, b.ray.p, b.counts.p, s);
    }
}

void tri_download(TriBuffers& b, double* X, uint8_t* status, uint8_t* keep_obs, double* residual, sfm_tri_stats* stats,
                  hipStream_t s) {
    const size_t no = (size_t)b.n_obs, np = (size_t)b.n_pt;
    if (X && np) SFM_HIP(hipMemcpyAsync(X, b.X.p, 3 * np * sizeof(double), hipMemcpyDeviceToHost, s));
    if (status && np) SFM_HIP(hipMemcpyAsync(status, b.status.p, np, hipMemcpyDeviceToHost, s));
    if (keep_obs && no) SFM_HIP(hipMemcpyAsync(keep_obs, b.keep_obs.p, no, hipMemcpyDeviceToHost, s));
    if (residual && no) SFM_HIP(hipMemcpyAsync(residual, b.residual.p, 2 * no * sizeof(double), hipMemcpyDeviceToHost, s));
    unsigned long long c[kTcCount] = {0};
    if (stats) SFM_HIP(hipMemcpyAsync(c, b.counts.p, sizeof c, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    if (stats) {
        stats->n_pt_ok = (int64_t)c[kTcPtOk];
        stats->n_pt_short = (int64_t)c[kTcPtShort];
        stats->n_pt_angle = (int64_t)c[kTcPtAngle];
        stats->n_pt_infinite = (int64_t)c[kTcPtInfinite];
        stats->n_obs_kept = (int64_t)c[kTcObsKept];
        stats->n_obs_bad = (int64_t)c[kTcObsBad];
        stats->n_obs_depth = (int64_t)c[kTcObsDepth];
        stats->n_obs_residual = (int64_t)c[kTcObsResidual];
    }
}

}  // namespace sfm
