// N-view track triangulation for CDNA4 (gfx950), fp64: OpenMVG's
// ComputeStructureFromKnownPoses step (TriangulateNViewAlgebraic, and a
// deterministic stand-in for its robust track triangulation), restated;
// semantics in include/sfmcore.h, arithmetic in tri_point.h.
//
//   obs pass    one lane per observation: the unit bearing b of the pixel (20
//               undistortion iterations for the radial models), the 10 unique
//               entries of C'C, C = (I - b b')[R|t], the world ray R' b and the
//               bad flag.  Streaming: reads image 4 B + pixel 16 B, writes
//               80 B + 24 B + 1 B per observation.
//   solve pass  a point of <= kTriGroup observations takes a lane group (64 /
//               kTriGroup points per wave), a longer one a whole wave.
//               LINEAR: M = sum of the good observations' Grams in observation
//               order, one 4x4 Jacobi.  ROBUST: a lane per two-view hypothesis
//               (Jacobi of two Grams, judged on every observation of the track
//               in order), the best score by a total order through shuffles,
//               then the N-view refit over its inliers.  Last, a lane per
//               observation: residual and reject code at the final X.
//   point pass  the wash's point pass over those codes and the measured rays:
//               survivors, the widest angle between two of them, the status;
//               X = NaN and keep_obs = 0 for a point that is not OK.
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
constexpr int kPtThreads = 256;
constexpr int kPtPerWave = 64 / kTriGroup;

template <int CM>
__global__ __launch_bounds__(kObsThreads) void tri_obs_kernel(TriInput in, double* __restrict__ gram,
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

struct SolveOpts {
    TriRule rule;
    int32_t max_hyp;
};

// the judgement of observation i of a point (first observation o0) at X
template <int CM>
__device__ __forceinline__ uint8_t judge_at(const TriInput& in, int64_t s, const double (&X)[3], const TriRule& R,
                                            double& r0, double& r1) {
    const int32_t img = in.obs_img[s];
    const double2 uv = reinterpret_cast<const double2*>(in.obs_uv)[s];
    return tri_judge<CM>(in.cp[img], in.intr + (int64_t)in.iw * in.img_intr[img], X, uv.x, uv.y, R, r0, r1);
}

// One point by the W lanes of a group (every lane of the wave calls it; a
// group without a point has n = 0).  g: the lane within the group.
template <int CM, bool ROBUST, int W>
__device__ __forceinline__ void solve_point(const TriInput& in, const SolveOpts& O, bool has, int64_t k, int32_t o0,
                                            int32_t n, int g, const double* __restrict__ gram,
                                            const uint8_t* __restrict__ badf, uint8_t* __restrict__ code, double* __restrict__ Xs,
                                            uint8_t* __restrict__ solved, double2* __restrict__ residual,
                                            unsigned (&c)[2]) {
    auto good = [&](int32_t i) { return badf[(int64_t)o0 + i] == 0; };
    int32_t m_loc = 0;
    for (int32_t i = g; i < n; i += W) m_loc += good(i);
    const int32_t m = group_sum<W>(m_loc);
    uint8_t fin = kTriNoSolve;
    double X[3] = {0.0, 0.0, 0.0};
    // M = the Grams of the chosen observations, summed in observation order
    auto add_gram = [&](double (&G)[10], int32_t i) {
        const double* gp = gram + 10 * ((int64_t)o0 + i);
#pragma unroll
        for (int e = 0; e < 10; ++e) G[e] += gp[e];
    };
    if constexpr (!ROBUST) {
        if (m >= 2) {
            double G[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int32_t i = 0; i < n; ++i)
                if (good(i)) add_gram(G, i);
            fin = tri_solve4(G, X) ? kTriSolved : kTriInfinite;
        }
    } else {
        auto img_of = [&](int32_t i) { return good(i) ? in.obs_img[(int64_t)o0 + i] : -1; };
        long long np_loc = 0;
        if (m >= 2)
            for (int32_t a = g; a < n; a += W) np_loc += tri_row_pairs(n, a, img_of);
        const long long npairs = group_sum<W>(np_loc);
        const long long H = npairs < O.max_hyp ? npairs : (long long)O.max_hyp;
        TriScore best{-1, 0.0, 0};
        double bX[3] = {0.0, 0.0, 0.0};
        for (long long h = g; h < H; h += W) {
            int32_t a, b;
            tri_unrank(n, img_of, tri_hyp_rank(h, npairs, O.max_hyp), a, b);
            double G[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, Xh[3] = {0.0, 0.0, 0.0};
            add_gram(G, a);
            add_gram(G, b);
            TriScore sc{0, 0.0, (int32_t)h};
            if (tri_solve4(G, Xh)) {
                for (int32_t i = 0; i < n; ++i) {
                    if (!good(i)) continue;
                    double r0, r1;
                    if (judge_at<CM>(in, (int64_t)o0 + i, Xh, O.rule, r0, r1) == kTriKeep) {
                        ++sc.cnt;
                        sc.ssq += r0 * r0 + r1 * r1;
                    }
                }
            }
            if (tri_better(sc, best)) {
                best = sc;
#pragma unroll
                for (int j = 0; j < 3; ++j) bX[j] = Xh[j];
            }
        }
#pragma unroll
        for (int o = W / 2; o > 0; o >>= 1) {
            TriScore ot{__shfl_xor(best.cnt, o, W), __shfl_xor(best.ssq, o, W), __shfl_xor(best.h, o, W)};
            const double x0 = __shfl_xor(bX[0], o, W), x1 = __shfl_xor(bX[1], o, W), x2 = __shfl_xor(bX[2], o, W);
            if (tri_better(ot, best)) {
                best = ot;
                bX[0] = x0; bX[1] = x1; bX[2] = x2;
            }
        }
        if (best.cnt >= 2) {   // the refit over the winner's inliers (the same in every lane)
            double G[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int32_t i = 0; i < n; ++i) {
                if (!good(i)) continue;
                double r0, r1;
                if (judge_at<CM>(in, (int64_t)o0 + i, bX, O.rule, r0, r1) == kTriKeep) add_gram(G, i);
            }
            fin = tri_solve4(G, X) ? kTriSolved : kTriInfinite;
        }
    }
    // the final judgement, a lane per observation
    const double nan = __builtin_nan("");
    for (int32_t i = g; i < n; i += W) {
        const int64_t s = (int64_t)o0 + i;
        uint8_t cd = kTriBad;
        double r0 = nan, r1 = nan;
        if (badf[s] == 0) {
            if (fin == kTriSolved) {
                cd = judge_at<CM>(in, s, X, O.rule, r0, r1);
                c[0] += cd == kTriDepth;
                c[1] += cd == kTriResidual;
            } else {
                cd = kTriNoPoint;
            }
        }
        residual[s] = make_double2(r0, r1);
        code[s] = cd;
    }
    if (has && g == 0) {
#pragma unroll
        for (int j = 0; j < 3; ++j) Xs[3 * k + j] = fin == kTriSolved ? X[j] : nan;
        solved[k] = fin;
    }
}

template <int CM, bool ROBUST>
__global__ __launch_bounds__(kPtThreads) void tri_solve_kernel(TriInput in, SolveOpts O,
                                                               const double* __restrict__ gram,
                                                               const uint8_t* __restrict__ badf,
                                                               uint8_t* __restrict__ code, double* __restrict__ Xs, uint8_t* __restrict__ solved,
                                                               double2* __restrict__ residual,
                                                               unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t kw = ((int64_t)blockIdx.x * (kPtThreads / 64) + wave) * kPtPerWave;   // the wave's first point
    unsigned c[2] = {0, 0};
    const int grp = lane / kTriGroup, g = lane % kTriGroup;
    const int64_t k = kw + grp;
    const bool has = k < in.n_pt;
    const int32_t o0 = has ? in.pt_off[k] : 0;
    const int32_t n = has ? in.pt_off[k + 1] - o0 : 0;
    if (!__any(n > kTriGroup)) {
        solve_point<CM, ROBUST, kTriGroup>(in, O, has, k, o0, n, g, gram, badf, code, Xs, solved, residual, c);
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

struct PointRule {
    double min_angle_deg;
    int32_t min_track;
};
// the first rule that applies (SFM_TRI_* status)
__device__ __forceinline__ int point_status(const PointRule& R, uint8_t fin, int survivors, double deg) {
    if (fin == kTriNoSolve) return SFM_TRI_SHORT;
    if (fin == kTriInfinite) return SFM_TRI_INFINITE;
    if (survivors < R.min_track) return SFM_TRI_SHORT;
    if (R.min_angle_deg > 0.0 && deg < R.min_angle_deg) return SFM_TRI_ANGLE;
    return SFM_TRI_OK;
}

// The wash's point pass (ba_wash.hip) over the triangulation's codes and the
// measured rays.
__global__ __launch_bounds__(kPtThreads) void tri_point_kernel(TriInput in, PointRule R,
                                                               const uint8_t* __restrict__ code,
                                                               const double* __restrict__ ray,
                                                               const uint8_t* __restrict__ solved,
                                                               double* __restrict__ X, uint8_t* __restrict__ status,
                                                               uint8_t* __restrict__ keep_obs,
                                                               unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t kw = ((int64_t)blockIdx.x * (kPtThreads / 64) + wave) * kPtPerWave;
    unsigned c[5] = {0, 0, 0, 0, 0};   // ok, short, angle, infinite, observations kept
    const double nan = __builtin_nan("");
    auto finish = [&](int64_t kk, int v) {   // one lane per point
        status[kk] = (uint8_t)v;
        if (v != SFM_TRI_OK) {
#pragma unroll
            for (int j = 0; j < 3; ++j) X[3 * kk + j] = nan;
        }
        c[0] += v == SFM_TRI_OK; c[1] += v == SFM_TRI_SHORT; c[2] += v == SFM_TRI_ANGLE; c[3] += v == SFM_TRI_INFINITE;
    };
    const int grp = lane / kTriGroup, g = lane % kTriGroup;
    const int64_t k = kw + grp;
    const bool has = k < in.n_pt;
    const int32_t o0 = has ? in.pt_off[k] : 0;
    const int32_t n = has ? in.pt_off[k + 1] - o0 : 0;
    if (!__any(n > kTriGroup)) {
        // ---- a lane group per point ----
        const bool mine = g < n;
        const int64_t s = (int64_t)o0 + g;
        const bool ok = mine && code[s] == kTriKeep;
        double a[3] = {0.0, 0.0, 0.0};
        if (ok) {
#pragma unroll
            for (int j = 0; j < 3; ++j) a[j] = ray[3 * s + j];
        }
        Widest best{0.0, 1.0};
        pair_rounds<kTriGroup>(g, a, ok, a, ok, 1, kTriGroup / 2, best);
        group_widest<kTriGroup>(best);
        const unsigned long long mk = __ballot(ok);
        const int survivors = __popcll((mk >> (grp * kTriGroup)) & ((1ull << kTriGroup) - 1));
        const int v = point_status(R, has ? solved[k] : (uint8_t)kTriNoSolve, survivors, widest_deg(best));
        if (has && g == 0) finish(k, v);
        if (mine) {
            const bool ko = v == SFM_TRI_OK && ok;
            keep_obs[s] = ko;
            c[4] += ko;
        }
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
                const bool a_ok = i < nq && code[(int64_t)q0 + i] == kTriKeep;
                double a[3] = {0.0, 0.0, 0.0};
                if (a_ok) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) a[j] = ray[3 * ((int64_t)q0 + i) + j];
                }
                survivors += __popcll(__ballot(a_ok));
                pair_rounds<64>(lane, a, a_ok, a, a_ok, 1, 32, best);
                for (int tj = ti + 1; tj < nt; ++tj) {
                    const int jn = tj * 64 + lane;
                    const bool b_ok = jn < nq && code[(int64_t)q0 + jn] == kTriKeep;
                    double b[3] = {0.0, 0.0, 0.0};
                    if (b_ok) {
#pragma unroll
                        for (int j = 0; j < 3; ++j) b[j] = ray[3 * ((int64_t)q0 + jn) + j];
                    }
                    pair_rounds<64>(lane, a, a_ok, b, b_ok, 0, 63, best);
                }
            }
            group_widest<64>(best);
            const int v = point_status(R, solved[kq], survivors, widest_deg(best));
            if (lane == 0) finish(kq, v);
            for (int i = lane; i < nq; i += 64) {
                const int64_t s = (int64_t)q0 + i;
                const bool ko = v == SFM_TRI_OK && code[s] == kTriKeep;
                keep_obs[s] = ko;
                c[4] += ko;
            }
        }
    }
    const int slot[5] = {kTcPtOk, kTcPtShort, kTcPtAngle, kTcPtInfinite, kTcObsKept};
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const unsigned v = group_sum<64>(c[t]);
        if (lane == 0 && v) atomicAdd(&counts[slot[t]], (unsigned long long)v);
    }
}

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

void tri_eval(const TriInput& in, const sfm_tri_opts& o, TriBuffers& b, hipStream_t s) {
    SFM_REQUIRE(b.n_pt == in.n_pt && b.n_obs == in.n_obs, SFM_ERR_INVALID_ARG, "internal: triangulation buffers of another size");
    b.counts.zero(s);
    if (in.n_obs > 0) {
        const unsigned grid = (unsigned)(((int64_t)in.n_obs + kObsThreads - 1) / kObsThreads);
        SFM_BY_MODEL_ALL(in, hipLaunchKernelGGL(tri_obs_kernel<CM>, dim3(grid), dim3(kObsThreads), 0, s, in, b.gram.p,
                                                b.ray.p, b.bad.p, b.counts.p));
        SFM_HIP(hipGetLastError());
    }
    if (in.n_pt > 0) {
        const int per_block = (kPtThreads / 64) * kPtPerWave;
        const unsigned grid = (unsigned)(((int64_t)in.n_pt + per_block - 1) / per_block);
        const SolveOpts O{TriRule{o.max_residual_px, o.cheirality}, o.max_hypotheses};
        by_flag(o.method == SFM_TRI_ROBUST, [&](auto robust) {
            SFM_BY_MODEL_ALL(in, hipLaunchKernelGGL((tri_solve_kernel<CM, decltype(robust)::value>), dim3(grid),
                                                    dim3(kPtThreads), 0, s, in, O, b.gram.p, b.bad.p, b.code.p, b.X.p,
                                                    b.solved.p, reinterpret_cast<double2*>(b.residual.p),
                                                    b.counts.p));
        });
        SFM_HIP(hipGetLastError());
        hipLaunchKernelGGL(tri_point_kernel, dim3(grid), dim3(kPtThreads), 0, s, in,
                           PointRule{o.min_angle_deg, o.min_track_len}, b.code.p, b.ray.p, b.solved.p, b.X.p,
                           b.status.p, b.keep_obs.p, b.counts.p);
        SFM_HIP(hipGetLastError());
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
