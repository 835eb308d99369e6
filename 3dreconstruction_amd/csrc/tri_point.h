// N-view track triangulation, per track (include/sfmcore.h, "Track
// triangulation"), written once for the device kernels
// (tri.hip) and the serial host loop (tri.cpp, sfm_triangulate_host): the
// bearing of a pixel, the Gram C'C of an observation, the 4x4 eigen solve, the
// hypothesis score, the pair unranking, and tri_solve_track, the LINEAR /
// ROBUST algorithm over them, written for the W lanes that share a track (16
// or 64 on the device, 1 on the host).  The judgement of an observation at a
// point is track.h's judge_obs.  Host and device run the same statements;
// only the reciprocal of the depth differs (track.h, depth_rcp), so the two
// agree to rounding, not bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ba_cand.h"
#include "ba_types.h"
#include "track.h"

namespace sfm {
namespace {

// what a point's solve left (the point pass turns it into a status)
enum : uint8_t { kTriSolved = 0, kTriNoSolve = 1, kTriInfinite = 3 };
// undistortion: fixed-point iterations p_u <- p_d / c(|p_u|^2)
constexpr int kTriUndistortIters = 20;

// the radial factor of a model at r2 = |p_u|^2 (include/sfmcore.h)
template <int CM>
__host__ __device__ inline double tri_radial(const double* in, double r2) {
    if constexpr (CM == SFM_CAM_RADIAL3) {
        const double r4 = r2 * r2, r6 = r4 * r2;
        return 1.0 + in[3] * r2 + in[4] * r4 + in[5] * r6;
    } else if constexpr (CM == SFM_CAM_SNAVELY) {
        return 1.0 + r2 * (in[1] + in[2] * r2);
    } else {
        return 1.0;
    }
}

// Unit bearing b of pixel (u, v) in the camera frame; false when it is not
// finite (a "bad" observation).
template <int CM>
__host__ __device__ inline bool tri_bearing(const double* in, double u, double v, double (&b)[3]) {
    double x, y, z = 1.0;
    if constexpr (CM == SFM_CAM_PINHOLE) {
        x = (u - in[2]) / in[0];
        y = (v - in[3]) / in[1];
    } else {
        double xd, yd;
        if constexpr (CM == SFM_CAM_RADIAL3) {
            xd = (u - in[1]) / in[0];
            yd = (v - in[2]) / in[0];
        } else {   // SNAVELY: p = -P / P2, the camera looks down -z
            xd = u / in[0];
            yd = v / in[0];
            z = -1.0;
        }
        x = xd; y = yd;
        for (int it = 0; it < kTriUndistortIters; ++it) {
            const double c = tri_radial<CM>(in, x * x + y * y);
            x = xd / c;
            y = yd / c;
        }
    }
    const double n = sqrt(x * x + y * y + 1.0);
    b[0] = x / n; b[1] = y / n; b[2] = z / n;
    return track_finite(b[0]) && track_finite(b[1]) && track_finite(b[2]);
}

// The 10 unique entries (rows 0..3, columns >= row) of C'C, C = (I - b b')[R|t]
// (OpenMVG TriangulateNViewAlgebraic's cost of one view).
__host__ __device__ inline void tri_gram(const CamPre& cp, const double (&b)[3], double (&G)[10]) {
    double c[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double a0 = j < 3 ? cp.R[j] : cp.t[0], a1 = j < 3 ? cp.R[3 + j] : cp.t[1],
                     a2 = j < 3 ? cp.R[6 + j] : cp.t[2];
        const double d = b[0] * a0 + b[1] * a1 + b[2] * a2;
        c[j][0] = a0 - b[0] * d; c[j][1] = a1 - b[1] * d; c[j][2] = a2 - b[2] * d;
    }
    int e = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = j; k < 4; ++k) G[e++] = c[j][0] * c[k][0] + c[j][1] * c[k][1] + c[j][2] * c[k][2];
}

// the measured ray of an observation in world axes, R' b
__host__ __device__ inline void tri_world_ray(const CamPre& cp, const double (&b)[3], double (&d)[3]) {
    for (int j = 0; j < 3; ++j) d[j] = cp.R[j] * b[0] + cp.R[3 + j] * b[1] + cp.R[6 + j] * b[2];
}

// X = v[0..2] / v[3] of the eigenvector v of the smallest eigenvalue of the
// symmetric M (its 10 unique entries): the cyclic Jacobi of geom::triangulate
// (include/sfm/actuator.hpp) -- its sweep order, 30-sweep cap and stop rule;
// the smallest diagonal, lowest index on a tie.  False: the point is at
// infinity (|v[3]| <= 1e-12) or not finite.
__host__ __device__ inline bool tri_solve4(const double (&G)[10], double (&X)[3]) {
    double M[4][4], V[4][4];
    {
        int e = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = j; k < 4; ++k) {
                M[j][k] = M[k][j] = G[e++];
            }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0, diag = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (r == c) diag += M[r][c] * M[r][c];
                else off += M[r][c] * M[r][c];
            }
        if (off <= 1e-30 * diag) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                if (M[p][q] == 0.0) continue;
                const double th = (M[q][q] - M[p][p]) / (2.0 * M[p][q]);
                const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {   // M <- J' M J
                    const double mkp = M[k][p], mkq = M[k][q];
                    M[k][p] = c * mkp - s * mkq;
                    M[k][q] = s * mkp + c * mkq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double mpk = M[p][k], mqk = M[q][k];
                    M[p][k] = c * mpk - s * mqk;
                    M[q][k] = s * mpk + c * mqk;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    double dm = M[0][0], v[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (M[k][k] < dm) {
            dm = M[k][k];
#pragma unroll
            for (int a = 0; a < 4; ++a) v[a] = V[a][k];
        }
    if (!(fabs(v[3]) > 1e-12)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) X[a] = v[a] / v[3];
    return track_finite(X[0]) && track_finite(X[1]) && track_finite(X[2]);
}

// A hypothesis' score: more inliers, then the smaller sum of their squared
// residuals, then the lower index (a total order: any reduction order gives
// the same winner).  cnt -1: no hypothesis.
struct TriScore {
    int32_t cnt;
    double ssq;
    int32_t h;
};
__host__ __device__ inline bool tri_better(const TriScore& a, const TriScore& b) {
    if (a.cnt != b.cnt) return a.cnt > b.cnt;
    if (a.ssq != b.ssq) return a.ssq < b.ssq;
    return a.h < b.h;
}

// Hypotheses are the pairs (a, b), a < b, of a point's observations that are
// both good and of different images, in lexicographic order.  img(i): the
// image of observation i of the point, or -1 for a bad one.
template <class ImgOf>
__host__ __device__ inline int64_t tri_row_pairs(int32_t n, int32_t a, ImgOf img) {
    const int32_t ia = img(a);
    if (ia < 0) return 0;
    int64_t c = 0;
    for (int32_t b = a + 1; b < n; ++b) {
        const int32_t ib = img(b);
        c += ib >= 0 && ib != ia;
    }
    return c;
}
// pair number `rank` (< the number of pairs)
template <class ImgOf>
__host__ __device__ inline void tri_unrank(int32_t n, ImgOf img, int64_t rank, int32_t& a, int32_t& b) {
    a = 0; b = 0;
    for (int32_t i = 0; i < n; ++i) {
        const int32_t ii = img(i);
        if (ii < 0) continue;
        for (int32_t j = i + 1; j < n; ++j) {
            const int32_t ij = img(j);
            if (ij < 0 || ij == ii) continue;
            if (rank == 0) {
                a = i; b = j;
                return;
            }
            --rank;
        }
    }
}
// the pair number of hypothesis h of H = min(npairs, max_hypotheses):
// floor(h * npairs / max_hypotheses) when the pairs are too many, in integers
// without overflow (h * (npairs / m) + h * (npairs % m) / m)
__host__ __device__ inline int64_t tri_hyp_rank(int64_t h, int64_t npairs, int64_t max_hyp) {
    if (npairs <= max_hyp) return h;
    return h * (npairs / max_hyp) + h * (npairs % max_hyp) / max_hyp;
}

// One track of n observations by the Lanes::W lanes that share it (every one
// of them calls it; a group without a point has n = 0).  Lanes supplies this
// lane's index g, sum(v) over the lanes and best(score, X), the reduction to
// the best hypothesis by tri_better's total order; on the host W = 1 and
// both are identities.  The caller's storage is behind accessors over the
// track's observation index i:
//   good(i)                 the observation has a bearing
//   add_gram(G, i)          G += its Gram
//   judge(i, X, r0, r1)     its reject code and residual at X (judge_obs)
//   img_of(i)               its image, -1 when not good
//   out(i, code, r0, r1)    its final code and residual, one lane each
// Returns what the solve left and, for kTriSolved, X (the same in every lane).
// LINEAR: M = the good observations' Grams summed in observation order, one
// solve.  ROBUST: a lane per two-view hypothesis (the solve of two Grams,
// scored on every good observation in order), the best of them, then the
// N-view refit over its inliers.
template <bool ROBUST, class Lanes, class Good, class AddGram, class Judge, class ImgOf, class Out>
__host__ __device__ inline uint8_t tri_solve_track(const Lanes& L, int32_t n, int32_t max_hyp, Good good,
                                                   AddGram add_gram, Judge judge, ImgOf img_of, Out out,
                                                   double (&X)[3]) {
    constexpr int W = Lanes::W;
    const int g = L.g;
    int32_t m_loc = 0;
    for (int32_t i = g; i < n; i += W) m_loc += good(i);
    const int32_t m = L.sum(m_loc);
    uint8_t fin = kTriNoSolve;
    X[0] = X[1] = X[2] = 0.0;
    if constexpr (!ROBUST) {
        if (m >= 2) {
            double G[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int32_t i = 0; i < n; ++i)
                if (good(i)) add_gram(G, i);
            fin = tri_solve4(G, X) ? kTriSolved : kTriInfinite;
        }
    } else {
        long long np_loc = 0;
        if (m >= 2)
            for (int32_t a = g; a < n; a += W) np_loc += tri_row_pairs(n, a, img_of);
        const long long npairs = L.sum(np_loc);
        const long long H = npairs < max_hyp ? npairs : (long long)max_hyp;
        TriScore best{-1, 0.0, 0};
        double bX[3] = {0.0, 0.0, 0.0};
        for (long long h = g; h < H; h += W) {
            int32_t a, b;
            tri_unrank(n, img_of, tri_hyp_rank(h, npairs, max_hyp), a, b);
            double G[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, Xh[3] = {0.0, 0.0, 0.0};
            add_gram(G, a);
            add_gram(G, b);
            TriScore sc{0, 0.0, (int32_t)h};
            if (tri_solve4(G, Xh)) {
                for (int32_t i = 0; i < n; ++i) {
                    if (!good(i)) continue;
                    double r0, r1;
                    if (judge(i, Xh, r0, r1) == kObsKeep) {
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
        L.best(best, bX);
        if (best.cnt >= 2) {   // the refit over the winner's inliers (the same in every lane)
            double G[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int32_t i = 0; i < n; ++i) {
                if (!good(i)) continue;
                double r0, r1;
                if (judge(i, bX, r0, r1) == kObsKeep) add_gram(G, i);
            }
            fin = tri_solve4(G, X) ? kTriSolved : kTriInfinite;
        }
    }
    // the final judgement, a lane per observation
    const double nan = __builtin_nan("");
    for (int32_t i = g; i < n; i += W) {
        uint8_t cd = kObsBad;
        double r0 = nan, r1 = nan;
        if (good(i)) cd = fin == kTriSolved ? judge(i, X, r0, r1) : (uint8_t)kObsNoPoint;
        out(i, cd, r0, r1);
    }
    return fin;
}

}  // namespace
}  // namespace sfm
