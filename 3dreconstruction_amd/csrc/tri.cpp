// N-view track triangulation, host side: the options, the serial host entry
// point (sfm_triangulate_host: per point, tri_point.h's tri_solve_track on
// one lane and a plain restatement of the point pass) and the one-shot device
// entry point (sfm_triangulate: a TrackUpload of the caller's arrays, the
// kernels of tri.hip).
// SFM_TRI_HOST_ONLY leaves the device entry point out, so that the host path
// builds with a plain host compiler (tests/cpp/triangulate_test.cpp).
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "ba_plan.h"
#include "tri_point.h"
#ifndef SFM_TRI_HOST_ONLY
#include "ba_kernels.h"
#include "tri.h"
#endif

using namespace sfm;

extern "C" void sfm_tri_default_options(sfm_tri_opts* o) {
    if (!o) return;
    // OpenMVG's robust track triangulation thresholds as its incremental engine
    // sets them: 4 px residual, 2 degrees, tracks of two or more views
    o->method = SFM_TRI_ROBUST;
    o->max_hypotheses = 64;
    o->max_residual_px = 4.0;
    o->min_angle_deg = 2.0;
    o->min_track_len = 2;
    o->cheirality = 1;
}

namespace {

sfm_tri_opts tri_options(const sfm_tri_opts* o) {
    sfm_tri_opts r;
    if (o) r = *o; else sfm_tri_default_options(&r);
    SFM_REQUIRE(r.method == SFM_TRI_LINEAR || r.method == SFM_TRI_ROBUST, SFM_ERR_INVALID_ARG,
                "unknown triangulation method %d", r.method);
    SFM_REQUIRE(r.min_track_len >= 2, SFM_ERR_INVALID_ARG, "min_track_len %d (must be >= 2)", r.min_track_len);
    SFM_REQUIRE(r.max_hypotheses >= 1, SFM_ERR_INVALID_ARG, "max_hypotheses %d (must be >= 1)", r.max_hypotheses);
    SFM_REQUIRE(r.max_residual_px == r.max_residual_px && r.min_angle_deg == r.min_angle_deg, SFM_ERR_INVALID_ARG,
                "NaN triangulation threshold");
    return r;
}

struct HostOut {
    double* X;
    uint8_t* status;
    uint8_t* keep_obs;
    double* residual;
    int64_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // sfm_tri_stats order
};

// tri_solve_track's lanes on the host: one
struct OneLane {
    static constexpr int W = 1;
    static constexpr int g = 0;
    template <class T>
    T sum(T v) const { return v; }
    void best(TriScore&, double (&)[3]) const {}
};

// every point of the problem, serially (tri.hip's three passes per point)
template <int CM, bool ROBUST>
void host_points(const sfm_ba_problem& P, const std::vector<CamPre>& cps, const double* intr, const sfm_tri_opts& O,
                 HostOut& out) {
    const int iw = sfm_ba_intr_width(CM);
    const ObsRule rule{O.max_residual_px, O.cheirality};
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> gram, ray;
    std::vector<uint8_t> bad, code;
    for (int64_t p = 0; p < P.n_pt; ++p) {
        const int64_t o0 = P.pt_offsets[p];
        const int32_t n = (int32_t)(P.pt_offsets[p + 1] - o0);
        gram.assign(10 * (size_t)n, 0.0);
        ray.assign(3 * (size_t)n, 0.0);
        bad.assign(n, 0);
        code.assign(n, kObsBad);
        auto in_of = [&](int32_t i) { return intr + (int64_t)iw * P.img_intr[P.obs_img[o0 + i]]; };
        auto cp_of = [&](int32_t i) -> const CamPre& { return cps[P.obs_img[o0 + i]]; };
        for (int32_t i = 0; i < n; ++i) {
            double b[3], G[10], d[3];
            bad[i] = !tri_bearing<CM>(in_of(i), P.obs_uv[2 * (o0 + i)], P.obs_uv[2 * (o0 + i) + 1], b);
            if (bad[i]) {
                ++out.c[5];
                continue;
            }
            tri_gram(cp_of(i), b, G);
            tri_world_ray(cp_of(i), b, d);
            std::memcpy(&gram[10 * (size_t)i], G, sizeof G);
            std::memcpy(&ray[3 * (size_t)i], d, sizeof d);
        }
        auto good = [&](int32_t i) { return bad[i] == 0; };
        auto add_gram = [&](double (&G)[10], int32_t i) {
            for (int e = 0; e < 10; ++e) G[e] += gram[10 * (size_t)i + e];
        };
        auto judge = [&](int32_t i, const double (&X)[3], double& r0, double& r1) {
            return judge_obs<CM>(cp_of(i), in_of(i), X, P.obs_uv[2 * (o0 + i)], P.obs_uv[2 * (o0 + i) + 1], rule, r0,
                                 r1);
        };
        auto img_of = [&](int32_t i) { return bad[i] ? -1 : P.obs_img[o0 + i]; };
        int32_t survivors = 0;
        auto emit = [&](int32_t i, uint8_t cd, double r0, double r1) {
            code[i] = cd;
            out.c[6] += cd == kObsDepth;
            out.c[7] += cd == kObsResidual;
            survivors += cd == kObsKeep;
            if (out.residual) {
                out.residual[2 * (o0 + i)] = r0;
                out.residual[2 * (o0 + i) + 1] = r1;
            }
        };
        double X[3];
        const uint8_t fin =
            tri_solve_track<ROBUST>(OneLane{}, n, O.max_hypotheses, good, add_gram, judge, img_of, emit, X);
        // the widest angle between two kept rays, atan2(|a x b|, a.b)
        double deg = 0.0;
        for (int32_t i = 0; i < n; ++i) {
            if (code[i] != kObsKeep) continue;
            const double* a = &ray[3 * (size_t)i];
            for (int32_t j = i + 1; j < n; ++j) {
                if (code[j] != kObsKeep) continue;
                const double* b = &ray[3 * (size_t)j];
                const double c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2],
                             c2 = a[0] * b[1] - a[1] * b[0];
                const double ang = std::atan2(std::sqrt(c0 * c0 + c1 * c1 + c2 * c2),
                                              a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) *
                                   (180.0 / 3.14159265358979323846);
                if (ang > deg) deg = ang;
            }
        }
        int st = SFM_TRI_OK;
        if (fin == kTriNoSolve) st = SFM_TRI_SHORT;
        else if (fin == kTriInfinite) st = SFM_TRI_INFINITE;
        else if (survivors < O.min_track_len) st = SFM_TRI_SHORT;
        else if (O.min_angle_deg > 0.0 && deg < O.min_angle_deg) st = SFM_TRI_ANGLE;
        ++out.c[st == SFM_TRI_OK ? 0 : st == SFM_TRI_SHORT ? 1 : st == SFM_TRI_ANGLE ? 2 : 3];
        if (out.status) out.status[p] = (uint8_t)st;
        if (out.X)
            for (int j = 0; j < 3; ++j) out.X[3 * p + j] = st == SFM_TRI_OK ? X[j] : nan;
        for (int32_t i = 0; i < n; ++i) {
            const bool ko = st == SFM_TRI_OK && code[i] == kObsKeep;
            out.c[4] += ko;
            if (out.keep_obs) out.keep_obs[o0 + i] = ko;
        }
    }
}

}  // namespace

extern "C" int sfm_triangulate_host(const sfm_ba_problem* prob, const double* extr, const double* intr,
                                    const sfm_tri_opts* opts, double* X, uint8_t* status, uint8_t* keep_obs,
                                    double* residual, sfm_tri_stats* stats) {
    return guarded([&] {
        const sfm_tri_opts O = tri_options(opts);
        SFM_REQUIRE(prob && extr && intr, SFM_ERR_INVALID_ARG, "null argument");
        validate_problem(*prob);
        std::vector<CamPre> cps((size_t)prob->n_img);
        for (int32_t i = 0; i < prob->n_img; ++i) cps[i] = make_campre(extr + 6 * (size_t)i);
        HostOut out{X, status, keep_obs, residual};
        auto by_method = [&](auto cm) {
            if (O.method == SFM_TRI_ROBUST) host_points<decltype(cm)::value, true>(*prob, cps, intr, O, out);
            else host_points<decltype(cm)::value, false>(*prob, cps, intr, O, out);
        };
        if (prob->camera_model == SFM_CAM_RADIAL3) by_method(std::integral_constant<int, SFM_CAM_RADIAL3>{});
        else if (prob->camera_model == SFM_CAM_SNAVELY) by_method(std::integral_constant<int, SFM_CAM_SNAVELY>{});
        else by_method(std::integral_constant<int, SFM_CAM_PINHOLE>{});
        if (stats) {
            stats->n_pt_ok = out.c[0]; stats->n_pt_short = out.c[1]; stats->n_pt_angle = out.c[2];
            stats->n_pt_infinite = out.c[3]; stats->n_obs_kept = out.c[4]; stats->n_obs_bad = out.c[5];
            stats->n_obs_depth = out.c[6]; stats->n_obs_residual = out.c[7];
        }
        return SFM_OK;
    });
}

#ifndef SFM_TRI_HOST_ONLY
extern "C" int sfm_triangulate(sfm_ctx* ctx, const sfm_ba_problem* prob, const double* extr, const double* intr,
                               const sfm_tri_opts* opts, double* X, uint8_t* status, uint8_t* keep_obs,
                               double* residual, sfm_tri_stats* stats) {
    return guarded([&] {
        const sfm_tri_opts O = tri_options(opts);
        SFM_REQUIRE(ctx && prob && extr && intr, SFM_ERR_INVALID_ARG, "null argument");
        validate_problem(*prob);
        CtxScope scope_(ctx);
        hipStream_t s = ctx->stream;
        TrackUpload up(*prob, extr, intr, nullptr, s);
        TriBuffers b;
        b.alloc(prob->n_pt, prob->n_obs);
        hipEvent_t* ev = nullptr;
        if (ctx->time_kernels) {   // the kernels alone: the uploads drained first
            ev = ctx_events(ctx);
            SFM_HIP(hipStreamSynchronize(s));
            SFM_HIP(hipEventRecord(ev[0], s));
        }
        ba_campre(up.extr.p, prob->n_img, up.cp.p, s);
        tri_eval(up.in, O, b, s);
        if (ev) {
            SFM_HIP(hipEventRecord(ev[1], s));
            SFM_HIP(hipEventSynchronize(ev[1]));
            float t = 0.f;
            SFM_HIP(hipEventElapsedTime(&t, ev[0], ev[1]));
            ctx->last_kernel_ms = t;
        }
        tri_download(b, X, status, keep_obs, residual, stats, s);
        return SFM_OK;
    });
}
#endif
