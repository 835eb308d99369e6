// Post-BA outlier rejection, host side: the options, the one-shot entry point
// (sfm_ba_wash: a TrackUpload of the caller-order arrays, identity maps) and
// the compaction of a problem by the masks a wash returned (sfm_ba_wash_apply,
// host only).  The resident entry point, sfm_ba_plan_wash, is in ba_solver.cpp
// next to the plan it reads; both run the kernels of ba_wash.hip.
#include "ba_wash.h"

#include <cstring>

#include "ba_kernels.h"
#include "ba_plan.h"

using namespace sfm;

extern "C" void sfm_ba_wash_default_options(sfm_ba_wash_opts* o) {
    if (!o) return;
    // OpenMVG badTrackRejector(4.0, ...): RemoveOutliers_PixelResidualError(4.0 px,
    // min track length 2), RemoveOutliers_AngleError(2.0 deg)
    o->max_residual_px = 4.0;
    o->min_angle_deg = 2.0;
    o->min_track_len = 2;
    o->cheirality = 1;
}

sfm_ba_wash_opts sfm::wash_options(const sfm_ba_wash_opts* o) {
    sfm_ba_wash_opts r;
    if (o) r = *o; else sfm_ba_wash_default_options(&r);
    SFM_REQUIRE(r.min_track_len >= 1, SFM_ERR_INVALID_ARG, "min_track_len %d (must be >= 1)", r.min_track_len);
    SFM_REQUIRE(r.max_residual_px == r.max_residual_px && r.min_angle_deg == r.min_angle_deg, SFM_ERR_INVALID_ARG,
                "NaN wash threshold");
    return r;
}

extern "C" int sfm_ba_wash(sfm_ctx* ctx, const sfm_ba_problem* prob, const double* extr, const double* intr,
                           const double* X, const sfm_ba_wash_opts* opts, double* residual, double* max_angle_deg,
                           uint8_t* keep_obs, uint8_t* keep_pt, sfm_ba_wash_stats* stats) {
    return guarded([&] {
        const sfm_ba_wash_opts O = wash_options(opts);
        SFM_REQUIRE(ctx && prob && extr && intr && (X || prob->n_pt == 0), SFM_ERR_INVALID_ARG, "null argument");
        validate_problem(*prob);
        CtxScope scope_(ctx);
        hipStream_t s = ctx->stream;
        TrackUpload up(*prob, extr, intr, X, s);
        ba_campre(up.extr.p, prob->n_img, up.cp.p, s);
        WashBuffers b;
        b.alloc(prob->n_pt, prob->n_obs);
        ba_wash_eval(up.in, O, b, s);
        ba_wash_download(b, residual, max_angle_deg, keep_obs, keep_pt, stats, s);
        return SFM_OK;
    });
}

extern "C" int sfm_ba_wash_apply(const sfm_ba_problem* prob, const double* X, const uint8_t* keep_obs,
                                 const uint8_t* keep_pt, int64_t* pt_offsets, int32_t* obs_img, double* obs_uv,
                                 double* X_out, int64_t* pt_map) {
    return guarded([&] {
        SFM_REQUIRE(prob && (keep_obs || prob->n_obs == 0) && (keep_pt || prob->n_pt == 0) && (X || !X_out),
                    SFM_ERR_INVALID_ARG, "null argument");
        validate_problem(*prob);
        int64_t k = 0, o = 0;
        if (pt_offsets) pt_offsets[0] = 0;
        for (int64_t p = 0; p < prob->n_pt; ++p) {
            const int64_t a = prob->pt_offsets[p], b = prob->pt_offsets[p + 1];
            if (!keep_pt[p]) {
                for (int64_t q = a; q < b; ++q)
                    SFM_REQUIRE(!keep_obs[q], SFM_ERR_INVALID_ARG,
                                "observation %lld is kept but its point %lld is removed", (long long)q, (long long)p);
                continue;
            }
            for (int64_t q = a; q < b; ++q) {
                if (!keep_obs[q]) continue;
                if (obs_img) obs_img[o] = prob->obs_img[q];
                if (obs_uv) {
                    obs_uv[2 * o] = prob->obs_uv[2 * q];
                    obs_uv[2 * o + 1] = prob->obs_uv[2 * q + 1];
                }
                ++o;
            }
            if (X_out) std::memcpy(X_out + 3 * k, X + 3 * p, 3 * sizeof(double));
            if (pt_map) pt_map[k] = p;
            ++k;
            if (pt_offsets) pt_offsets[k] = o;
        }
        return SFM_OK;
    });
}
