// Incremental reconstruction, host side (include/sfmcore.h, "Incremental
// reconstruction"): the resident tracks handle and its argument checks, the
// serial host twins of the three round queries, and the driver
// (sfm_reconstruct / sfm_reconstruct_host: one function over either kind of
// handle and either set of stage entry points), plus the file-staged
// sfm_sparse_reconstruct and sfm_sparse_reconstruct_colorize.  The round
// kernels are recon.hip's.
//
// Deviations from OpenMVG's SequentialSfMReconstructionEngine:
// no bundle adjustment of the initial pair alone (no fixed-intrinsics solve
// here); the robust triangulation is sfm_triangulate's deterministic one and is
// not re-run for solved points (a late observation joins through
// select(SOLVED) and is judged by the wash); resection candidates are counted
// per reconstructed point, not per track id; the washed problem is not carried
// from one repeat to the next but selected again from the resident tracks,
// which gives the same sub-problem.
// SFM_RECON_HOST_ONLY leaves every device path out, so that the host twin
// builds with a plain host compiler (tests/cpp/recon_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "colorize.h"
#include "recon.h"
#include "relpose_best.h"

using namespace sfm;

extern "C" void sfm_recon_default_options(sfm_recon_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    sfm_relpose_default_options(&o->relpose);
    sfm_resect_default_options(&o->resect);
    sfm_tri_default_options(&o->tri);
    sfm_ba_default_options(&o->ba);
    sfm_ba_wash_default_options(&o->wash);
    o->initial_pair[0] = o->initial_pair[1] = -1;
    // AutomaticInitialPairChoice: more than 100 inliers, more than 3 degrees
    o->pair_min_inliers = 100;
    o->pair_min_angle_deg = 3.0;
    o->adjust = 1;
    o->group_ratio = 0.75;        // dThresholdGroup
    o->wash_repeat_above = 50;    // the engine's "while (badTrackRejector(4.0, 50))"
    o->max_adjust_repeats = 8;
    o->min_track_len = 2;
}

namespace {

void ok_or_throw(int rc) {
    if (rc != SFM_OK) throw SfmError{rc};
}

// ---- the handle (its checks and its index: recon.h, shared with colorize.cpp) -------
int create_handle(const char* who, sfm_ctx* ctx, bool device, const sfm_ba_problem* prob, sfm_recon_tracks** out) {
    return guarded([&] {
        SFM_REQUIRE(out, SFM_ERR_INVALID_ARG, "%s: null argument", who);
        *out = nullptr;
        SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
        recon_check_tracks(who, prob);
        std::unique_ptr<sfm_recon_tracks> t(new sfm_recon_tracks);
        t->n_img = prob->n_img;
        t->n_pt = prob->n_pt;
        t->n_obs = prob->n_obs;
        const ReconIndex ix = recon_build_index(*prob, t->img_off);
        if (device) {
#ifndef SFM_RECON_HOST_ONLY
            t->ctx = ctx;
            t->dev = recon_device_create(ctx, prob->n_img, (int32_t)prob->n_pt, (int32_t)prob->n_obs, ix, prob->obs_img,
                                         prob->obs_uv);
#endif
        } else {
            t->pt_off.assign(prob->pt_offsets, prob->pt_offsets + prob->n_pt + 1);
            t->obs_img.assign(prob->obs_img, prob->obs_img + prob->n_obs);
            t->obs_uv.assign(prob->obs_uv, prob->obs_uv + 2 * prob->n_obs);
            t->dead.assign((size_t)prob->n_obs, 0);
        }
        *out = t.release();
        return SFM_OK;
    });
}

// ---- the host twins -----------------------------------------------------------------
void host_visibility(const sfm_recon_tracks& t, const uint8_t* pt_ok, int32_t* count) {
    std::vector<int64_t> last((size_t)t.n_img, -1);
    for (int64_t p = 0; p < t.n_pt; ++p) {
        if (!pt_ok[p]) continue;
        for (int64_t o = t.pt_off[p]; o < t.pt_off[p + 1]; ++o) {
            const int32_t im = t.obs_img[o];
            if (t.dead[o] || last[im] == p) continue;
            last[im] = p;
            ++count[im];
        }
    }
}

// sfm_resect_gather's walk, over the alive observations
void host_gather(const sfm_recon_tracks& t, const double* X, const uint8_t* pt_ok, const int32_t* images,
                 int32_t n_images, bool rows, ReconGather& out) {
    std::vector<int32_t> slot((size_t)t.n_img, -1);
    for (int32_t q = 0; q < n_images; ++q) slot[images[q]] = q;
    out.off.assign((size_t)n_images + 1, 0);
    for (int pass = 0; pass < (rows ? 2 : 1); ++pass) {
        std::vector<int64_t> at(out.off.begin(), out.off.end() - 1);   // (second pass: where each image's next one goes)
        for (int64_t p = 0; p < t.n_pt; ++p) {
            if (!pt_ok[p]) continue;
            for (int64_t o = t.pt_off[p]; o < t.pt_off[p + 1]; ++o) {
                const int32_t q = slot[t.obs_img[o]];
                if (q < 0 || t.dead[o]) continue;
                if (pass == 0) {
                    ++out.off[(size_t)q + 1];
                } else {
                    const int64_t k = at[q]++;
                    for (int a = 0; a < 3; ++a) out.X3[3 * k + a] = X[3 * p + a];
                    out.uv[2 * k] = t.obs_uv[2 * o];
                    out.uv[2 * k + 1] = t.obs_uv[2 * o + 1];
                    out.obs[k] = o;
                }
            }
        }
        if (pass == 0) {
            for (int32_t q = 0; q < n_images; ++q) out.off[(size_t)q + 1] += out.off[q];
            if (rows) {
                out.X3.resize(3 * (size_t)out.off[n_images]);
                out.uv.resize(2 * (size_t)out.off[n_images]);
                out.obs.resize((size_t)out.off[n_images]);
            }
        }
    }
}

void host_select(const sfm_recon_tracks& t, const uint8_t* registered, const uint8_t* pt_ok, int32_t mode,
                 int32_t min_len, bool rows, ReconSelect& out) {
    out = ReconSelect{};
    out.pt_offsets.assign(1, 0);
    for (int64_t p = 0; p < t.n_pt; ++p) {
        if ((pt_ok[p] != 0) != (mode == SFM_RECON_SOLVED)) continue;
        int64_t n = 0;
        int32_t first = -1;
        bool two = false;
        for (int64_t o = t.pt_off[p]; o < t.pt_off[p + 1]; ++o) {
            const int32_t im = t.obs_img[o];
            if (t.dead[o] || !registered[im]) continue;
            ++n;
            if (first < 0) first = im;
            else two = two || im != first;
        }
        if (!(mode == SFM_RECON_SOLVED ? n >= min_len && n >= 1 : two)) continue;
        ++out.n_pt;
        out.n_obs += n;
        if (!rows) continue;
        out.pt_map.push_back(p);
        for (int64_t o = t.pt_off[p]; o < t.pt_off[p + 1]; ++o) {
            if (t.dead[o] || !registered[t.obs_img[o]]) continue;
            out.obs_map.push_back(o);
            out.obs_img.push_back(t.obs_img[o]);
            out.obs_uv.push_back(t.obs_uv[2 * o]);
            out.obs_uv.push_back(t.obs_uv[2 * o + 1]);
        }
        out.pt_offsets.push_back((int64_t)out.obs_map.size());
    }
    if (!rows) {
        out.pt_offsets.assign((size_t)out.n_pt + 1, 0);
        out.pt_offsets[out.n_pt] = out.n_obs;
    }
}

// ---- the queries over either kind of handle (arguments already checked) --------------
void q_visibility(sfm_recon_tracks* t, const uint8_t* pt_ok, int32_t* count) {
    if (t->n_img == 0) return;
    std::fill(count, count + t->n_img, 0);
    if (t->n_obs == 0) return;
#ifndef SFM_RECON_HOST_ONLY
    if (t->dev) return recon_device_visibility(t->dev, pt_ok, count);
#endif
    host_visibility(*t, pt_ok, count);
}

void check_images(const char* who, const sfm_recon_tracks* t, const int32_t* images, int32_t n_images) {
    SFM_REQUIRE(n_images >= 0 && (n_images == 0 || images), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    std::vector<uint8_t> listed((size_t)std::max(t->n_img, 1), 0);
    for (int32_t q = 0; q < n_images; ++q) {
        SFM_REQUIRE(images[q] >= 0 && images[q] < t->n_img && !listed[images[q]], SFM_ERR_INVALID_ARG,
                    "%s: image %d is out of range or listed twice", who, images[q]);
        listed[images[q]] = 1;
    }
}

void q_gather(sfm_recon_tracks* t, const double* X, const uint8_t* pt_ok, const int32_t* images, int32_t n_images,
              bool rows, ReconGather& out) {
#ifndef SFM_RECON_HOST_ONLY
    if (t->dev) {
        std::vector<int32_t> seg_off((size_t)n_images + 1, 0), seg_base((size_t)std::max(n_images, 1), 0);
        for (int32_t q = 0; q < n_images; ++q) {
            seg_base[q] = t->img_off[images[q]];
            seg_off[(size_t)q + 1] = seg_off[q] + (t->img_off[(size_t)images[q] + 1] - t->img_off[images[q]]);
        }
        return recon_device_gather(t->dev, X, pt_ok, n_images, seg_off.data(), seg_base.data(), rows, out);
    }
#endif
    host_gather(*t, X, pt_ok, images, n_images, rows, out);
}

void q_select(sfm_recon_tracks* t, const uint8_t* registered, const uint8_t* pt_ok, int32_t mode, int32_t min_len,
              bool rows, ReconSelect& out) {
#ifndef SFM_RECON_HOST_ONLY
    if (t->dev) return recon_device_select(t->dev, registered, pt_ok, mode, min_len, rows, out);
#endif
    host_select(*t, registered, pt_ok, mode, min_len, rows, out);
}

void q_drop(sfm_recon_tracks* t, const std::vector<int64_t>& obs) {
    if (obs.empty()) return;
#ifndef SFM_RECON_HOST_ONLY
    if (t->dev) {
        const std::vector<int32_t> o32(obs.begin(), obs.end());
        return recon_device_drop(t->dev, o32.data(), (int64_t)o32.size());
    }
#endif
    for (int64_t o : obs) t->dead[o] = 1;
}

}  // namespace

extern "C" int sfm_recon_tracks_create(sfm_ctx* ctx, const sfm_ba_problem* prob, sfm_recon_tracks** out) {
#ifdef SFM_RECON_HOST_ONLY
    return guarded([&]() -> int {
        SFM_REQUIRE(false, SFM_ERR_UNSUPPORTED, "sfm_recon_tracks_create: a host-only build");
        return SFM_OK;
    });
#else
    return create_handle("sfm_recon_tracks_create", ctx, true, prob, out);
#endif
}

extern "C" int sfm_recon_tracks_create_host(const sfm_ba_problem* prob, sfm_recon_tracks** out) {
    return create_handle("sfm_recon_tracks_create_host", nullptr, false, prob, out);
}

extern "C" int sfm_recon_tracks_destroy(sfm_recon_tracks* t) {
    return guarded([&] {
        if (!t) return SFM_OK;
#ifndef SFM_RECON_HOST_ONLY
        recon_device_destroy(t->dev);
#endif
        delete t;
        return SFM_OK;
    });
}

extern "C" int sfm_recon_tracks_drop_obs(sfm_recon_tracks* t, const int64_t* obs, int64_t n) {
    return guarded([&] {
        SFM_REQUIRE(t && n >= 0 && (n == 0 || obs), SFM_ERR_INVALID_ARG, "sfm_recon_tracks_drop_obs: null argument");
        for (int64_t k = 0; k < n; ++k)
            SFM_REQUIRE(obs[k] >= 0 && obs[k] < t->n_obs, SFM_ERR_INVALID_ARG,
                        "sfm_recon_tracks_drop_obs: observation %lld of %lld", (long long)obs[k], (long long)t->n_obs);
        q_drop(t, std::vector<int64_t>(obs, obs + n));
        return SFM_OK;
    });
}

extern "C" int sfm_recon_visibility(sfm_recon_tracks* t, const uint8_t* pt_ok, int32_t* count) {
    return guarded([&] {
        SFM_REQUIRE(t && (t->n_pt == 0 || pt_ok) && (t->n_img == 0 || count), SFM_ERR_INVALID_ARG,
                    "sfm_recon_visibility: null argument");
        q_visibility(t, pt_ok, count);
        return SFM_OK;
    });
}

extern "C" int sfm_recon_gather(sfm_recon_tracks* t, const double* X, const uint8_t* pt_ok, const int32_t* images,
                                int32_t n_images, int64_t* off, double* X3, double* uv, int64_t* obs, int64_t cap) {
    return guarded([&] {
        SFM_REQUIRE(t && off && (t->n_pt == 0 || pt_ok) && cap >= 0, SFM_ERR_INVALID_ARG,
                    "sfm_recon_gather: null argument");
        SFM_REQUIRE((X3 == nullptr) == (uv == nullptr) && (!X3 || X || t->n_pt == 0) && (!obs || X3), SFM_ERR_INVALID_ARG,
                    "sfm_recon_gather: X3 and uv go together, and need X; obs goes with them");
        check_images("sfm_recon_gather", t, images, n_images);
        ReconGather g;
        q_gather(t, X, pt_ok, images, n_images, X3 != nullptr, g);
        std::copy(g.off.begin(), g.off.end(), off);
        if (X3 && g.off[n_images] <= cap) {
            std::copy(g.X3.begin(), g.X3.end(), X3);
            std::copy(g.uv.begin(), g.uv.end(), uv);
            if (obs) std::copy(g.obs.begin(), g.obs.end(), obs);
        }
        return SFM_OK;
    });
}

extern "C" int sfm_recon_select(sfm_recon_tracks* t, const uint8_t* registered, const uint8_t* pt_ok, int32_t mode,
                                int32_t min_track_len, int64_t* n_pt_out, int64_t* n_obs_out, int64_t* pt_offsets,
                                int32_t* obs_img, double* obs_uv, int64_t* pt_map, int64_t* obs_map, int64_t cap_pt,
                                int64_t cap_obs) {
    return guarded([&] {
        SFM_REQUIRE(t && n_pt_out && n_obs_out && (t->n_img == 0 || registered) && (t->n_pt == 0 || pt_ok) &&
                        cap_pt >= 0 && cap_obs >= 0,
                    SFM_ERR_INVALID_ARG, "sfm_recon_select: null argument");
        SFM_REQUIRE(mode == SFM_RECON_NEW || mode == SFM_RECON_SOLVED, SFM_ERR_INVALID_ARG,
                    "sfm_recon_select: unknown mode %d", mode);
        SFM_REQUIRE(mode == SFM_RECON_NEW || min_track_len >= 1, SFM_ERR_INVALID_ARG,
                    "sfm_recon_select: min_track_len %d (must be >= 1)", min_track_len);
        const bool rows = pt_offsets || obs_img || obs_uv || pt_map || obs_map;
        ReconSelect s;
        q_select(t, registered, pt_ok, mode, min_track_len, rows, s);
        *n_pt_out = s.n_pt;
        *n_obs_out = s.n_obs;
        if (rows && s.n_pt <= cap_pt && s.n_obs <= cap_obs) {
            if (pt_offsets) std::copy(s.pt_offsets.begin(), s.pt_offsets.end(), pt_offsets);
            if (obs_img) std::copy(s.obs_img.begin(), s.obs_img.end(), obs_img);
            if (obs_uv) std::copy(s.obs_uv.begin(), s.obs_uv.end(), obs_uv);
            if (pt_map) std::copy(s.pt_map.begin(), s.pt_map.end(), pt_map);
            if (obs_map) std::copy(s.obs_map.begin(), s.obs_map.end(), obs_map);
        }
        return SFM_OK;
    });
}

// ---- the driver -------------------------------------------------------------------------
namespace {

struct HandleGuard {
    sfm_recon_tracks* t = nullptr;
    ~HandleGuard() { sfm_recon_tracks_destroy(t); }
};

struct Log {
    sfm_recon_round* rounds;
    int32_t cap_rounds;
    sfm_recon_cand* cands;
    int32_t cap_cands;
    int32_t n_rounds = 0, n_cands = 0;
    void cand(const sfm_recon_cand& c) {
        if (n_cands < cap_cands) cands[n_cands] = c;
        ++n_cands;
    }
    void round(const sfm_recon_round& r) {
        if (n_rounds < cap_rounds) rounds[n_rounds] = r;
        ++n_rounds;
    }
};

struct Lap {   // adds the time since its construction to *acc
    double* acc;
    double t0;
    explicit Lap(double* a) : acc(a), t0(seconds_now()) {}
    ~Lap() { *acc += seconds_now() - t0; }
};
enum { kSecPair = 0, kSecVisibility, kSecGather, kSecSelect, kSecResect, kSecTri, kSecSolve, kSecWash };

int reconstruct(const char* who, sfm_ctx* ctx, bool device, const sfm_ba_problem* prob, double* intr, const int32_t* wh,
                const int32_t* pairs, int64_t n_pairs, const sfm_recon_opts* opts, double* extr, double* X,
                uint8_t* registered, uint8_t* pt_ok, uint8_t* keep_obs, sfm_recon_round* rounds, int32_t cap_rounds,
                sfm_recon_cand* cands, int32_t cap_cands, sfm_recon_stats* stats) {
    return guarded([&] {
        // ---- every check, before any device call ----
        sfm_recon_opts O;
        if (opts) O = *opts; else sfm_recon_default_options(&O);
        SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
        recon_check_tracks(who, prob);
        const sfm_ba_problem& P = *prob;
        const int iw = sfm_ba_intr_width(P.camera_model);
        SFM_REQUIRE(iw > 0, SFM_ERR_INVALID_ARG, "%s: unknown camera_model %d", who, P.camera_model);
        SFM_REQUIRE(P.n_img >= 1 && P.n_intr >= 1 && P.img_intr && intr && wh && extr && registered, SFM_ERR_INVALID_ARG,
                    "%s: null argument", who);
        SFM_REQUIRE((P.n_pt == 0 || (X && pt_ok)) && (P.n_obs == 0 || keep_obs), SFM_ERR_INVALID_ARG,
                    "%s: null argument", who);
        for (int32_t i = 0; i < P.n_img; ++i) {
            SFM_REQUIRE(P.img_intr[i] >= 0 && P.img_intr[i] < P.n_intr, SFM_ERR_INVALID_ARG,
                        "%s: image %d names intrinsics block %d of %d", who, i, P.img_intr[i], P.n_intr);
            SFM_REQUIRE(wh[2 * i] > 0 && wh[2 * i + 1] > 0, SFM_ERR_INVALID_ARG, "%s: image %d has a non-positive size",
                        who, i);
        }
        SFM_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || pairs), SFM_ERR_INVALID_ARG, "%s: null pairs", who);
        for (int64_t q = 0; q < n_pairs; ++q)
            SFM_REQUIRE(pairs[2 * q] >= 0 && pairs[2 * q] < P.n_img && pairs[2 * q + 1] >= 0 &&
                            pairs[2 * q + 1] < P.n_img && pairs[2 * q] != pairs[2 * q + 1],
                        SFM_ERR_INVALID_ARG, "%s: pair %lld names an image out of range or twice", who, (long long)q);
        SFM_REQUIRE(cap_rounds >= 0 && cap_cands >= 0 && (cap_rounds == 0 || rounds) && (cap_cands == 0 || cands),
                    SFM_ERR_INVALID_ARG, "%s: bad log capacity", who);
        const bool forced = O.initial_pair[0] >= 0 || O.initial_pair[1] >= 0;
        SFM_REQUIRE(!forced || (O.initial_pair[0] >= 0 && O.initial_pair[0] < P.n_img && O.initial_pair[1] >= 0 &&
                                O.initial_pair[1] < P.n_img && O.initial_pair[0] != O.initial_pair[1]),
                    SFM_ERR_INVALID_ARG, "%s: initial_pair (%d, %d)", who, O.initial_pair[0], O.initial_pair[1]);
        SFM_REQUIRE(O.group_ratio > 0.0 && O.group_ratio <= 1.0 && O.max_adjust_repeats >= 1 && O.min_track_len >= 1 &&
                        O.pair_min_angle_deg == O.pair_min_angle_deg,
                    SFM_ERR_INVALID_ARG, "%s: bad options", who);
        // the stages' own option checks, so that none of them fails after device work
        SFM_REQUIRE(O.relpose.max_iterations >= 1 && O.relpose.precision == O.relpose.precision &&
                        O.relpose.front_ratio == O.relpose.front_ratio,
                    SFM_ERR_INVALID_ARG, "%s: bad relpose options", who);
        SFM_REQUIRE(O.resect.max_iterations >= 1 && O.resect.refine_iterations >= 0 &&
                        O.resect.precision == O.resect.precision,
                    SFM_ERR_INVALID_ARG, "%s: bad resect options", who);
        SFM_REQUIRE((O.tri.method == SFM_TRI_LINEAR || O.tri.method == SFM_TRI_ROBUST) && O.tri.min_track_len >= 2 &&
                        O.tri.max_hypotheses >= 1 && O.tri.max_residual_px == O.tri.max_residual_px &&
                        O.tri.min_angle_deg == O.tri.min_angle_deg,
                    SFM_ERR_INVALID_ARG, "%s: bad triangulation options", who);
        SFM_REQUIRE(O.wash.min_track_len >= 1, SFM_ERR_INVALID_ARG, "%s: bad wash options", who);
        SFM_REQUIRE(device || !O.adjust, SFM_ERR_UNSUPPORTED,
                    "%s: the library has no host bundle adjustment (adjust must be 0)", who);

        const double nan = std::numeric_limits<double>::quiet_NaN();
        std::fill(extr, extr + 6 * (size_t)P.n_img, 0.0);
        std::fill(registered, registered + P.n_img, (uint8_t)0);
        if (P.n_pt) {
            std::fill(X, X + 3 * (size_t)P.n_pt, nan);
            std::fill(pt_ok, pt_ok + P.n_pt, (uint8_t)0);
        }
        if (P.n_obs) std::fill(keep_obs, keep_obs + P.n_obs, (uint8_t)0);
        sfm_recon_stats st;
        std::memset(&st, 0, sizeof st);
        st.status = SFM_RECON_NO_INITIAL_PAIR;
        st.initial_pair[0] = st.initial_pair[1] = -1;
        Log log{rounds, cap_rounds, cands, cap_cands};
        auto finish = [&] {
            st.n_rounds = log.n_rounds;
            st.n_cands = log.n_cands;
            if (stats) *stats = st;
            return SFM_OK;
        };

        // ---- the initial pair ----
        std::vector<int32_t> plist;
        if (forced) plist = {O.initial_pair[0], O.initial_pair[1]};
        else plist.assign(pairs, pairs + 2 * n_pairs);
        const int64_t np = (int64_t)plist.size() / 2;
        if (np == 0) return finish();
        int64_t chosen = -1;
        std::vector<sfm_relpose_result> rel((size_t)np);
        std::vector<int64_t> off((size_t)np + 1, 0);
        {
            Lap lap(&st.seconds[kSecPair]);
            // a pair's correspondences: the tracks that hold both images, in track
            // order, each image at its first observation in the track
            std::unordered_map<int64_t, std::vector<int32_t>> by_key;
            for (int64_t q = 0; q < np; ++q) {
                const int64_t a = std::min(plist[2 * q], plist[2 * q + 1]), b = std::max(plist[2 * q], plist[2 * q + 1]);
                by_key[a * P.n_img + b].push_back((int32_t)q);
            }
            std::vector<std::vector<int64_t>> common((size_t)np);   // (observation of I, observation of J)
            std::vector<int64_t> first_of((size_t)P.n_img, -1);
            std::vector<std::pair<int32_t, int64_t>> firsts;
            for (int64_t p = 0; p < P.n_pt; ++p) {
                firsts.clear();
                for (int64_t o = P.pt_offsets[p]; o < P.pt_offsets[p + 1]; ++o) {
                    const int32_t im = P.obs_img[o];
                    if (first_of[im] == p) continue;
                    first_of[im] = p;
                    firsts.emplace_back(im, o);
                }
                for (size_t u = 0; u < firsts.size(); ++u)
                    for (size_t v = u + 1; v < firsts.size(); ++v) {
                        const bool swap = firsts[u].first > firsts[v].first;
                        const auto& lo = swap ? firsts[v] : firsts[u];
                        const auto& hi = swap ? firsts[u] : firsts[v];
                        const auto it = by_key.find((int64_t)lo.first * P.n_img + hi.first);
                        if (it == by_key.end()) continue;
                        for (int32_t q : it->second) {
                            const bool I_is_lo = plist[2 * q] == lo.first;
                            common[q].push_back(I_is_lo ? lo.second : hi.second);
                            common[q].push_back(I_is_lo ? hi.second : lo.second);
                        }
                    }
            }
            std::vector<double> xy;
            std::vector<int32_t> pair_intr((size_t)(2 * np)), wh4((size_t)(4 * np));
            for (int64_t q = 0; q < np; ++q) {
                for (size_t k = 0; k < common[q].size(); ++k) {
                    xy.push_back(P.obs_uv[2 * common[q][k]]);
                    xy.push_back(P.obs_uv[2 * common[q][k] + 1]);
                }
                off[(size_t)q + 1] = (int64_t)xy.size() / 4;
                for (int sd = 0; sd < 2; ++sd) {
                    const int32_t im = plist[2 * q + sd];
                    pair_intr[2 * q + sd] = P.img_intr[im];
                    wh4[4 * q + 2 * sd] = wh[2 * im];
                    wh4[4 * q + 2 * sd + 1] = wh[2 * im + 1];
                }
            }
            std::vector<int32_t> inl(xy.size() / 4 + 1, -1);
            xy.resize(xy.size() + 4, 0.0);   // (never empty)
#ifndef SFM_RECON_HOST_ONLY
            if (device)
                ok_or_throw(sfm_relpose(ctx, P.camera_model, np, off.data(), xy.data(), pair_intr.data(), intr, P.n_intr,
                                        wh4.data(), &O.relpose, rel.data(), inl.data()));
            else
#endif
                ok_or_throw(sfm_relpose_host(P.camera_model, np, off.data(), xy.data(), pair_intr.data(), intr, P.n_intr,
                                             wh4.data(), &O.relpose, rel.data(), inl.data()));
            chosen = forced ? (rel[0].status == SFM_RELPOSE_OK ? 0 : -1)
                            : relpose_best(rel.data(), np, O.pair_min_inliers, O.pair_min_angle_deg);
        }
        if (chosen < 0) return finish();
        const int32_t img_a = plist[2 * chosen], img_b = plist[2 * chosen + 1];
        st.status = SFM_RECON_OK;
        st.initial_pair[0] = img_a;
        st.initial_pair[1] = img_b;
        registered[img_a] = registered[img_b] = 1;
        std::copy(rel[chosen].pose, rel[chosen].pose + 6, extr + 6 * (size_t)img_b);

        HandleGuard hg;
        ok_or_throw(device ? sfm_recon_tracks_create(ctx, prob, &hg.t) : sfm_recon_tracks_create_host(prob, &hg.t));
        sfm_recon_tracks* T = hg.t;

        std::vector<int64_t> drop;
        // `points`: select(NEW) -> triangulation
        auto triangulate_new = [&](sfm_recon_round& R) {
            ReconSelect S;
            {
                Lap lap(&st.seconds[kSecSelect]);
                q_select(T, registered, pt_ok, SFM_RECON_NEW, 0, true, S);
            }
            if (S.n_pt == 0) return;
            Lap lap(&st.seconds[kSecTri]);
            sfm_ba_problem sub = P;
            sub.n_pt = S.n_pt; sub.n_obs = S.n_obs;
            sub.pt_offsets = S.pt_offsets.data(); sub.obs_img = S.obs_img.data(); sub.obs_uv = S.obs_uv.data();
            sub.const_img = -1;
            std::vector<double> Xs(3 * (size_t)S.n_pt);
            std::vector<uint8_t> status((size_t)S.n_pt), ko((size_t)S.n_obs);
#ifndef SFM_RECON_HOST_ONLY
            if (device)
                ok_or_throw(sfm_triangulate(ctx, &sub, extr, intr, &O.tri, Xs.data(), status.data(), ko.data(), nullptr,
                                            nullptr));
            else
#endif
                ok_or_throw(sfm_triangulate_host(&sub, extr, intr, &O.tri, Xs.data(), status.data(), ko.data(), nullptr,
                                                 nullptr));
            drop.clear();
            for (int64_t k = 0; k < S.n_pt; ++k) {
                if (status[k] != SFM_TRI_OK) continue;
                const int64_t p = S.pt_map[k];
                pt_ok[p] = 1;
                for (int a = 0; a < 3; ++a) X[3 * p + a] = Xs[3 * k + a];
                ++R.points_added;
                for (int64_t o = S.pt_offsets[k]; o < S.pt_offsets[k + 1]; ++o)
                    if (!ko[o]) drop.push_back(S.obs_map[o]);
            }
            R.obs_dropped += (int64_t)drop.size();
            q_drop(T, drop);
        };
        // `adjust`: select(SOLVED) -> solve -> wash, repeated; returns what the last wash took out
        auto adjust = [&](sfm_recon_round& R, int64_t repeat_above) -> int64_t {
            int64_t removed = 0;
#ifndef SFM_RECON_HOST_ONLY
            for (int32_t rep = 0; rep < O.max_adjust_repeats; ++rep) {
                ReconSelect S;
                {
                    Lap lap(&st.seconds[kSecSelect]);
                    q_select(T, registered, pt_ok, SFM_RECON_SOLVED, O.min_track_len, true, S);
                }
                removed = 0;
                if (S.n_pt == 0) break;
                sfm_ba_problem sub = P;
                sub.n_pt = S.n_pt; sub.n_obs = S.n_obs;
                sub.pt_offsets = S.pt_offsets.data(); sub.obs_img = S.obs_img.data(); sub.obs_uv = S.obs_uv.data();
                sub.const_img = img_a;
                std::vector<double> Xs(3 * (size_t)S.n_pt);
                for (int64_t k = 0; k < S.n_pt; ++k)
                    for (int a = 0; a < 3; ++a) Xs[3 * k + a] = X[3 * S.pt_map[k] + a];
                {
                    Lap lap(&st.seconds[kSecSolve]);
                    std::memset(&R.ba, 0, sizeof R.ba);
                    R.ba_rc = sfm_ba_solve(ctx, &sub, extr, intr, Xs.data(), &O.ba, &R.ba);
                    ++R.adjust_repeats;
                }
                if (R.ba_rc == SFM_ERR_SOLVER || R.ba_rc == SFM_ERR_NOT_FINITE) break;
                ok_or_throw(R.ba_rc);
                if (!R.ba.usable) break;
                for (int64_t k = 0; k < S.n_pt; ++k)
                    for (int a = 0; a < 3; ++a) X[3 * S.pt_map[k] + a] = Xs[3 * k + a];
                std::vector<uint8_t> ko((size_t)S.n_obs), kp((size_t)S.n_pt);
                {
                    Lap lap(&st.seconds[kSecWash]);
                    ok_or_throw(sfm_ba_wash(ctx, &sub, extr, intr, Xs.data(), &O.wash, nullptr, nullptr, ko.data(),
                                            kp.data(), &R.wash));
                }
                removed = S.n_obs - R.wash.n_obs_kept;
                drop.clear();
                for (int64_t k = 0; k < S.n_pt; ++k) {
                    const int64_t p = S.pt_map[k];
                    if (!kp[k]) {
                        pt_ok[p] = 0;
                        for (int a = 0; a < 3; ++a) X[3 * p + a] = nan;
                        ++R.points_removed;
                        continue;
                    }
                    for (int64_t o = S.pt_offsets[k]; o < S.pt_offsets[k + 1]; ++o)
                        if (!ko[o]) drop.push_back(S.obs_map[o]);
                }
                R.obs_dropped += (int64_t)drop.size();
                q_drop(T, drop);
                if (removed <= repeat_above) break;
            }
#endif
            return removed;
        };

        // round 0: the pair
        {
            sfm_recon_round R;
            std::memset(&R, 0, sizeof R);
            R.first_cand = log.n_cands;
            R.n_cand = 2;
            R.n_registered = 2;
            const int32_t n_common = (int32_t)(off[(size_t)chosen + 1] - off[chosen]);
            log.cand(sfm_recon_cand{0, img_a, n_common, rel[chosen].status, rel[chosen].n_inliers, 0});
            log.cand(sfm_recon_cand{0, img_b, n_common, rel[chosen].status, rel[chosen].n_inliers, 0});
            triangulate_new(R);
            log.round(R);
        }

        // ---- the rounds ----
        std::vector<uint8_t> tried((size_t)P.n_img, 0);
        std::vector<int32_t> count((size_t)P.n_img), cand;
        for (;;) {
            {
                Lap lap(&st.seconds[kSecVisibility]);
                q_visibility(T, pt_ok, count.data());
            }
            int32_t best = 0;
            for (int32_t i = 0; i < P.n_img; ++i)
                if (!registered[i] && !tried[i]) best = std::max(best, count[i]);
            if (best == 0) break;
            cand.clear();
            for (int32_t i = 0; i < P.n_img; ++i)
                if (!registered[i] && !tried[i] && count[i] > 0 && (double)count[i] >= O.group_ratio * (double)best)
                    cand.push_back(i);
            const int32_t nc = (int32_t)cand.size();
            ReconGather G;
            {
                Lap lap(&st.seconds[kSecGather]);
                q_gather(T, X, pt_ok, cand.data(), nc, true, G);
            }
            std::vector<int32_t> c_intr((size_t)nc), c_wh((size_t)(2 * nc));
            for (int32_t q = 0; q < nc; ++q) {
                c_intr[q] = P.img_intr[cand[q]];
                c_wh[2 * q] = wh[2 * cand[q]];
                c_wh[2 * q + 1] = wh[2 * cand[q] + 1];
            }
            std::vector<sfm_resect_result> res((size_t)nc);
            std::vector<int32_t> inl((size_t)std::max<int64_t>(G.off[nc], 1), -1);
            {
                Lap lap(&st.seconds[kSecResect]);
#ifndef SFM_RECON_HOST_ONLY
                if (device)
                    ok_or_throw(sfm_resect(ctx, P.camera_model, nc, G.off.data(), G.X3.data(), G.uv.data(), c_intr.data(),
                                           intr, P.n_intr, c_wh.data(), &O.resect, res.data(), inl.data()));
                else
#endif
                    ok_or_throw(sfm_resect_host(P.camera_model, nc, G.off.data(), G.X3.data(), G.uv.data(), c_intr.data(),
                                                intr, P.n_intr, c_wh.data(), &O.resect, res.data(), inl.data()));
            }
            sfm_recon_round R;
            std::memset(&R, 0, sizeof R);
            R.first_cand = log.n_cands;
            R.n_cand = nc;
            drop.clear();
            for (int32_t q = 0; q < nc; ++q) {
                const int32_t im = cand[q];
                tried[im] = 1;
                log.cand(sfm_recon_cand{log.n_rounds, im, count[im], res[q].status, res[q].n_inliers, 0});
                if (res[q].status != SFM_RESECT_OK) continue;
                registered[im] = 1;
                std::copy(res[q].pose, res[q].pose + 6, extr + 6 * (size_t)im);
                ++R.n_registered;
                // the engine adds the resection's inliers to the landmarks, nothing else of the image
                std::vector<uint8_t> is_inl((size_t)(G.off[(size_t)q + 1] - G.off[q]), 0);
                for (int32_t k = 0; k < res[q].n_inliers; ++k) is_inl[inl[G.off[q] + k]] = 1;
                for (size_t k = 0; k < is_inl.size(); ++k)
                    if (!is_inl[k]) drop.push_back(G.obs[G.off[q] + k]);
            }
            R.obs_dropped += (int64_t)drop.size();
            q_drop(T, drop);
            if (R.n_registered) {
                triangulate_new(R);
                if (O.adjust) adjust(R, O.wash_repeat_above);
            }
            log.round(R);
        }
        // ---- the end ----
        if (O.adjust) st.final_removed = adjust(st.final_adjust, 0);

        for (int32_t i = 0; i < P.n_img; ++i) st.n_registered += registered[i] != 0;
        if (P.n_obs) {
            // the alive flags live in the handle: ask it for everything registered and solved
            ReconSelect S;
            q_select(T, registered, pt_ok, SFM_RECON_SOLVED, 1, true, S);
            for (int64_t o : S.obs_map) keep_obs[o] = 1;
            st.n_obs_kept = S.n_obs;
        }
        for (int64_t p = 0; p < P.n_pt; ++p) st.n_points += pt_ok[p] != 0;
        return finish();
    });
}

}  // namespace

extern "C" int sfm_reconstruct_host(const sfm_ba_problem* tracks, double* intr, const int32_t* wh, const int32_t* pairs,
                                    int64_t n_pairs, const sfm_recon_opts* opts, double* extr, double* X,
                                    uint8_t* registered, uint8_t* pt_ok, uint8_t* keep_obs, sfm_recon_round* rounds,
                                    int32_t cap_rounds, sfm_recon_cand* cands, int32_t cap_cands,
                                    sfm_recon_stats* stats) {
    return reconstruct("sfm_reconstruct_host", nullptr, false, tracks, intr, wh, pairs, n_pairs, opts, extr, X,
                       registered, pt_ok, keep_obs, rounds, cap_rounds, cands, cap_cands, stats);
}

#ifndef SFM_RECON_HOST_ONLY
extern "C" int sfm_reconstruct(sfm_ctx* ctx, const sfm_ba_problem* tracks, double* intr, const int32_t* wh,
                               const int32_t* pairs, int64_t n_pairs, const sfm_recon_opts* opts, double* extr,
                               double* X, uint8_t* registered, uint8_t* pt_ok, uint8_t* keep_obs,
                               sfm_recon_round* rounds, int32_t cap_rounds, sfm_recon_cand* cands, int32_t cap_cands,
                               sfm_recon_stats* stats) {
    return reconstruct("sfm_reconstruct", ctx, true, tracks, intr, wh, pairs, n_pairs, opts, extr, X, registered,
                       pt_ok, keep_obs, rounds, cap_rounds, cands, cap_cands, stats);
}

// sparseBuilder::reconstruction(), file-staged: the scene in memory, shared by
// sfm_sparse_reconstruct and sfm_sparse_reconstruct_colorize
namespace {

struct SparseScene {
    int32_t n_img = 0;
    std::vector<int64_t> pt_off;
    std::vector<int32_t> obs_img, img_intr, wh;
    std::vector<double> obs_uv, intr, extr, X;
    std::vector<uint8_t> reg, pt_ok, keep;
    sfm_ba_problem P;
    sfm_recon_stats st;
    std::string out_dir;   // with its trailing '/'
};

// before_device(n_img): the caller's remaining argument checks, run once the
// number of views is known and before any device call
template <class Check>
void sparse_scene(const char* who, sfm_ctx* ctx, const char* matches_dir, const char* out_dir, double focal,
                  const sfm_recon_opts* opts, const Check& before_device, SparseScene& sc) {
    SFM_REQUIRE(ctx && matches_dir && out_dir, SFM_ERR_INVALID_ARG, "%s: null argument", who);
    std::string dir(matches_dir);
    sc.out_dir = out_dir;
    if (!dir.empty() && dir.back() != '/') dir += '/';
    if (!sc.out_dir.empty() && sc.out_dir.back() != '/') sc.out_dir += '/';
    const std::string data = dir + "sfm_data.json";
    int32_t n_img = 0;
    ok_or_throw(sfm_mvg_load_views(data.c_str(), nullptr, 0, &n_img));
    SFM_REQUIRE(n_img >= 2, SFM_ERR_INVALID_ARG, "%s: %d views", who, n_img);
    before_device(n_img);
    std::vector<sfm_mvg_view> views((size_t)n_img);
    ok_or_throw(sfm_mvg_load_views(data.c_str(), views.data(), n_img, &n_img));
    std::map<uint32_t, int32_t> slot;
    for (int32_t k = 0; k < n_img; ++k) slot[views[k].id_view] = k;
    // the candidate pairs: those of the matches file
    const std::string mpath = dir + "matches.f.bin";
    int64_t np = 0, nm = 0;
    ok_or_throw(sfm_mvg_load_matches(mpath.c_str(), nullptr, nullptr, nullptr, nullptr, 0, 0, &np, &nm));
    std::vector<int32_t> pairs(2 * (size_t)std::max<int64_t>(np, 1));
    ok_or_throw(sfm_mvg_load_matches(mpath.c_str(), pairs.data(), nullptr, nullptr, nullptr, np, nm, &np, &nm));
    for (int64_t k = 0; k < 2 * np; ++k) {
        const auto it = slot.find((uint32_t)pairs[k]);
        SFM_REQUIRE(it != slot.end(), SFM_ERR_INVALID_ARG, "%s: a match names view %d", who, pairs[k]);
        pairs[k] = it->second;
    }
    // the tracks
    struct TracksGuard {
        sfm_tracks* t = nullptr;
        ~TracksGuard() { sfm_tracks_destroy(t); }
    } tg;
    ok_or_throw(sfm_sparse_tracks(ctx, matches_dir, nullptr, nullptr, &tg.t));
    sfm_tracks_stats ts;
    ok_or_throw(sfm_tracks_get_stats(tg.t, &ts));
    sc.pt_off.resize((size_t)ts.n_tracks + 1);
    sc.obs_img.resize((size_t)std::max<int64_t>(ts.n_obs, 1));
    sc.obs_uv.resize(2 * (size_t)std::max<int64_t>(ts.n_obs, 1));
    ok_or_throw(sfm_tracks_fetch(tg.t, sc.pt_off.data(), sc.obs_img.data(), nullptr, sc.obs_uv.data()));
    // PINHOLE_CAMERA_RADIAL3, one block per view, no distortion as the initial guess
    sc.n_img = n_img;
    sc.img_intr.resize((size_t)n_img);
    sc.wh.resize(2 * (size_t)n_img);
    sc.intr.assign(6 * (size_t)n_img, 0.0);
    for (int32_t k = 0; k < n_img; ++k) {
        const double w = views[k].width, h = views[k].height;
        sc.img_intr[k] = k;
        sc.wh[2 * k] = (int32_t)views[k].width;
        sc.wh[2 * k + 1] = (int32_t)views[k].height;
        sc.intr[6 * k] = focal > 0.0 ? focal : 1.2 * std::max(w, h);
        sc.intr[6 * k + 1] = 0.5 * w;
        sc.intr[6 * k + 2] = 0.5 * h;
    }
    sfm_ba_problem& P = sc.P;
    std::memset(&P, 0, sizeof P);
    P.n_img = n_img; P.n_intr = n_img; P.n_pt = ts.n_tracks; P.n_obs = ts.n_obs;
    P.pt_offsets = sc.pt_off.data(); P.obs_img = sc.obs_img.data(); P.obs_uv = sc.obs_uv.data();
    P.img_intr = sc.img_intr.data();
    P.const_img = -1; P.camera_model = SFM_CAM_RADIAL3; P.huber_a = 4.0;
    sc.extr.resize(6 * (size_t)n_img);
    sc.X.resize(3 * (size_t)std::max<int64_t>(P.n_pt, 1));
    sc.reg.resize((size_t)n_img);
    sc.pt_ok.resize((size_t)std::max<int64_t>(P.n_pt, 1));
    sc.keep.resize((size_t)std::max<int64_t>(P.n_obs, 1));
    ok_or_throw(sfm_reconstruct(ctx, &P, sc.intr.data(), sc.wh.data(), pairs.data(), np, opts, sc.extr.data(),
                                sc.X.data(), sc.reg.data(), sc.pt_ok.data(), sc.keep.data(), nullptr, 0, nullptr, 0,
                                &sc.st));
    // cloud_and_poses.ply: the points in white, then the camera centres C = -R' t in green
    write_ply(who, (sc.out_dir + "cloud_and_poses.ply").c_str(), P.n_pt, sc.X.data(), sc.pt_ok.data(), nullptr, n_img,
              sc.extr.data(), sc.reg.data());
}

}  // namespace

extern "C" int sfm_sparse_reconstruct(sfm_ctx* ctx, const char* matches_dir, const char* out_dir, double focal,
                                      const sfm_recon_opts* opts, sfm_recon_stats* stats) {
    return guarded([&] {
        SparseScene sc;
        sparse_scene("sfm_sparse_reconstruct", ctx, matches_dir, out_dir, focal, opts, [](int32_t) {}, sc);
        if (stats) *stats = sc.st;
        return SFM_OK;
    });
}

// sparseBuilder::reconstruction() + colorize(), file-staged
extern "C" int sfm_sparse_reconstruct_colorize(sfm_ctx* ctx, const char* matches_dir, const char* out_dir,
                                               double focal, const sfm_recon_opts* opts, const int32_t* channels,
                                               const int64_t* img_off, const uint8_t* pixels,
                                               sfm_recon_stats* recon_stats, sfm_colorize_stats* color_stats) {
    return guarded([&] {
        const char* who = "sfm_sparse_reconstruct_colorize";
        SparseScene sc;
        sparse_scene(who, ctx, matches_dir, out_dir, focal, opts, [&](int32_t n_img) {
            SFM_REQUIRE(channels && img_off, SFM_ERR_INVALID_ARG, "%s: null argument", who);
            for (int32_t i = 0; i < n_img; ++i)
                SFM_REQUIRE(img_off[i] < 0 || (pixels && (channels[i] == 1 || channels[i] == 3)), SFM_ERR_INVALID_ARG,
                            "%s: image %d has %d channels, or no pixels", who, i, channels[i]);
        }, sc);
        if (recon_stats) *recon_stats = sc.st;
        std::vector<uint8_t> rgb(3 * (size_t)std::max<int64_t>(sc.P.n_pt, 1));
        ok_or_throw(sfm_colorize(ctx, &sc.P, sc.wh.data(), sc.pt_ok.data(), sc.keep.data(), channels, img_off, pixels,
                                 rgb.data(), nullptr, color_stats));
        write_ply(who, (sc.out_dir + "colorized.ply").c_str(), sc.P.n_pt, sc.X.data(), sc.pt_ok.data(), rgb.data(),
                  sc.n_img, sc.extr.data(), sc.reg.data());
        return SFM_OK;
    });
}
#endif
