// Dense depth maps, host side (include/sfmcore.h, "Dense depth maps"): the
// argument checks, view selection, the per-pair matrices (in double, rounded
// once), the host twins of the estimation and of the filter (threads over rows;
// a colour pass ends before the next begins), and the entry points over either
// backend.  The kernels and the transfers are depthmap.hip's.
// SFM_DEPTHMAP_HOST_ONLY leaves the device entry points out, so that the host
// twins build with a plain host compiler (tests/cpp/depthmap_test.cpp).
#pragma clang fp contract(off)

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "depthmap.h"

using namespace sfm;

namespace sfm {

static void mul33(const double* a, const double* b, double* o) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[3 * r + c] = a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + a[3 * r + 2] * b[6 + c];
}
static bool inv33(const double* m, double* o) {
    const double c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c0 + m[1] * c1 + m[2] * c2;
    if (!std::isfinite(det) || det == 0.0) return false;
    o[0] = c0 / det;
    o[1] = (m[2] * m[7] - m[1] * m[8]) / det;
    o[2] = (m[1] * m[5] - m[2] * m[4]) / det;
    o[3] = c1 / det;
    o[4] = (m[0] * m[8] - m[2] * m[6]) / det;
    o[5] = (m[2] * m[3] - m[0] * m[5]) / det;
    o[6] = c2 / det;
    o[7] = (m[1] * m[6] - m[0] * m[7]) / det;
    o[8] = (m[0] * m[4] - m[1] * m[3]) / det;
    return true;
}

// A = K_j R_j R_i' K_i^-1, b = K_j R_j (C_i - C_j): in double, rounded once
void depth_pair_matrices(const DepthCameras& m, int32_t i, int32_t j, float* A_out, float* b_out) {
    double Kinv[9] = {}, Rt[9], KR[9], T[9], A[9];
    inv33(m.K + 9 * i, Kinv);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rt[3 * r + c] = m.R[9 * i + 3 * c + r];
    mul33(m.K + 9 * j, m.R + 9 * j, KR);
    mul33(KR, Rt, T);
    mul33(T, Kinv, A);
    const double dc[3] = {m.C[3 * i] - m.C[3 * j], m.C[3 * i + 1] - m.C[3 * j + 1], m.C[3 * i + 2] - m.C[3 * j + 2]};
    for (int a = 0; a < 9; ++a) A_out[a] = (float)A[a];
    for (int r = 0; r < 3; ++r) b_out[r] = (float)(KR[3 * r] * dc[0] + KR[3 * r + 1] * dc[1] + KR[3 * r + 2] * dc[2]);
}

// The checks that the estimation and the filter share, and the views and pairs
// of the call.  channels / img_off / drange NULL: the filter (every image counts
// as loaded, no ranges).
void depth_build_problem(const char* who, const DepthCameras& m, const int32_t* channels, const int64_t* img_off,
                   const uint8_t* pixels, const float* drange, DepthProblem& P) {
    SFM_REQUIRE(m.n_img >= 0, SFM_ERR_INVALID_ARG, "%s: negative n_img", who);
    P.n_img = m.n_img;
    if (m.n_img == 0) return;
    SFM_REQUIRE(m.n_img <= 65535, SFM_ERR_UNSUPPORTED, "%s: more than 65535 images in one call", who);
    SFM_REQUIRE(m.wh && m.K && m.R && m.C && m.nb_off, SFM_ERR_INVALID_ARG, "%s: null argument", who);
    SFM_REQUIRE(m.nb_off[0] == 0, SFM_ERR_INVALID_ARG, "%s: nb_off[0] is %lld, not 0", who, (long long)m.nb_off[0]);
    std::vector<double> Kinv((size_t)9 * m.n_img, 0.0);
    P.views.resize((size_t)m.n_img);
    int64_t gray_bytes = 0;
    // This stage's checks of image i run before the shared ones of image i + 1, as they always did: a
    // later image of 2^31 pixels (SFM_ERR_UNSUPPORTED) does not hide an earlier SFM_ERR_INVALID_ARG.
    // channels come with img_off (depth_prepare checks it); without pixels the first loaded image fails.
    DenseImages D;
    dense_images_prepare(who, m.n_img, m.wh, channels, img_off, channels ? pixels : nullptr, m.K, m.R, m.C, D, [&](int32_t i) {
        const int32_t w = D.img[(size_t)i].w, h = D.img[(size_t)i].h;
        const int64_t n_nb = m.nb_off[i + 1] - m.nb_off[i];
        SFM_REQUIRE(n_nb >= 0, SFM_ERR_INVALID_ARG, "%s: nb_off decreases at image %d", who, i);
        SFM_REQUIRE(n_nb <= kDepthMaxNeighbors, SFM_ERR_INVALID_ARG, "%s: image %d has %lld neighbours, more than %d", who,
                    i, (long long)n_nb, kDepthMaxNeighbors);
        SFM_REQUIRE(n_nb == 0 || m.nb_view, SFM_ERR_INVALID_ARG, "%s: null nb_view", who);
        const bool loaded = !img_off || img_off[i] >= 0;
        SFM_REQUIRE(!(loaded && channels) || pixels, SFM_ERR_INVALID_ARG, "%s: null pixels", who);
        SFM_REQUIRE(inv33(m.K + 9 * i, &Kinv[9 * (size_t)i]), SFM_ERR_INVALID_ARG, "%s: K of image %d is singular", who, i);
        DepthView& V = P.views[(size_t)i];
        std::memset(&V, 0, sizeof V);
        for (int a = 0; a < 9; ++a) V.Ki[a] = (float)Kinv[9 * (size_t)i + a];
        V.w = w;
        V.h = h;
        V.nb0 = (int32_t)m.nb_off[i];
        V.nb1 = (int32_t)m.nb_off[i + 1];
        V.active = loaded && n_nb > 0;
        V.map_off = D.img[(size_t)i].map_off;
        V.gray_off = -1;
        if (loaded && channels) {
            V.gray_off = gray_bytes;
            gray_bytes += depth_align_image((int64_t)w * h);
        }
        if (drange && n_nb > 0) {
            const float lo = drange[2 * i], hi = drange[2 * i + 1];
            SFM_REQUIRE(lo > 0.0f && lo < hi && std::isfinite(hi), SFM_ERR_INVALID_ARG,
                        "%s: image %d has the depth range [%g, %g], not 0 < d_min < d_max", who, i, (double)lo, (double)hi);
            V.dmin = lo;
            V.dmax = hi;
            V.imin = 1.0f / hi;
            V.imax = 1.0f / lo;
        }
        if (V.active) {
            P.max_w = std::max(P.max_w, w);
            P.max_h = std::max(P.max_h, h);
        }
    });
    P.n_map = D.n_map;
    P.pairs.resize((size_t)m.nb_off[m.n_img]);
    for (int32_t i = 0; i < m.n_img; ++i)
        for (int64_t q = m.nb_off[i]; q < m.nb_off[i + 1]; ++q) {
            const int32_t j = m.nb_view[q];
            SFM_REQUIRE(j >= 0 && j < m.n_img && j != i, SFM_ERR_INVALID_ARG,
                        "%s: image %d names the neighbour %d (of %d images, itself excluded)", who, i, j, m.n_img);
            DepthPair& Q = P.pairs[(size_t)q];
            std::memset(&Q, 0, sizeof Q);
            depth_pair_matrices(m, i, j, Q.A, Q.b);
            const DepthView& J = P.views[(size_t)j];
            Q.view = j;
            Q.w = J.w;
            Q.h = J.h;
            Q.loaded = !channels || J.gray_off >= 0;
            Q.gray_off = std::max<int64_t>(J.gray_off, 0);
            Q.map_off = J.map_off;
        }
    if (!channels) return;
    // the gray pool: (77 r + 150 g + 29 b + 128) >> 8, or the byte of a 1-channel image
    P.gray.assign((size_t)std::max<int64_t>(gray_bytes, 1), 0);
    std::vector<int32_t> loaded;
    for (int32_t i = 0; i < m.n_img; ++i)
        if (P.views[(size_t)i].gray_off >= 0) loaded.push_back(i);
    dense_parallel_for(loaded.size(), [&](size_t at) {
        const int32_t i = loaded[at];
        const DepthView& V = P.views[(size_t)i];
        const uint8_t* src = pixels + img_off[i];
        uint8_t* dst = P.gray.data() + V.gray_off;
        const int64_t n = (int64_t)V.w * V.h;
        if (channels[i] == 1) {
            std::memcpy(dst, src, (size_t)n);
            return;
        }
        for (int64_t p = 0; p < n; ++p)
            dst[p] = (uint8_t)((77u * src[3 * p] + 150u * src[3 * p + 1] + 29u * src[3 * p + 2] + 128u) >> 8);
    });
}

// sfm_depthmap's checks (all but the output pointers), and what the call works on
void depth_prepare(const char* who, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                   const uint8_t* pixels, const double* K, const double* R, const double* C, const int64_t* nb_off,
                   const int32_t* nb_view, const float* drange, const float* init_depth, const float* init_normal,
                   const sfm_depthmap_opts* opts, DepthCall& call) {
    sfm_depthmap_opts o;
    sfm_depthmap_default_options(&o);
    if (opts) o = *opts;
    SFM_REQUIRE(o.half_window >= 1 && o.half_window <= kDepthMaxHalfWindow, SFM_ERR_INVALID_ARG,
                "%s: half_window %d is outside 1..%d", who, o.half_window, kDepthMaxHalfWindow);
    SFM_REQUIRE(o.iterations >= 0 && o.iterations <= kDepthMaxIterations, SFM_ERR_INVALID_ARG,
                "%s: iterations %d is outside 0..%d", who, o.iterations, kDepthMaxIterations);
    SFM_REQUIRE(o.n_best >= 1, SFM_ERR_INVALID_ARG, "%s: n_best %d is not positive", who, o.n_best);
    SFM_REQUIRE(o.device_bytes >= 0, SFM_ERR_INVALID_ARG, "%s: negative device_bytes", who);
    SFM_REQUIRE(n_img <= 0 || (channels && img_off && drange), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    SFM_REQUIRE(!init_depth == !init_normal, SFM_ERR_INVALID_ARG, "%s: init_depth and init_normal go together", who);
    DepthProblem& P = call.P;
    depth_build_problem(who, DepthCameras{n_img, wh, K, R, C, nb_off, nb_view}, channels, img_off, pixels, drange, P);
    sfm_depthmap_stats& st = call.st;
    std::memset(&st, 0, sizeof st);
    for (const DepthView& V : P.views) st.n_images += V.active;
    // what the device holds: the gray pool, the five floats of every map pixel, the views and pairs
    st.resident_bytes = (int64_t)P.gray.size() + 5 * (int64_t)sizeof(float) * P.n_map +
                        (int64_t)(P.views.size() * sizeof(DepthView) + P.pairs.size() * sizeof(DepthPair));
    const int64_t budget = o.device_bytes > 0 ? o.device_bytes : kDepthDefaultDeviceBytes;
    SFM_REQUIRE(st.resident_bytes <= budget, SFM_ERR_UNSUPPORTED,
                "%s: the images and maps need %lld resident bytes, device_bytes is %lld (streaming is not built)", who,
                (long long)st.resident_bytes, (long long)budget);
    call.prm = DepthParams{o.half_window, o.iterations, o.n_best, 0, o.seed};
}

// sfm_depthmap_filter's option check
void depth_filter_prepare(const char* who, const sfm_depthmap_filter_opts* opts, DepthFilterParams& prm) {
    sfm_depthmap_filter_opts o;
    sfm_depthmap_filter_default_options(&o);
    if (opts) o = *opts;
    SFM_REQUIRE(o.max_cost >= 0.0f && o.rel_tol >= 0.0f && o.min_consistent >= 0, SFM_ERR_INVALID_ARG,
                "%s: max_cost, rel_tol or min_consistent is negative or not a number", who);
    prm = DepthFilterParams{o.max_cost, o.rel_tol, o.min_consistent, 0};
}

// the initial state of the maps on the host: images without maps of their own
// are all zero; the others start from the caller's planes
void depth_init_maps(const DepthProblem& P, const float* init_depth, const float* init_normal, float* depth,
                     float* normal, float* cost) {
    for (const DepthView& V : P.views) {
        const size_t n = (size_t)V.w * V.h, at = (size_t)V.map_off;
        if (V.active && init_depth) {
            std::memmove(depth + at, init_depth + at, n * sizeof(float));
            std::memmove(normal + 3 * at, init_normal + 3 * at, 3 * n * sizeof(float));
        } else if (!V.active) {
            std::memset(depth + at, 0, n * sizeof(float));
            std::memset(normal + 3 * at, 0, 3 * n * sizeof(float));
            if (cost) std::memset(cost + at, 0, n * sizeof(float));
        }
    }
}

}  // namespace sfm

namespace {

// rows of the active images, one item each
struct RowItem {
    int32_t img, y;
};
std::vector<RowItem> rows_of(const DepthProblem& P, bool active_only) {
    std::vector<RowItem> items;
    for (int32_t i = 0; i < P.n_img; ++i) {
        if (active_only && !P.views[(size_t)i].active) continue;
        for (int32_t y = 0; y < P.views[(size_t)i].h; ++y) items.push_back(RowItem{i, y});
    }
    return items;
}

void depthmap_host(const DepthProblem& P, const DepthParams& prm, bool init_given, float* depth, float* normal,
                   float* cost, int64_t* n_estimated, int64_t* n_invalid) {
    const std::vector<RowItem> items = rows_of(P, true);
    const DepthPair* pairs = P.pairs.data();
    const uint8_t* gray = P.gray.data();
    auto maps = [&](const DepthView& V, float*& d, float*& n, float*& c) {
        d = depth + V.map_off;
        n = normal + 3 * V.map_off;
        c = cost + V.map_off;
    };
    dense_parallel_for(items.size(), [&](size_t at) {
        const DepthView& V = P.views[(size_t)items[at].img];
        const DepthRef ref{gray + V.gray_off, V.w, 0, 0};
        const int32_t y = items[at].y;
        float *d, *n, *c;
        maps(V, d, n, c);
        for (int32_t x = 0; x < V.w; ++x) {
            const int64_t idx = (int64_t)y * V.w + x;
            if (depth_estimated(V, prm.r, x, y)) {
                depth_init_pixel(V, pairs, gray, ref, prm, init_given, items[at].img, x, y, d, n, c);
            } else {
                d[idx] = 0.0f;
                n[3 * idx] = n[3 * idx + 1] = n[3 * idx + 2] = 0.0f;
                c[idx] = kDepthWorstCost;
            }
        }
    });
    for (int32_t it = 0; it < prm.iterations; ++it)
        for (int32_t colour = 0; colour < 2; ++colour)
            dense_parallel_for(items.size(), [&](size_t at) {
                const DepthView& V = P.views[(size_t)items[at].img];
                const DepthRef ref{gray + V.gray_off, V.w, 0, 0};
                const int32_t y = items[at].y;
                if (y < prm.r || y >= V.h - prm.r) return;
                float *d, *n, *c;
                maps(V, d, n, c);
                for (int32_t x = prm.r + ((prm.r + y + colour) & 1); x < V.w - prm.r; x += 2)
                    depth_update_pixel(V, pairs, gray, ref, prm, it, items[at].img, x, y, d, n, c);
            });
    int64_t est = 0, inv = 0;
    for (const RowItem& item : items) {
        const DepthView& V = P.views[(size_t)item.img];
        for (int32_t x = 0; x < V.w; ++x)
            if (depth_estimated(V, prm.r, x, item.y)) {
                ++est;
                inv += cost[V.map_off + (int64_t)item.y * V.w + x] >= kDepthWorstCost;
            }
    }
    *n_estimated = est;
    *n_invalid = inv;
}

void filter_host(const DepthProblem& P, const DepthFilterParams& prm, const float* depth, const float* cost,
                 float* depth_out, uint8_t* n_agree, int64_t* counts) {
    const std::vector<RowItem> items = rows_of(P, false);
    std::vector<std::atomic<int64_t>> acc((size_t)2 * P.n_img);
    for (auto& a : acc) a = 0;
    dense_parallel_for(items.size(), [&](size_t at) {
        const int32_t i = items[at].img, y = items[at].y;
        const DepthView& V = P.views[(size_t)i];
        const int32_t need = std::min(prm.min_consistent, V.nb1 - V.nb0);
        int64_t cand = 0, kept = 0;
        for (int32_t x = 0; x < V.w; ++x) {
            const int64_t idx = V.map_off + (int64_t)y * V.w + x;
            const int32_t a = depth_filter_pixel(V, P.pairs.data(), prm, x, y, depth, cost);
            const bool keep = a >= 0 && a >= need;
            cand += a >= 0;
            kept += keep;
            depth_out[idx] = keep ? depth[idx] : 0.0f;
            n_agree[idx] = (uint8_t)(a > 0 ? a : 0);
        }
        acc[(size_t)2 * i] += cand;
        acc[(size_t)2 * i + 1] += kept;
    });
    for (size_t k = 0; k < acc.size(); ++k) counts[k] = acc[k];
}

int depthmap(const char* who, sfm_ctx* ctx, bool device, int32_t n_img, const int32_t* wh, const int32_t* channels,
             const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R, const double* C,
             const int64_t* nb_off, const int32_t* nb_view, const float* drange, const float* init_depth,
             const float* init_normal, const sfm_depthmap_opts* opts, float* depth, float* normal, float* cost,
             sfm_depthmap_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    DepthCall call;
    depth_prepare(who, n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange, init_depth, init_normal,
                  opts, call);
    const DepthProblem& P = call.P;
    const DepthParams& prm = call.prm;
    sfm_depthmap_stats& st = call.st;
    SFM_REQUIRE(P.n_map == 0 || (depth && normal && cost), SFM_ERR_INVALID_ARG, "%s: null output", who);
    if (P.n_map > 0) depth_init_maps(P, init_depth, init_normal, depth, normal, cost);
    if (st.n_images > 0) {
        if (device) {
#ifndef SFM_DEPTHMAP_HOST_ONLY
            depthmap_device(ctx, P, prm, init_depth != nullptr, depth, normal, cost, &st.n_estimated, &st.n_invalid,
                            st.seconds);
#endif
        } else {
            const double t0 = seconds_now();
            depthmap_host(P, prm, init_depth != nullptr, depth, normal, cost, &st.n_estimated, &st.n_invalid);
            st.seconds[1] = seconds_now() - t0;
        }
    }
    if (stats) *stats = st;
    return SFM_OK;
}

int depthmap_filter(const char* who, sfm_ctx* ctx, bool device, int32_t n_img, const int32_t* wh, const double* K,
                    const double* R, const double* C, const int64_t* nb_off, const int32_t* nb_view, const float* depth,
                    const float* cost, const sfm_depthmap_filter_opts* opts, float* depth_out, uint8_t* n_agree,
                    int64_t* counts, sfm_depthmap_filter_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    DepthFilterParams prm;
    depth_filter_prepare(who, opts, prm);
    DepthProblem P;
    depth_build_problem(who, DepthCameras{n_img, wh, K, R, C, nb_off, nb_view}, nullptr, nullptr, nullptr, nullptr, P);
    SFM_REQUIRE(P.n_map == 0 || (depth && cost && depth_out && n_agree), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    sfm_depthmap_filter_stats st;
    std::memset(&st, 0, sizeof st);
    std::vector<int64_t> cnt((size_t)2 * std::max(n_img, 1), 0);
    if (P.n_map > 0) {
        if (device) {
#ifndef SFM_DEPTHMAP_HOST_ONLY
            depthmap_filter_device(ctx, P, prm, depth, cost, depth_out, n_agree, cnt.data(), st.seconds);
#endif
        } else {
            const double t0 = seconds_now();
            filter_host(P, prm, depth, cost, depth_out, n_agree, cnt.data());
            st.seconds[1] = seconds_now() - t0;
        }
    }
    for (int32_t i = 0; i < n_img; ++i) {
        st.n_candidates += cnt[(size_t)2 * i];
        st.n_kept += cnt[(size_t)2 * i + 1];
    }
    if (counts && n_img > 0) std::memcpy(counts, cnt.data(), (size_t)2 * n_img * sizeof(int64_t));
    if (stats) *stats = st;
    return SFM_OK;
}

}  // namespace

extern "C" void sfm_depth_views_default_options(sfm_depth_views_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->opt_angle = 10.0;
    o->min_angle = 3.0;
    o->max_scale = 1.6;
    o->range_margin = 0.25;
    o->min_shared = 10;
    o->max_neighbors = 4;
}

extern "C" int sfm_depth_views_select(int32_t n_platforms, int32_t n_images, int64_t n_vertices, const double* K,
                                      const int32_t* image_platform, const double* R, const double* C,
                                      const float* vert_X, const int64_t* vert_off, const uint32_t* vert_view,
                                      const sfm_depth_views_opts* opts, int64_t* nb_off, int32_t* nb_view,
                                      double* nb_score, float* drange) {
    return guarded([&] {
        const char* who = "sfm_depth_views_select";
        sfm_depth_views_opts o;
        sfm_depth_views_default_options(&o);
        if (opts) o = *opts;
        SFM_REQUIRE(n_platforms >= 0 && n_images >= 0 && n_vertices >= 0, SFM_ERR_INVALID_ARG, "%s: negative count", who);
        SFM_REQUIRE(o.max_neighbors >= 0 && o.max_neighbors <= kDepthMaxNeighbors, SFM_ERR_INVALID_ARG,
                    "%s: max_neighbors %d is outside 0..%d", who, o.max_neighbors, kDepthMaxNeighbors);
        SFM_REQUIRE(o.opt_angle > 0.0 && o.min_angle >= 0.0 && o.max_scale >= 1.0 && o.range_margin >= 0.0 &&
                        o.min_shared >= 0,
                    SFM_ERR_INVALID_ARG, "%s: opt_angle, min_angle, max_scale, range_margin or min_shared out of range", who);
        SFM_REQUIRE(nb_off, SFM_ERR_INVALID_ARG, "%s: null nb_off", who);
        nb_off[0] = 0;
        if (n_images == 0) return (int)SFM_OK;
        SFM_REQUIRE(K && image_platform && R && C && nb_view && nb_score && drange && vert_off, SFM_ERR_INVALID_ARG,
                    "%s: null argument", who);
        SFM_REQUIRE(n_vertices == 0 || (vert_X && vert_view), SFM_ERR_INVALID_ARG, "%s: null vertices", who);
        for (int32_t i = 0; i < n_images; ++i) {
            SFM_REQUIRE(image_platform[i] >= 0 && image_platform[i] < n_platforms, SFM_ERR_INVALID_ARG,
                        "%s: image %d names platform %d of %d", who, i, image_platform[i], n_platforms);
            for (int a = 0; a < 9; ++a)
                SFM_REQUIRE(std::isfinite(R[9 * i + a]) && std::isfinite(C[3 * i + a % 3]) &&
                                std::isfinite(K[9 * image_platform[i] + a]),
                            SFM_ERR_INVALID_ARG, "%s: the camera of image %d is not finite", who, i);
        }
        for (int64_t v = 0; v < n_vertices; ++v)
            for (int64_t k = vert_off[v]; k < vert_off[v + 1]; ++k)
                SFM_REQUIRE(vert_view[k] < (uint32_t)n_images, SFM_ERR_INVALID_ARG, "%s: vertex %lld names image %u of %d",
                            who, (long long)v, vert_view[k], n_images);
        const size_t n = (size_t)n_images;
        // depth of every (vertex, view) it is seen in; per image the range; per pair the sums
        std::vector<double> score(n * n, 0.0), angle(n * n, 0.0), zmin(n, 0.0), zmax(n, 0.0);
        std::vector<int64_t> shared(n * n, 0);
        const double deg = 180.0 / 3.14159265358979323846;
        std::vector<double> z, foc;
        for (int64_t v = 0; v < n_vertices; ++v) {
            const int64_t k0 = vert_off[v], k1 = vert_off[v + 1];
            const double X[3] = {(double)vert_X[3 * v], (double)vert_X[3 * v + 1], (double)vert_X[3 * v + 2]};
            z.assign((size_t)(k1 - k0), 0.0);
            foc.assign((size_t)(k1 - k0), 0.0);
            for (int64_t k = k0; k < k1; ++k) {
                const uint32_t i = vert_view[k];
                const double* Ri = R + 9 * (size_t)i;
                const double* Ci = C + 3 * (size_t)i;
                const double zi = Ri[6] * (X[0] - Ci[0]) + Ri[7] * (X[1] - Ci[1]) + Ri[8] * (X[2] - Ci[2]);
                z[(size_t)(k - k0)] = zi;
                foc[(size_t)(k - k0)] = K[9 * (size_t)image_platform[i]];
                if (zi > 0.0) {
                    if (zmax[i] == 0.0 || zi < zmin[i]) zmin[i] = zi;
                    if (zi > zmax[i]) zmax[i] = zi;
                }
            }
            for (int64_t a = k0; a < k1; ++a)
                for (int64_t b = k0; b < k1; ++b) {
                    const uint32_t i = vert_view[a], j = vert_view[b];
                    if (i == j) continue;
                    const double* Ci = C + 3 * (size_t)i;
                    const double* Cj = C + 3 * (size_t)j;
                    const double u[3] = {Ci[0] - X[0], Ci[1] - X[1], Ci[2] - X[2]};
                    const double w[3] = {Cj[0] - X[0], Cj[1] - X[1], Cj[2] - X[2]};
                    const double nu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
                    const double nw = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
                    double c = (u[0] * w[0] + u[1] * w[1] + u[2] * w[2]) / (nu * nw);
                    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
                    const double theta = std::acos(c) * deg;
                    const double w_angle = std::pow(std::min(theta / o.opt_angle, 1.0), 1.5);
                    const double s = (foc[(size_t)(a - k0)] / z[(size_t)(a - k0)]) / (foc[(size_t)(b - k0)] / z[(size_t)(b - k0)]);
                    const double w_scale = s < 1.0 ? s * s : (s > o.max_scale ? (o.max_scale / s) * (o.max_scale / s) : 1.0);
                    if (!std::isfinite(theta) || !std::isfinite(w_scale)) continue;
                    score[i * n + j] += w_angle * w_scale;
                    angle[i * n + j] += theta;
                    shared[i * n + j] += 1;
                }
        }
        std::vector<int32_t> cand;
        for (size_t i = 0; i < n; ++i) {
            cand.clear();
            for (size_t j = 0; j < n; ++j) {
                const int64_t sh = shared[i * n + j];
                if (j == i || sh == 0 || sh < o.min_shared || angle[i * n + j] / (double)sh < o.min_angle) continue;
                cand.push_back((int32_t)j);
            }
            std::stable_sort(cand.begin(), cand.end(),
                             [&](int32_t a, int32_t b) { return score[i * n + a] > score[i * n + b]; });
            if ((int32_t)cand.size() > o.max_neighbors) cand.resize((size_t)o.max_neighbors);
            int64_t at = nb_off[i];
            for (int32_t j : cand) {
                nb_view[at] = j;
                nb_score[at] = score[i * n + j];
                ++at;
            }
            nb_off[i + 1] = at;
            const bool ranged = !cand.empty() && zmax[i] > 0.0;
            drange[2 * i] = ranged ? (float)(zmin[i] / (1.0 + o.range_margin)) : 0.0f;
            drange[2 * i + 1] = ranged ? (float)(zmax[i] * (1.0 + o.range_margin)) : 0.0f;
        }
        return (int)SFM_OK;
    });
}

extern "C" void sfm_depthmap_default_options(sfm_depthmap_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->half_window = 3;
    o->iterations = 3;
    o->n_best = 2;
}

extern "C" void sfm_depthmap_filter_default_options(sfm_depthmap_filter_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->max_cost = 0.5f;
    o->rel_tol = 0.01f;
    o->min_consistent = 2;
}

extern "C" int sfm_depthmap_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                 const uint8_t* pixels, const double* K, const double* R, const double* C,
                                 const int64_t* nb_off, const int32_t* nb_view, const float* drange,
                                 const float* init_depth, const float* init_normal, const sfm_depthmap_opts* opts,
                                 float* depth, float* normal, float* cost, sfm_depthmap_stats* stats) {
    return guarded([&] {
        return depthmap("sfm_depthmap_host", nullptr, false, n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view,
                        drange, init_depth, init_normal, opts, depth, normal, cost, stats);
    });
}

extern "C" int sfm_depthmap_filter_host(int32_t n_img, const int32_t* wh, const double* K, const double* R,
                                        const double* C, const int64_t* nb_off, const int32_t* nb_view,
                                        const float* depth, const float* cost, const sfm_depthmap_filter_opts* opts,
                                        float* depth_out, uint8_t* n_agree, int64_t* counts,
                                        sfm_depthmap_filter_stats* stats) {
    return guarded([&] {
        return depthmap_filter("sfm_depthmap_filter_host", nullptr, false, n_img, wh, K, R, C, nb_off, nb_view, depth, cost,
                               opts, depth_out, n_agree, counts, stats);
    });
}

#ifndef SFM_DEPTHMAP_HOST_ONLY
extern "C" int sfm_depthmap(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels,
                            const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R,
                            const double* C, const int64_t* nb_off, const int32_t* nb_view, const float* drange,
                            const float* init_depth, const float* init_normal, const sfm_depthmap_opts* opts, float* depth,
                            float* normal, float* cost, sfm_depthmap_stats* stats) {
    return guarded([&] {
        return depthmap("sfm_depthmap", ctx, true, n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange,
                        init_depth, init_normal, opts, depth, normal, cost, stats);
    });
}

extern "C" int sfm_depthmap_filter(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const double* K, const double* R,
                                   const double* C, const int64_t* nb_off, const int32_t* nb_view, const float* depth,
                                   const float* cost, const sfm_depthmap_filter_opts* opts, float* depth_out,
                                   uint8_t* n_agree, int64_t* counts, sfm_depthmap_filter_stats* stats) {
    return guarded([&] {
        return depthmap_filter("sfm_depthmap_filter", ctx, true, n_img, wh, K, R, C, nb_off, nb_view, depth, cost, opts,
                               depth_out, n_agree, counts, stats);
    });
}
#endif
