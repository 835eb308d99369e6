// Track colouring, host side (include/sfmcore.h, "Track colouring"): the
// argument checks, the serial host twin of the assignment, the sampling from
// the caller's images, sfm_colorize over either, and the PLY writer that
// cloud_and_poses.ply and colorized.ply share.  The kernels are colorize.hip's.
// SFM_COLORIZE_HOST_ONLY leaves the device entry points out, so that the host
// twin builds with a plain host compiler (tests/cpp/colorize_test.cpp).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "colorize.h"

using namespace sfm;

namespace {

struct Masks {
    const uint8_t* pt_ok;
    const uint8_t* keep;
    bool ok(int64_t p) const { return !pt_ok || pt_ok[p]; }
    bool live(int64_t o) const { return !keep || keep[o]; }
};

// every check of the assignment; nothing has touched the device yet
void check_assign(const char* who, const sfm_ba_problem* P, const int32_t* wh, const Masks& m, const int32_t* view,
                  const int64_t* obs, const int32_t* px, const int32_t* order, const int32_t* n_rounds) {
    SFM_REQUIRE(P, SFM_ERR_INVALID_ARG, "%s: null problem", who);
    SFM_REQUIRE(P->n_obs < INT32_MAX && P->n_pt < INT32_MAX, SFM_ERR_INVALID_ARG,
                "%s: 2^31 - 1 or more points or observations", who);
    recon_check_tracks(who, P);
    SFM_REQUIRE(n_rounds && (P->n_img == 0 || (wh && order)) && (P->n_pt == 0 || (view && obs && px)),
                SFM_ERR_INVALID_ARG, "%s: null argument", who);
    for (int32_t i = 0; i < P->n_img; ++i)
        SFM_REQUIRE(wh[2 * i] > 0 && wh[2 * i + 1] > 0, SFM_ERR_INVALID_ARG, "%s: image %d has a non-positive size", who,
                    i);
    for (int64_t p = 0; p < P->n_pt; ++p) {
        if (!m.ok(p)) continue;
        for (int64_t o = P->pt_offsets[p]; o < P->pt_offsets[p + 1]; ++o)
            SFM_REQUIRE(!m.live(o) || (std::isfinite(P->obs_uv[2 * o]) && std::isfinite(P->obs_uv[2 * o + 1])),
                        SFM_ERR_INVALID_ARG, "%s: observation %lld is not finite", who, (long long)o);
    }
}

// the images' pixels: channels 1 or 3 where loaded
void check_images(const char* who, int32_t n_img, const int32_t* channels, const int64_t* img_off,
                  const uint8_t* pixels) {
    SFM_REQUIRE(n_img == 0 || (channels && img_off), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    for (int32_t i = 0; i < n_img; ++i) {
        if (img_off[i] < 0) continue;
        SFM_REQUIRE(pixels, SFM_ERR_INVALID_ARG, "%s: null pixels", who);
        SFM_REQUIRE(channels[i] == 1 || channels[i] == 3, SFM_ERR_INVALID_ARG, "%s: image %d has %d channels", who, i,
                    channels[i]);
    }
}

// The serial twin: the device's algorithm, statement by statement (counts kept
// incrementally over the per-image lists of the shared index).
void host_assign(const sfm_ba_problem& P, const int32_t* wh, const Masks& m, int32_t* view, int64_t* obs, int32_t* px,
                 int32_t* order, int32_t* n_rounds, sfm_colorize_stats& st) {
    double t0 = seconds_now();
    std::vector<int32_t> img_off;
    const ReconIndex ix = recon_build_index(P, img_off);
    auto first_in_image = [&](int64_t p, int64_t o) {
        if (!ix.dup[o]) return true;
        for (int64_t q = P.pt_offsets[p]; q < o; ++q)
            if (m.live(q) && P.obs_img[q] == P.obs_img[o]) return false;
        return true;
    };
    std::vector<int32_t> count((size_t)P.n_img, 0);
    std::vector<uint8_t> todo((size_t)P.n_pt, 0);
    int64_t left = 0;
    for (int64_t p = 0; p < P.n_pt; ++p) {
        if (!m.ok(p)) continue;
        bool any = false;
        for (int64_t o = P.pt_offsets[p]; o < P.pt_offsets[p + 1]; ++o) {
            if (!m.live(o)) continue;
            any = true;
            if (first_in_image(p, o)) ++count[P.obs_img[o]];
        }
        todo[p] = any;
        left += any;
    }
    st.n_to_colour = left;
    double t1 = seconds_now();
    st.seconds[0] = t1 - t0;
    while (left > 0) {
        int32_t bc = 0, v = -1;
        for (int32_t i = 0; i < P.n_img; ++i)
            if (count[i] > bc) {
                bc = count[i];
                v = i;
            }
        if (v < 0) break;
        order[(*n_rounds)++] = v;
        for (int32_t k = img_off[v]; k < img_off[(size_t)v + 1]; ++k) {
            const int64_t o = ix.img_obs[k];
            if (!m.live(o)) continue;
            const int64_t p = ix.obs_pt[o];
            if (!todo[p] || !first_in_image(p, o)) continue;
            view[p] = v;
            obs[p] = o;
            px[2 * p] = colorize_pixel(P.obs_uv[2 * o], wh[2 * v]);
            px[2 * p + 1] = colorize_pixel(P.obs_uv[2 * o + 1], wh[2 * v + 1]);
            todo[p] = 0;
            for (int64_t q = P.pt_offsets[p]; q < P.pt_offsets[p + 1]; ++q)
                if (m.live(q) && first_in_image(p, q)) --count[P.obs_img[q]];
            --left;
        }
    }
    st.n_coloured = st.n_to_colour - left;
    st.seconds[1] = seconds_now() - t1;
}

int assign(const char* who, sfm_ctx* ctx, bool device, const sfm_ba_problem* P, const int32_t* wh,
           const uint8_t* pt_ok, const uint8_t* keep_obs, int32_t* view, int64_t* obs, int32_t* px, int32_t* order,
           int32_t* n_rounds, sfm_colorize_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    const Masks m{pt_ok, keep_obs};
    check_assign(who, P, wh, m, view, obs, px, order, n_rounds);
    sfm_colorize_stats st;
    std::memset(&st, 0, sizeof st);
    *n_rounds = 0;
    std::fill(order, order + P->n_img, -1);
    std::fill(view, view + P->n_pt, -1);
    std::fill(obs, obs + P->n_pt, (int64_t)-1);
    std::fill(px, px + 2 * P->n_pt, 0);
    if (P->n_obs > 0) {
        if (device) {
#ifndef SFM_COLORIZE_HOST_ONLY
            const double t0 = seconds_now();
            std::vector<int32_t> img_off;
            const ReconIndex ix = recon_build_index(*P, img_off);
            const double t_index = seconds_now() - t0;
            colorize_device_assign(ctx, P->n_img, (int32_t)P->n_pt, (int32_t)P->n_obs, ix, P->obs_img, P->obs_uv, wh,
                                   pt_ok, keep_obs, view, obs, px, order, n_rounds, &st.n_to_colour, &st.n_coloured,
                                   st.seconds);
            st.seconds[0] += t_index;
#endif
        } else {
            host_assign(*P, wh, m, view, obs, px, order, n_rounds, st);
        }
    }
    st.n_rounds = *n_rounds;
    if (stats) *stats = st;
    return SFM_OK;
}

void sample(const char* who, int64_t n_pt, const int32_t* view, const int32_t* px, int32_t n_img, const int32_t* wh,
            const int32_t* channels, const int64_t* img_off, const uint8_t* pixels, uint8_t* rgb) {
    SFM_REQUIRE(n_pt >= 0 && n_img >= 0 && (n_pt == 0 || (view && px && rgb)) && (n_img == 0 || wh),
                SFM_ERR_INVALID_ARG, "%s: null argument", who);
    check_images(who, n_img, channels, img_off, pixels);
    for (int64_t p = 0; p < n_pt; ++p) {
        uint8_t* c = rgb + 3 * p;
        const int32_t v = view[p];
        if (v < 0) {
            SFM_REQUIRE(v == -1, SFM_ERR_INVALID_ARG, "%s: point %lld names view %d", who, (long long)p, v);
            c[0] = c[1] = c[2] = 0;
            continue;
        }
        SFM_REQUIRE(v < n_img, SFM_ERR_INVALID_ARG, "%s: point %lld names view %d of %d", who, (long long)p, v, n_img);
        SFM_REQUIRE(img_off[v] >= 0, SFM_ERR_INVALID_ARG, "%s: image %d colours point %lld and is not loaded", who, v,
                    (long long)p);
        const int64_t w = wh[2 * v], h = wh[2 * v + 1], x = px[2 * p], y = px[2 * p + 1];
        SFM_REQUIRE(x >= 0 && x < w && y >= 0 && y < h, SFM_ERR_INVALID_ARG,
                    "%s: point %lld reads pixel (%lld, %lld) of a %lld x %lld image", who, (long long)p, (long long)x,
                    (long long)y, (long long)w, (long long)h);
        const int64_t ch = channels[v];
        const uint8_t* at = pixels + img_off[v] + (y * w + x) * ch;
        c[0] = at[0];
        c[1] = at[ch == 3 ? 1 : 0];
        c[2] = at[ch == 3 ? 2 : 0];
    }
}

int colorize(const char* who, sfm_ctx* ctx, bool device, const sfm_ba_problem* P, const int32_t* wh,
             const uint8_t* pt_ok, const uint8_t* keep_obs, const int32_t* channels, const int64_t* img_off,
             const uint8_t* pixels, uint8_t* rgb, int32_t* view_out, sfm_colorize_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    SFM_REQUIRE(P, SFM_ERR_INVALID_ARG, "%s: null problem", who);
    SFM_REQUIRE(P->n_obs < INT32_MAX && P->n_pt < INT32_MAX, SFM_ERR_INVALID_ARG,
                "%s: 2^31 - 1 or more points or observations", who);
    recon_check_tracks(who, P);
    SFM_REQUIRE(P->n_pt == 0 || rgb, SFM_ERR_INVALID_ARG, "%s: null argument", who);
    check_images(who, P->n_img, channels, img_off, pixels);
    const Masks m{pt_ok, keep_obs};
    for (int64_t p = 0; p < P->n_pt; ++p) {
        if (!m.ok(p)) continue;
        for (int64_t o = P->pt_offsets[p]; o < P->pt_offsets[p + 1]; ++o)
            SFM_REQUIRE(!m.live(o) || img_off[P->obs_img[o]] >= 0, SFM_ERR_INVALID_ARG,
                        "%s: image %d has a live observation of point %lld and is not loaded", who, P->obs_img[o],
                        (long long)p);
    }
    const size_t NP = (size_t)P->n_pt + 1, NI = (size_t)P->n_img + 1;
    std::vector<int32_t> view(NP), px(2 * NP), order(NI);
    std::vector<int64_t> obs(NP);
    int32_t n_rounds = 0;
    assign(who, ctx, device, P, wh, pt_ok, keep_obs, view.data(), obs.data(), px.data(), order.data(), &n_rounds, stats);
    sample(who, P->n_pt, view.data(), px.data(), P->n_img, wh, channels, img_off, pixels, rgb);
    if (view_out) std::copy(view.begin(), view.end() - 1, view_out);
    return SFM_OK;
}

}  // namespace

namespace sfm {

void write_ply(const char* who, const char* path, int64_t n_pt, const double* X, const uint8_t* pt_ok,
               const uint8_t* rgb, int32_t n_img, const double* extr, const uint8_t* registered) {
    SFM_REQUIRE(path && n_pt >= 0 && n_img >= 0 && (n_pt == 0 || X) && (n_img == 0 || extr), SFM_ERR_INVALID_ARG,
                "%s: null argument", who);
    int64_t n_vertex = 0;
    for (int64_t p = 0; p < n_pt; ++p) n_vertex += !pt_ok || pt_ok[p];
    for (int32_t k = 0; k < n_img; ++k) n_vertex += !registered || registered[k];
    std::FILE* f = std::fopen(path, "w");
    SFM_REQUIRE(f, SFM_ERR_INVALID_ARG, "%s: cannot write %s", who, path);
    std::fprintf(f,
                 "ply\nformat ascii 1.0\nelement vertex %lld\nproperty double x\nproperty double y\n"
                 "property double z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n",
                 (long long)n_vertex);
    for (int64_t p = 0; p < n_pt; ++p) {
        if (pt_ok && !pt_ok[p]) continue;
        const int r = rgb ? rgb[3 * p] : 255, g = rgb ? rgb[3 * p + 1] : 255, b = rgb ? rgb[3 * p + 2] : 255;
        std::fprintf(f, "%.16f %.16f %.16f %d %d %d\n", X[3 * p], X[3 * p + 1], X[3 * p + 2], r, g, b);
    }
    for (int32_t k = 0; k < n_img; ++k) {
        if (registered && !registered[k]) continue;
        const double* e = &extr[6 * (size_t)k];
        // C = -R' t, R' t by Rodrigues' formula with the angle negated
        const double th2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2], th = std::sqrt(th2);
        double C[3] = {e[3], e[4], e[5]};
        if (th > 0.0) {
            const double u[3] = {-e[0] / th, -e[1] / th, -e[2] / th}, c = std::cos(th), s = std::sin(th);
            const double* t = e + 3;
            const double d = u[0] * t[0] + u[1] * t[1] + u[2] * t[2];
            const double x[3] = {u[1] * t[2] - u[2] * t[1], u[2] * t[0] - u[0] * t[2], u[0] * t[1] - u[1] * t[0]};
            for (int a = 0; a < 3; ++a) C[a] = t[a] * c + x[a] * s + u[a] * d * (1 - c);
        }
        std::fprintf(f, "%.16f %.16f %.16f 0 255 0\n", -C[0], -C[1], -C[2]);
    }
    const bool good = std::fclose(f) == 0;
    SFM_REQUIRE(good, SFM_ERR_INVALID_ARG, "%s: writing %s failed", who, path);
}

}  // namespace sfm

extern "C" int sfm_colorize_assign_host(const sfm_ba_problem* tracks, const int32_t* wh, const uint8_t* pt_ok,
                                        const uint8_t* keep_obs, int32_t* view, int64_t* obs, int32_t* px,
                                        int32_t* order, int32_t* n_rounds, sfm_colorize_stats* stats) {
    return guarded([&] {
        return assign("sfm_colorize_assign_host", nullptr, false, tracks, wh, pt_ok, keep_obs, view, obs, px, order,
                      n_rounds, stats);
    });
}

extern "C" int sfm_colorize_sample(int64_t n_pt, const int32_t* view, const int32_t* px, int32_t n_img,
                                   const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                   const uint8_t* pixels, uint8_t* rgb) {
    return guarded([&] {
        sample("sfm_colorize_sample", n_pt, view, px, n_img, wh, channels, img_off, pixels, rgb);
        return SFM_OK;
    });
}

extern "C" int sfm_colorize_host(const sfm_ba_problem* tracks, const int32_t* wh, const uint8_t* pt_ok,
                                 const uint8_t* keep_obs, const int32_t* channels, const int64_t* img_off,
                                 const uint8_t* pixels, uint8_t* rgb, int32_t* view, sfm_colorize_stats* stats) {
    return guarded([&] {
        return colorize("sfm_colorize_host", nullptr, false, tracks, wh, pt_ok, keep_obs, channels, img_off, pixels, rgb,
                        view, stats);
    });
}

extern "C" int sfm_colorize_write_ply(const char* path, int64_t n_pt, const double* X, const uint8_t* pt_ok,
                                      const uint8_t* rgb, int32_t n_img, const double* extr,
                                      const uint8_t* registered) {
    return guarded([&] {
        write_ply("sfm_colorize_write_ply", path, n_pt, X, pt_ok, rgb, n_img, extr, registered);
        return SFM_OK;
    });
}

#ifndef SFM_COLORIZE_HOST_ONLY
extern "C" int sfm_colorize_assign(sfm_ctx* ctx, const sfm_ba_problem* tracks, const int32_t* wh, const uint8_t* pt_ok,
                                   const uint8_t* keep_obs, int32_t* view, int64_t* obs, int32_t* px, int32_t* order,
                                   int32_t* n_rounds, sfm_colorize_stats* stats) {
    return guarded([&] {
        return assign("sfm_colorize_assign", ctx, true, tracks, wh, pt_ok, keep_obs, view, obs, px, order, n_rounds,
                      stats);
    });
}

extern "C" int sfm_colorize(sfm_ctx* ctx, const sfm_ba_problem* tracks, const int32_t* wh, const uint8_t* pt_ok,
                            const uint8_t* keep_obs, const int32_t* channels, const int64_t* img_off,
                            const uint8_t* pixels, uint8_t* rgb, int32_t* view, sfm_colorize_stats* stats) {
    return guarded([&] {
        return colorize("sfm_colorize", ctx, true, tracks, wh, pt_ok, keep_obs, channels, img_off, pixels, rgb, view,
                        stats);
    });
}
#endif
