// Depth-map fusion, host side (include/sfmcore.h, "Dense fusion"): the
// argument checks (the images': dense_views.cpp), the fusion pair lists, the host
// twin (threads over rows: fates, a prefix over the rows, points), the CSR
// expansion of the view lists, the cloud's PLY (dense_ply.cpp), and the entry
// points over either backend, sfm_densify among them.  The kernels and
// the transfers are fuse.hip's.  SFM_DEPTHMAP_HOST_ONLY leaves the device entry
// points out (tests/cpp/depthfuse_test.cpp).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dense_ply.h"
#include "fuse.h"

using namespace sfm;

namespace {

// the fusion pair list of every image: lists[i] in list order, and what was dropped
int64_t fusion_lists(int32_t n_img, const int64_t* nb_off, const int32_t* nb_view,
                     std::vector<std::vector<int32_t>>& lists) {
    lists.assign((size_t)n_img, {});
    std::vector<std::vector<int32_t>> reverse((size_t)n_img);
    for (int32_t i = 0; i < n_img; ++i)
        for (int64_t q = nb_off[i]; q < nb_off[i + 1]; ++q) {
            lists[(size_t)i].push_back(nb_view[q]);
            reverse[(size_t)nb_view[q]].push_back(i);   // ascending i by construction
        }
    int64_t dropped = 0;
    for (int32_t i = 0; i < n_img; ++i) {
        std::vector<int32_t>& L = lists[(size_t)i];
        const size_t own = L.size();
        for (int32_t j : reverse[(size_t)i])
            if (std::find(L.begin(), L.begin() + (std::ptrdiff_t)own, j) == L.begin() + (std::ptrdiff_t)own &&
                (L.size() == own || L.back() != j))
                L.push_back(j);
        if (L.size() > (size_t)kFuseMaxPairs) {
            dropped += (int64_t)L.size() - kFuseMaxPairs;
            L.resize((size_t)kFuseMaxPairs);
        }
    }
    return dropped;
}

void check_lists(const char* who, int32_t n_img, const int64_t* nb_off, const int32_t* nb_view) {
    SFM_REQUIRE(n_img >= 0, SFM_ERR_INVALID_ARG, "%s: negative n_img", who);
    if (n_img == 0) return;
    SFM_REQUIRE(nb_off && nb_off[0] == 0, SFM_ERR_INVALID_ARG, "%s: nb_off is null or does not start at 0", who);
    for (int32_t i = 0; i < n_img; ++i) {
        SFM_REQUIRE(nb_off[i + 1] >= nb_off[i], SFM_ERR_INVALID_ARG, "%s: nb_off decreases at image %d", who, i);
        SFM_REQUIRE(nb_off[i + 1] == nb_off[i] || nb_view, SFM_ERR_INVALID_ARG, "%s: null nb_view", who);
        for (int64_t q = nb_off[i]; q < nb_off[i + 1]; ++q)
            SFM_REQUIRE(nb_view[q] >= 0 && nb_view[q] < n_img && nb_view[q] != i, SFM_ERR_INVALID_ARG,
                        "%s: image %d names the neighbour %d (of %d images, itself excluded)", who, i, nb_view[q], n_img);
    }
}

// one row of an image
struct RowItem {
    int32_t img, y;
};

void fuse_host(const FuseProblem& F, const float* depth, const float* normal, const uint8_t* pixels, const FuseOut& out,
               int64_t* n_points, int64_t* n_suppressed) {
    std::vector<RowItem> rows;
    for (int32_t i = 0; i < F.images.n_img; ++i)
        for (int32_t y = 0; y < F.views[(size_t)i].h; ++y) rows.push_back(RowItem{i, y});
    std::vector<uint32_t> mask((size_t)F.images.n_map);
    std::vector<uint8_t> fate((size_t)F.images.n_map);
    std::vector<int64_t> base(rows.size() + 1, 0), supp(rows.size(), 0);
    const FuseView* views = F.views.data();
    const FusePair* pairs = F.pairs.data();
    dense_parallel_for(rows.size(), [&](size_t at) {
        const int32_t i = rows[at].img, y = rows[at].y;
        const FuseView& V = views[i];
        int64_t emitted = 0, suppressed = 0;
        for (int32_t x = 0; x < V.w; ++x) {
            const size_t idx = (size_t)(V.map_off + (int64_t)y * V.w + x);
            const int32_t f = fuse_pixel_fate(views, pairs, F.prm, i, x, y, depth, normal, &mask[idx]);
            fate[idx] = (uint8_t)f;
            emitted += f == kFuseEmitted;
            suppressed += f == kFuseSuppressed;
        }
        base[at + 1] = emitted;
        supp[at] = suppressed;
    });
    int64_t total_supp = 0;
    for (size_t at = 0; at < rows.size(); ++at) {
        base[at + 1] += base[at];
        total_supp += supp[at];
    }
    *n_points = base[rows.size()];
    *n_suppressed = total_supp;
    SFM_REQUIRE(*n_points <= out.cap_points, SFM_ERR_INVALID_ARG,
                "sfm_depthmap_fuse_host: the cloud has %lld points, cap_points is %lld", (long long)*n_points,
                (long long)out.cap_points);
    dense_parallel_for(rows.size(), [&](size_t at) {
        const int32_t i = rows[at].img, y = rows[at].y;
        const FuseView& V = views[i];
        int64_t rank = base[at];
        for (int32_t x = 0; x < V.w; ++x) {
            const size_t idx = (size_t)(V.map_off + (int64_t)y * V.w + x);
            if (fate[idx] != kFuseEmitted) continue;
            float X[3], N[3];
            uint8_t rgb[3] = {0, 0, 0};
            const int32_t m = fuse_pixel_point(views, pairs, F.prm, i, x, y, mask[idx], depth, normal, pixels, X, N, rgb);
            for (int c = 0; c < 3; ++c) {
                out.X[3 * rank + c] = X[c];
                if (out.N) out.N[3 * rank + c] = N[c];
                if (out.rgb && F.prm.use_color) out.rgb[3 * rank + c] = rgb[c];
            }
            if (out.n_views) out.n_views[rank] = (uint8_t)m;
            if (out.view_mask) out.view_mask[rank] = mask[idx];
            if (out.src_image) out.src_image[rank] = i;
            if (out.src_pixel) out.src_pixel[rank] = y * V.w + x;
            ++rank;
        }
    });
}

int fuse(const char* who, sfm_ctx* ctx, bool device, int32_t n_img, const int32_t* wh, const int32_t* channels,
         const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R, const double* C,
         const int64_t* nb_off, const int32_t* nb_view, const float* depth, const float* normal,
         const sfm_depthmap_fuse_opts* opts, const FuseOut& out, sfm_depthmap_fuse_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    FuseProblem F;
    sfm_depthmap_fuse_stats st;
    std::memset(&st, 0, sizeof st);
    fuse_prepare(who, DepthCameras{n_img, wh, K, R, C, nb_off, nb_view}, channels, img_off, pixels, opts, F,
                 &st.resident_bytes);
    st.n_pairs_dropped = F.n_pairs_dropped;
    SFM_REQUIRE(out.cap_points >= 0, SFM_ERR_INVALID_ARG, "%s: negative cap_points", who);
    SFM_REQUIRE(F.images.n_map == 0 || (depth && normal), SFM_ERR_INVALID_ARG, "%s: null depth or normal", who);
    SFM_REQUIRE(out.cap_points == 0 || out.X, SFM_ERR_INVALID_ARG, "%s: null X", who);
    if (F.images.n_map > 0) {
        try {
            if (device) {
#ifndef SFM_DEPTHMAP_HOST_ONLY
                fuse_device(ctx, F, depth, normal, pixels, out, &st.n_points, &st.n_suppressed, st.seconds);
#endif
            } else {
                const double t0 = seconds_now();
                fuse_host(F, depth, normal, pixels ? pixels + F.images.pool_lo : nullptr, out, &st.n_points, &st.n_suppressed);
                st.seconds[1] = seconds_now() - t0;
            }
        } catch (const SfmError&) {
            if (stats) *stats = st;   // cap_points too small: the need
            throw;
        }
    }
    if (stats) *stats = st;
    return SFM_OK;
}

int densify_chain(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                  const uint8_t* pixels, const double* K, const double* R, const double* C, const int64_t* nb_off,
                  const int32_t* nb_view, const float* drange, const float* init_depth, const float* init_normal,
                  const sfm_depthmap_opts* opts, const sfm_depthmap_filter_opts* filter_opts,
                  const sfm_depthmap_fuse_opts* fuse_opts, const FuseOut& out, float* depth, float* normal, float* cost,
                  float* depth_filtered, uint8_t* n_agree, int64_t* counts, sfm_densify_stats* stats) {
    int64_t n_map = 0;
    for (int32_t i = 0; i < n_img && wh; ++i) n_map += (int64_t)std::max(wh[2 * i], 0) * std::max(wh[2 * i + 1], 0);
    const size_t n = (size_t)std::max<int64_t>(n_map, 1);
    std::vector<float> d, nn, c, f;
    std::vector<uint8_t> a;
    if (!depth) d.resize(n), depth = d.data();
    if (!normal) nn.resize(3 * n), normal = nn.data();
    if (!cost) c.resize(n), cost = c.data();
    if (!depth_filtered) f.resize(n), depth_filtered = f.data();
    if (!n_agree) a.resize(n), n_agree = a.data();
    sfm_densify_stats st;
    std::memset(&st, 0, sizeof st);
    int rc = sfm_depthmap_host(n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange, init_depth,
                               init_normal, opts, depth, normal, cost, &st.depthmap);
    if (rc == SFM_OK)
        rc = sfm_depthmap_filter_host(n_img, wh, K, R, C, nb_off, nb_view, depth, cost, filter_opts, depth_filtered,
                                      n_agree, counts, &st.filter);
    if (rc == SFM_OK)
        rc = sfm_depthmap_fuse_host(n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, depth_filtered, normal,
                                    fuse_opts, out.cap_points, out.X, out.N, out.rgb, out.n_views, out.view_mask,
                                    out.src_image, out.src_pixel, &st.fuse);
    st.seconds[1] = st.depthmap.seconds[1] + st.filter.seconds[1] + st.fuse.seconds[1];
    if (stats) *stats = st;
    return rc;
}

}  // namespace

namespace sfm {

void fuse_prepare(const char* who, const DepthCameras& m, const int32_t* channels, const int64_t* img_off,
                  const uint8_t* pixels, const sfm_depthmap_fuse_opts* opts, FuseProblem& F, int64_t* resident_bytes) {
    sfm_depthmap_fuse_opts o;
    sfm_depthmap_fuse_default_options(&o);
    if (opts) o = *opts;
    SFM_REQUIRE(o.rel_tol >= 0.0f, SFM_ERR_INVALID_ARG, "%s: rel_tol is negative or not a number", who);
    SFM_REQUIRE(o.min_normal_cos <= 1.0f, SFM_ERR_INVALID_ARG, "%s: min_normal_cos is above 1 or not a number", who);
    SFM_REQUIRE(o.device_bytes >= 0, SFM_ERR_INVALID_ARG, "%s: negative device_bytes", who);
    // sizes, cameras, neighbours: the filter's checks (every image counts as loaded there)
    DepthProblem P;
    depth_build_problem(who, m, nullptr, nullptr, nullptr, nullptr, P);
    F.images.n_img = m.n_img;
    F.prm = FuseParams{o.rel_tol, o.min_normal_cos, o.min_normal_cos > -1.0f, pixels != nullptr};
    if (m.n_img <= 0) {
        *resident_bytes = 0;
        return;
    }
    SFM_REQUIRE(!pixels || (channels && img_off), SFM_ERR_INVALID_ARG, "%s: pixels without channels or img_off", who);
    // the channels and the colour pool's window (sizes and cameras passed above)
    dense_images_prepare(who, m.n_img, m.wh, channels, img_off, pixels, m.K, m.R, m.C, F.images);
    std::vector<std::vector<int32_t>> lists;
    F.n_pairs_dropped = fusion_lists(m.n_img, m.nb_off, m.nb_view, lists);
    F.views.resize((size_t)m.n_img);
    for (int32_t i = 0; i < m.n_img; ++i) {
        const DenseImage& I = F.images.img[(size_t)i];
        FuseView& V = F.views[(size_t)i];
        std::memset(&V, 0, sizeof V);
        for (int a = 0; a < 9; ++a) {
            V.Ki[a] = P.views[(size_t)i].Ki[a];
            V.R[a] = (float)m.R[9 * i + a];
        }
        dense_C(m.C, i, V.C);
        V.w = I.w;
        V.h = I.h;
        V.map_off = I.map_off;
        V.pix_off = I.pix_off;
        V.loaded = I.loaded;
        V.channels = I.channels;
        const int64_t n = (int64_t)V.w * V.h;
        V.blk_off = F.n_blocks;
        const int64_t blocks = (n + kFuseBlock - 1) / kFuseBlock;
        F.n_blocks += blocks;
        F.max_blocks = std::max(F.max_blocks, blocks);
        V.p0 = (int32_t)F.pairs.size();
        for (int32_t j : lists[(size_t)i]) {
            FusePair Q;
            std::memset(&Q, 0, sizeof Q);
            depth_pair_matrices(m, i, j, Q.A, Q.b);
            Q.view = j;
            F.pairs.push_back(Q);
        }
        V.p1 = (int32_t)F.pairs.size();
    }
    *resident_bytes = F.images.n_map * (int64_t)(4 * sizeof(float) + sizeof(uint32_t) + 1) +
                      (F.images.pool_hi - F.images.pool_lo) +
                      (int64_t)(F.views.size() * sizeof(FuseView) + F.pairs.size() * sizeof(FusePair)) +
                      F.n_blocks * (int64_t)(sizeof(int32_t) + sizeof(int64_t));
    const int64_t budget = o.device_bytes > 0 ? o.device_bytes : kFuseDefaultDeviceBytes;
    SFM_REQUIRE(*resident_bytes <= budget, SFM_ERR_UNSUPPORTED,
                "%s: the maps and colours need %lld resident bytes, device_bytes is %lld (streaming is not built)", who,
                (long long)*resident_bytes, (long long)budget);
}

}  // namespace sfm

extern "C" void sfm_depthmap_fuse_default_options(sfm_depthmap_fuse_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->rel_tol = 0.01f;
    o->min_normal_cos = -1.0f;
}

extern "C" int sfm_depthmap_fuse_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                      const uint8_t* pixels, const double* K, const double* R, const double* C,
                                      const int64_t* nb_off, const int32_t* nb_view, const float* depth,
                                      const float* normal, const sfm_depthmap_fuse_opts* opts, int64_t cap_points,
                                      float* X, float* N, uint8_t* rgb, uint8_t* n_views, uint32_t* view_mask,
                                      int32_t* src_image, int32_t* src_pixel, sfm_depthmap_fuse_stats* stats) {
    return guarded([&] {
        return fuse("sfm_depthmap_fuse_host", nullptr, false, n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view,
                    depth, normal, opts, FuseOut{cap_points, X, N, rgb, n_views, view_mask, src_image, src_pixel}, stats);
    });
}

extern "C" int sfm_dense_cloud_views(int32_t n_img, const int64_t* nb_off, const int32_t* nb_view, int64_t n_points,
                                     const int32_t* src_image, const uint32_t* view_mask, int64_t* view_off,
                                     int32_t* view_idx) {
    return guarded([&] {
        const char* who = "sfm_dense_cloud_views";
        SFM_REQUIRE(n_points >= 0 && view_off, SFM_ERR_INVALID_ARG, "%s: negative n_points or null view_off", who);
        SFM_REQUIRE(n_points == 0 || (src_image && view_mask), SFM_ERR_INVALID_ARG, "%s: null argument", who);
        check_lists(who, n_img, nb_off, nb_view);
        std::vector<std::vector<int32_t>> lists;
        fusion_lists(n_img, nb_off, nb_view, lists);
        view_off[0] = 0;
        for (int64_t k = 0; k < n_points; ++k) {
            const int32_t i = src_image[k];
            SFM_REQUIRE(i >= 0 && i < n_img, SFM_ERR_INVALID_ARG, "%s: point %lld names image %d of %d", who, (long long)k, i,
                        n_img);
            const std::vector<int32_t>& L = lists[(size_t)i];
            SFM_REQUIRE(L.size() >= 32 || (view_mask[k] >> L.size()) == 0, SFM_ERR_INVALID_ARG,
                        "%s: point %lld sets a bit beyond the %d fusion pairs of image %d", who, (long long)k, (int)L.size(), i);
            int64_t at = view_off[k];
            if (view_idx) view_idx[at] = i;
            ++at;
            for (uint32_t rest = view_mask[k]; rest; rest &= rest - 1) {
                if (view_idx) view_idx[at] = L[(size_t)__builtin_ctz(rest)];
                ++at;
            }
            view_off[k + 1] = at;
        }
        return (int)SFM_OK;
    });
}

extern "C" int sfm_dense_cloud_write_ply(const char* path, int64_t n_points, const float* X, const float* N,
                                         const uint8_t* rgb) {
    return guarded([&] {
        const char* who = "sfm_dense_cloud_write_ply";
        SFM_REQUIRE(path && n_points >= 0 && (n_points == 0 || X), SFM_ERR_INVALID_ARG, "%s: null path or X, or negative n_points",
                    who);
        std::string elements = "element vertex " + std::to_string(n_points) + "\nproperty float x\nproperty float y\nproperty float z\n";
        if (N) elements += "property float nx\nproperty float ny\nproperty float nz\n";
        if (rgb) elements += "property uchar red\nproperty uchar green\nproperty uchar blue\n";
        PlyWriter ply(who, path, elements);
        ply.records(n_points, 12 + (N ? 12 : 0) + (rgb ? 3 : 0), [&](int64_t k, uint8_t* p) {
            std::memcpy(p, X + 3 * k, 12);
            if (N) std::memcpy(p + 12, N + 3 * k, 12);
            if (rgb) std::memcpy(p + (N ? 24 : 12), rgb + 3 * k, 3);
        });
        ply.close();
        return (int)SFM_OK;
    });
}

extern "C" int sfm_densify_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                const uint8_t* pixels, const double* K, const double* R, const double* C,
                                const int64_t* nb_off, const int32_t* nb_view, const float* drange,
                                const float* init_depth, const float* init_normal, const sfm_depthmap_opts* opts,
                                const sfm_depthmap_filter_opts* filter_opts, const sfm_depthmap_fuse_opts* fuse_opts,
                                int64_t cap_points, float* X, float* N, uint8_t* rgb, uint8_t* n_views,
                                uint32_t* view_mask, int32_t* src_image, int32_t* src_pixel, float* depth, float* normal,
                                float* cost, float* depth_filtered, uint8_t* n_agree, int64_t* counts,
                                sfm_densify_stats* stats) {
    return guarded([&] {
        return densify_chain(n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange, init_depth, init_normal,
                             opts, filter_opts, fuse_opts,
                             FuseOut{cap_points, X, N, rgb, n_views, view_mask, src_image, src_pixel}, depth, normal, cost,
                             depth_filtered, n_agree, counts, stats);
    });
}

#ifndef SFM_DEPTHMAP_HOST_ONLY
extern "C" int sfm_depthmap_fuse(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels,
                                 const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R,
                                 const double* C, const int64_t* nb_off, const int32_t* nb_view, const float* depth,
                                 const float* normal, const sfm_depthmap_fuse_opts* opts, int64_t cap_points, float* X,
                                 float* N, uint8_t* rgb, uint8_t* n_views, uint32_t* view_mask, int32_t* src_image,
                                 int32_t* src_pixel, sfm_depthmap_fuse_stats* stats) {
    return guarded([&] {
        return fuse("sfm_depthmap_fuse", ctx, true, n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, depth,
                    normal, opts, FuseOut{cap_points, X, N, rgb, n_views, view_mask, src_image, src_pixel}, stats);
    });
}

extern "C" int sfm_densify(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels,
                           const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R,
                           const double* C, const int64_t* nb_off, const int32_t* nb_view, const float* drange,
                           const float* init_depth, const float* init_normal, const sfm_depthmap_opts* opts,
                           const sfm_depthmap_filter_opts* filter_opts, const sfm_depthmap_fuse_opts* fuse_opts,
                           int64_t cap_points, float* X, float* N, uint8_t* rgb, uint8_t* n_views, uint32_t* view_mask,
                           int32_t* src_image, int32_t* src_pixel, float* depth, float* normal, float* cost,
                           float* depth_filtered, uint8_t* n_agree, int64_t* counts, sfm_densify_stats* stats) {
    return guarded([&] {
        const char* who = "sfm_densify";
        SFM_REQUIRE(ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
        sfm_densify_stats st;
        std::memset(&st, 0, sizeof st);
        DepthCall call;
        depth_prepare(who, n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange, init_depth, init_normal,
                      opts, call);
        DepthFilterParams fprm;
        depth_filter_prepare(who, filter_opts, fprm);
        FuseProblem F;
        fuse_prepare(who, DepthCameras{n_img, wh, K, R, C, nb_off, nb_view}, channels, img_off, pixels, fuse_opts, F,
                     &st.fuse.resident_bytes);
        const FuseOut out{cap_points, X, N, rgb, n_views, view_mask, src_image, src_pixel};
        SFM_REQUIRE(cap_points >= 0 && (cap_points == 0 || X), SFM_ERR_INVALID_ARG, "%s: negative cap_points or null X", who);
        st.depthmap = call.st;
        st.fuse.n_pairs_dropped = F.n_pairs_dropped;
        if (call.P.n_map > 0) {
            try {
                densify_device(ctx, call, init_depth != nullptr, init_depth, init_normal, fprm, F, pixels, out,
                               DensifyMaps{depth, normal, cost, depth_filtered, n_agree, counts}, &st);
            } catch (const SfmError&) {
                if (stats) *stats = st;
                throw;
            }
        }
        if (stats) *stats = st;
        return (int)SFM_OK;
    });
}
#endif
