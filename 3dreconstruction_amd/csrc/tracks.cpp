// Track building, host side: the options, the argument checks and the edge
// list both builds read, the serial host twin (sfm_tracks_build_host: a
// union-find, then the same grouping, verdicts and canonical order as
// tracks.hip), the handle's accessors, the device entry point
// (sfm_tracks_build) and the file-staged one (sfm_sparse_tracks).
// SFM_TRACKS_HOST_ONLY leaves the two device entry points out, so that the
// host path builds with a plain host compiler (tests/cpp/tracks_test.cpp).
#include <algorithm>
#include <climits>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "tracks.h"

using namespace sfm;

extern "C" void sfm_tracks_default_options(sfm_tracks_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->min_track_len = 2;   // OpenMVG's Filter(nLengthSupTo = 2)
}

namespace {

sfm_tracks_opts tracks_options(const sfm_tracks_opts* o) {
    sfm_tracks_opts r;
    if (o) r = *o; else sfm_tracks_default_options(&r);
    SFM_REQUIRE(r.min_track_len >= 2, SFM_ERR_INVALID_ARG, "min_track_len %d (must be >= 2)", r.min_track_len);
    return r;
}

// the checked input in 32 bits: the offsets and one (node, node) per match
struct Staged {
    std::vector<int32_t> off, eu, ev;
    TracksInput input(int32_t n_img, const double* xy, int32_t min_len) const {
        TracksInput in;
        in.n_img = n_img;
        in.n_space = off[n_img];
        in.n_edges = (int32_t)eu.size();
        in.min_len = min_len;
        in.feat_off = off.data();
        in.eu = eu.data();
        in.ev = ev.data();
        in.xy = xy;
        return in;
    }
};

void stage(int32_t n_img, const int64_t* feat_off, int64_t n_pairs, const int32_t* pairs, const int64_t* counts,
           const uint32_t* mi, const uint32_t* mj, Staged& s) {
    SFM_REQUIRE(n_img >= 0 && feat_off && n_pairs >= 0 && (n_pairs == 0 || (pairs && counts)), SFM_ERR_INVALID_ARG,
                "sfm_tracks_build: bad argument");
    SFM_REQUIRE(feat_off[0] >= 0, SFM_ERR_INVALID_ARG, "feat_off[0] = %lld (must be >= 0)", (long long)feat_off[0]);
    for (int32_t k = 0; k < n_img; ++k)
        SFM_REQUIRE(feat_off[k + 1] >= feat_off[k], SFM_ERR_INVALID_ARG, "feat_off decreases at image %d", k);
    SFM_REQUIRE(feat_off[n_img] <= INT32_MAX, SFM_ERR_UNSUPPORTED, "%lld nodes (at most 2^31 - 1)",
                (long long)feat_off[n_img]);
    int64_t total = 0;
    for (int64_t q = 0; q < n_pairs; ++q) {
        SFM_REQUIRE(counts[q] >= 0, SFM_ERR_INVALID_ARG, "pair %lld: negative match count", (long long)q);
        SFM_REQUIRE(counts[q] <= INT32_MAX - total, SFM_ERR_UNSUPPORTED, "more than 2^31 - 1 matches");
        total += counts[q];
    }
    SFM_REQUIRE(total == 0 || (mi && mj), SFM_ERR_INVALID_ARG, "null match arrays");
    s.off.resize((size_t)n_img + 1);
    for (int32_t k = 0; k <= n_img; ++k) s.off[k] = (int32_t)feat_off[k];
    s.eu.resize((size_t)total);
    s.ev.resize((size_t)total);
    int64_t k = 0;
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int32_t I = pairs[2 * q], J = pairs[2 * q + 1];
        SFM_REQUIRE(I >= 0 && I < n_img && J >= 0 && J < n_img, SFM_ERR_INVALID_ARG,
                    "pair %lld = (%d, %d) outside the %d images", (long long)q, I, J, n_img);
        SFM_REQUIRE(I != J, SFM_ERR_INVALID_ARG, "pair %lld matches image %d with itself", (long long)q, I);
        const uint32_t ci = (uint32_t)(s.off[I + 1] - s.off[I]), cj = (uint32_t)(s.off[J + 1] - s.off[J]);
        for (const int64_t end = k + counts[q]; k < end; ++k) {
            SFM_REQUIRE(mi[k] < ci && mj[k] < cj, SFM_ERR_INVALID_ARG,
                        "pair (%d, %d): match (%u, %u) outside the features (%u, %u)", I, J, mi[k], mj[k], ci, cj);
            s.eu[k] = s.off[I] + (int32_t)mi[k];
            s.ev[k] = s.off[J] + (int32_t)mj[k];
        }
    }
}

void empty_tracks(const TracksInput& in, sfm_tracks& out) {
    out.pt_offsets.assign(1, 0);
    out.has_uv = in.xy != nullptr;
    out.st = sfm_tracks_stats{};
}

int32_t find_root(std::vector<int32_t>& parent, int32_t x) {
    while (parent[x] != x) {
        parent[x] = parent[parent[x]];   // path halving
        x = parent[x];
    }
    return x;
}

// The serial twin.  The larger root goes under the smaller, so a component's
// root is its smallest node: walking the nodes in id order (image-major) meets
// the components in track order and each one's members in image order.
void host_build(const TracksInput& in, sfm_tracks& out) {
    empty_tracks(in, out);
    const int32_t N = in.n_space;
    std::vector<int32_t> parent((size_t)N);
    std::vector<uint8_t> touched((size_t)N, 0);
    for (int32_t v = 0; v < N; ++v) parent[v] = v;
    for (int32_t e = 0; e < in.n_edges; ++e) {
        touched[in.eu[e]] = touched[in.ev[e]] = 1;
        const int32_t a = find_root(parent, in.eu[e]), b = find_root(parent, in.ev[e]);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    // component sizes at the roots, then each component's slab in root order
    std::vector<int32_t> size((size_t)N, 0), slab_at((size_t)N, 0);
    int64_t n_nodes = 0;
    for (int32_t v = 0; v < N; ++v)
        if (touched[v]) {
            ++size[find_root(parent, v)];
            ++n_nodes;
        }
    std::vector<int32_t> roots;
    {
        int32_t at = 0;
        for (int32_t v = 0; v < N; ++v)
            if (size[v]) {
                roots.push_back(v);
                slab_at[v] = at;
                at += size[v];
            }
    }
    std::vector<int32_t> slab((size_t)n_nodes), fill(slab_at);
    for (int32_t v = 0; v < N; ++v)
        if (touched[v]) slab[fill[find_root(parent, v)]++] = v;
    sfm_tracks_stats& st = out.st;
    st.n_nodes = n_nodes;
    st.n_edges = in.n_edges;
    st.n_components = (int64_t)roots.size();
    std::vector<int32_t> img;
    for (const int32_t r : roots) {
        const int32_t n = size[r];
        const int32_t* m = &slab[slab_at[r]];
        bool conflict = n > in.n_img;   // pigeonhole
        if (!conflict) {
            img.resize(n);
            for (int32_t k = 0; k < n; ++k)   // the image I with feat_off[I] <= m[k] < feat_off[I + 1]
                img[k] = (int32_t)(std::upper_bound(in.feat_off, in.feat_off + in.n_img + 1, m[k]) - in.feat_off) - 1;
            for (int32_t k = 1; k < n; ++k) conflict |= img[k] == img[k - 1];   // (members are in image order)
        }
        if (conflict) {
            ++st.n_conflict;
            continue;
        }
        if (n < in.min_len) {
            ++st.n_short;
            continue;
        }
        for (int32_t k = 0; k < n; ++k) {
            out.obs_img.push_back(img[k]);
            out.obs_feat.push_back((uint32_t)(m[k] - in.feat_off[img[k]]));
            if (in.xy) {
                out.obs_uv.push_back(in.xy[2 * (size_t)m[k]]);
                out.obs_uv.push_back(in.xy[2 * (size_t)m[k] + 1]);
            }
        }
        out.pt_offsets.push_back((int64_t)out.obs_img.size());
        ++st.n_tracks;
        st.n_obs += n;
        st.max_track_len = std::max<int64_t>(st.max_track_len, n);
    }
}

}  // namespace

extern "C" int sfm_tracks_build_host(int32_t n_img, const int64_t* feat_off, int64_t n_pairs, const int32_t* pairs,
                                     const int64_t* counts, const uint32_t* i, const uint32_t* j, const double* xy,
                                     const sfm_tracks_opts* opts, sfm_tracks** out) {
    return guarded([&] {
        const sfm_tracks_opts O = tracks_options(opts);
        SFM_REQUIRE(out, SFM_ERR_INVALID_ARG, "null output");
        Staged s;
        stage(n_img, feat_off, n_pairs, pairs, counts, i, j, s);
        auto t = std::make_unique<sfm_tracks>();
        host_build(s.input(n_img, xy, O.min_track_len), *t);
        *out = t.release();
        return SFM_OK;
    });
}

extern "C" int sfm_tracks_get_stats(sfm_tracks* t, sfm_tracks_stats* stats) {
    return guarded([&] {
        SFM_REQUIRE(t && stats, SFM_ERR_INVALID_ARG, "null argument");
        *stats = t->st;
        return SFM_OK;
    });
}

extern "C" int sfm_tracks_fetch(sfm_tracks* t, int64_t* pt_offsets, int32_t* obs_img, uint32_t* obs_feat,
                                double* obs_uv) {
    return guarded([&] {
        SFM_REQUIRE(t, SFM_ERR_INVALID_ARG, "null tracks");
        SFM_REQUIRE(!obs_uv || t->has_uv, SFM_ERR_INVALID_ARG, "obs_uv asked of tracks built without xy");
        if (pt_offsets) std::copy(t->pt_offsets.begin(), t->pt_offsets.end(), pt_offsets);
        if (obs_img) std::copy(t->obs_img.begin(), t->obs_img.end(), obs_img);
        if (obs_feat) std::copy(t->obs_feat.begin(), t->obs_feat.end(), obs_feat);
        if (obs_uv) std::copy(t->obs_uv.begin(), t->obs_uv.end(), obs_uv);
        return SFM_OK;
    });
}

extern "C" int sfm_tracks_destroy(sfm_tracks* t) {
    return guarded([&] {
        delete t;
        return SFM_OK;
    });
}

#ifndef SFM_TRACKS_HOST_ONLY
extern "C" int sfm_tracks_build(sfm_ctx* ctx, int32_t n_img, const int64_t* feat_off, int64_t n_pairs,
                                const int32_t* pairs, const int64_t* counts, const uint32_t* i, const uint32_t* j,
                                const double* xy, const sfm_tracks_opts* opts, sfm_tracks** out) {
    return guarded([&] {
        const sfm_tracks_opts O = tracks_options(opts);
        SFM_REQUIRE(ctx && out, SFM_ERR_INVALID_ARG, "null argument");
        Staged s;
        stage(n_img, feat_off, n_pairs, pairs, counts, i, j, s);   // every check, before any device call
        const TracksInput in = s.input(n_img, xy, O.min_track_len);
        auto t = std::make_unique<sfm_tracks>();
        if (in.n_edges == 0) {
            empty_tracks(in, *t);
            if (ctx->time_kernels) ctx->last_kernel_ms = 0.0;   // (no kernel ran)
        } else {
            CtxScope scope_(ctx);
            tracks_device_build(ctx, in, *t);
        }
        *out = t.release();
        return SFM_OK;
    });
}

extern "C" int sfm_sparse_tracks(sfm_ctx* ctx, const char* matches_dir, const char* matches_file,
                                 const sfm_tracks_opts* opts, sfm_tracks** out) {
    return guarded([&] {
        SFM_REQUIRE(ctx && matches_dir && out, SFM_ERR_INVALID_ARG, "null argument");
        auto ok = [](int rc) {
            if (rc != SFM_OK) throw SfmError{rc};
        };
        std::string dir(matches_dir);
        if (!dir.empty() && dir.back() != '/') dir += '/';
        // the views: image I = the I-th view in id_view order
        const std::string data = dir + "sfm_data.json";
        int32_t n_img = 0;
        ok(sfm_mvg_load_views(data.c_str(), nullptr, 0, &n_img));
        std::vector<sfm_mvg_view> views((size_t)std::max(n_img, 1));
        ok(sfm_mvg_load_views(data.c_str(), views.data(), n_img, &n_img));
        std::map<uint32_t, int32_t> slot;
        for (int32_t k = 0; k < n_img; ++k) slot[views[k].id_view] = k;
        // <stem>.feat of every view: the counts, and x y as xy
        std::vector<int64_t> off((size_t)n_img + 1, 0);
        std::vector<double> xy;
        std::vector<float> feat;
        for (int32_t k = 0; k < n_img; ++k) {
            std::string stem(views[k].img_path);   // stlplus::basename_part
            const size_t sl = stem.find_last_of('/');
            if (sl != std::string::npos) stem = stem.substr(sl + 1);
            const size_t dot = stem.find_last_of('.');
            if (dot != std::string::npos && dot > 0) stem = stem.substr(0, dot);
            const std::string path = dir + stem + ".feat";
            int64_t n = 0;
            ok(sfm_mvg_read_feat(path.c_str(), nullptr, 0, &n));
            feat.resize(4 * (size_t)std::max<int64_t>(n, 1));
            ok(sfm_mvg_read_feat(path.c_str(), feat.data(), n, &n));
            off[k + 1] = off[k] + n;
            for (int64_t f = 0; f < n; ++f) {
                xy.push_back(feat[4 * f]);
                xy.push_back(feat[4 * f + 1]);
            }
        }
        if (xy.empty()) xy.push_back(0.0);   // (a non-null xy: the handle serves obs_uv)
        const std::string mpath = dir + (matches_file ? matches_file : "matches.f.bin");
        int64_t np = 0, nm = 0;
        ok(sfm_mvg_load_matches(mpath.c_str(), nullptr, nullptr, nullptr, nullptr, 0, 0, &np, &nm));
        std::vector<int32_t> pairs(2 * (size_t)std::max<int64_t>(np, 1));
        std::vector<int64_t> counts((size_t)std::max<int64_t>(np, 1));
        std::vector<uint32_t> mi((size_t)std::max<int64_t>(nm, 1)), mj(mi.size());
        ok(sfm_mvg_load_matches(mpath.c_str(), pairs.data(), counts.data(), mi.data(), mj.data(), np, nm, &np, &nm));
        for (int64_t q = 0; q < 2 * np; ++q) {   // view ids -> image indices
            const auto it = slot.find((uint32_t)pairs[q]);
            SFM_REQUIRE(it != slot.end(), SFM_ERR_INVALID_ARG, "matches reference view %d not in sfm_data.json",
                        pairs[q]);
            pairs[q] = it->second;
        }
        ok(sfm_tracks_build(ctx, n_img, off.data(), np, pairs.data(), counts.data(), mi.data(), mj.data(), xy.data(),
                            opts, out));
        return SFM_OK;
    });
}
#endif
