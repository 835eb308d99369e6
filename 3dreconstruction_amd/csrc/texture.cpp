// Mesh texturing, host side (include/sfmcore.h, "Mesh texture"): the argument
// checks (the images': dense_views.cpp), the atlas fit, the host twins (face
// views: threads over chunks of faces, an atomic minimum per covered pixel;
// bake: threads over rows of the atlas), the textured PLY (dense_ply.cpp) and
// the entry points over either backend.  The kernels and the transfers are
// texture.hip's.  SFM_DEPTHMAP_HOST_ONLY leaves the device entry points out
// (tests/cpp/texture_test.cpp).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dense_ply.h"
#include "texture.h"

using namespace sfm;

namespace {

enum : int { kViews = 1, kBake = 2 };
constexpr size_t kFaceChunk = 1024;   // faces a task of the host twin

void atlas_fit(const char* who, int64_t n_triangles, int32_t cell, TexAtlas& A) {
    SFM_REQUIRE(n_triangles >= 0, SFM_ERR_INVALID_ARG, "%s: negative n_triangles", who);
    SFM_REQUIRE(cell >= kTexMinCell && cell <= kTexMaxCell, SFM_ERR_INVALID_ARG, "%s: cell is %d, outside %d .. %d", who, cell,
                kTexMinCell, kTexMaxCell);
    SFM_REQUIRE(n_triangles < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED, "%s: 2^31 triangles or more", who);
    const int64_t n_sq = (n_triangles + 1) / 2;
    int64_t cols = (int64_t)std::sqrt((double)n_sq);
    while (cols * cols < n_sq) ++cols;
    while (cols > 0 && (cols - 1) * (cols - 1) >= n_sq) --cols;
    const int64_t rows = cols ? (n_sq + cols - 1) / cols : 0;
    SFM_REQUIRE(cols * cell <= kTexMaxAtlas && rows * cell <= kTexMaxAtlas, SFM_ERR_UNSUPPORTED,
                "%s: an atlas of %lld x %lld texels is beyond %d", who, (long long)(cols * cell), (long long)(rows * cell),
                kTexMaxAtlas);
    A.s = cell;
    A.cols = (int32_t)cols;
    A.W = (int32_t)(cols * cell);
    A.H = (int32_t)(rows * cell);
}

void prepare(const char* who, int mode, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
             const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices, const float* V,
             const uint8_t* vertex_rgb, int64_t n_triangles, const int32_t* tri, const int32_t* face_view,
             const sfm_mesh_texture_opts* opts, TexProblem& P, int64_t* resident_bytes) {
    sfm_mesh_texture_opts o;
    sfm_mesh_texture_default_options(&o);
    if (opts) o = *opts;
    SFM_REQUIRE(o.device_bytes >= 0, SFM_ERR_INVALID_ARG, "%s: negative device_bytes", who);
    SFM_REQUIRE(n_img >= 0 && n_vertices >= 0 && n_triangles >= 0, SFM_ERR_INVALID_ARG, "%s: a negative count", who);
    SFM_REQUIRE(n_img == 0 || (wh && K && R && C), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    SFM_REQUIRE(!pixels || (channels && img_off), SFM_ERR_INVALID_ARG, "%s: pixels without channels or img_off", who);
    SFM_REQUIRE((n_vertices == 0 || V) && (n_triangles == 0 || tri), SFM_ERR_INVALID_ARG, "%s: null V or tri", who);
    SFM_REQUIRE(n_vertices < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED, "%s: 2^31 vertices or more", who);
    atlas_fit(who, n_triangles, o.cell, P.atlas);
    std::memcpy(P.fill, o.fill, 3);
    P.n_vertices = n_vertices;
    P.n_triangles = n_triangles;
    dense_images_prepare(who, n_img, wh, channels, img_off, pixels, K, R, C, P.images);
    P.views.resize((size_t)n_img);
    const bool sample = (mode & kBake) != 0;
    for (int32_t i = 0; i < n_img; ++i) {
        const DenseImage& I = P.images.img[(size_t)i];
        TexView& T = P.views[(size_t)i];
        std::memset(&T, 0, sizeof T);
        dense_KR(K, R, i, T.M);
        dense_C(C, i, T.C);
        T.w = I.w;
        T.h = I.h;
        T.channels = I.channels;
        T.loaded = I.loaded;
        T.pix_off = I.pix_off;
        if (T.loaded) P.max_pixels = std::max(P.max_pixels, (int64_t)T.w * T.h);
    }
    for (int64_t k = 0; k < 3 * n_vertices; ++k)
        SFM_REQUIRE(std::isfinite(V[k]), SFM_ERR_INVALID_ARG, "%s: vertex %lld is not finite", who, (long long)(k / 3));
    require_triangles(who, n_triangles, tri, n_vertices);
    if (face_view)
        for (int64_t f = 0; f < n_triangles; ++f) {
            const int32_t v = face_view[f];
            SFM_REQUIRE(v >= -1 && v < n_img, SFM_ERR_INVALID_ARG, "%s: face %lld has the view %d of %d", who, (long long)f, v,
                        n_img);
            SFM_REQUIRE(v < 0 || P.views[(size_t)v].channels, SFM_ERR_INVALID_ARG, "%s: face %lld names image %d, which is skipped",
                        who, (long long)f, v);
        }
    int64_t bytes = (int64_t)(P.views.size() * sizeof(TexView)) + 12 * n_vertices + 24 * n_triangles;
    if (mode & kViews) bytes += 8 * P.max_pixels;
    if (sample)
        bytes += (P.images.pool_hi - P.images.pool_lo) + (vertex_rgb ? 3 * n_vertices : 0) + 3 * (int64_t)P.atlas.W * P.atlas.H + 24 * n_triangles;
    *resident_bytes = bytes;
    const int64_t budget = o.device_bytes > 0 ? o.device_bytes : kTexDefaultDeviceBytes;
    SFM_REQUIRE(bytes <= budget, SFM_ERR_UNSUPPORTED,
                "%s: the images, the mesh, the identity buffer and the texture need %lld resident bytes, device_bytes is %lld "
                "(streaming is not built)",
                who, (long long)bytes, (long long)budget);
}

void atomic_min(uint64_t* p, uint64_t key) {
    uint64_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (key < cur && !__atomic_compare_exchange_n(p, &cur, key, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {
    }
}

void face_views_host(const TexProblem& P, const float* V, const int32_t* tri, int32_t* face_view, int32_t* face_pixels,
                     sfm_mesh_face_views_stats* st) {
    const size_t n = (size_t)P.n_triangles, chunks = (n + kFaceChunk - 1) / kFaceChunk;
    std::fill(face_view, face_view + n, -1);
    std::fill(face_pixels, face_pixels + n, 0);
    std::vector<uint64_t> id((size_t)P.max_pixels);
    std::vector<int64_t> refused(chunks, 0);
    for (int32_t v = 0; v < P.images.n_img; ++v) {
        const TexView& T = P.views[(size_t)v];
        if (!T.loaded) continue;
        std::fill(id.begin(), id.begin() + (size_t)T.w * T.h, ~(uint64_t)0);
        dense_parallel_for(chunks, [&](size_t c) {
            for (size_t f = c * kFaceChunk; f < std::min(n, (c + 1) * kFaceChunk); ++f) {
                TexFace F;
                if (!tex_face_setup(T, V, tri, (int64_t)f, F)) {
                    ++refused[c];
                    continue;
                }
                if (!F.box()) continue;
                for (int32_t py = F.py0; py <= F.py1; ++py)
                    for (int32_t px = F.px0; px <= F.px1; ++px) {
                        uint64_t key;
                        if (tex_pixel(F, (uint32_t)f, px, py, &key)) atomic_min(&id[(size_t)py * T.w + px], key);
                    }
            }
        });
        dense_parallel_for(chunks, [&](size_t c) {
            for (size_t f = c * kFaceChunk; f < std::min(n, (c + 1) * kFaceChunk); ++f) {
                TexFace F;
                if (!tex_face_setup(T, V, tri, (int64_t)f, F) || !F.box()) continue;
                int64_t covered = 0, won = 0;
                for (int32_t py = F.py0; py <= F.py1; ++py)
                    for (int32_t px = F.px0; px <= F.px1; ++px) {
                        uint64_t key;
                        if (!tex_pixel(F, (uint32_t)f, px, py, &key)) continue;
                        ++covered;
                        won += (uint32_t)id[(size_t)py * T.w + px] == (uint32_t)f;
                    }
                tex_score(F, true, covered, won, v, &face_view[f], &face_pixels[f]);
            }
        });
    }
    for (int64_t r : refused) st->n_not_drawable += r;
    for (size_t f = 0; f < n; ++f) {
        st->n_textured += face_view[f] >= 0;
        st->sum_pixels += face_pixels[f];
    }
    st->n_untextured = P.n_triangles - st->n_textured;
}

void bake_host(const TexProblem& P, const uint8_t* pixels, const float* V, const uint8_t* vertex_rgb, const int32_t* tri,
               const int32_t* face_view, uint8_t* texture, float* uv) {
    const TexAtlas& A = P.atlas;
    const uint32_t fill = tex_pack(P.fill);
    dense_parallel_for((size_t)A.H, [&](size_t row) {
        const int32_t ty = (int32_t)row;
        for (int32_t tx = 0; tx < A.W; ++tx) {
            uint8_t* out = texture + 3 * ((size_t)ty * A.W + tx);
            float l1, l2;
            const int64_t f = tex_texel_face(A, P.n_triangles, tx, ty, &l1, &l2);
            uint32_t rgb = fill;
            if (f >= 0)
                rgb = face_view[f] < 0 ? tex_fallback(vertex_rgb, tri, f, l1, l2, fill)
                                       : tex_sample(P.views[(size_t)face_view[f]], pixels, V, tri, f, l1, l2, fill);
            tex_unpack(rgb, out);
        }
    });
    for (int64_t f = 0; f < P.n_triangles; ++f) tex_uv(A, f, uv + 6 * f);
}

void bake_stats(const TexProblem& P, int64_t resident, sfm_mesh_bake_stats* st) {
    st->W = P.atlas.W;
    st->H = P.atlas.H;
    st->cols = P.atlas.cols;
    st->resident_bytes = resident;
}

int face_views(const char* who, sfm_ctx* ctx, bool device, int32_t n_img, const int32_t* wh, const int32_t* channels,
               const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R, const double* C,
               int64_t n_vertices, const float* V, int64_t n_triangles, const int32_t* tri, const sfm_mesh_texture_opts* opts,
               int32_t* face_view, int32_t* face_pixels, sfm_mesh_face_views_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    TexProblem P;
    sfm_mesh_face_views_stats st;
    std::memset(&st, 0, sizeof st);
    prepare(who, kViews, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, nullptr, n_triangles, tri, nullptr, opts,
            P, &st.resident_bytes);
    SFM_REQUIRE(n_triangles == 0 || (face_view && face_pixels), SFM_ERR_INVALID_ARG, "%s: null face_view or face_pixels", who);
    if (n_triangles > 0) {
        if (device) {
#ifndef SFM_DEPTHMAP_HOST_ONLY
            tex_face_views_device(ctx, P, V, tri, face_view, face_pixels, &st);
#endif
        } else {
            const double t0 = seconds_now();
            face_views_host(P, V, tri, face_view, face_pixels, &st);
            st.seconds[1] = seconds_now() - t0;
        }
    }
    if (stats) *stats = st;
    return SFM_OK;
}

int bake(const char* who, sfm_ctx* ctx, bool device, int32_t n_img, const int32_t* wh, const int32_t* channels,
         const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
         const float* V, const uint8_t* vertex_rgb, int64_t n_triangles, const int32_t* tri, const int32_t* face_view,
         const sfm_mesh_texture_opts* opts, uint8_t* texture, float* uv, sfm_mesh_bake_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    SFM_REQUIRE(n_triangles <= 0 || face_view, SFM_ERR_INVALID_ARG, "%s: null face_view", who);
    TexProblem P;
    sfm_mesh_bake_stats st;
    std::memset(&st, 0, sizeof st);
    int64_t resident = 0;
    prepare(who, kBake, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb, n_triangles, tri, face_view,
            opts, P, &resident);
    bake_stats(P, resident, &st);
    SFM_REQUIRE(n_triangles == 0 || (texture && uv), SFM_ERR_INVALID_ARG, "%s: null texture or uv", who);
    if (n_triangles > 0) {
        if (device) {
#ifndef SFM_DEPTHMAP_HOST_ONLY
            tex_bake_device(ctx, P, pixels, V, vertex_rgb, tri, face_view, texture, uv, &st);
#endif
        } else {
            const double t0 = seconds_now();
            bake_host(P, pixels ? pixels + P.images.pool_lo : nullptr, V, vertex_rgb, tri, face_view, texture, uv);
            st.seconds[1] = seconds_now() - t0;
        }
    }
    if (stats) *stats = st;
    return SFM_OK;
}

// the checks of sfm_mesh_texture: both calls', before anything runs
void prepare_texture(const char* who, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                     const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
                     const float* V, const uint8_t* vertex_rgb, int64_t n_triangles, const int32_t* tri,
                     const sfm_mesh_texture_opts* opts, const uint8_t* texture, const float* uv, TexProblem& P,
                     sfm_mesh_texture_stats* st) {
    // every image that could be chosen must be one the bake can sample
    SFM_REQUIRE(pixels || n_img <= 0, SFM_ERR_INVALID_ARG, "%s: null pixels", who);
    prepare(who, kViews | kBake, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb, n_triangles, tri,
            nullptr, opts, P, &st->resident_bytes);
    SFM_REQUIRE(n_triangles == 0 || (texture && uv), SFM_ERR_INVALID_ARG, "%s: null texture or uv", who);
    bake_stats(P, st->resident_bytes, &st->bake);
    st->views.resident_bytes = st->resident_bytes;
}

}  // namespace

extern "C" void sfm_mesh_texture_default_options(sfm_mesh_texture_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->cell = kTexDefaultCell;
}

extern "C" int sfm_mesh_atlas_fit(int64_t n_triangles, int32_t cell, int32_t* W, int32_t* H, int32_t* cols) {
    return guarded([&] {
        const char* who = "sfm_mesh_atlas_fit";
        SFM_REQUIRE(W && H && cols, SFM_ERR_INVALID_ARG, "%s: null argument", who);
        TexAtlas A;
        atlas_fit(who, n_triangles, cell, A);
        *W = A.W;
        *H = A.H;
        *cols = A.cols;
        return (int)SFM_OK;
    });
}

extern "C" int sfm_mesh_face_views_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                        const uint8_t* pixels, const double* K, const double* R, const double* C,
                                        int64_t n_vertices, const float* V, int64_t n_triangles, const int32_t* tri,
                                        const sfm_mesh_texture_opts* opts, int32_t* face_view, int32_t* face_pixels,
                                        sfm_mesh_face_views_stats* stats) {
    return guarded([&] {
        return face_views("sfm_mesh_face_views_host", nullptr, false, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V,
                          n_triangles, tri, opts, face_view, face_pixels, stats);
    });
}

extern "C" int sfm_mesh_texture_bake_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                          const uint8_t* pixels, const double* K, const double* R, const double* C,
                                          int64_t n_vertices, const float* V, const uint8_t* vertex_rgb, int64_t n_triangles,
                                          const int32_t* tri, const int32_t* face_view, const sfm_mesh_texture_opts* opts,
                                          uint8_t* texture, float* uv, sfm_mesh_bake_stats* stats) {
    return guarded([&] {
        return bake("sfm_mesh_texture_bake_host", nullptr, false, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V,
                    vertex_rgb, n_triangles, tri, face_view, opts, texture, uv, stats);
    });
}

extern "C" int sfm_mesh_texture_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                     const uint8_t* pixels, const double* K, const double* R, const double* C,
                                     int64_t n_vertices, const float* V, const uint8_t* vertex_rgb, int64_t n_triangles,
                                     const int32_t* tri, const sfm_mesh_texture_opts* opts, int32_t* face_view,
                                     int32_t* face_pixels, uint8_t* texture, float* uv, sfm_mesh_texture_stats* stats) {
    return guarded([&] {
        const char* who = "sfm_mesh_texture_host";
        sfm_mesh_texture_stats st;
        std::memset(&st, 0, sizeof st);
        TexProblem P;
        prepare_texture(who, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb, n_triangles, tri, opts,
                        texture, uv, P, &st);
        const int64_t resident = st.resident_bytes;
        std::vector<int32_t> fv, fp;
        if (!face_view) fv.resize((size_t)std::max<int64_t>(n_triangles, 1)), face_view = fv.data();
        if (!face_pixels) fp.resize((size_t)std::max<int64_t>(n_triangles, 1)), face_pixels = fp.data();
        int rc = sfm_mesh_face_views_host(n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, n_triangles, tri, opts,
                                          face_view, face_pixels, &st.views);
        if (rc == SFM_OK)
            rc = sfm_mesh_texture_bake_host(n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb, n_triangles,
                                            tri, face_view, opts, texture, uv, &st.bake);
        st.views.resident_bytes = st.bake.resident_bytes = st.resident_bytes = resident;
        st.seconds[1] = st.views.seconds[1] + st.bake.seconds[1];
        if (stats) *stats = st;
        return rc;
    });
}

extern "C" int sfm_mesh_write_textured_ply(const char* path, const char* texture_name, int64_t n_vertices, const float* V,
                                           int64_t n_triangles, const int32_t* tri, const float* uv) {
    return guarded([&] {
        const char* who = "sfm_mesh_write_textured_ply";
        SFM_REQUIRE(path && texture_name && n_vertices >= 0 && n_triangles >= 0 && (n_vertices == 0 || V) &&
                        (n_triangles == 0 || (tri && uv)),
                    SFM_ERR_INVALID_ARG, "%s: null path, name, V, tri or uv, or a negative count", who);
        SFM_REQUIRE(!std::strpbrk(texture_name, "\r\n"), SFM_ERR_INVALID_ARG, "%s: the texture's name holds a line break", who);
        require_triangles(who, n_triangles, tri, n_vertices);
        PlyWriter ply(who, path,
                      std::string("comment TextureFile ") + texture_name + "\nelement vertex " + std::to_string(n_vertices) +
                          "\nproperty float x\nproperty float y\nproperty float z\nelement face " + std::to_string(n_triangles) +
                          "\nproperty list uchar int vertex_indices\nproperty list uchar float texcoord\n");
        ply.records(n_vertices, 12, [&](int64_t k, uint8_t* p) { std::memcpy(p, V + 3 * k, 12); });
        ply.records(n_triangles, 38, [&](int64_t k, uint8_t* p) {
            p[0] = 3;
            std::memcpy(p + 1, tri + 3 * k, 12);
            p[13] = 6;
            std::memcpy(p + 14, uv + 6 * k, 24);
        });
        ply.close();
        return (int)SFM_OK;
    });
}

#ifndef SFM_DEPTHMAP_HOST_ONLY
extern "C" int sfm_mesh_face_views(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels,
                                   const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R,
                                   const double* C, int64_t n_vertices, const float* V, int64_t n_triangles, const int32_t* tri,
                                   const sfm_mesh_texture_opts* opts, int32_t* face_view, int32_t* face_pixels,
                                   sfm_mesh_face_views_stats* stats) {
    return guarded([&] {
        return face_views("sfm_mesh_face_views", ctx, true, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V,
                          n_triangles, tri, opts, face_view, face_pixels, stats);
    });
}

extern "C" int sfm_mesh_texture_bake(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels,
                                     const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R,
                                     const double* C, int64_t n_vertices, const float* V, const uint8_t* vertex_rgb,
                                     int64_t n_triangles, const int32_t* tri, const int32_t* face_view,
                                     const sfm_mesh_texture_opts* opts, uint8_t* texture, float* uv, sfm_mesh_bake_stats* stats) {
    return guarded([&] {
        return bake("sfm_mesh_texture_bake", ctx, true, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb,
                    n_triangles, tri, face_view, opts, texture, uv, stats);
    });
}

extern "C" int sfm_mesh_texture(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                const uint8_t* pixels, const double* K, const double* R, const double* C, int64_t n_vertices,
                                const float* V, const uint8_t* vertex_rgb, int64_t n_triangles, const int32_t* tri,
                                const sfm_mesh_texture_opts* opts, int32_t* face_view, int32_t* face_pixels, uint8_t* texture,
                                float* uv, sfm_mesh_texture_stats* stats) {
    return guarded([&] {
        const char* who = "sfm_mesh_texture";
        SFM_REQUIRE(ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
        sfm_mesh_texture_stats st;
        std::memset(&st, 0, sizeof st);
        TexProblem P;
        prepare_texture(who, n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb, n_triangles, tri, opts,
                        texture, uv, P, &st);
        if (n_triangles > 0) tex_texture_device(ctx, P, pixels, V, vertex_rgb, tri, face_view, face_pixels, texture, uv, &st);
        if (stats) *stats = st;
        return (int)SFM_OK;
    });
}
#endif
