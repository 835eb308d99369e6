// The mesh stage, host side (include/sfmcore.h, "Mesh"): the argument checks
// (the images': dense_views.cpp), the grid fit, the host twins (threads over
// rows of the lattice: integration; marks, a prefix over the points, vertices
// and triangles), the mesh's PLY (dense_ply.cpp) and the entry points over
// either backend.  The kernels and the transfers are mesh.hip's.  SFM_DEPTHMAP_HOST_ONLY
// leaves the device entry points out (tests/cpp/mesh_test.cpp).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dense_ply.h"
#include "mesh.h"

using namespace sfm;

namespace {

void prepare_grid(const char* who, const sfm_mesh_grid* grid, MeshGrid& g, int64_t* n_vox) {
    SFM_REQUIRE(grid, SFM_ERR_INVALID_ARG, "%s: null grid", who);
    SFM_REQUIRE(grid->voxel > 0.0f && std::isfinite(grid->voxel), SFM_ERR_INVALID_ARG,
                "%s: the voxel is %g, not positive and finite", who, (double)grid->voxel);
    for (int c = 0; c < 3; ++c) {
        SFM_REQUIRE(std::isfinite(grid->origin[c]), SFM_ERR_INVALID_ARG, "%s: the origin is not finite", who);
        SFM_REQUIRE(grid->dims[c] >= 1, SFM_ERR_INVALID_ARG, "%s: dims are %d %d %d, each must be at least 1", who,
                    grid->dims[0], grid->dims[1], grid->dims[2]);
    }
    const int64_t nxy = (int64_t)grid->dims[0] * grid->dims[1];
    SFM_REQUIRE(nxy < ((int64_t)1 << 31) && nxy * grid->dims[2] < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED,
                "%s: a grid of %d x %d x %d has 2^31 lattice points or more", who, grid->dims[0], grid->dims[1],
                grid->dims[2]);
    SFM_REQUIRE(grid->dims[1] <= kMeshMaxNy && grid->dims[2] <= kMeshMaxNz, SFM_ERR_UNSUPPORTED,
                "%s: ny is above %d or nz above %d", who, kMeshMaxNy, kMeshMaxNz);
    std::memcpy(&g, grid, sizeof g);
    g.pad = 0;
    *n_vox = nxy * grid->dims[2];
}

void prepare_tsdf(const char* who, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                  const uint8_t* pixels, const double* K, const double* R, const double* C, const float* depth,
                  const sfm_mesh_grid* grid, const sfm_tsdf_opts* opts, MeshProblem& P, int64_t* resident_bytes) {
    sfm_tsdf_opts o;
    sfm_tsdf_default_options(&o);
    if (opts) o = *opts;
    SFM_REQUIRE(o.trunc >= 0.0f && std::isfinite(o.trunc), SFM_ERR_INVALID_ARG,
                "%s: trunc is negative or not a number", who);
    SFM_REQUIRE(o.device_bytes >= 0, SFM_ERR_INVALID_ARG, "%s: negative device_bytes", who);
    prepare_grid(who, grid, P.g, &P.n_vox);
    P.trunc = o.trunc > 0.0f ? o.trunc : 3.0f * P.g.voxel;
    SFM_REQUIRE(n_img >= 0, SFM_ERR_INVALID_ARG, "%s: negative n_img", who);
    SFM_REQUIRE(n_img == 0 || (wh && K && R && C), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    SFM_REQUIRE(!pixels || (channels && img_off), SFM_ERR_INVALID_ARG, "%s: pixels without channels or img_off", who);
    dense_images_prepare(who, n_img, wh, channels, img_off, pixels, K, R, C, P.images);
    P.views.resize((size_t)n_img);
    for (int32_t i = 0; i < n_img; ++i) {
        const DenseImage& I = P.images.img[(size_t)i];
        MeshView& V = P.views[(size_t)i];
        std::memset(&V, 0, sizeof V);
        dense_KR(K, R, i, V.M);
        dense_C(C, i, V.C);
        V.w = I.w;
        V.h = I.h;
        V.channels = I.channels;
        V.loaded = I.loaded;
        V.map_off = I.map_off;
        V.pix_off = I.pix_off;
    }
    SFM_REQUIRE(P.images.n_map == 0 || depth, SFM_ERR_INVALID_ARG, "%s: null depth", who);
    *resident_bytes = P.images.n_map * (int64_t)sizeof(float) + (P.images.pool_hi - P.images.pool_lo) +
                      (int64_t)(P.views.size() * sizeof(MeshView)) + P.n_vox * 9 +
                      mesh_blocks(P.n_vox) * (int64_t)(sizeof(int32_t) + sizeof(int64_t));
    const int64_t budget = o.device_bytes > 0 ? o.device_bytes : kMeshDefaultDeviceBytes;
    SFM_REQUIRE(*resident_bytes <= budget, SFM_ERR_UNSUPPORTED,
                "%s: the maps, colours and volume need %lld resident bytes, device_bytes is %lld (streaming is not built)",
                who, (long long)*resident_bytes, (long long)budget);
}

int32_t prepare_extract(const char* who, const sfm_mesh_grid* grid, const float* tsdf, const uint8_t* weight,
                        const uint8_t* rgb, const uint8_t* has_rgb, const sfm_mesh_opts* opts, const MeshOut& out,
                        bool volume_given, MeshGrid& g, int64_t* n_vox) {
    sfm_mesh_opts o;
    sfm_mesh_default_options(&o);
    if (opts) o = *opts;
    prepare_grid(who, grid, g, n_vox);
    SFM_REQUIRE(o.min_weight >= 1 && o.min_weight <= 255, SFM_ERR_INVALID_ARG, "%s: min_weight is %d, outside 1 .. 255", who,
                o.min_weight);
    SFM_REQUIRE(out.cap_vertices >= 0 && out.cap_triangles >= 0, SFM_ERR_INVALID_ARG,
                "%s: negative cap_vertices or cap_triangles", who);
    SFM_REQUIRE((out.cap_vertices == 0 || out.V) && (out.cap_triangles == 0 || out.tri), SFM_ERR_INVALID_ARG,
                "%s: null V or tri", who);
    if (volume_given) {
        SFM_REQUIRE(tsdf && weight, SFM_ERR_INVALID_ARG, "%s: null tsdf or weight", who);
        SFM_REQUIRE(!rgb == !has_rgb, SFM_ERR_INVALID_ARG, "%s: rgb and has_rgb go together", who);
    }
    return o.min_weight;
}

// a row of the lattice: the points (0 .. nx - 1, j, k), row = k ny + j
void tsdf_host(const MeshProblem& P, const float* depth, const uint8_t* pixels, float* tsdf, uint8_t* weight,
               uint8_t* rgb, uint8_t* has_rgb, int64_t* n_observed) {
    const MeshGrid& g = P.g;
    const size_t rows = (size_t)g.ny * g.nz;
    std::vector<int64_t> seen(rows, 0);
    dense_parallel_for(rows, [&](size_t row) {
        const int32_t j = (int32_t)(row % (size_t)g.ny), k = (int32_t)(row / (size_t)g.ny);
        int64_t n = 0;
        for (int32_t i = 0; i < g.nx; ++i) {
            const int64_t at = mesh_raster(g, i, j, k);
            uint8_t c[3] = {0, 0, 0}, has = 0;
            const int32_t wgt = mesh_integrate_point(P.views.data(), P.images.n_img, g, P.trunc, depth, pixels, i, j, k, &tsdf[at], c, &has);
            weight[at] = (uint8_t)wgt;
            n += wgt > 0;
            if (pixels) {
                if (rgb) std::memcpy(rgb + 3 * at, c, 3);
                if (has_rgb) has_rgb[at] = has;
            }
        }
        seen[row] = n;
    });
    *n_observed = 0;
    for (int64_t n : seen) *n_observed += n;
}

void extract_host(const char* who, const MeshGrid& g, int64_t n_vox, int32_t min_weight, const float* tsdf,
                  const uint8_t* weight, const uint8_t* rgb, const uint8_t* has_rgb, const MeshOut& out,
                  sfm_mesh_stats* st) {
    const size_t rows = (size_t)g.ny * g.nz;
    std::vector<uint8_t> mask((size_t)n_vox), ntri((size_t)n_vox);
    std::vector<int32_t> vert_base((size_t)n_vox);
    std::vector<int64_t> row_v(rows + 1, 0), row_t(rows + 1, 0), row_d(rows, 0);
    dense_parallel_for(rows, [&](size_t row) {
        const int32_t j = (int32_t)(row % (size_t)g.ny), k = (int32_t)(row / (size_t)g.ny);
        int64_t nv = 0, nt = 0, nd = 0;
        for (int32_t i = 0; i < g.nx; ++i) {
            const int64_t at = mesh_raster(g, i, j, k);
            int32_t t, d;
            const uint32_t m = mesh_point_marks(g, tsdf, weight, min_weight, i, j, k, &t, &d);
            mask[(size_t)at] = (uint8_t)m;
            ntri[(size_t)at] = (uint8_t)t;
            nv += __builtin_popcount(m);
            nt += t;
            nd += d;
        }
        row_v[row + 1] = nv;
        row_t[row + 1] = nt;
        row_d[row] = nd;
    });
    st->n_degenerate = 0;
    for (size_t r = 0; r < rows; ++r) {
        row_v[r + 1] += row_v[r];
        row_t[r + 1] += row_t[r];
        st->n_degenerate += row_d[r];
    }
    st->n_vertices = row_v[rows];
    st->n_triangles = row_t[rows];
    mesh_require_indexable(who, st->n_vertices);
    mesh_require_caps(who, *st, out);
    dense_parallel_for(rows, [&](size_t row) {
        const int32_t j = (int32_t)(row % (size_t)g.ny), k = (int32_t)(row / (size_t)g.ny);
        int64_t rank = row_v[row];
        for (int32_t i = 0; i < g.nx; ++i) {
            const int64_t at = mesh_raster(g, i, j, k);
            vert_base[(size_t)at] = (int32_t)rank;
            for (int s = 0; s < 7; ++s)
                if ((mask[(size_t)at] >> s) & 1) {
                    uint8_t c[3] = {0, 0, 0};
                    mesh_edge_vertex(g, tsdf, rgb, has_rgb, i, j, k, s, out.V + 3 * rank, c);
                    if (rgb && out.rgb) std::memcpy(out.rgb + 3 * rank, c, 3);
                    ++rank;
                }
        }
    });
    dense_parallel_for(rows, [&](size_t row) {
        const int32_t j = (int32_t)(row % (size_t)g.ny), k = (int32_t)(row / (size_t)g.ny);
        int64_t rank = row_t[row];
        for (int32_t i = 0; i < g.nx; ++i) {
            const int64_t at = mesh_raster(g, i, j, k);
            if (ntri[(size_t)at]) rank += mesh_cell_triangles(g, tsdf, vert_base.data(), mask.data(), i, j, k, out.tri + 3 * rank);
        }
    });
}

int integrate(const char* who, sfm_ctx* ctx, bool device, int32_t n_img, const int32_t* wh, const int32_t* channels,
              const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R, const double* C,
              const float* depth, const sfm_mesh_grid* grid, const sfm_tsdf_opts* opts, float* tsdf, uint8_t* weight,
              uint8_t* rgb, uint8_t* has_rgb, sfm_tsdf_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    MeshProblem P;
    sfm_tsdf_stats st;
    std::memset(&st, 0, sizeof st);
    prepare_tsdf(who, n_img, wh, channels, img_off, pixels, K, R, C, depth, grid, opts, P, &st.resident_bytes);
    SFM_REQUIRE(tsdf && weight, SFM_ERR_INVALID_ARG, "%s: null tsdf or weight", who);
    SFM_REQUIRE(!pixels || (rgb && has_rgb), SFM_ERR_INVALID_ARG, "%s: pixels without rgb or has_rgb", who);
    if (device) {
#ifndef SFM_DEPTHMAP_HOST_ONLY
        tsdf_device(ctx, P, depth, pixels, tsdf, weight, rgb, has_rgb, &st.n_observed, st.seconds);
#endif
    } else {
        const double t0 = seconds_now();
        tsdf_host(P, depth, pixels ? pixels + P.images.pool_lo : nullptr, tsdf, weight, rgb, has_rgb, &st.n_observed);
        st.seconds[1] = seconds_now() - t0;
    }
    if (stats) *stats = st;
    return SFM_OK;
}

int extract(const char* who, sfm_ctx* ctx, bool device, const sfm_mesh_grid* grid, const float* tsdf,
            const uint8_t* weight, const uint8_t* rgb, const uint8_t* has_rgb, const sfm_mesh_opts* opts,
            const MeshOut& out, sfm_mesh_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    MeshGrid g;
    int64_t n_vox = 0;
    sfm_mesh_stats st;
    std::memset(&st, 0, sizeof st);
    const int32_t min_weight = prepare_extract(who, grid, tsdf, weight, rgb, has_rgb, opts, out, true, g, &n_vox);
    try {
        if (device) {
#ifndef SFM_DEPTHMAP_HOST_ONLY
            mesh_extract_device(ctx, g, min_weight, tsdf, weight, rgb, has_rgb, out, &st);
#endif
        } else {
            const double t0 = seconds_now();
            extract_host(who, g, n_vox, min_weight, tsdf, weight, rgb, has_rgb, out, &st);
            st.seconds[1] = seconds_now() - t0;
        }
    } catch (const SfmError&) {
        if (stats) *stats = st;   // a cap too small: the needs
        throw;
    }
    if (stats) *stats = st;
    return SFM_OK;
}

}  // namespace

namespace sfm {

void mesh_require_caps(const char* who, const sfm_mesh_stats& st, const MeshOut& out) {
    SFM_REQUIRE(st.n_vertices <= out.cap_vertices && st.n_triangles <= out.cap_triangles, SFM_ERR_INVALID_ARG,
                "%s: the mesh has %lld vertices and %lld triangles, cap_vertices is %lld and cap_triangles is %lld", who,
                (long long)st.n_vertices, (long long)st.n_triangles, (long long)out.cap_vertices,
                (long long)out.cap_triangles);
}

void mesh_require_indexable(const char* who, int64_t n_vertices) {
    SFM_REQUIRE(n_vertices <= 0x7fffffffLL, SFM_ERR_UNSUPPORTED, "%s: the mesh has %lld vertices, more than 2^31 - 1", who,
                (long long)n_vertices);
}

}  // namespace sfm

extern "C" void sfm_tsdf_default_options(sfm_tsdf_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
}

extern "C" void sfm_mesh_default_options(sfm_mesh_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->min_weight = 1;
}

extern "C" int sfm_mesh_grid_fit(int64_t n_points, const float* X, int32_t resolution, int32_t margin_voxels,
                                 sfm_mesh_grid* grid) {
    return guarded([&] {
        const char* who = "sfm_mesh_grid_fit";
        SFM_REQUIRE(n_points >= 1 && X && grid, SFM_ERR_INVALID_ARG, "%s: no points, or a null argument", who);
        SFM_REQUIRE(resolution >= 1 && margin_voxels >= 0, SFM_ERR_INVALID_ARG,
                    "%s: resolution below 1 or negative margin_voxels", who);
        double lo[3], hi[3];
        for (int c = 0; c < 3; ++c) lo[c] = hi[c] = (double)X[c];
        for (int64_t p = 0; p < n_points; ++p)
            for (int c = 0; c < 3; ++c) {
                const double v = (double)X[3 * p + c];
                SFM_REQUIRE(std::isfinite(v), SFM_ERR_INVALID_ARG, "%s: point %lld is not finite", who, (long long)p);
                lo[c] = std::min(lo[c], v);
                hi[c] = std::max(hi[c], v);
            }
        const double side = std::max(hi[0] - lo[0], std::max(hi[1] - lo[1], hi[2] - lo[2]));
        SFM_REQUIRE(side > 0.0, SFM_ERR_INVALID_ARG, "%s: the cloud has no extent", who);
        const double voxel = side / resolution;
        sfm_mesh_grid g;
        std::memset(&g, 0, sizeof g);
        g.voxel = (float)voxel;
        double dims[3];
        for (int c = 0; c < 3; ++c) {
            g.origin[c] = (float)(lo[c] - margin_voxels * voxel);
            dims[c] = std::floor((hi[c] - lo[c]) / voxel) + 2.0 + 2.0 * margin_voxels;
        }
        SFM_REQUIRE(dims[0] * dims[1] * dims[2] < 2147483648.0 && dims[1] <= kMeshMaxNy && dims[2] <= kMeshMaxNz,
                    SFM_ERR_UNSUPPORTED, "%s: a grid of %.0f x %.0f x %.0f is beyond the limits", who, dims[0], dims[1],
                    dims[2]);
        for (int c = 0; c < 3; ++c) g.dims[c] = (int32_t)dims[c];
        *grid = g;
        return (int)SFM_OK;
    });
}

extern "C" int sfm_tsdf_integrate_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                       const uint8_t* pixels, const double* K, const double* R, const double* C,
                                       const float* depth, const sfm_mesh_grid* grid, const sfm_tsdf_opts* opts,
                                       float* tsdf, uint8_t* weight, uint8_t* rgb, uint8_t* has_rgb,
                                       sfm_tsdf_stats* stats) {
    return guarded([&] {
        return integrate("sfm_tsdf_integrate_host", nullptr, false, n_img, wh, channels, img_off, pixels, K, R, C, depth, grid,
                         opts, tsdf, weight, rgb, has_rgb, stats);
    });
}

extern "C" int sfm_mesh_extract_host(const sfm_mesh_grid* grid, const float* tsdf, const uint8_t* weight,
                                     const uint8_t* rgb, const uint8_t* has_rgb, const sfm_mesh_opts* opts,
                                     int64_t cap_vertices, int64_t cap_triangles, float* V, uint8_t* vertex_rgb,
                                     int32_t* tri, sfm_mesh_stats* stats) {
    return guarded([&] {
        return extract("sfm_mesh_extract_host", nullptr, false, grid, tsdf, weight, rgb, has_rgb, opts,
                       MeshOut{cap_vertices, cap_triangles, V, vertex_rgb, tri}, stats);
    });
}

extern "C" int sfm_mesh_reconstruct_host(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                                         const uint8_t* pixels, const double* K, const double* R, const double* C,
                                         const float* depth, const sfm_mesh_grid* grid, const sfm_tsdf_opts* tsdf_opts,
                                         const sfm_mesh_opts* mesh_opts, int64_t cap_vertices, int64_t cap_triangles,
                                         float* V, uint8_t* vertex_rgb, int32_t* tri, float* tsdf, uint8_t* weight,
                                         sfm_mesh_reconstruct_stats* stats) {
    return guarded([&] {
        const char* who = "sfm_mesh_reconstruct_host";
        sfm_mesh_reconstruct_stats st;
        std::memset(&st, 0, sizeof st);
        // the checks of both calls first
        MeshGrid g;
        int64_t n_vox = 0;
        const MeshOut out{cap_vertices, cap_triangles, V, vertex_rgb, tri};
        prepare_extract(who, grid, nullptr, nullptr, nullptr, nullptr, mesh_opts, out, false, g, &n_vox);
        std::vector<float> t;
        std::vector<uint8_t> w, c((size_t)(pixels ? 3 * n_vox : 0)), has((size_t)(pixels ? n_vox : 0));
        if (!tsdf) t.resize((size_t)n_vox), tsdf = t.data();
        if (!weight) w.resize((size_t)n_vox), weight = w.data();
        int rc = sfm_tsdf_integrate_host(n_img, wh, channels, img_off, pixels, K, R, C, depth, grid, tsdf_opts, tsdf, weight,
                                         pixels ? c.data() : nullptr, pixels ? has.data() : nullptr, &st.tsdf);
        if (rc == SFM_OK)
            rc = sfm_mesh_extract_host(grid, tsdf, weight, pixels ? c.data() : nullptr, pixels ? has.data() : nullptr,
                                       mesh_opts, cap_vertices, cap_triangles, V, vertex_rgb, tri, &st.mesh);
        st.seconds[1] = st.tsdf.seconds[1] + st.mesh.seconds[1];
        if (stats) *stats = st;
        return rc;
    });
}

extern "C" int sfm_mesh_write_ply(const char* path, int64_t n_vertices, const float* V, const uint8_t* rgb,
                                  int64_t n_triangles, const int32_t* tri) {
    return guarded([&] {
        const char* who = "sfm_mesh_write_ply";
        SFM_REQUIRE(path && n_vertices >= 0 && n_triangles >= 0 && (n_vertices == 0 || V) && (n_triangles == 0 || tri),
                    SFM_ERR_INVALID_ARG, "%s: null path, V or tri, or a negative count", who);
        require_triangles(who, n_triangles, tri, n_vertices);
        PlyWriter ply(who, path,
                      "element vertex " + std::to_string(n_vertices) + "\nproperty float x\nproperty float y\nproperty float z\n" +
                          (rgb ? "property uchar red\nproperty uchar green\nproperty uchar blue\n" : "") + "element face " +
                          std::to_string(n_triangles) + "\nproperty list uchar int vertex_indices\n");
        ply.records(n_vertices, 12 + (rgb ? 3 : 0), [&](int64_t k, uint8_t* p) {
            std::memcpy(p, V + 3 * k, 12);
            if (rgb) std::memcpy(p + 12, rgb + 3 * k, 3);
        });
        ply.records(n_triangles, 13, [&](int64_t k, uint8_t* p) {
            p[0] = 3;
            std::memcpy(p + 1, tri + 3 * k, 12);
        });
        ply.close();
        return (int)SFM_OK;
    });
}

#ifndef SFM_DEPTHMAP_HOST_ONLY
extern "C" int sfm_tsdf_integrate(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels,
                                  const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R,
                                  const double* C, const float* depth, const sfm_mesh_grid* grid,
                                  const sfm_tsdf_opts* opts, float* tsdf, uint8_t* weight, uint8_t* rgb, uint8_t* has_rgb,
                                  sfm_tsdf_stats* stats) {
    return guarded([&] {
        return integrate("sfm_tsdf_integrate", ctx, true, n_img, wh, channels, img_off, pixels, K, R, C, depth, grid, opts, tsdf,
                         weight, rgb, has_rgb, stats);
    });
}

extern "C" int sfm_mesh_extract(sfm_ctx* ctx, const sfm_mesh_grid* grid, const float* tsdf, const uint8_t* weight,
                                const uint8_t* rgb, const uint8_t* has_rgb, const sfm_mesh_opts* opts,
                                int64_t cap_vertices, int64_t cap_triangles, float* V, uint8_t* vertex_rgb, int32_t* tri,
                                sfm_mesh_stats* stats) {
    return guarded([&] {
        return extract("sfm_mesh_extract", ctx, true, grid, tsdf, weight, rgb, has_rgb, opts,
                       MeshOut{cap_vertices, cap_triangles, V, vertex_rgb, tri}, stats);
    });
}

extern "C" int sfm_mesh_reconstruct(sfm_ctx* ctx, int32_t n_img, const int32_t* wh, const int32_t* channels,
                                    const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R,
                                    const double* C, const float* depth, const sfm_mesh_grid* grid,
                                    const sfm_tsdf_opts* tsdf_opts, const sfm_mesh_opts* mesh_opts, int64_t cap_vertices,
                                    int64_t cap_triangles, float* V, uint8_t* vertex_rgb, int32_t* tri, float* tsdf,
                                    uint8_t* weight, sfm_mesh_reconstruct_stats* stats) {
    return guarded([&] {
        const char* who = "sfm_mesh_reconstruct";
        SFM_REQUIRE(ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
        sfm_mesh_reconstruct_stats st;
        std::memset(&st, 0, sizeof st);
        MeshProblem P;
        prepare_tsdf(who, n_img, wh, channels, img_off, pixels, K, R, C, depth, grid, tsdf_opts, P, &st.tsdf.resident_bytes);
        MeshGrid g;
        int64_t n_vox = 0;
        const MeshOut out{cap_vertices, cap_triangles, V, vertex_rgb, tri};
        const int32_t min_weight =
            prepare_extract(who, grid, nullptr, nullptr, nullptr, nullptr, mesh_opts, out, false, g, &n_vox);
        try {
            mesh_reconstruct_device(ctx, P, depth, pixels, min_weight, out, tsdf, weight, &st);
        } catch (const SfmError&) {
            if (stats) *stats = st;
            throw;
        }
        if (stats) *stats = st;
        return (int)SFM_OK;
    });
}
#endif
