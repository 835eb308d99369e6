// The mesh stage (the first step of meshWork(): ReconstructMesh):
//   MeshReconstructor  the filtered depth maps of a DepthMapEstimator's images into a
//                      TSDF volume (integrate(): sfm_tsdf_integrate), its zero level set
//                      as a Mesh (extract(): sfm_mesh_extract), or both in one call with
//                      the volume left where the backend computes it (reconstruct():
//                      sfm_mesh_reconstruct); fitGrid() puts the lattice around a cloud
//                      (sfm_mesh_grid_fit).  Over a backend policy with integrate(),
//                      extract() and reconstruct(); sfm.hpp binds it to the GPU,
//                      HostMeshBackend is the host twin, with the same bytes.
//   Mesh               vertices, optional colours and triangles, in the contract's order;
//                      write_ply() (sfm_mesh_write_ply).
//   MeshTexturer       the last step of meshWork() (TextureMesh): every face of a Mesh
//                      chooses the view that sees it best (chooseViews():
//                      sfm_mesh_face_views), a texture atlas is baked from the chosen
//                      views (bake(): sfm_mesh_texture_bake), or both in one call
//                      (texture(): sfm_mesh_texture).  Over a backend policy; sfm.hpp
//                      binds it to the GPU, HostTextureBackend is the host twin.
//   TexturedMesh       the mesh, its texture coordinates and the atlas; write()
//                      (sfm_mesh_write_textured_ply and sfm_undistort_write_pnm).
// RefineMesh is not built.
// Header-only.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../../include/sfmcore.h"
#include "colorize.hpp"

namespace sfm {

struct HostMeshBackend {
    int integrate(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                  const double* K, const double* R, const double* C, const float* depth, const sfm_mesh_grid* grid,
                  const sfm_tsdf_opts* opts, float* tsdf, uint8_t* weight, uint8_t* rgb, uint8_t* has_rgb,
                  sfm_tsdf_stats* stats) const {
        return sfm_tsdf_integrate_host(n_img, wh, channels, img_off, pixels, K, R, C, depth, grid, opts, tsdf, weight, rgb,
                                       has_rgb, stats);
    }
    int extract(const sfm_mesh_grid* grid, const float* tsdf, const uint8_t* weight, const uint8_t* rgb,
                const uint8_t* has_rgb, const sfm_mesh_opts* opts, int64_t cap_vertices, int64_t cap_triangles, float* V,
                uint8_t* vertex_rgb, int32_t* tri, sfm_mesh_stats* stats) const {
        return sfm_mesh_extract_host(grid, tsdf, weight, rgb, has_rgb, opts, cap_vertices, cap_triangles, V, vertex_rgb, tri,
                                     stats);
    }
    int reconstruct(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                    const uint8_t* pixels, const double* K, const double* R, const double* C, const float* depth,
                    const sfm_mesh_grid* grid, const sfm_tsdf_opts* tsdf_opts, const sfm_mesh_opts* mesh_opts,
                    int64_t cap_vertices, int64_t cap_triangles, float* V, uint8_t* vertex_rgb, int32_t* tri, float* tsdf,
                    uint8_t* weight, sfm_mesh_reconstruct_stats* stats) const {
        return sfm_mesh_reconstruct_host(n_img, wh, channels, img_off, pixels, K, R, C, depth, grid, tsdf_opts, mesh_opts,
                                         cap_vertices, cap_triangles, V, vertex_rgb, tri, tsdf, weight, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

struct Mesh {
    std::vector<float> V;        // [3 n]
    std::vector<uint8_t> rgb;    // [3 n], or empty
    std::vector<int32_t> tri;    // [3 m]
    size_t vertices() const { return V.size() / 3; }
    size_t triangles() const { return tri.size() / 3; }
    bool write_ply(const std::string& path) const {
        const float none_v[3] = {0.f, 0.f, 0.f};
        const int32_t none_t[3] = {0, 0, 0};
        return sfm_mesh_write_ply(path.c_str(), (int64_t)vertices(), V.empty() ? none_v : V.data(),
                                  rgb.size() == V.size() && !rgb.empty() ? rgb.data() : nullptr, (int64_t)triangles(),
                                  tri.empty() ? none_t : tri.data()) == SFM_OK;
    }
};

// The mesh of the images' filtered depth maps (image k's map starts at pixel
// sum of w h of the images before it; data null: the image is not loaded and
// its map does not count).  K is per image (9 doubles each), R and C as the
// dense scene holds them.  Every step returns false when its call failed.
template <class Backend>
class MeshReconstructor {
   public:
    MeshReconstructor(const Backend& backend, const std::vector<ColorImage>& images, const std::vector<double>& K,
                      const std::vector<double>& R, const std::vector<double>& C, const std::vector<float>& depth)
        : backend_(backend), images_(images), K_(K), R_(R), C_(C), depth_(depth) {
        for (const auto& im : images_) {
            wh_.push_back(im.w);
            wh_.push_back(im.h);
            channels_.push_back(im.channels);
            img_off_.push_back(im.data ? (int64_t)pool_.size() : -1);
            if (im.data && im.w > 0 && im.h > 0 && im.channels > 0)
                pool_.insert(pool_.end(), im.data, im.data + (size_t)im.w * im.h * im.channels);
        }
        // padded so that nothing is empty
        pool_.push_back(0);
        wh_.resize(wh_.size() + 2, 1);
        channels_.push_back(1);
        img_off_.push_back(-1);
        K_.resize(K_.size() + 9, 1.0);
        R_.resize(R_.size() + 9, 1.0);
        C_.resize(C_.size() + 3, 0.0);
        depth_.push_back(0.f);
    }

    // the lattice around a cloud X [3 n]: its longest side in `resolution` voxels
    bool fitGrid(const std::vector<float>& X, int32_t resolution, int32_t margin_voxels = 2) {
        const int rc = sfm_mesh_grid_fit((int64_t)(X.size() / 3), X.data(), resolution, margin_voxels, &grid);
        return rc == SFM_OK || fail("fitGrid", sfm_last_error(), rc);
    }

    bool integrate(const sfm_tsdf_opts* opts = nullptr) {
        const size_t n = points();
        if (!n) return fail("integrate", "no grid: fitGrid() first, or set grid", 0);
        tsdf.assign(n, 0.f);
        weight.assign(n, 0);
        volume_rgb.assign(3 * n, 0);
        has_rgb.assign(n, 0);
        const int rc = backend_.integrate((int32_t)images_.size(), wh_.data(), channels_.data(), img_off_.data(), pool_.data(),
                                          K_.data(), R_.data(), C_.data(), depth_.data(), &grid, opts, tsdf.data(),
                                          weight.data(), volume_rgb.data(), has_rgb.data(), &tsdf_stats);
        return rc == SFM_OK || fail("integrate", backend_.last_error(), rc);
    }

    // the mesh of the volume (integrate() first): one call for the needs, one with them
    bool extract(const sfm_mesh_opts* opts = nullptr) {
        if (tsdf.size() != points() || tsdf.empty()) return fail("extract", "no volume: integrate() first", 0);
        mesh = Mesh();
        int rc = backend_.extract(&grid, tsdf.data(), weight.data(), volume_rgb.data(), has_rgb.data(), opts, 0, 0, nullptr,
                                  nullptr, nullptr, &mesh_stats);
        if (rc == SFM_ERR_INVALID_ARG && mesh_stats.n_vertices > 0) {
            reserve((size_t)mesh_stats.n_vertices, (size_t)mesh_stats.n_triangles);
            rc = backend_.extract(&grid, tsdf.data(), weight.data(), volume_rgb.data(), has_rgb.data(), opts,
                                  mesh_stats.n_vertices, mesh_stats.n_triangles, mesh.V.data(), mesh.rgb.data(),
                                  mesh.tri.data(), &mesh_stats);
        }
        if (rc != SFM_OK) return fail("extract", backend_.last_error(), rc);
        finish();
        return true;
    }

    // integrate() and extract() in one call; with keep_volume tsdf and weight are fetched
    bool reconstruct(const sfm_tsdf_opts* tsdf_opts = nullptr, const sfm_mesh_opts* mesh_opts = nullptr,
                     bool keep_volume = false) {
        const size_t n = points();
        if (!n) return fail("reconstruct", "no grid: fitGrid() first, or set grid", 0);
        tsdf.assign(keep_volume ? n : 0, 0.f);
        weight.assign(keep_volume ? n : 0, 0);
        volume_rgb.clear();
        has_rgb.clear();
        mesh = Mesh();
        auto call = [&](int64_t cv, int64_t ct) {
            return backend_.reconstruct((int32_t)images_.size(), wh_.data(), channels_.data(), img_off_.data(), pool_.data(),
                                        K_.data(), R_.data(), C_.data(), depth_.data(), &grid, tsdf_opts, mesh_opts, cv, ct,
                                        cv ? mesh.V.data() : nullptr, cv ? mesh.rgb.data() : nullptr,
                                        ct ? mesh.tri.data() : nullptr, keep_volume ? tsdf.data() : nullptr,
                                        keep_volume ? weight.data() : nullptr, &stats);
        };
        int rc = call(0, 0);
        if (rc == SFM_ERR_INVALID_ARG && stats.mesh.n_vertices > 0) {
            reserve((size_t)stats.mesh.n_vertices, (size_t)stats.mesh.n_triangles);
            rc = call(stats.mesh.n_vertices, stats.mesh.n_triangles);
        }
        if (rc != SFM_OK) return fail("reconstruct", backend_.last_error(), rc);
        tsdf_stats = stats.tsdf;
        mesh_stats = stats.mesh;
        finish();
        return true;
    }

    sfm_mesh_grid grid{};
    Mesh mesh;
    std::vector<float> tsdf;
    std::vector<uint8_t> weight, volume_rgb, has_rgb;
    sfm_tsdf_stats tsdf_stats{};
    sfm_mesh_stats mesh_stats{};
    sfm_mesh_reconstruct_stats stats{};

   private:
    size_t points() const {
        return grid.dims[0] > 0 && grid.dims[1] > 0 && grid.dims[2] > 0 ? (size_t)grid.dims[0] * grid.dims[1] * grid.dims[2] : 0;
    }
    void reserve(size_t nv, size_t nt) {
        mesh.V.assign(3 * nv, 0.f);
        mesh.rgb.assign(3 * nv, 0);
        mesh.tri.assign(3 * nt + 3, 0);
    }
    void finish() {
        mesh.V.resize(3 * (size_t)mesh_stats.n_vertices);
        mesh.rgb.resize(3 * (size_t)mesh_stats.n_vertices);
        mesh.tri.resize(3 * (size_t)mesh_stats.n_triangles);
    }
    static bool fail(const char* step, const char* why, int rc) {
        std::fprintf(stderr, "MeshReconstructor::%s failed: %s (code %d)\n", step, why, rc);
        return false;
    }

    const Backend backend_;
    const std::vector<ColorImage> images_;
    std::vector<double> K_, R_, C_;
    std::vector<float> depth_;
    std::vector<int32_t> wh_, channels_;
    std::vector<int64_t> img_off_;
    std::vector<uint8_t> pool_;
};

struct HostTextureBackend {
    int face_views(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                   const double* K, const double* R, const double* C, int64_t n_vertices, const float* V, int64_t n_triangles,
                   const int32_t* tri, const sfm_mesh_texture_opts* opts, int32_t* face_view, int32_t* face_pixels,
                   sfm_mesh_face_views_stats* stats) const {
        return sfm_mesh_face_views_host(n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, n_triangles, tri, opts,
                                        face_view, face_pixels, stats);
    }
    int bake(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
             const double* K, const double* R, const double* C, int64_t n_vertices, const float* V, const uint8_t* vertex_rgb,
             int64_t n_triangles, const int32_t* tri, const int32_t* face_view, const sfm_mesh_texture_opts* opts,
             uint8_t* texture, float* uv, sfm_mesh_bake_stats* stats) const {
        return sfm_mesh_texture_bake_host(n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb, n_triangles,
                                          tri, face_view, opts, texture, uv, stats);
    }
    int texture(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                const double* K, const double* R, const double* C, int64_t n_vertices, const float* V, const uint8_t* vertex_rgb,
                int64_t n_triangles, const int32_t* tri, const sfm_mesh_texture_opts* opts, int32_t* face_view,
                int32_t* face_pixels, uint8_t* texture, float* uv, sfm_mesh_texture_stats* stats) const {
        return sfm_mesh_texture_host(n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb, n_triangles, tri,
                                     opts, face_view, face_pixels, texture, uv, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

struct TexturedMesh {
    std::vector<float> V;          // [3 n]
    std::vector<int32_t> tri;      // [3 m]
    std::vector<float> uv;         // [6 m]
    std::vector<uint8_t> texture;  // [3 W H], top row first
    int32_t W = 0, H = 0;
    size_t triangles() const { return tri.size() / 3; }
    // <stem>.ply and <stem>.ppm beside it
    bool write(const std::string& stem) const {
        const size_t cut = stem.find_last_of('/');
        const std::string name = (cut == std::string::npos ? stem : stem.substr(cut + 1)) + ".ppm";
        const float none_v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const int32_t none_t[3] = {0, 0, 0};
        if (sfm_mesh_write_textured_ply((stem + ".ply").c_str(), name.c_str(), (int64_t)(V.size() / 3),
                                        V.empty() ? none_v : V.data(), (int64_t)triangles(), tri.empty() ? none_t : tri.data(),
                                        uv.empty() ? none_v : uv.data()) != SFM_OK)
            return false;
        return W == 0 || sfm_undistort_write_pnm((stem + ".ppm").c_str(), W, H, 3, texture.data()) == SFM_OK;
    }
};

// The texture of a Mesh from the images it was built from (data null: the
// image is skipped).  Every step returns false when its call failed.
template <class Backend>
class MeshTexturer {
   public:
    MeshTexturer(const Backend& backend, const std::vector<ColorImage>& images, const std::vector<double>& K,
                 const std::vector<double>& R, const std::vector<double>& C, const Mesh& mesh)
        : backend_(backend), n_img_((int32_t)images.size()), K_(K), R_(R), C_(C), mesh_(mesh) {
        for (const auto& im : images) {
            wh_.push_back(im.w);
            wh_.push_back(im.h);
            channels_.push_back(im.channels);
            img_off_.push_back(im.data ? (int64_t)pool_.size() : -1);
            if (im.data && im.w > 0 && im.h > 0 && im.channels > 0)
                pool_.insert(pool_.end(), im.data, im.data + (size_t)im.w * im.h * im.channels);
        }
        // padded so that nothing is empty
        pool_.push_back(0);
        wh_.resize(wh_.size() + 2, 1);
        channels_.push_back(1);
        img_off_.push_back(-1);
        K_.resize(K_.size() + 9, 1.0);
        R_.resize(R_.size() + 9, 1.0);
        C_.resize(C_.size() + 3, 0.0);
        mesh_.V.resize(mesh_.V.size() + 3, 0.f);
        mesh_.tri.resize(mesh_.tri.size() + 3, 0);
        n_v_ = (int64_t)mesh.vertices();
        n_t_ = (int64_t)mesh.triangles();
    }

    bool chooseViews(const sfm_mesh_texture_opts* opts = nullptr) {
        face_view.assign((size_t)n_t_ + 1, -1);
        face_pixels.assign((size_t)n_t_ + 1, 0);
        const int rc = backend_.face_views(n_img_, wh_.data(), channels_.data(), img_off_.data(), pool_.data(), K_.data(),
                                           R_.data(), C_.data(), n_v_, mesh_.V.data(), n_t_, mesh_.tri.data(), opts,
                                           face_view.data(), face_pixels.data(), &views_stats);
        face_view.resize((size_t)n_t_);
        face_pixels.resize((size_t)n_t_);
        return rc == SFM_OK || fail("chooseViews", backend_.last_error(), rc);
    }

    // the atlas of face_view (chooseViews() first, or the caller's choice)
    bool bake(const sfm_mesh_texture_opts* opts = nullptr) {
        if ((int64_t)face_view.size() != n_t_) return fail("bake", "no face_view: chooseViews() first", 0);
        if (!reserve(opts)) return false;
        std::vector<int32_t> fv(face_view);
        fv.push_back(-1);
        const int rc = backend_.bake(n_img_, wh_.data(), channels_.data(), img_off_.data(), pool_.data(), K_.data(), R_.data(),
                                     C_.data(), n_v_, mesh_.V.data(), colours(), n_t_, mesh_.tri.data(), fv.data(), opts,
                                     textured.texture.data(), textured.uv.data(), &bake_stats);
        return rc == SFM_OK ? finish() : fail("bake", backend_.last_error(), rc);
    }

    // chooseViews() and bake() in one call
    bool texture(const sfm_mesh_texture_opts* opts = nullptr) {
        if (!reserve(opts)) return false;
        face_view.assign((size_t)n_t_ + 1, -1);
        face_pixels.assign((size_t)n_t_ + 1, 0);
        const int rc = backend_.texture(n_img_, wh_.data(), channels_.data(), img_off_.data(), pool_.data(), K_.data(), R_.data(),
                                        C_.data(), n_v_, mesh_.V.data(), colours(), n_t_, mesh_.tri.data(), opts,
                                        face_view.data(), face_pixels.data(), textured.texture.data(), textured.uv.data(),
                                        &stats);
        face_view.resize((size_t)n_t_);
        face_pixels.resize((size_t)n_t_);
        views_stats = stats.views;
        bake_stats = stats.bake;
        return rc == SFM_OK ? finish() : fail("texture", backend_.last_error(), rc);
    }

    TexturedMesh textured;
    std::vector<int32_t> face_view, face_pixels;
    sfm_mesh_face_views_stats views_stats{};
    sfm_mesh_bake_stats bake_stats{};
    sfm_mesh_texture_stats stats{};

   private:
    const uint8_t* colours() const { return mesh_.rgb.size() == 3 * (size_t)n_v_ && n_v_ ? mesh_.rgb.data() : nullptr; }
    bool reserve(const sfm_mesh_texture_opts* opts) {
        sfm_mesh_texture_opts o;
        sfm_mesh_texture_default_options(&o);
        if (opts) o = *opts;
        int32_t cols = 0;
        textured = TexturedMesh();
        const int rc = sfm_mesh_atlas_fit(n_t_, o.cell, &textured.W, &textured.H, &cols);
        if (rc != SFM_OK) return fail("atlas", sfm_last_error(), rc);
        textured.texture.assign(3 * (size_t)textured.W * textured.H + 1, 0);
        textured.uv.assign(6 * (size_t)n_t_ + 1, 0.f);
        return true;
    }
    bool finish() {
        textured.texture.resize(3 * (size_t)textured.W * textured.H);
        textured.uv.resize(6 * (size_t)n_t_);
        textured.V.assign(mesh_.V.begin(), mesh_.V.begin() + 3 * n_v_);
        textured.tri.assign(mesh_.tri.begin(), mesh_.tri.begin() + 3 * n_t_);
        return true;
    }
    static bool fail(const char* step, const char* why, int rc) {
        std::fprintf(stderr, "MeshTexturer::%s failed: %s (code %d)\n", step, why, rc);
        return false;
    }

    const Backend backend_;
    int32_t n_img_;
    std::vector<double> K_, R_, C_;
    Mesh mesh_;
    int64_t n_v_ = 0, n_t_ = 0;
    std::vector<int32_t> wh_, channels_;
    std::vector<int64_t> img_off_;
    std::vector<uint8_t> pool_;
};

}  // namespace sfm
