// Reference-shaped C++ surface over libsfmcore.so (C-ABI include/sfmcore.h):
//
//   BundleAdjuster        src/adjuster/BundleAdjuster.h:32-188
//   Matcher               cv::BFMatcher(NORM_L2, crossCheck=true) as created by
//                         SequentialActuator.h:77 (exact mutual nearest neighbour)
//   LocalFrame/GlobalFrame src/frame/LocalFrame.h:19-83, GlobalFrame.h:15-160
//   Triangulator          every world point from its track and the current
//                         poses (triangulator.hpp; sfm_triangulate)
//   Localizer             the pose of an image from the world points it observes
//                         (localizer.hpp; sfm_resect)
//   RelativePoser         the relative pose of image pairs from their matches and
//                         the engine's choice of the initial pair
//                         (relative_pose.hpp; sfm_relpose)
//   SequentialSfMReconstructionEngine  OpenMVG's incremental engine over the
//                         stages above (reconstruction.hpp; sfm_reconstruct), and
//                         sparseBuilder::reconstruction() file-staged
//   ColorizeTracks        OpenMVG's greedy track colouring, what colorize() runs
//                         (colorize.hpp; sfm_colorize), and sparseBuilder::colorize()
//                         file-staged
//   UndistortImages, DenseBuilder  the dense hand-off: every image undistorted
//                         (sfm_undistort) and the scene DenseBuilder::save()
//                         collects (dense.hpp; sfm_dense_scene_*)
//   DepthMapEstimator     the depth-map phase of DensifyPointCloud: view selection,
//                         PatchMatch depth maps, the consistency filter (dense.hpp;
//                         sfm_depth_views_select, sfm_depthmap, sfm_depthmap_filter,
//                         sfm_depthmap_fuse, sfm_densify; DenseCloud is its product)
//   MeshReconstructor     the first step of meshWork(): the filtered depth maps into a
//                         TSDF volume and its zero level set as a Mesh (mesh.hpp;
//                         sfm_tsdf_integrate, sfm_mesh_extract, sfm_mesh_reconstruct)
//   MeshTexturer          the last step of meshWork(): per-face view choice and a texture
//                         atlas (mesh.hpp; sfm_mesh_face_views, sfm_mesh_texture_bake,
//                         sfm_mesh_texture; TexturedMesh is its product)
//   SIFT_Image_describer  src/nonFree/sift/SIFT_describer.hpp and detectFeature()
//                         (sparseBuilder.cpp:575-756) on 8-bit gray buffers
//                         (sift.hpp; sfm_sift)
//   TracksBuilder         OpenMVG's tracks::TracksBuilder, the first step of the
//                         engine reconstruction() runs (sparseBuilder.cpp:1474-1508):
//                         pairwise matches into tracks (tracks.hpp; sfm_tracks_build)
//   sparse::sparseBuilder src/sparseBuilder/sparseBuilder.h:14-39 — matchPair()
//                         (exhaustive pairs, .cpp:758-807) and match()
//                         (Matcher_Regions(0.8, BRUTE_FORCE_L2), .cpp:809-1023)
//                         file-staged over <base>/output/matches in OpenMVG's
//                         formats (csrc/mvg_io.cpp), or on in-memory regions.
//
// Header-only; link with -lsfmcore.  Errors: the reference prints and leaves
// the world untouched on BA failure (BundleAdjuster.h:128-131); so does this
// façade.  Matching failures throw sfm::Error.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/sfmcore.h"
#include "actuator.hpp"
#include "adjuster.hpp"
#include "colorize.hpp"
#include "dense.hpp"
#include "frames.hpp"
#include "localizer.hpp"
#include "mesh.hpp"
#include "reconstruction.hpp"
#include "relative_pose.hpp"
#include "sift.hpp"
#include "tracks.hpp"
#include "triangulator.hpp"
#include "world.hpp"

namespace sfm {

inline void check(int rc, const char* where) {
    if (rc != SFM_OK) throw Error(rc, where, sfm_last_error());
}

// One HIP device (+ RCCL communicator for landmark-sharded BA).
class Context {
   public:
    explicit Context(int device = 0, int rank = 0, int world = 1, const uint8_t* comm_id = nullptr) {
        sfm_ctx_opts o{};
        o.device = device; o.rank = rank; o.world_size = world; o.comm_id = comm_id;
        check(sfm_ctx_create(&o, &ctx_), "sfm_ctx_create");
    }
    ~Context() { sfm_ctx_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    sfm_ctx* get() const { return ctx_; }
    // the reference constructs a BundleAdjuster per call; share one context per thread
    static Context& thread_default() {
        thread_local Context c(0);
        return c;
    }

   private:
    sfm_ctx* ctx_ = nullptr;
};

// ---------------------------------------------------------------------------
// Exact descriptor matcher on the GPU (stands in for the cv::BFMatcher).
// ---------------------------------------------------------------------------
class Matcher {
   public:
    explicit Matcher(Context& ctx = Context::thread_default()) : ctx_(&ctx) {}
    // knnMatch(query, train, out, k=1) with crossCheck: rows without a mutual
    // partner are empty (LocalFrame.h:37-44 skips them).
    void knnMatch(const std::vector<uint8_t>& query, const std::vector<uint8_t>& train,
                  std::vector<std::vector<DMatch>>& out, int k = 1) const {
        if (k != 1) throw std::invalid_argument("crossCheck matcher supports k = 1 only");
        const int nq = (int)(query.size() / 128), nt = (int)(train.size() / 128);
        std::vector<int32_t> idx(std::max(nq, 1)), d2(std::max(nq, 1));
        sfm_match_options o{SFM_MATCH_MUTUAL, 0.8f};
        check(sfm_match_dense(ctx_->get(), query.data(), nq, train.data(), nt, &o, idx.data(), d2.data()),
              "sfm_match_dense");
        out.assign(nq, {});
        for (int q = 0; q < nq; ++q)
            if (idx[q] >= 0) out[q].push_back(DMatch{q, idx[q], 0, std::sqrt((float)d2[q])});
    }
    // the same over float rows, the cv::Mat CV_32F cv::SIFT produces
    // (LocalFrame.h:38, Image.h:39-41): integer-valued rows take the exact u8
    // path, others the f32 one (sfm_match_dense_f32)
    void knnMatch(const std::vector<float>& query, const std::vector<float>& train,
                  std::vector<std::vector<DMatch>>& out, int k = 1) const {
        if (k != 1) throw std::invalid_argument("crossCheck matcher supports k = 1 only");
        const int nq = (int)(query.size() / 128), nt = (int)(train.size() / 128);
        std::vector<int32_t> idx(std::max(nq, 1));
        std::vector<float> d2(std::max(nq, 1));
        sfm_match_options o{SFM_MATCH_MUTUAL, 0.8f};
        check(sfm_match_dense_f32(ctx_->get(), query.data(), nq, train.data(), nt, &o, idx.data(), d2.data()),
              "sfm_match_dense_f32");
        out.assign(nq, {});
        for (int q = 0; q < nq; ++q)
            if (idx[q] >= 0) out[q].push_back(DMatch{q, idx[q], 0, std::sqrt(d2[q])});
    }
    Context& context() const { return *ctx_; }

   private:
    Context* ctx_;
};

// ---------------------------------------------------------------------------
// BundleAdjuster (BundleAdjuster.h:32-188) on the GPU solver
// ---------------------------------------------------------------------------
struct GpuSolver {
    Context* ctx;
    int solve(const sfm_ba_problem& pr, double* extr, double* intr, double* X, const sfm_ba_options& o,
              sfm_ba_summary& s) const {
        return sfm_ba_solve(ctx->get(), &pr, extr, intr, X, &o, &s);
    }
    const char* last_error() const { return sfm_last_error(); }
};

class BundleAdjuster : public BasicBundleAdjuster<GpuSolver> {
   public:
    explicit BundleAdjuster(Context& ctx = Context::thread_default(), Options opt = Options())
        : BasicBundleAdjuster<GpuSolver>(GpuSolver{&ctx}, opt) {}
};

// ---------------------------------------------------------------------------
// Triangulator (triangulator.hpp) on the GPU: sfm_triangulate
// ---------------------------------------------------------------------------
struct GpuTriBackend {
    Context* ctx;
    int triangulate(const sfm_ba_problem& pr, const double* extr, const double* intr, const sfm_tri_opts& o, double* X,
                    uint8_t* status, uint8_t* keep_obs, sfm_tri_stats& st) const {
        return sfm_triangulate(ctx->get(), &pr, extr, intr, &o, X, status, keep_obs, nullptr, &st);
    }
    const char* last_error() const { return sfm_last_error(); }
};

class Triangulator : public BasicTriangulator<GpuTriBackend> {
   public:
    explicit Triangulator(Context& ctx = Context::thread_default())
        : BasicTriangulator<GpuTriBackend>(GpuTriBackend{&ctx}) {}
};

// ---------------------------------------------------------------------------
// Localizer (localizer.hpp) on the GPU: sfm_resect
// ---------------------------------------------------------------------------
struct GpuResectBackend {
    Context* ctx;
    int resect(int32_t cm, int64_t n_img, const int64_t* off, const double* X, const double* uv,
               const int32_t* img_intr, const double* intr, int32_t n_intr, const int32_t* wh,
               const sfm_resect_opts& o, sfm_resect_result* results, int32_t* inliers) const {
        return sfm_resect(ctx->get(), cm, n_img, off, X, uv, img_intr, intr, n_intr, wh, &o, results, inliers);
    }
    const char* last_error() const { return sfm_last_error(); }
};

class Localizer : public BasicLocalizer<GpuResectBackend> {
   public:
    explicit Localizer(Context& ctx = Context::thread_default())
        : BasicLocalizer<GpuResectBackend>(GpuResectBackend{&ctx}) {}
};

// ---------------------------------------------------------------------------
// RelativePoser (relative_pose.hpp) on the GPU: sfm_relpose
// ---------------------------------------------------------------------------
struct GpuRelposeBackend {
    Context* ctx;
    int relpose(int32_t cm, int64_t n_pairs, const int64_t* off, const double* xy, const int32_t* pair_intr,
                const double* intr, int32_t n_intr, const int32_t* wh, const sfm_relpose_opts& o,
                sfm_relpose_result* results, int32_t* inliers) const {
        return sfm_relpose(ctx->get(), cm, n_pairs, off, xy, pair_intr, intr, n_intr, wh, &o, results, inliers);
    }
    const char* last_error() const { return sfm_last_error(); }
};

class RelativePoser : public BasicRelativePoser<GpuRelposeBackend> {
   public:
    explicit RelativePoser(Context& ctx = Context::thread_default())
        : BasicRelativePoser<GpuRelposeBackend>(GpuRelposeBackend{&ctx}) {}
};

// ---------------------------------------------------------------------------
// SequentialSfMReconstructionEngine (reconstruction.hpp) on the GPU:
// sfm_reconstruct
// ---------------------------------------------------------------------------
struct GpuReconBackend {
    static constexpr bool adjusts = true;
    Context* ctx;
    int reconstruct(const sfm_ba_problem& tracks, double* intr, const int32_t* wh, const int32_t* pairs, int64_t n_pairs,
                    const sfm_recon_opts& o, double* extr, double* X, uint8_t* registered, uint8_t* pt_ok,
                    uint8_t* keep_obs, sfm_recon_round* rounds, int32_t cap_rounds, sfm_recon_cand* cands,
                    int32_t cap_cands, sfm_recon_stats* stats) const {
        return sfm_reconstruct(ctx->get(), &tracks, intr, wh, pairs, n_pairs, &o, extr, X, registered, pt_ok, keep_obs,
                               rounds, cap_rounds, cands, cap_cands, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

class SequentialSfMReconstructionEngine : public BasicSequentialSfMReconstructionEngine<GpuReconBackend> {
   public:
    SequentialSfMReconstructionEngine(WorldStructure::Ptr world, std::vector<Image::Ptr> images, int32_t width,
                                      int32_t height, Context& ctx = Context::thread_default())
        : BasicSequentialSfMReconstructionEngine<GpuReconBackend>(GpuReconBackend{&ctx}, std::move(world),
                                                                  std::move(images), width, height) {}
};

// ---------------------------------------------------------------------------
// ColorizeTracks (colorize.hpp) on the GPU: sfm_colorize
// ---------------------------------------------------------------------------
struct GpuColorizeBackend {
    Context* ctx;
    int colorize(const sfm_ba_problem& tracks, const int32_t* wh, const uint8_t* pt_ok, const uint8_t* keep_obs,
                 const int32_t* channels, const int64_t* img_off, const uint8_t* pixels, uint8_t* rgb, int32_t* view,
                 sfm_colorize_stats* stats) const {
        return sfm_colorize(ctx->get(), &tracks, wh, pt_ok, keep_obs, channels, img_off, pixels, rgb, view, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

inline bool ColorizeTracks(const WorldStructure& world, const std::vector<Image::Ptr>& images,
                           const std::vector<ColorImage>& pixels, std::vector<std::array<uint8_t, 3>>& colors,
                           Context& ctx = Context::thread_default(), const std::vector<uint8_t>* pt_ok = nullptr,
                           sfm_colorize_stats* stats = nullptr) {
    return ColorizeTracks(GpuColorizeBackend{&ctx}, world, images, pixels, colors, pt_ok, stats);
}

// ---------------------------------------------------------------------------
// UndistortImages / DenseBuilder::exportUndistorted (dense.hpp) on the GPU: sfm_undistort
// ---------------------------------------------------------------------------
struct GpuUndistortBackend {
    Context* ctx;
    int undistort(int32_t camera_model, int32_t n_img, int32_t n_intr, const int32_t* img_intr, const double* intr,
                  const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                  const sfm_undistort_opts* opts, uint8_t* out, sfm_undistort_stats* stats) const {
        return sfm_undistort(ctx->get(), camera_model, n_img, n_intr, img_intr, intr, wh, channels, img_off, pixels, opts,
                             out, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

inline bool UndistortImages(int32_t camera_model, const std::vector<int32_t>& img_intr, const std::vector<double>& intr,
                            const std::vector<ColorImage>& images, std::vector<std::vector<uint8_t>>& undistorted,
                            Context& ctx = Context::thread_default(), const sfm_undistort_opts* opts = nullptr,
                            sfm_undistort_stats* stats = nullptr) {
    return UndistortImages(GpuUndistortBackend{&ctx}, camera_model, img_intr, intr, images, undistorted, opts, stats);
}

// ---------------------------------------------------------------------------
// DepthMapEstimator (dense.hpp) on the GPU: sfm_depthmap, sfm_depthmap_filter,
// sfm_depthmap_fuse, sfm_densify
// ---------------------------------------------------------------------------
struct GpuDepthMapBackend {
    Context* ctx;
    int depthmap(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                 const double* K, const double* R, const double* C, const int64_t* nb_off, const int32_t* nb_view,
                 const float* drange, const float* init_depth, const float* init_normal, const sfm_depthmap_opts* opts,
                 float* depth, float* normal, float* cost, sfm_depthmap_stats* stats) const {
        return sfm_depthmap(ctx->get(), n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange, init_depth,
                            init_normal, opts, depth, normal, cost, stats);
    }
    int filter(int32_t n_img, const int32_t* wh, const double* K, const double* R, const double* C, const int64_t* nb_off,
               const int32_t* nb_view, const float* depth, const float* cost, const sfm_depthmap_filter_opts* opts,
               float* depth_out, uint8_t* n_agree, int64_t* counts, sfm_depthmap_filter_stats* stats) const {
        return sfm_depthmap_filter(ctx->get(), n_img, wh, K, R, C, nb_off, nb_view, depth, cost, opts, depth_out, n_agree,
                                   counts, stats);
    }
    int fuse(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
             const double* K, const double* R, const double* C, const int64_t* nb_off, const int32_t* nb_view,
             const float* depth, const float* normal, const sfm_depthmap_fuse_opts* opts, int64_t cap_points, float* X,
             float* N, uint8_t* rgb, uint8_t* n_views, uint32_t* view_mask, int32_t* src_image, int32_t* src_pixel,
             sfm_depthmap_fuse_stats* stats) const {
        return sfm_depthmap_fuse(ctx->get(), n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, depth, normal, opts, cap_points,
                                      X, N, rgb, n_views, view_mask, src_image, src_pixel, stats);
    }
    int densify(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                const double* K, const double* R, const double* C, const int64_t* nb_off, const int32_t* nb_view,
                const float* drange, const float* init_depth, const float* init_normal, const sfm_depthmap_opts* opts,
                const sfm_depthmap_filter_opts* filter_opts, const sfm_depthmap_fuse_opts* fuse_opts, int64_t cap_points,
                float* X, float* N, uint8_t* rgb, uint8_t* n_views, uint32_t* view_mask, int32_t* src_image,
                int32_t* src_pixel, float* depth, float* normal, float* cost, float* depth_filtered, uint8_t* n_agree,
                int64_t* counts, sfm_densify_stats* stats) const {
        return sfm_densify(ctx->get(), n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange, init_depth, init_normal,
                                opts, filter_opts, fuse_opts, cap_points, X, N, rgb, n_views, view_mask, src_image, src_pixel,
                                depth, normal, cost, depth_filtered, n_agree, counts, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};
using GpuDepthMapEstimator = DepthMapEstimator<GpuDepthMapBackend>;

// ---------------------------------------------------------------------------
// MeshReconstructor (mesh.hpp) on the GPU: sfm_tsdf_integrate, sfm_mesh_extract,
// sfm_mesh_reconstruct
// ---------------------------------------------------------------------------
struct GpuMeshBackend {
    Context* ctx;
    int integrate(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                  const double* K, const double* R, const double* C, const float* depth, const sfm_mesh_grid* grid,
                  const sfm_tsdf_opts* opts, float* tsdf, uint8_t* weight, uint8_t* rgb, uint8_t* has_rgb,
                  sfm_tsdf_stats* stats) const {
        return sfm_tsdf_integrate(ctx->get(), n_img, wh, channels, img_off, pixels, K, R, C, depth, grid, opts, tsdf, weight,
                                  rgb, has_rgb, stats);
    }
    int extract(const sfm_mesh_grid* grid, const float* tsdf, const uint8_t* weight, const uint8_t* rgb,
                const uint8_t* has_rgb, const sfm_mesh_opts* opts, int64_t cap_vertices, int64_t cap_triangles, float* V,
                uint8_t* vertex_rgb, int32_t* tri, sfm_mesh_stats* stats) const {
        return sfm_mesh_extract(ctx->get(), grid, tsdf, weight, rgb, has_rgb, opts, cap_vertices, cap_triangles, V,
                                vertex_rgb, tri, stats);
    }
    int reconstruct(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                    const uint8_t* pixels, const double* K, const double* R, const double* C, const float* depth,
                    const sfm_mesh_grid* grid, const sfm_tsdf_opts* tsdf_opts, const sfm_mesh_opts* mesh_opts,
                    int64_t cap_vertices, int64_t cap_triangles, float* V, uint8_t* vertex_rgb, int32_t* tri, float* tsdf,
                    uint8_t* weight, sfm_mesh_reconstruct_stats* stats) const {
        return sfm_mesh_reconstruct(ctx->get(), n_img, wh, channels, img_off, pixels, K, R, C, depth, grid, tsdf_opts,
                                    mesh_opts, cap_vertices, cap_triangles, V, vertex_rgb, tri, tsdf, weight, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};
using GpuMeshReconstructor = MeshReconstructor<GpuMeshBackend>;

// ---------------------------------------------------------------------------
// MeshTexturer (mesh.hpp) on the GPU: sfm_mesh_face_views, sfm_mesh_texture_bake,
// sfm_mesh_texture
// ---------------------------------------------------------------------------
struct GpuTextureBackend {
    Context* ctx;
    int face_views(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                   const double* K, const double* R, const double* C, int64_t n_vertices, const float* V, int64_t n_triangles,
                   const int32_t* tri, const sfm_mesh_texture_opts* opts, int32_t* face_view, int32_t* face_pixels,
                   sfm_mesh_face_views_stats* stats) const {
        return sfm_mesh_face_views(ctx->get(), n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, n_triangles, tri,
                                   opts, face_view, face_pixels, stats);
    }
    int bake(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
             const double* K, const double* R, const double* C, int64_t n_vertices, const float* V, const uint8_t* vertex_rgb,
             int64_t n_triangles, const int32_t* tri, const int32_t* face_view, const sfm_mesh_texture_opts* opts,
             uint8_t* texture, float* uv, sfm_mesh_bake_stats* stats) const {
        return sfm_mesh_texture_bake(ctx->get(), n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb,
                                     n_triangles, tri, face_view, opts, texture, uv, stats);
    }
    int texture(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                const double* K, const double* R, const double* C, int64_t n_vertices, const float* V, const uint8_t* vertex_rgb,
                int64_t n_triangles, const int32_t* tri, const sfm_mesh_texture_opts* opts, int32_t* face_view,
                int32_t* face_pixels, uint8_t* texture, float* uv, sfm_mesh_texture_stats* stats) const {
        return sfm_mesh_texture(ctx->get(), n_img, wh, channels, img_off, pixels, K, R, C, n_vertices, V, vertex_rgb, n_triangles,
                                tri, opts, face_view, face_pixels, texture, uv, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};
using GpuMeshTexturer = MeshTexturer<GpuTextureBackend>;

// ---------------------------------------------------------------------------
// SIFT_Image_describer (sift.hpp) on the GPU: sfm_sift
// ---------------------------------------------------------------------------
struct GpuSiftBackend {
    Context* ctx;
    int sift(const uint8_t* gray, int32_t n_img, int32_t w, int32_t h, const sfm_sift_options& o, int64_t cap,
             float* xyso, uint8_t* desc, int64_t* n_feat, sfm_sift_summary* sm) const {
        return sfm_sift(ctx->get(), gray, n_img, w, h, &o, cap, xyso, desc, n_feat, sm);
    }
    const char* last_error() const { return sfm_last_error(); }
};

class SIFT_Image_describer : public BasicSiftDescriber<GpuSiftBackend> {
   public:
    explicit SIFT_Image_describer(const Params& params = Params(), bool bOrientation = true,
                                  Context& ctx = Context::thread_default())
        : BasicSiftDescriber<GpuSiftBackend>(GpuSiftBackend{&ctx}, params, bOrientation) {}
};

// ---------------------------------------------------------------------------
// TracksBuilder (tracks.hpp) on the GPU: sfm_tracks_build
// ---------------------------------------------------------------------------
struct GpuTracksBackend {
    Context* ctx;
    int build(int32_t n_img, const int64_t* feat_off, int64_t n_pairs, const int32_t* pairs, const int64_t* counts,
              const uint32_t* i, const uint32_t* j, const sfm_tracks_opts& o, sfm_tracks** out) const {
        return sfm_tracks_build(ctx->get(), n_img, feat_off, n_pairs, pairs, counts, i, j, nullptr, &o, out);
    }
    const char* last_error() const { return sfm_last_error(); }
};

class TracksBuilder : public BasicTracksBuilder<GpuTracksBackend> {
   public:
    explicit TracksBuilder(Context& ctx = Context::thread_default())
        : BasicTracksBuilder<GpuTracksBackend>(GpuTracksBackend{&ctx}) {}
};

// ---------------------------------------------------------------------------
// SequentialActuator (SequentialActuator.h:16-236) on the GPU matcher and
// adjuster (BASELINE.json config C5)
// ---------------------------------------------------------------------------
struct GpuSeqBackend {
    Matcher m;
    Context* ctx;
    Matcher& matcher() { return m; }
    BundleAdjuster make_adjuster(const BundleAdjusterOptions& o) const { return BundleAdjuster(*ctx, o); }
};

class SequentialActuator : public BasicSequentialActuator<GpuSeqBackend> {
   public:
    explicit SequentialActuator(Camera::Ptr camera, Context& ctx = Context::thread_default(),
                                SeqOptions opt = SeqOptions())
        : BasicSequentialActuator<GpuSeqBackend>(GpuSeqBackend{Matcher(ctx), &ctx}, std::move(camera), opt) {}
};

namespace sparse {

struct IndMatch {  // openMVG::matching::IndMatch
    uint32_t i_, j_;
};
using Pair = std::pair<uint32_t, uint32_t>;
using PairWiseMatches = std::map<Pair, std::vector<IndMatch>>;

// sparse::sparseBuilder (sparseBuilder.h:14-39).  Constructed on a base path
// like the reference's, matchPair() / match() are the file-staged stages of
// sparseBuilder.cpp:758-1023 over <base>/output/matches (sfm_data.json,
// image_describer.json, <stem>.desc/.feat, pairs.bin -> matches.putative.bin,
// preemptive_pairs.txt), with the GPU matcher in place of the OpenMVG
// collection matcher.  Errors print and return, as the reference's
// OPENMVG_LOG_ERROR + return does (:825-878); lastError() keeps the code.
// exhaustive() / matchRegions() are the same stages on in-memory regions.
class sparseBuilder {
   public:
    explicit sparseBuilder(Context& ctx = Context::thread_default()) : ctx_(&ctx) {}
    explicit sparseBuilder(const std::string& base_path, Context& ctx = Context::thread_default())
        : ctx_(&ctx), matches_dir_(base_path + "/output/matches") {}

    const std::string& matchesDir() const { return matches_dir_; }
    int lastError() const { return last_rc_; }

    // exhaustivePairs(#views) -> pairs.bin (:758-807)
    void matchPair() {
        last_rc_ = sfm_sparse_match_pair(matches_dir_.c_str());
        if (last_rc_ != SFM_OK) std::fprintf(stderr, "matchPair failed: %s\n", sfm_last_error());
    }
    // sNearestMatchingMethod (:814, :911-925) -> SFM_MATCH_*: "AUTO" on SIFT
    // regions is Cascade_Hashing_Matcher_Regions, "BRUTEFORCEL2" is
    // Matcher_Regions(BRUTE_FORCE_L2); others are not provided (-1).
    static int matchingMode(const std::string& method) {
        if (method == "AUTO" || method == "CASCADEHASHINGL2" || method == "FASTCASCADEHASHINGL2")
            return SFM_MATCH_CASCADE;
        if (method == "BRUTEFORCEL2") return SFM_MATCH_RATIO;
        return -1;
    }
    // match() over pairs.bin (:809-1023), fDistRatio = 0.8f, method "AUTO"
    void match(float dist_ratio = 0.8f, bool force = false, const std::string& method = "AUTO") {
        const int mode = matchingMode(method);
        if (mode < 0) {
            last_rc_ = SFM_ERR_UNSUPPORTED;
            std::fprintf(stderr, "match failed: unsupported nearest matching method %s\n", method.c_str());
            return;
        }
        sfm_sparse_match_opts o{mode, dist_ratio, force ? 1 : 0, 1, {0, 0}};
        last_rc_ = sfm_sparse_match(ctx_->get(), matches_dir_.c_str(), &o, &stats_);
        if (last_rc_ != SFM_OK) std::fprintf(stderr, "match failed: %s\n", sfm_last_error());
    }
    const sfm_sparse_match_stats& stats() const { return stats_; }

    // filter() (:1025-1280) with its settings: sGeometricModel "f" ->
    // GeometricFilter_FMatrix_AC(4.0, imax_iteration = 2048), no guided
    // matching: matches.putative.bin -> matches.f.bin
    void filter(double precision = 4.0, int max_iterations = 2048) {
        sfm_fmatrix_opts o{precision, max_iterations, 0};
        last_rc_ = sfm_sparse_filter(ctx_->get(), matches_dir_.c_str(), &o, &filter_stats_);
        if (last_rc_ != SFM_OK) std::fprintf(stderr, "filter failed: %s\n", sfm_last_error());
    }
    const sfm_sparse_filter_stats& filterStats() const { return filter_stats_; }

    // reconstruction() (:1283-1599) with its settings: engine INCREMENTAL,
    // PINHOLE_CAMERA_RADIAL3, ADJUST_ALL, no initial pair given: sfm_data.json
    // + <stem>.feat + matches.f.bin -> <base>/output/reconstruction/cloud_and_poses.ply
    // (the directory has to exist).  focal <= 0: 1.2 * max(w, h).  sfm_data.bin
    // is not written.
    void reconstruction(double focal = -1.0, const std::string& out_dir = std::string()) {
        const std::string out =
            !out_dir.empty() ? out_dir
            : matches_dir_.size() >= 7 ? matches_dir_.substr(0, matches_dir_.size() - 7) + "reconstruction"
                                       : std::string(".");
        last_rc_ = sfm_sparse_reconstruct(ctx_->get(), matches_dir_.c_str(), out.c_str(), focal, nullptr, &recon_stats_);
        if (last_rc_ != SFM_OK) std::fprintf(stderr, "reconstruction failed: %s\n", sfm_last_error());
    }
    const sfm_recon_stats& reconstructionStats() const { return recon_stats_; }

    // colorize() (:1601-1630) after reconstruction(): sfm_data.bin is not
    // written, so no file carries the scene from one stage to the next, and
    // this runs both (sfm_sparse_reconstruct_colorize): cloud_and_poses.ply as
    // reconstruction() writes it, and colorized.ply beside it, by default
    // <base>/output/reconstruction/colorized.ply.  images: the views' pixels in
    // the view order of sfm_data.json (data == nullptr: not loaded).  The
    // reference concatenates reconstruction_dir + "colorized.ply" without a
    // separator (sparseBuilder.cpp:1604, main.cpp:281), which puts the file
    // beside the directory under the name "reconstructioncolorized.ply"; that
    // is not copied here.
    void colorize(const std::vector<ColorImage>& images, double focal = -1.0, const std::string& out_dir = std::string()) {
        const std::string out =
            !out_dir.empty() ? out_dir
            : matches_dir_.size() >= 7 ? matches_dir_.substr(0, matches_dir_.size() - 7) + "reconstruction"
                                       : std::string(".");
        const ColorPool pool(images);
        last_rc_ = sfm_sparse_reconstruct_colorize(ctx_->get(), matches_dir_.c_str(), out.c_str(), focal, nullptr,
                                                   pool.channels.data(), pool.img_off.data(), pool.pixels, &recon_stats_,
                                                   &color_stats_);
        if (last_rc_ != SFM_OK) std::fprintf(stderr, "colorize failed: %s\n", sfm_last_error());
    }
    const sfm_colorize_stats& colorizeStats() const { return color_stats_; }

    // in-memory regions: per view, n x 128 uint8 descriptors
    void setRegions(std::vector<std::vector<uint8_t>> regions) { regions_ = std::move(regions); }
    // exhaustivePairs(N) (:786)
    std::vector<Pair> exhaustive() const {
        std::vector<Pair> p;
        const uint32_t n = (uint32_t)regions_.size();
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = i + 1; j < n; ++j) p.emplace_back(i, j);
        return p;
    }
    PairWiseMatches matchRegions(const std::vector<Pair>& pairs, float dist_ratio = 0.8f,
                                 const std::string& method = "AUTO") const {
        const int mode = matchingMode(method);
        if (mode < 0) throw Error(SFM_ERR_UNSUPPORTED, "unsupported nearest matching method " + method);
        std::vector<uint8_t> desc;
        std::vector<int64_t> off(1, 0);
        for (auto& r : regions_) {
            desc.insert(desc.end(), r.begin(), r.end());
            off.push_back(off.back() + (int64_t)(r.size() / 128));
        }
        sfm_match_plan* plan = nullptr;
        check(sfm_match_plan_create(ctx_->get(), desc.data(), off.data(), (int32_t)regions_.size(), &plan),
              "sfm_match_plan_create");
        std::vector<int32_t> pv;
        for (auto& p : pairs) { pv.push_back((int32_t)p.first); pv.push_back((int32_t)p.second); }
        sfm_match_options o{mode, dist_ratio};
        int64_t total = 0;
        int rc = sfm_match_plan_run(plan, pv.data(), (int64_t)pairs.size(), &o, &total);
        std::vector<int64_t> counts(pairs.size());
        std::vector<uint32_t> ii(std::max<int64_t>(total, 1)), jj(ii.size());
        std::vector<int32_t> dd(ii.size());
        if (rc == SFM_OK) rc = sfm_match_plan_fetch(plan, counts.data(), ii.data(), jj.data(), dd.data());
        sfm_match_plan_destroy(plan);
        check(rc, "sfm_match_plan");
        PairWiseMatches out;
        int64_t k = 0;
        for (std::size_t p = 0; p < pairs.size(); ++p) {
            auto& v = out[pairs[p]];
            for (int64_t c = 0; c < counts[p]; ++c, ++k) v.push_back(IndMatch{ii[k], jj[k]});
        }
        return out;
    }

   private:
    Context* ctx_;
    std::string matches_dir_;
    int last_rc_ = SFM_OK;
    sfm_sparse_match_stats stats_{};
    sfm_sparse_filter_stats filter_stats_{};
    sfm_recon_stats recon_stats_{};
    sfm_colorize_stats color_stats_{};
    std::vector<std::vector<uint8_t>> regions_;
};

}  // namespace sparse
}  // namespace sfm
