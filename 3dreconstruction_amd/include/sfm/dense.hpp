// The dense hand-off (what denseWork() does before any MVS runs):
//   UndistortImages   every image undistorted (sfm_undistort), over a backend policy
//       int undistort(int32_t camera_model, int32_t n_img, int32_t n_intr, const int32_t* img_intr,
//                     const double* intr, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
//                     const uint8_t* pixels, const sfm_undistort_opts* opts, uint8_t* out,
//                     sfm_undistort_stats* stats) const;   // SFM_OK / SFM_ERR_*
//       const char* last_error() const;
//     sfm.hpp binds it to the GPU; HostUndistortBackend is the host twin, with the same bytes.
//   DenseBuilder      the reference's class (src/denseBuilder/DenseBuilder.h) over a
//                     WorldStructure: scene() returns the arrays that save() collects
//                     (sfm_dense_scene_*), exportUndistorted() writes <stem>.pgm / .ppm.
//                     The .mvs archive itself is not written.
//   DepthMapEstimator the depth-map phase of DensifyPointCloud over a DenseScene and the
//                     undistorted images: selectViews() (sfm_depth_views_select),
//                     estimate() (sfm_depthmap), filter() (sfm_depthmap_filter), fuse()
//                     (sfm_depthmap_fuse) into a DenseCloud, densify() (sfm_densify: the three
//                     in one call), over a backend policy with depthmap(), filter(), fuse()
//                     and densify(); sfm.hpp binds it to
//                     the GPU, HostDepthMapBackend is the host twin, with the same bytes.
// Header-only.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/sfmcore.h"
#include "colorize.hpp"
#include "world.hpp"

namespace sfm {

struct HostUndistortBackend {
    int undistort(int32_t camera_model, int32_t n_img, int32_t n_intr, const int32_t* img_intr, const double* intr,
                  const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                  const sfm_undistort_opts* opts, uint8_t* out, sfm_undistort_stats* stats) const {
        return sfm_undistort_host(camera_model, n_img, n_intr, img_intr, intr, wh, channels, img_off, pixels, opts, out,
                                  stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

// undistorted[k] = image k undistorted (empty where images[k].data is null),
// under intrinsics block img_intr[k] of intr (camera_model's width).  The C-ABI
// wants `out` at the offsets of `pixels`, so the images are packed into one pool
// first (one copy of each).  False when the call failed.
template <class Backend>
bool UndistortImages(const Backend& backend, int32_t camera_model, const std::vector<int32_t>& img_intr,
                     const std::vector<double>& intr, const std::vector<ColorImage>& images,
                     std::vector<std::vector<uint8_t>>& undistorted, const sfm_undistort_opts* opts = nullptr,
                     sfm_undistort_stats* stats = nullptr) {
    const size_t n = images.size();
    if (img_intr.size() != n) {
        std::fprintf(stderr, "UndistortImages failed: %zu images, %zu intrinsics indices\n", n, img_intr.size());
        return false;
    }
    std::vector<int32_t> wh, channels;
    std::vector<int64_t> img_off;
    std::vector<uint8_t> pool;
    for (const auto& im : images) {
        wh.push_back(im.w);
        wh.push_back(im.h);
        channels.push_back(im.channels);
        img_off.push_back(im.data ? (int64_t)pool.size() : -1);
        if (im.data && im.w > 0 && im.h > 0 && im.channels > 0)
            pool.insert(pool.end(), im.data, im.data + (size_t)im.w * im.h * im.channels);
    }
    const int iw = camera_model == SFM_CAM_RADIAL3 ? 6 : 4;
    std::vector<uint8_t> out(pool.size() + 1);
    pool.push_back(0);   // (never empty)
    wh.resize(wh.size() + 2, 1);
    channels.push_back(1);
    img_off.push_back(-1);
    std::vector<int32_t> ii(img_intr);
    ii.push_back(0);
    std::vector<double> kk(intr);
    kk.resize(kk.size() + 6, 1.0);
    const int rc = backend.undistort(camera_model, (int32_t)n, (int32_t)(intr.size() / iw), ii.data(), kk.data(),
                                     wh.data(), channels.data(), img_off.data(), pool.data(), opts, out.data(), stats);
    if (rc != SFM_OK) {
        std::fprintf(stderr, "UndistortImages failed: %s (code %d)\n", backend.last_error(), rc);
        return false;
    }
    undistorted.assign(n, {});
    for (size_t k = 0; k < n; ++k)
        if (img_off[k] >= 0)
            undistorted[k].assign(out.begin() + img_off[k],
                                  out.begin() + img_off[k] + (size_t)images[k].w * images[k].h * images[k].channels);
    return true;
}

// the arrays of sfm_dense_scene_fetch
struct DenseScene {
    sfm_dense_scene_info info{};
    std::vector<double> K, R, C;
    std::vector<int32_t> platform_wh, image_src, image_platform, image_pose;
    std::vector<float> vert_X;
    std::vector<int64_t> vert_off, vert_pt;
    std::vector<uint32_t> vert_view;
};

class DenseBuilder {
   public:
    explicit DenseBuilder(const WorldStructure::Ptr& structure) : structure_(structure) {}

    // The scene over `images` (every one registered, in this order; images[k]
    // is wh[2k..] pixels large): one platform per distinct Camera in order of
    // first use (SFM_CAM_PINHOLE: the Camera's fx fy cx cy are the K of the
    // undistorted images), the poses of the images, the points of the world.
    // False when the call failed.
    bool scene(const std::vector<Image::Ptr>& images, const std::vector<int32_t>& wh, DenseScene& out) const {
        if (wh.size() != 2 * images.size()) {
            std::fprintf(stderr, "DenseBuilder::scene failed: %zu images, %zu sizes\n", images.size(), wh.size() / 2);
            return false;
        }
        std::unordered_map<const Image*, int32_t> slot;
        std::vector<int32_t> img_intr, obs_img, sizes(wh);
        std::vector<double> intr, extr, X, uv(2, 0.0);
        cameras(images, img_intr, intr);
        for (size_t k = 0; k < images.size(); ++k) {
            slot[images[k].get()] = (int32_t)k;
            extr.insert(extr.end(), images[k]->pose().begin(), images[k]->pose().end());
        }
        std::vector<int64_t> off(1, 0);
        for (const auto& p : structure_->pointsByIdx()) {
            for (const auto& ob : p->observed_frames_) {
                const auto it = slot.find(ob.first.get());
                if (it != slot.end()) obs_img.push_back(it->second);
            }
            off.push_back((int64_t)obs_img.size());
            X.insert(X.end(), p->world_pos_.begin(), p->world_pos_.end());
        }
        sfm_ba_problem P{};
        P.n_img = (int32_t)images.size();
        P.n_intr = (int32_t)(intr.size() / 4);
        P.n_pt = (int64_t)off.size() - 1;
        P.n_obs = (int64_t)obs_img.size();
        uv.resize(2 * obs_img.size() + 2, 0.0);
        obs_img.push_back(0);   // (never empty)
        img_intr.push_back(0);
        intr.resize(intr.size() + 4, 1.0);
        extr.resize(extr.size() + 6, 0.0);
        X.resize(X.size() + 3, 0.0);
        sizes.resize(sizes.size() + 2, 1);
        P.pt_offsets = off.data();
        P.obs_img = obs_img.data();
        P.obs_uv = uv.data();
        P.img_intr = img_intr.data();
        P.const_img = -1;
        P.camera_model = SFM_CAM_PINHOLE;
        sfm_dense_scene* h = nullptr;
        int rc = sfm_dense_scene_build(&P, intr.data(), extr.data(), X.data(), sizes.data(), nullptr, nullptr, nullptr, &h);
        if (rc == SFM_OK) rc = sfm_dense_scene_get_info(h, &out.info);
        if (rc == SFM_OK) {
            const size_t np = (size_t)out.info.n_platforms, ni = (size_t)out.info.n_images,
                         nv = (size_t)out.info.n_vertices, nw = (size_t)out.info.n_views;
            out.K.assign(9 * np, 0.0);
            out.platform_wh.assign(2 * np, 0);
            out.image_src.assign(ni, 0);
            out.image_platform.assign(ni, 0);
            out.image_pose.assign(ni, 0);
            out.R.assign(9 * ni, 0.0);
            out.C.assign(3 * ni, 0.0);
            out.vert_X.assign(3 * nv, 0.f);
            out.vert_off.assign(nv + 1, 0);
            out.vert_view.assign(nw, 0);
            out.vert_pt.assign(nv, 0);
            rc = sfm_dense_scene_fetch(h, out.K.data(), out.platform_wh.data(), out.image_src.data(),
                                       out.image_platform.data(), out.image_pose.data(), out.R.data(), out.C.data(),
                                       out.vert_X.data(), out.vert_off.data(), out.vert_view.data(), out.vert_pt.data());
        }
        sfm_dense_scene_destroy(h);
        if (rc != SFM_OK) std::fprintf(stderr, "DenseBuilder::scene failed: %s (code %d)\n", sfm_last_error(), rc);
        return rc == SFM_OK;
    }

    // Writes dir/<stems[k]>.pgm (1 channel) or .ppm (3) for every loaded image,
    // undistorted.  radial3 (optional): k1 k2 k3 per distinct Camera, in order of
    // first use; the images are then resampled as SFM_CAM_RADIAL3 {fx, cx, cy,
    // k1, k2, k3}.  Without it the cameras carry no distortion and the images
    // are written as they are (SFM_CAM_PINHOLE: a byte copy).
    template <class Backend>
    bool exportUndistorted(const Backend& backend, const std::string& dir, const std::vector<Image::Ptr>& images,
                           const std::vector<std::string>& stems, const std::vector<ColorImage>& pixels,
                           const std::vector<double>* radial3 = nullptr, sfm_undistort_stats* stats = nullptr) const {
        if (stems.size() != images.size() || pixels.size() != images.size()) {
            std::fprintf(stderr, "DenseBuilder::exportUndistorted failed: %zu images, %zu names, %zu pixel arrays\n",
                         images.size(), stems.size(), pixels.size());
            return false;
        }
        std::vector<int32_t> img_intr;
        std::vector<double> pin, intr;
        cameras(images, img_intr, pin);
        if (radial3) {
            if (radial3->size() != pin.size() / 4 * 3) {
                std::fprintf(stderr, "DenseBuilder::exportUndistorted failed: %zu cameras, %zu distortion values\n",
                             pin.size() / 4, radial3->size());
                return false;
            }
            for (size_t b = 0; b < pin.size() / 4; ++b)
                intr.insert(intr.end(), {pin[4 * b], pin[4 * b + 2], pin[4 * b + 3], (*radial3)[3 * b],
                                         (*radial3)[3 * b + 1], (*radial3)[3 * b + 2]});
        } else {
            intr = pin;
        }
        std::vector<std::vector<uint8_t>> und;
        if (!UndistortImages(backend, radial3 ? SFM_CAM_RADIAL3 : SFM_CAM_PINHOLE, img_intr, intr, pixels, und, nullptr,
                             stats))
            return false;
        for (size_t k = 0; k < images.size(); ++k) {
            if (und[k].empty()) continue;
            const std::string path = dir + "/" + stems[k] + (pixels[k].channels == 1 ? ".pgm" : ".ppm");
            const int rc = sfm_undistort_write_pnm(path.c_str(), pixels[k].w, pixels[k].h, pixels[k].channels, und[k].data());
            if (rc != SFM_OK) {
                std::fprintf(stderr, "DenseBuilder::exportUndistorted failed: %s (code %d)\n", sfm_last_error(), rc);
                return false;
            }
        }
        return true;
    }

   private:
    // the distinct cameras of the images in order of first use, as {fx, fy, cx, cy} blocks
    static void cameras(const std::vector<Image::Ptr>& images, std::vector<int32_t>& img_intr, std::vector<double>& intr) {
        std::unordered_map<const Camera*, int32_t> block;
        for (const auto& im : images) {
            const Camera* c = im->getCamera().get();
            auto it = block.find(c);
            if (it == block.end()) {
                it = block.emplace(c, (int32_t)block.size()).first;
                const auto k = c->getIntrinsic();
                intr.insert(intr.end(), k.begin(), k.end());
            }
            img_intr.push_back(it->second);
        }
    }

    const WorldStructure::Ptr structure_;
};

struct HostDepthMapBackend {
    int depthmap(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                 const double* K, const double* R, const double* C, const int64_t* nb_off, const int32_t* nb_view,
                 const float* drange, const float* init_depth, const float* init_normal, const sfm_depthmap_opts* opts,
                 float* depth, float* normal, float* cost, sfm_depthmap_stats* stats) const {
        return sfm_depthmap_host(n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange, init_depth,
                                 init_normal, opts, depth, normal, cost, stats);
    }
    int filter(int32_t n_img, const int32_t* wh, const double* K, const double* R, const double* C, const int64_t* nb_off,
               const int32_t* nb_view, const float* depth, const float* cost, const sfm_depthmap_filter_opts* opts,
               float* depth_out, uint8_t* n_agree, int64_t* counts, sfm_depthmap_filter_stats* stats) const {
        return sfm_depthmap_filter_host(n_img, wh, K, R, C, nb_off, nb_view, depth, cost, opts, depth_out, n_agree, counts,
                                        stats);
    }
    int fuse(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
             const double* K, const double* R, const double* C, const int64_t* nb_off, const int32_t* nb_view,
             const float* depth, const float* normal, const sfm_depthmap_fuse_opts* opts, int64_t cap_points, float* X,
             float* N, uint8_t* rgb, uint8_t* n_views, uint32_t* view_mask, int32_t* src_image, int32_t* src_pixel,
             sfm_depthmap_fuse_stats* stats) const {
        return sfm_depthmap_fuse_host(n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, depth, normal, opts, cap_points,
                                      X, N, rgb, n_views, view_mask, src_image, src_pixel, stats);
    }
    int densify(int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off, const uint8_t* pixels,
                const double* K, const double* R, const double* C, const int64_t* nb_off, const int32_t* nb_view,
                const float* drange, const float* init_depth, const float* init_normal, const sfm_depthmap_opts* opts,
                const sfm_depthmap_filter_opts* filter_opts, const sfm_depthmap_fuse_opts* fuse_opts, int64_t cap_points,
                float* X, float* N, uint8_t* rgb, uint8_t* n_views, uint32_t* view_mask, int32_t* src_image,
                int32_t* src_pixel, float* depth, float* normal, float* cost, float* depth_filtered, uint8_t* n_agree,
                int64_t* counts, sfm_densify_stats* stats) const {
        return sfm_densify_host(n_img, wh, channels, img_off, pixels, K, R, C, nb_off, nb_view, drange, init_depth, init_normal,
                                opts, filter_opts, fuse_opts, cap_points, X, N, rgb, n_views, view_mask, src_image, src_pixel,
                                depth, normal, cost, depth_filtered, n_agree, counts, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

// The product of DensifyPointCloud: one point per emitted pixel, in ascending
// (image, y, x) order, with its normal, colour and the images that see it
// (view_off / view_idx: sfm_dense_cloud_views' CSR, own image first).
struct DenseCloud {
    std::vector<float> X, N;               // [3 n]
    std::vector<uint8_t> rgb, n_views;     // [3 n], [n]
    std::vector<uint32_t> view_mask;
    std::vector<int32_t> src_image, src_pixel, view_idx;
    std::vector<int64_t> view_off;
    size_t size() const { return src_image.size(); }
    bool writePly(const std::string& path) const {
        const float none[3] = {0.f, 0.f, 0.f};
        return sfm_dense_cloud_write_ply(path.c_str(), (int64_t)size(), size() ? X.data() : none, size() ? N.data() : none,
                                         size() ? rgb.data() : (const uint8_t*)"\0\0\0") == SFM_OK;
    }
};

// The depth-map phase over the scene's images (scene ID order; images[k] is the
// undistorted image of scene image k, data null where it is not loaded).
// selectViews() fills the neighbour lists and depth ranges (or set them
// yourself), estimate() the maps, filter() the filtered depth, fuse() the cloud
// from them; densify() does the three in one call and keeps the maps where the
// backend computes them.  Image k's maps start at pixel map_off[k].  Every step returns false when its call failed.
template <class Backend>
class DepthMapEstimator {
   public:
    DepthMapEstimator(const Backend& backend, const DenseScene& scene, const std::vector<ColorImage>& images)
        : backend_(backend), scene_(scene), images_(images) {
        int64_t at = 0;
        for (const auto& im : images_) {
            map_off.push_back(at);
            at += (int64_t)(im.w > 0 ? im.w : 0) * (im.h > 0 ? im.h : 0);
        }
        map_off.push_back(at);
    }

    bool selectViews(const sfm_depth_views_opts* opts = nullptr) {
        sfm_depth_views_opts o;
        sfm_depth_views_default_options(&o);
        if (opts) o = *opts;
        const size_t n = images_.size(), cap = n * (size_t)(o.max_neighbors > 0 ? o.max_neighbors : 0) + 1;
        if (n != (size_t)scene_.info.n_images) return fail("selectViews", "the scene and the images differ in number", 0);
        nb_off.assign(n + 1, 0);
        nb_view.assign(cap, 0);
        nb_score.assign(cap, 0.0);
        drange.assign(2 * n + 2, 0.f);
        const float none_x[3] = {0.f, 0.f, 0.f};
        const uint32_t none_v = 0;
        const int rc = sfm_depth_views_select(
            scene_.info.n_platforms, scene_.info.n_images, scene_.info.n_vertices, scene_.K.data(),
            scene_.image_platform.data(), scene_.R.data(), scene_.C.data(),
            scene_.vert_X.empty() ? none_x : scene_.vert_X.data(), scene_.vert_off.data(),
            scene_.vert_view.empty() ? &none_v : scene_.vert_view.data(), &o, nb_off.data(), nb_view.data(),
            nb_score.data(), drange.data());
        if (rc != SFM_OK) return fail("selectViews", sfm_last_error(), rc);
        nb_view.resize((size_t)nb_off[n]);
        nb_score.resize((size_t)nb_off[n]);
        return true;
    }

    bool estimate(const sfm_depthmap_opts* opts = nullptr, const float* init_depth = nullptr,
                  const float* init_normal = nullptr) {
        const size_t n = images_.size(), n_map = (size_t)map_off.back();
        if (nb_off.size() != n + 1 || drange.size() < 2 * n) return fail("estimate", "no neighbour lists: selectViews() first", 0);
        cameras();
        std::vector<int32_t> channels;
        std::vector<int64_t> img_off;
        std::vector<uint8_t> pool;
        for (const auto& im : images_) {
            channels.push_back(im.channels);
            img_off.push_back(im.data ? (int64_t)pool.size() : -1);
            if (im.data && im.w > 0 && im.h > 0 && im.channels > 0)
                pool.insert(pool.end(), im.data, im.data + (size_t)im.w * im.h * im.channels);
        }
        pool.push_back(0);   // (never empty)
        channels.push_back(1);
        img_off.push_back(-1);
        depth.assign(n_map + 1, 0.f);
        normal.assign(3 * n_map + 1, 0.f);
        cost.assign(n_map + 1, 0.f);
        std::vector<int32_t> nbv(nb_view);
        nbv.push_back(0);
        const int rc = backend_.depthmap((int32_t)n, wh_.data(), channels.data(), img_off.data(), pool.data(), K_.data(),
                                         scene_.R.data(), scene_.C.data(), nb_off.data(), nbv.data(), drange.data(),
                                         init_depth, init_normal, opts, depth.data(), normal.data(), cost.data(), &stats);
        if (rc != SFM_OK) return fail("estimate", backend_.last_error(), rc);
        depth.resize(n_map);
        normal.resize(3 * n_map);
        cost.resize(n_map);
        return true;
    }

    bool filter(const sfm_depthmap_filter_opts* opts = nullptr) {
        const size_t n = images_.size(), n_map = (size_t)map_off.back();
        if (depth.size() != n_map || cost.size() != n_map) return fail("filter", "no maps: estimate() first", 0);
        cameras();
        filtered.assign(n_map + 1, 0.f);
        n_agree.assign(n_map + 1, 0);
        counts.assign(2 * n + 2, 0);
        std::vector<int32_t> nbv(nb_view);
        nbv.push_back(0);
        std::vector<float> d(depth), c(cost);
        d.push_back(0.f);
        c.push_back(0.f);
        const int rc = backend_.filter((int32_t)n, wh_.data(), K_.data(), scene_.R.data(), scene_.C.data(), nb_off.data(),
                                       nbv.data(), d.data(), c.data(), opts, filtered.data(), n_agree.data(),
                                       counts.data(), &filter_stats);
        if (rc != SFM_OK) return fail("filter", backend_.last_error(), rc);
        filtered.resize(n_map);
        n_agree.resize(n_map);
        counts.resize(2 * n);
        return true;
    }

    // the cloud of the filtered maps (estimate() and filter() first)
    bool fuse(const sfm_depthmap_fuse_opts* opts = nullptr) {
        const size_t n = images_.size(), n_map = (size_t)map_off.back();
        if (filtered.size() != n_map || normal.size() != 3 * n_map) return fail("fuse", "no filtered maps: filter() first", 0);
        cameras();
        pool();
        std::vector<int32_t> nbv(nb_view);
        nbv.push_back(0);
        std::vector<float> d(filtered), nn(normal);
        d.push_back(0.f);
        nn.resize(nn.size() + 3, 0.f);
        int64_t cap = 0;
        for (size_t k = 0; k < n_map; ++k) cap += filtered[k] > 0.f;
        reserve_cloud((size_t)cap);
        const int rc = backend_.fuse((int32_t)n, wh_.data(), channels_.data(), img_off_.data(), pool_.data(), K_.data(),
                                     scene_.R.data(), scene_.C.data(), nb_off.data(), nbv.data(), d.data(), nn.data(), opts,
                                     cap, cloud.X.data(), cloud.N.data(), cloud.rgb.data(), cloud.n_views.data(),
                                     cloud.view_mask.data(), cloud.src_image.data(), cloud.src_pixel.data(), &fuse_stats);
        if (rc != SFM_OK) return fail("fuse", backend_.last_error(), rc);
        return finish_cloud((size_t)fuse_stats.n_points, nbv);
    }

    // estimate(), filter() and fuse() in one call; with keep_maps the maps are fetched as those steps leave them
    bool densify(const sfm_depthmap_opts* opts = nullptr, const sfm_depthmap_filter_opts* filter_opts = nullptr,
                 const sfm_depthmap_fuse_opts* fuse_opts = nullptr, bool keep_maps = false) {
        const size_t n = images_.size(), n_map = (size_t)map_off.back();
        if (nb_off.size() != n + 1 || drange.size() < 2 * n) return fail("densify", "no neighbour lists: selectViews() first", 0);
        cameras();
        pool();
        std::vector<int32_t> nbv(nb_view);
        nbv.push_back(0);
        reserve_cloud(n_map);
        const size_t m = keep_maps ? n_map + 1 : 0;
        depth.assign(m, 0.f);
        normal.assign(3 * m, 0.f);
        cost.assign(m, 0.f);
        filtered.assign(m, 0.f);
        n_agree.assign(m, 0);
        counts.assign(keep_maps ? 2 * n + 2 : 0, 0);
        const int rc = backend_.densify(
            (int32_t)n, wh_.data(), channels_.data(), img_off_.data(), pool_.data(), K_.data(), scene_.R.data(),
            scene_.C.data(), nb_off.data(), nbv.data(), drange.data(), nullptr, nullptr, opts, filter_opts, fuse_opts,
            (int64_t)n_map, cloud.X.data(), cloud.N.data(), cloud.rgb.data(), cloud.n_views.data(), cloud.view_mask.data(),
            cloud.src_image.data(), cloud.src_pixel.data(), keep_maps ? depth.data() : nullptr,
            keep_maps ? normal.data() : nullptr, keep_maps ? cost.data() : nullptr, keep_maps ? filtered.data() : nullptr,
            keep_maps ? n_agree.data() : nullptr, keep_maps ? counts.data() : nullptr, &densify_stats);
        if (rc != SFM_OK) return fail("densify", backend_.last_error(), rc);
        stats = densify_stats.depthmap;
        filter_stats = densify_stats.filter;
        fuse_stats = densify_stats.fuse;
        if (keep_maps) {
            depth.resize(n_map);
            normal.resize(3 * n_map);
            cost.resize(n_map);
            filtered.resize(n_map);
            n_agree.resize(n_map);
            counts.resize(2 * n);
        }
        return finish_cloud((size_t)fuse_stats.n_points, nbv);
    }

    DenseCloud cloud;
    sfm_depthmap_fuse_stats fuse_stats{};
    sfm_densify_stats densify_stats{};
    std::vector<int64_t> map_off, nb_off, counts;
    std::vector<int32_t> nb_view;
    std::vector<double> nb_score;
    std::vector<float> drange, depth, normal, cost, filtered;
    std::vector<uint8_t> n_agree;
    sfm_depthmap_stats stats{};
    sfm_depthmap_filter_stats filter_stats{};

   private:
    // K per image (the platform's) and the sizes, padded so that nothing is empty
    void cameras() {
        K_.clear();
        wh_.clear();
        for (size_t k = 0; k < images_.size(); ++k) {
            const double* Kp = scene_.K.data() + 9 * (size_t)scene_.image_platform[k];
            K_.insert(K_.end(), Kp, Kp + 9);
            wh_.push_back(images_[k].w);
            wh_.push_back(images_[k].h);
        }
        K_.resize(K_.size() + 9, 1.0);
        wh_.resize(wh_.size() + 2, 1);
    }
    // the images as one byte pool, padded so that nothing is empty
    void pool() {
        channels_.clear();
        img_off_.clear();
        pool_.clear();
        for (const auto& im : images_) {
            channels_.push_back(im.channels);
            img_off_.push_back(im.data ? (int64_t)pool_.size() : -1);
            if (im.data && im.w > 0 && im.h > 0 && im.channels > 0)
                pool_.insert(pool_.end(), im.data, im.data + (size_t)im.w * im.h * im.channels);
        }
        pool_.push_back(0);
        channels_.push_back(1);
        img_off_.push_back(-1);
    }
    void reserve_cloud(size_t cap) {
        cloud = DenseCloud();
        cloud.X.assign(3 * cap + 3, 0.f);
        cloud.N.assign(3 * cap + 3, 0.f);
        cloud.rgb.assign(3 * cap + 3, 0);
        cloud.n_views.assign(cap + 1, 0);
        cloud.view_mask.assign(cap + 1, 0);
        cloud.src_image.assign(cap + 1, 0);
        cloud.src_pixel.assign(cap + 1, 0);
    }
    bool finish_cloud(size_t n_points, const std::vector<int32_t>& nbv) {
        cloud.X.resize(3 * n_points);
        cloud.N.resize(3 * n_points);
        cloud.rgb.resize(3 * n_points);
        cloud.n_views.resize(n_points);
        cloud.view_mask.resize(n_points);
        cloud.src_image.resize(n_points);
        cloud.src_pixel.resize(n_points);
        const int32_t none_i = 0;
        const uint32_t none_m = 0;
        cloud.view_off.assign(n_points + 1, 0);
        for (int pass = 0; pass < 2; ++pass) {
            if (pass) cloud.view_idx.assign((size_t)cloud.view_off[n_points] + 1, 0);
            const int rc = sfm_dense_cloud_views((int32_t)images_.size(), nb_off.data(), nbv.data(), (int64_t)n_points,
                                                 n_points ? cloud.src_image.data() : &none_i,
                                                 n_points ? cloud.view_mask.data() : &none_m, cloud.view_off.data(),
                                                 pass ? cloud.view_idx.data() : nullptr);
            if (rc != SFM_OK) return fail("fuse", sfm_last_error(), rc);
        }
        cloud.view_idx.resize((size_t)cloud.view_off[n_points]);
        return true;
    }
    static bool fail(const char* step, const char* why, int rc) {
        std::fprintf(stderr, "DepthMapEstimator::%s failed: %s (code %d)\n", step, why, rc);
        return false;
    }

    const Backend backend_;
    const DenseScene& scene_;
    const std::vector<ColorImage> images_;
    std::vector<double> K_;
    std::vector<int32_t> wh_, channels_;
    std::vector<int64_t> img_off_;
    std::vector<uint8_t> pool_;
};

}  // namespace sfm
