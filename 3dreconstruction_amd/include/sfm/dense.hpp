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

}  // namespace sfm
