// Localizer: the poses of images of a WorldStructure from the world points
// they observe (OpenMVG's SfM_Localizer::Localize + RefinePose, what its
// incremental engine runs for every image it adds), over a backend policy
//   int resect(int32_t camera_model, int64_t n_img, const int64_t* off, const double* X, const double* uv,
//              const int32_t* img_intr, const double* intr, int32_t n_intr, const int32_t* wh,
//              const sfm_resect_opts&, sfm_resect_result* results, int32_t* inliers);   // SFM_OK / SFM_ERR_*
//   const char* last_error() const;
// sfm.hpp binds it to the GPU (sfm_resect); HostResectBackend is the serial
// host twin (sfm_resect_host).  An image's correspondences are the
// observations of it among the world points' observed_frames_, points in index
// order.  The pose is written back (Image::setPose) for the images that come
// out SFM_RESECT_OK only; the others keep theirs.  The incremental loop
// (actuator.hpp) keeps its own Gauss-Newton stand-in.  Header-only.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <vector>

#include "../../../include/sfmcore.h"
#include "world.hpp"

namespace sfm {

struct HostResectBackend {
    int resect(int32_t cm, int64_t n_img, const int64_t* off, const double* X, const double* uv,
               const int32_t* img_intr, const double* intr, int32_t n_intr, const int32_t* wh,
               const sfm_resect_opts& o, sfm_resect_result* results, int32_t* inliers) const {
        return sfm_resect_host(cm, n_img, off, X, uv, img_intr, intr, n_intr, wh, &o, results, inliers);
    }
    const char* last_error() const { return sfm_last_error(); }
};

template <class Backend>
class BasicLocalizer {
   public:
    explicit BasicLocalizer(Backend backend) : backend_(std::move(backend)) { sfm_resect_default_options(&opt_); }
    sfm_resect_opts& options() { return opt_; }
    int lastError() const { return last_rc_; }
    // per image of the last call, in the order given: the result, and the
    // inliers as indices into that image's correspondences
    const std::vector<sfm_resect_result>& results() const { return results_; }
    const std::vector<std::vector<int32_t>>& inliers() const { return inliers_; }

    // Resects every image of `images` (all of one size, width x height) and
    // returns the number of poses written.
    int64_t operator()(WorldStructure::Ptr& world, const std::vector<Image::Ptr>& images, int32_t width,
                       int32_t height) {
        std::unordered_map<const Image*, int32_t> slot;
        std::unordered_map<const Camera*, int32_t> cam_slot;
        std::vector<double> intr;
        std::vector<int32_t> img_intr, wh;
        for (const auto& im : images) {
            if (!slot.emplace(im.get(), (int32_t)slot.size()).second) continue;   // (listed twice: once)
            const Camera* cam = im->getCamera().get();
            auto ct = cam_slot.find(cam);
            if (ct == cam_slot.end()) {
                ct = cam_slot.emplace(cam, (int32_t)cam_slot.size()).first;
                const auto v = cam->getIntrinsic();
                intr.insert(intr.end(), v.begin(), v.end());
            }
            img_intr.push_back(ct->second);
            wh.push_back(width);
            wh.push_back(height);
        }
        const int64_t n_img = (int64_t)slot.size();
        std::vector<std::vector<double>> Xs(n_img), uvs(n_img);
        for (const auto& p : world->pointsByIdx())
            for (const auto& ob : p->observed_frames_) {
                const auto it = slot.find(ob.first.get());
                if (it == slot.end()) continue;
                Xs[it->second].insert(Xs[it->second].end(), p->world_pos_.begin(), p->world_pos_.end());
                uvs[it->second].push_back(ob.second.x);
                uvs[it->second].push_back(ob.second.y);
            }
        std::vector<int64_t> off(n_img + 1, 0);
        std::vector<double> X, uv;
        for (int64_t q = 0; q < n_img; ++q) {
            X.insert(X.end(), Xs[q].begin(), Xs[q].end());
            uv.insert(uv.end(), uvs[q].begin(), uvs[q].end());
            off[q + 1] = (int64_t)(uv.size() / 2);
        }
        results_.assign(n_img, sfm_resect_result{});
        inliers_.assign(n_img, {});
        last_rc_ = SFM_OK;
        if (n_img == 0) return 0;
        std::vector<int32_t> inl(uv.size() / 2 + 1, -1);
        last_rc_ = backend_.resect(SFM_CAM_PINHOLE, n_img, off.data(), X.data(), uv.data(), img_intr.data(),
                                   intr.data(), (int32_t)cam_slot.size(), wh.data(), opt_, results_.data(), inl.data());
        if (last_rc_ != SFM_OK) {
            std::fprintf(stderr, "Resection failed: %s (code %d)\n", backend_.last_error(), last_rc_);
            return 0;
        }
        int64_t written = 0;
        for (const auto& im : images) {
            const int32_t q = slot[im.get()];
            const sfm_resect_result& r = results_[q];
            inliers_[q].assign(inl.begin() + off[q], inl.begin() + off[q] + r.n_inliers);
            if (r.status != SFM_RESECT_OK) continue;
            im->setPose({r.pose[0], r.pose[1], r.pose[2], r.pose[3], r.pose[4], r.pose[5]});
            ++written;
        }
        return written;
    }

   private:
    Backend backend_;
    sfm_resect_opts opt_{};
    std::vector<sfm_resect_result> results_;
    std::vector<std::vector<int32_t>> inliers_;
    int last_rc_ = SFM_OK;
};

class HostLocalizer : public BasicLocalizer<HostResectBackend> {
   public:
    HostLocalizer() : BasicLocalizer<HostResectBackend>(HostResectBackend{}) {}
};

}  // namespace sfm
