// Triangulator: every point of a WorldStructure re-triangulated from its
// observed_frames_ and the current poses (OpenMVG's
// ComputeStructureFromKnownPoses; the reference triangulates two views at a
// time, SequentialActuator.h:206-223), over a backend policy
//   int triangulate(const sfm_ba_problem&, const double* extr, const double* intr,
//                   const sfm_tri_opts&, double* X, uint8_t* status, uint8_t* keep_obs,
//                   sfm_tri_stats&);                         // SFM_OK / SFM_ERR_*
//   const char* last_error() const;
// sfm.hpp binds it to the GPU (sfm_triangulate); HostTriBackend is the serial
// host loop (sfm_triangulate_host).  Positions are written back for the points
// that come out SFM_TRI_OK only; the others keep theirs.  The incremental loop
// (actuator.hpp) keeps its own two-view triangulation.  Header-only.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <vector>

#include "../../../include/sfmcore.h"
#include "world.hpp"

namespace sfm {

struct HostTriBackend {
    int triangulate(const sfm_ba_problem& pr, const double* extr, const double* intr, const sfm_tri_opts& o, double* X,
                    uint8_t* status, uint8_t* keep_obs, sfm_tri_stats& st) const {
        return sfm_triangulate_host(&pr, extr, intr, &o, X, status, keep_obs, nullptr, &st);
    }
    const char* last_error() const { return sfm_last_error(); }
};

template <class Backend>
class BasicTriangulator {
   public:
    explicit BasicTriangulator(Backend backend) : backend_(std::move(backend)) { sfm_tri_default_options(&opt_); }
    sfm_tri_opts& options() { return opt_; }
    const sfm_tri_stats& stats() const { return stats_; }
    int lastError() const { return last_rc_; }
    // status (SFM_TRI_*) of every point, in index order, and whether each
    // observation was kept, points in index order and each point's in its
    // observed_frames_ order
    const std::vector<uint8_t>& status() const { return status_; }
    const std::vector<uint8_t>& keptObservations() const { return keep_; }

    // Returns the number of points whose position was written.
    int64_t operator()(WorldStructure::Ptr& world) {
        const std::vector<WorldPoint::Ptr>& pts = world->pointsByIdx();
        std::unordered_map<const Image*, int32_t> img_slot;
        std::unordered_map<const Camera*, int32_t> cam_slot;
        std::vector<double> extr, intr, uv;
        std::vector<int32_t> img_intr, obs_img;
        std::vector<int64_t> off(pts.size() + 1, 0);
        for (std::size_t k = 0; k < pts.size(); ++k) {
            for (const auto& ob : pts[k]->observed_frames_) {
                auto it = img_slot.find(ob.first.get());
                if (it == img_slot.end()) {   // images and cameras in order of first appearance
                    it = img_slot.emplace(ob.first.get(), (int32_t)img_slot.size()).first;
                    const auto& p = ob.first->pose();
                    extr.insert(extr.end(), p.begin(), p.end());
                    const Camera* cam = ob.first->getCamera().get();
                    auto ct = cam_slot.find(cam);
                    if (ct == cam_slot.end()) {
                        ct = cam_slot.emplace(cam, (int32_t)cam_slot.size()).first;
                        const auto v = cam->getIntrinsic();
                        intr.insert(intr.end(), v.begin(), v.end());
                    }
                    img_intr.push_back(ct->second);
                }
                obs_img.push_back(it->second);
                uv.push_back(ob.second.x);
                uv.push_back(ob.second.y);
            }
            off[k + 1] = (int64_t)obs_img.size();
        }
        stats_ = sfm_tri_stats{};
        status_.assign(pts.size(), SFM_TRI_SHORT);
        keep_.assign(obs_img.size(), 0);
        last_rc_ = SFM_OK;
        if (pts.empty() || img_slot.empty()) return 0;
        sfm_ba_problem pr{};
        pr.n_img = (int32_t)img_slot.size();
        pr.n_intr = (int32_t)cam_slot.size();
        pr.n_pt = (int64_t)pts.size();
        pr.n_obs = (int64_t)obs_img.size();
        pr.pt_offsets = off.data();
        pr.obs_img = obs_img.data();
        pr.obs_uv = uv.data();
        pr.img_intr = img_intr.data();
        pr.const_img = -1;
        pr.camera_model = SFM_CAM_PINHOLE;
        std::vector<double> X(3 * pts.size());
        last_rc_ = backend_.triangulate(pr, extr.data(), intr.data(), opt_, X.data(), status_.data(), keep_.data(),
                                        stats_);
        if (last_rc_ != SFM_OK) {
            std::fprintf(stderr, "Triangulation failed: %s (code %d)\n", backend_.last_error(), last_rc_);
            return 0;
        }
        int64_t written = 0;
        for (std::size_t k = 0; k < pts.size(); ++k)
            if (status_[k] == SFM_TRI_OK) {
                pts[k]->setPos({X[3 * k], X[3 * k + 1], X[3 * k + 2]});
                ++written;
            }
        return written;
    }

   private:
    Backend backend_;
    sfm_tri_opts opt_{};
    sfm_tri_stats stats_{};
    std::vector<uint8_t> status_, keep_;
    int last_rc_ = SFM_OK;
};

class HostTriangulator : public BasicTriangulator<HostTriBackend> {
   public:
    HostTriangulator() : BasicTriangulator<HostTriBackend>(HostTriBackend{}) {}
};

}  // namespace sfm
