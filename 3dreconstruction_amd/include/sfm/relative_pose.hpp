// RelativePoser: the relative poses of image pairs from their matched
// keypoints (OpenMVG's robustRelativePose: AC-RANSAC over the five-point
// solver and the cheirality selection, what its incremental engine runs on
// every matched pair to choose the pair it starts from), over a backend policy
//   int relpose(int32_t camera_model, int64_t n_pairs, const int64_t* off, const double* xy,
//               const int32_t* pair_intr, const double* intr, int32_t n_intr, const int32_t* wh,
//               const sfm_relpose_opts&, sfm_relpose_result* results, int32_t* inliers);   // SFM_OK / SFM_ERR_*
//   const char* last_error() const;
// sfm.hpp binds it to the GPU (sfm_relpose); HostRelposeBackend is the serial
// host twin (sfm_relpose_host).  best() is the engine's choice of the initial
// pair (AutomaticInitialPairChoice).  Nothing is written to the images: the
// caller places the pair (identity, result) and goes on with the
// Triangulator.  The incremental loop (actuator.hpp) keeps its own stand-ins.
// Header-only.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../../include/sfmcore.h"
#include "../../csrc/relpose_best.h"
#include "world.hpp"

namespace sfm {

// one image pair and its matched keypoints: xy[k] = (x_I, y_I, x_J, y_J)
struct MatchedPair {
    Image::Ptr I, J;
    std::vector<std::array<double, 4>> xy;
};

struct HostRelposeBackend {
    int relpose(int32_t cm, int64_t n_pairs, const int64_t* off, const double* xy, const int32_t* pair_intr,
                const double* intr, int32_t n_intr, const int32_t* wh, const sfm_relpose_opts& o,
                sfm_relpose_result* results, int32_t* inliers) const {
        return sfm_relpose_host(cm, n_pairs, off, xy, pair_intr, intr, n_intr, wh, &o, results, inliers);
    }
    const char* last_error() const { return sfm_last_error(); }
};

template <class Backend>
class BasicRelativePoser {
   public:
    explicit BasicRelativePoser(Backend backend) : backend_(std::move(backend)) {
        sfm_relpose_default_options(&opt_);
    }
    sfm_relpose_opts& options() { return opt_; }
    int lastError() const { return last_rc_; }
    // per pair of the last call, in the order given: the result, and the
    // inliers as indices into that pair's matches
    const std::vector<sfm_relpose_result>& results() const { return results_; }
    const std::vector<std::vector<int32_t>>& inliers() const { return inliers_; }

    // Estimates every pair of `pairs` (all images of one size, width x
    // height) and returns the number that came out SFM_RELPOSE_OK.
    int64_t operator()(const std::vector<MatchedPair>& pairs, int32_t width, int32_t height) {
        std::unordered_map<const Camera*, int32_t> cam_slot;
        std::vector<double> intr, xy;
        std::vector<int32_t> pair_intr, wh;
        std::vector<int64_t> off(1, 0);
        for (const auto& p : pairs) {
            for (const Image::Ptr& im : {p.I, p.J}) {
                const Camera* cam = im->getCamera().get();
                auto ct = cam_slot.find(cam);
                if (ct == cam_slot.end()) {
                    ct = cam_slot.emplace(cam, (int32_t)cam_slot.size()).first;
                    const auto v = cam->getIntrinsic();
                    intr.insert(intr.end(), v.begin(), v.end());
                }
                pair_intr.push_back(ct->second);
                wh.push_back(width);
                wh.push_back(height);
            }
            for (const auto& m : p.xy) xy.insert(xy.end(), m.begin(), m.end());
            off.push_back((int64_t)(xy.size() / 4));
        }
        const int64_t n_pairs = (int64_t)pairs.size();
        results_.assign(n_pairs, sfm_relpose_result{});
        inliers_.assign(n_pairs, {});
        last_rc_ = SFM_OK;
        if (n_pairs == 0) return 0;
        std::vector<int32_t> inl(xy.size() / 4 + 1, -1);
        xy.resize(xy.size() + 4, 0.0);   // (never empty)
        last_rc_ = backend_.relpose(SFM_CAM_PINHOLE, n_pairs, off.data(), xy.data(), pair_intr.data(), intr.data(),
                                    (int32_t)cam_slot.size(), wh.data(), opt_, results_.data(), inl.data());
        if (last_rc_ != SFM_OK) {
            std::fprintf(stderr, "Relative pose failed: %s (code %d)\n", backend_.last_error(), last_rc_);
            return 0;
        }
        int64_t ok = 0;
        for (int64_t q = 0; q < n_pairs; ++q) {
            inliers_[q].assign(inl.begin() + off[q], inl.begin() + off[q] + results_[q].n_inliers);
            ok += results_[q].status == SFM_RELPOSE_OK;
        }
        return ok;
    }

    // The engine's choice among the pairs of the last call: of those that came
    // out SFM_RELPOSE_OK with more than min_inliers inliers in front of both
    // cameras (n_front, the inliers the angle is taken over) and an
    // angle_median above min_angle_deg, the one with the largest angle_median
    // (the first on a tie); -1 when there is none.
    int64_t best(int32_t min_inliers = 100, double min_angle_deg = 3.0) const {
        return relpose_best(results_.data(), (int64_t)results_.size(), min_inliers, min_angle_deg);
    }

   private:
    Backend backend_;
    sfm_relpose_opts opt_{};
    std::vector<sfm_relpose_result> results_;
    std::vector<std::vector<int32_t>> inliers_;
    int last_rc_ = SFM_OK;
};

class HostRelativePoser : public BasicRelativePoser<HostRelposeBackend> {
   public:
    HostRelativePoser() : BasicRelativePoser<HostRelposeBackend>(HostRelposeBackend{}) {}
};

}  // namespace sfm
