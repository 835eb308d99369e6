// SequentialSfMReconstructionEngine: OpenMVG's incremental engine (what
// sparseBuilder::reconstruction() runs, sparseBuilder.cpp:1283-1599) over a
// WorldStructure whose points carry their tracks (observed_frames_) and whose
// positions and poses are not known yet, over a backend policy
//   int reconstruct(const sfm_ba_problem& tracks, double* intr, const int32_t* wh, const int32_t* pairs,
//                   int64_t n_pairs, const sfm_recon_opts&, double* extr, double* X, uint8_t* registered,
//                   uint8_t* pt_ok, uint8_t* keep_obs, sfm_recon_round* rounds, int32_t cap_rounds,
//                   sfm_recon_cand* cands, int32_t cap_cands, sfm_recon_stats* stats);   // SFM_OK / SFM_ERR_*
//   const char* last_error() const;
// sfm.hpp binds it to the GPU (sfm_reconstruct); HostReconBackend is the host
// twin (sfm_reconstruct_host: no bundle adjustment, so its options start with
// adjust = 0).  Process() chooses the initial pair, registers the images round
// by round, triangulates and (GPU) adjusts; it writes the pose of every
// registered image, the position of every reconstructed point and the refined
// intrinsics of the cameras.  Cameras are the reference's pinhole Camera.
// Header-only.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../../include/sfmcore.h"
#include "world.hpp"

namespace sfm {

struct HostReconBackend {
    static constexpr bool adjusts = false;
    int reconstruct(const sfm_ba_problem& tracks, double* intr, const int32_t* wh, const int32_t* pairs, int64_t n_pairs,
                    const sfm_recon_opts& o, double* extr, double* X, uint8_t* registered, uint8_t* pt_ok,
                    uint8_t* keep_obs, sfm_recon_round* rounds, int32_t cap_rounds, sfm_recon_cand* cands,
                    int32_t cap_cands, sfm_recon_stats* stats) const {
        return sfm_reconstruct_host(&tracks, intr, wh, pairs, n_pairs, &o, extr, X, registered, pt_ok, keep_obs, rounds,
                                    cap_rounds, cands, cap_cands, stats);
    }
    const char* last_error() const { return sfm_last_error(); }
};

template <class Backend>
class BasicSequentialSfMReconstructionEngine {
   public:
    // images: the views in the order the tracks' images are numbered by (all of one size)
    BasicSequentialSfMReconstructionEngine(Backend backend, WorldStructure::Ptr world, std::vector<Image::Ptr> images,
                                           int32_t width, int32_t height)
        : backend_(std::move(backend)), world_(std::move(world)), images_(std::move(images)), w_(width), h_(height) {
        sfm_recon_default_options(&opt_);
        if (!Backend::adjusts) opt_.adjust = 0;
    }
    sfm_recon_opts& options() { return opt_; }
    // the engine's setInitialPair: positions in `images`
    void setInitialPair(int32_t i, int32_t j) {
        opt_.initial_pair[0] = i;
        opt_.initial_pair[1] = j;
    }
    // the candidate pairs of the initial pair search (default: every pair)
    void setPairs(std::vector<std::pair<int32_t, int32_t>> pairs) {
        pairs_ = std::move(pairs);
        has_pairs_ = true;
    }
    int lastError() const { return last_rc_; }
    const sfm_recon_stats& stats() const { return stats_; }
    const std::vector<sfm_recon_round>& rounds() const { return rounds_; }
    const std::vector<sfm_recon_cand>& candidates() const { return cands_; }
    // per image of `images` / per world point in index order
    const std::vector<uint8_t>& registered() const { return registered_; }
    const std::vector<uint8_t>& reconstructed() const { return pt_ok_; }

    // False when the call failed or no initial pair was found (nothing is written then).
    bool Process() {
        const int32_t n_img = (int32_t)images_.size();
        std::unordered_map<const Image*, int32_t> slot;
        std::unordered_map<const Camera*, int32_t> cam_slot;
        std::vector<Camera*> cams;
        std::vector<int32_t> img_intr, wh;
        std::vector<double> intr;
        for (int32_t k = 0; k < n_img; ++k) {
            slot[images_[k].get()] = k;
            Camera* cam = images_[k]->getCamera().get();
            auto ct = cam_slot.find(cam);
            if (ct == cam_slot.end()) {
                ct = cam_slot.emplace(cam, (int32_t)cam_slot.size()).first;
                cams.push_back(cam);
                const auto v = cam->getIntrinsic();
                intr.insert(intr.end(), v.begin(), v.end());
            }
            img_intr.push_back(ct->second);
            wh.push_back(w_);
            wh.push_back(h_);
        }
        // the tracks: every world point's observations in the listed images
        const auto& pts = world_->pointsByIdx();
        std::vector<int64_t> off(1, 0);
        std::vector<int32_t> obs_img;
        std::vector<double> obs_uv;
        for (const auto& p : pts) {
            for (const auto& ob : p->observed_frames_) {
                const auto it = slot.find(ob.first.get());
                if (it == slot.end()) continue;
                obs_img.push_back(it->second);
                obs_uv.push_back(ob.second.x);
                obs_uv.push_back(ob.second.y);
            }
            off.push_back((int64_t)obs_img.size());
        }
        std::vector<int32_t> pairs;
        if (has_pairs_) {
            for (const auto& pr : pairs_) {
                pairs.push_back(pr.first);
                pairs.push_back(pr.second);
            }
        } else {
            for (int32_t i = 0; i < n_img; ++i)
                for (int32_t j = i + 1; j < n_img; ++j) {
                    pairs.push_back(i);
                    pairs.push_back(j);
                }
        }
        sfm_ba_problem P{};
        P.n_img = n_img;
        P.n_intr = (int32_t)cams.size();
        P.n_pt = (int64_t)pts.size();
        P.n_obs = (int64_t)obs_img.size();
        obs_img.push_back(0);   // (never empty)
        obs_uv.resize(obs_uv.size() + 2, 0.0);
        pairs.resize(pairs.size() + 2, 0);
        P.pt_offsets = off.data();
        P.obs_img = obs_img.data();
        P.obs_uv = obs_uv.data();
        P.img_intr = img_intr.data();
        P.const_img = -1;
        P.camera_model = SFM_CAM_PINHOLE;
        P.huber_a = 4.0;
        std::vector<double> extr(6 * (size_t)n_img + 6), X(3 * pts.size() + 3);
        std::vector<uint8_t> keep((size_t)P.n_obs + 1);
        registered_.assign((size_t)n_img + 1, 0);
        pt_ok_.assign(pts.size() + 1, 0);
        rounds_.assign((size_t)n_img + 2, sfm_recon_round{});
        cands_.assign(4 * (size_t)n_img + 2, sfm_recon_cand{});
        stats_ = sfm_recon_stats{};
        last_rc_ = backend_.reconstruct(P, intr.data(), wh.data(), pairs.data(), (int64_t)(pairs.size() / 2) - 1, opt_,
                                        extr.data(), X.data(), registered_.data(), pt_ok_.data(), keep.data(),
                                        rounds_.data(), (int32_t)rounds_.size(), cands_.data(), (int32_t)cands_.size(),
                                        &stats_);
        registered_.resize((size_t)n_img);
        pt_ok_.resize(pts.size());
        rounds_.resize(std::min<size_t>(rounds_.size(), last_rc_ == SFM_OK ? (size_t)stats_.n_rounds : 0));
        cands_.resize(std::min<size_t>(cands_.size(), last_rc_ == SFM_OK ? (size_t)stats_.n_cands : 0));
        if (last_rc_ != SFM_OK) {
            std::fprintf(stderr, "Reconstruction failed: %s (code %d)\n", backend_.last_error(), last_rc_);
            return false;
        }
        if (stats_.status != SFM_RECON_OK) return false;
        for (int32_t k = 0; k < n_img; ++k) {
            if (!registered_[k]) continue;
            std::array<double, 6> pose;
            for (int a = 0; a < 6; ++a) pose[a] = extr[6 * (size_t)k + a];
            images_[k]->setPose(pose);
        }
        for (size_t p = 0; p < pts.size(); ++p)
            if (pt_ok_[p]) pts[p]->setPos({X[3 * p], X[3 * p + 1], X[3 * p + 2]});
        for (size_t c = 0; c < cams.size(); ++c)
            cams[c]->setIntrinsic({intr[4 * c], intr[4 * c + 1], intr[4 * c + 2], intr[4 * c + 3]});
        return true;
    }

   private:
    Backend backend_;
    WorldStructure::Ptr world_;
    std::vector<Image::Ptr> images_;
    int32_t w_, h_;
    sfm_recon_opts opt_{};
    std::vector<std::pair<int32_t, int32_t>> pairs_;
    bool has_pairs_ = false;
    sfm_recon_stats stats_{};
    std::vector<sfm_recon_round> rounds_;
    std::vector<sfm_recon_cand> cands_;
    std::vector<uint8_t> registered_, pt_ok_;
    int last_rc_ = SFM_OK;
};

class HostSequentialSfMReconstructionEngine : public BasicSequentialSfMReconstructionEngine<HostReconBackend> {
   public:
    HostSequentialSfMReconstructionEngine(WorldStructure::Ptr world, std::vector<Image::Ptr> images, int32_t width,
                                          int32_t height)
        : BasicSequentialSfMReconstructionEngine<HostReconBackend>(HostReconBackend{}, std::move(world),
                                                                   std::move(images), width, height) {}
};

}  // namespace sfm
