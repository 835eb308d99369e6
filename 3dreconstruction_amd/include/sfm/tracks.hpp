// TracksBuilder: pairwise matches into tracks, with the call shape of OpenMVG's
// tracks::TracksBuilder (Build, Filter, ExportToSTL, NbTracks) over plain
// stand-ins for its types, and a backend policy
//   int build(int32_t n_img, const int64_t* feat_off, int64_t n_pairs, const int32_t* pairs,
//             const int64_t* counts, const uint32_t* i, const uint32_t* j,
//             const sfm_tracks_opts&, sfm_tracks** out);       // SFM_OK / SFM_ERR_*
//   const char* last_error() const;
// sfm.hpp binds it to the GPU (sfm_tracks_build); HostTracksBackend is the
// serial union-find (sfm_tracks_build_host).
//
// Two differences from OpenMVG, both in what the library defines
// (include/sfmcore.h): track ids are canonical (0, 1, ... by smallest (image,
// feature)), not union-find roots; and the conflict and length rules are part
// of the build, so Build() already gives the tracks of Filter(2), and
// Filter(n) with another n builds again.  Header-only.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <map>
#include <utility>
#include <vector>

#include "../../../include/sfmcore.h"

namespace sfm {

using IndexT = uint32_t;
struct IndMatch {
    IndexT i_, j_;
};
using IndMatches = std::vector<IndMatch>;
using Pair = std::pair<IndexT, IndexT>;
using PairWiseMatches = std::map<Pair, IndMatches>;
using submapTrack = std::map<IndexT, IndexT>;       // image -> feature
using STLMAPTracks = std::map<IndexT, submapTrack>;  // track id -> track

struct HostTracksBackend {
    int build(int32_t n_img, const int64_t* feat_off, int64_t n_pairs, const int32_t* pairs, const int64_t* counts,
              const uint32_t* i, const uint32_t* j, const sfm_tracks_opts& o, sfm_tracks** out) const {
        return sfm_tracks_build_host(n_img, feat_off, n_pairs, pairs, counts, i, j, nullptr, &o, out);
    }
    const char* last_error() const { return sfm_last_error(); }
};

template <class Backend>
class BasicTracksBuilder {
   public:
    explicit BasicTracksBuilder(Backend backend) : backend_(std::move(backend)) {}
    BasicTracksBuilder(const BasicTracksBuilder&) = delete;
    BasicTracksBuilder& operator=(const BasicTracksBuilder&) = delete;
    ~BasicTracksBuilder() { reset(); }

    // The tracks of the matches (those of Filter(2)).  An image has as many
    // features as its largest matched index says.
    bool Build(const PairWiseMatches& matches) {
        pairs_.clear(); counts_.clear(); i_.clear(); j_.clear();
        std::vector<int64_t> n_feat;
        auto seen = [&](IndexT img, IndexT feat) {
            if (n_feat.size() <= img) n_feat.resize((std::size_t)img + 1, 0);
            n_feat[img] = std::max<int64_t>(n_feat[img], (int64_t)feat + 1);
        };
        for (const auto& kv : matches) {
            pairs_.push_back((int32_t)kv.first.first);
            pairs_.push_back((int32_t)kv.first.second);
            counts_.push_back((int64_t)kv.second.size());
            for (const IndMatch& m : kv.second) {
                seen(kv.first.first, m.i_);
                seen(kv.first.second, m.j_);
                i_.push_back(m.i_);
                j_.push_back(m.j_);
            }
        }
        off_.assign(n_feat.size() + 1, 0);
        for (std::size_t k = 0; k < n_feat.size(); ++k) off_[k + 1] = off_[k] + n_feat[k];
        return run(2);
    }

    // Keeps the tracks of at least nLengthSupTo observations (conflicts are gone already).
    bool Filter(std::size_t nLengthSupTo = 2) {
        if (nLengthSupTo < 2) nLengthSupTo = 2;
        return (int32_t)nLengthSupTo == len_ && tracks_ ? true : run((int32_t)nLengthSupTo);
    }

    std::size_t NbTracks() const { return (std::size_t)stats_.n_tracks; }
    const sfm_tracks_stats& stats() const { return stats_; }
    int lastError() const { return last_rc_; }

    void ExportToSTL(STLMAPTracks& out) const {
        out.clear();
        if (!tracks_) return;
        std::vector<int64_t> off((std::size_t)stats_.n_tracks + 1);
        std::vector<int32_t> img((std::size_t)stats_.n_obs);
        std::vector<uint32_t> feat((std::size_t)stats_.n_obs);
        if (sfm_tracks_fetch(tracks_, off.data(), img.data(), feat.data(), nullptr) != SFM_OK) return;
        for (int64_t t = 0; t < stats_.n_tracks; ++t) {
            submapTrack& tr = out[(IndexT)t];
            for (int64_t o = off[t]; o < off[t + 1]; ++o) tr.emplace_hint(tr.end(), (IndexT)img[o], feat[o]);
        }
    }

   private:
    void reset() {
        if (tracks_) sfm_tracks_destroy(tracks_);
        tracks_ = nullptr;
        stats_ = sfm_tracks_stats{};
    }
    bool run(int32_t min_len) {
        reset();
        len_ = min_len;
        if (off_.empty()) off_.assign(1, 0);
        sfm_tracks_opts o;
        sfm_tracks_default_options(&o);
        o.min_track_len = min_len;
        last_rc_ = backend_.build((int32_t)off_.size() - 1, off_.data(), (int64_t)counts_.size(), pairs_.data(),
                                  counts_.data(), i_.data(), j_.data(), o, &tracks_);
        if (last_rc_ == SFM_OK) last_rc_ = sfm_tracks_get_stats(tracks_, &stats_);
        if (last_rc_ != SFM_OK) {
            std::fprintf(stderr, "Track building failed: %s (code %d)\n", backend_.last_error(), last_rc_);
            reset();
            return false;
        }
        return true;
    }

    Backend backend_;
    std::vector<int64_t> off_, counts_;
    std::vector<int32_t> pairs_;
    std::vector<uint32_t> i_, j_;
    sfm_tracks* tracks_ = nullptr;
    sfm_tracks_stats stats_{};
    int32_t len_ = 2;
    int last_rc_ = SFM_OK;
};

class HostTracksBuilder : public BasicTracksBuilder<HostTracksBackend> {
   public:
    HostTracksBuilder() : BasicTracksBuilder<HostTracksBackend>(HostTracksBackend{}) {}
};

}  // namespace sfm
