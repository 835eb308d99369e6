// Track building (sfm_tracks_build): what tracks.cpp (argument checks, the
// host twin, the staging) and tracks.hip (the kernels) share.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"

// The handle of either build: the tracks on the host, in canonical order.
struct sfm_tracks {
    std::vector<int64_t> pt_offsets;   // [n_tracks + 1]
    std::vector<int32_t> obs_img;      // [n_obs]
    std::vector<uint32_t> obs_feat;    // [n_obs]
    std::vector<double> obs_uv;        // [2 * n_obs], built with xy only
    bool has_uv = false;
    sfm_tracks_stats st{};
};

namespace sfm {

// The checked input, as both builds read it: node ids in [0, n_space), image I
// owning feat_off[I] .. feat_off[I + 1] - 1, one edge per match.
struct TracksInput {
    int32_t n_img = 0, n_space = 0, n_edges = 0, min_len = 2;
    const int32_t* feat_off = nullptr;   // [n_img + 1]
    const int32_t* eu = nullptr;         // [n_edges]
    const int32_t* ev = nullptr;         // [n_edges]
    const double* xy = nullptr;          // [2 * n_space] or null
};

// the device build (tracks.hip); n_edges > 0
void tracks_device_build(sfm_ctx* ctx, const TracksInput& in, sfm_tracks& out);

}  // namespace sfm
