// Dense depth maps (include/sfmcore.h, "Dense depth maps"): what depthmap.cpp
// (host: checks, view selection, the per-pair matrices, the host twins) and
// depthmap.hip (the kernels and the launches) share.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"
#include "depthmap_point.h"

namespace sfm {

// The kernels' tile of the reference image.  A workgroup stages the tile and
// its half_window halo in LDS as bytes; in a colour pass a lane owns one pixel
// of the active colour, so a workgroup is kDepthTileW * kDepthTileH / 2 lanes.
constexpr int kDepthTileW = 32;
constexpr int kDepthTileH = 16;
// every image's gray bytes start at a multiple of this in the resident pool
constexpr int kDepthImageAlign = 256;
// sfm_depthmap_opts.device_bytes == 0
constexpr int64_t kDepthDefaultDeviceBytes = (int64_t)4 << 30;

inline int64_t depth_align_image(int64_t bytes) {
    return (bytes + kDepthImageAlign - 1) / kDepthImageAlign * kDepthImageAlign;
}

// What a call works on, checked and precomputed on the host (depthmap.cpp).
struct DepthProblem {
    int32_t n_img = 0;
    std::vector<DepthView> views;     // [n_img]
    std::vector<DepthPair> pairs;     // [nb_off[n_img]], the CSR's order
    std::vector<uint8_t> gray;        // the gray pool (DepthView::gray_off), images aligned
    int64_t n_map = 0;                // pixels of all maps (DepthView::map_off)
    int32_t max_w = 0, max_h = 0;     // over the active images
};

#ifndef SFM_DEPTHMAP_HOST_ONLY
// depthmap.hip.  Arguments already checked.  depth / normal / cost hold the
// initial planes where init is set (cost is overwritten); seconds[3]: upload,
// kernels, download.
void depthmap_device(sfm_ctx* ctx, const DepthProblem& P, const DepthParams& prm, bool init_given, float* depth,
                     float* normal, float* cost, int64_t* n_estimated, int64_t* n_invalid, double* seconds);
void depthmap_filter_device(sfm_ctx* ctx, const DepthProblem& P, const DepthFilterParams& prm, const float* depth,
                            const float* cost, float* depth_out, uint8_t* n_agree, int64_t* counts, double* seconds);
#endif

}  // namespace sfm
