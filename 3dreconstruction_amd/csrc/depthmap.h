// Dense depth maps (include/sfmcore.h, "Dense depth maps"): what depthmap.cpp
// (host: checks, view selection, the per-pair matrices, the host twins) and
// depthmap.hip (the kernels and the launches) share.
#pragma once
#include <cstdint>
#include <vector>

#include "dense_views.h"
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

// The cameras and neighbour lists of a call, as the C-ABI passes them.
struct DepthCameras {
    int32_t n_img;
    const int32_t* wh;
    const double *K, *R, *C;
    const int64_t* nb_off;
    const int32_t* nb_view;
};
// What sfm_depthmap works on after its checks (depth_prepare).
struct DepthCall {
    DepthProblem P;
    DepthParams prm;
    sfm_depthmap_stats st;
};

// depthmap.cpp, shared with fuse.cpp.
// A and b of the pair (reference i, neighbour j), in double, rounded once
void depth_pair_matrices(const DepthCameras& m, int32_t i, int32_t j, float* A, float* b);
// The checks that the estimation, the filter and the fusion share, and the views
// and pairs of the call.  channels / img_off / drange NULL: every image counts
// as loaded, no ranges.
void depth_build_problem(const char* who, const DepthCameras& m, const int32_t* channels, const int64_t* img_off,
                         const uint8_t* pixels, const float* drange, DepthProblem& P);
void depth_prepare(const char* who, int32_t n_img, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                   const uint8_t* pixels, const double* K, const double* R, const double* C, const int64_t* nb_off,
                   const int32_t* nb_view, const float* drange, const float* init_depth, const float* init_normal,
                   const sfm_depthmap_opts* opts, DepthCall& call);
void depth_filter_prepare(const char* who, const sfm_depthmap_filter_opts* opts, DepthFilterParams& prm);
void depth_init_maps(const DepthProblem& P, const float* init_depth, const float* init_normal, float* depth,
                     float* normal, float* cost);

#ifndef SFM_DEPTHMAP_HOST_ONLY
// depthmap.hip.  The device buffers of a call; sfm_densify keeps them for the
// filter and the fusion (fuse.hip).
struct DepthResident {
    DBuf<DepthView> views;
    DBuf<DepthPair> pairs;
    DBuf<uint8_t> gray;
    DBuf<float> depth, normal, cost;
    DBuf<unsigned long long> count;       // pixels at cost 2
    DBuf<float> filtered;                 // the filter's depth_out
    DBuf<uint8_t> agree;
    DBuf<unsigned long long> fcounts;     // [2 n_img] candidates, kept
};
// allocates and uploads what the estimation reads (depth / normal: the initial
// planes where init_given), enqueues its launches; n_estimated / n_invalid come
// from depth_estimate_counts once the stream has been synchronised
void depth_estimate_upload(hipStream_t s, const DepthProblem& P, bool init_given, const float* depth,
                           const float* normal, DepthResident& r);
void depth_estimate_launch(hipStream_t s, const DepthProblem& P, const DepthParams& prm, bool init_given,
                           DepthResident& r);
void depth_estimate_counts(const DepthProblem& P, const DepthParams& prm, unsigned long long at_worst,
                           int64_t* n_estimated, int64_t* n_invalid);
// the filter over r.depth / r.cost into r.filtered / r.agree / r.fcounts (allocated here; views and pairs resident)
void depth_filter_launch(hipStream_t s, const DepthProblem& P, const DepthFilterParams& prm, DepthResident& r);
// depthmap.hip.  Arguments already checked.  depth / normal / cost hold the
// initial planes where init is set (cost is overwritten); seconds[3]: upload,
// kernels, download.
void depthmap_device(sfm_ctx* ctx, const DepthProblem& P, const DepthParams& prm, bool init_given, float* depth,
                     float* normal, float* cost, int64_t* n_estimated, int64_t* n_invalid, double* seconds);
void depthmap_filter_device(sfm_ctx* ctx, const DepthProblem& P, const DepthFilterParams& prm, const float* depth,
                            const float* cost, float* depth_out, uint8_t* n_agree, int64_t* counts, double* seconds);
#endif

}  // namespace sfm
