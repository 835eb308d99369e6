// Depth-map fusion (include/sfmcore.h, "Dense fusion"): what fuse.cpp (host:
// checks, the fusion pair lists, the host twin, the CSR expansion, the cloud's
// PLY) and fuse.hip (the kernels and the launches) share.
#pragma once
#include <cstdint>
#include <vector>

#include "depthmap.h"
#include "fuse_point.h"

namespace sfm {

// sfm_depthmap_fuse_opts.device_bytes == 0
constexpr int64_t kFuseDefaultDeviceBytes = (int64_t)4 << 30;

// What a fusion works on, checked and precomputed on the host (fuse.cpp).
struct FuseProblem {
    DenseImages images;               // sizes, maps, the colour pool's window
    std::vector<FuseView> views;      // [n_img]
    std::vector<FusePair> pairs;      // the fusion pair lists, image after image
    int64_t n_blocks = 0;             // blocks of kFuseBlock pixels of all images
    int64_t max_blocks = 0;           // of one image
    int64_t n_pairs_dropped = 0;
    FuseParams prm;
};

// The cloud's arrays as the caller passes them (each but X may be NULL).
struct FuseOut {
    int64_t cap_points;
    float *X, *N;
    uint8_t *rgb, *n_views;
    uint32_t* view_mask;
    int32_t *src_image, *src_pixel;
};

// fuse.cpp: sfm_depthmap_fuse's checks and its problem; resident_bytes is what
// the device holds apart from the cloud
void fuse_prepare(const char* who, const DepthCameras& m, const int32_t* channels, const int64_t* img_off,
                  const uint8_t* pixels, const sfm_depthmap_fuse_opts* opts, FuseProblem& F, int64_t* resident_bytes);

#ifndef SFM_DEPTHMAP_HOST_ONLY
// fuse.hip.  Arguments already checked; seconds[3]: upload, kernels, download.
// When the cloud needs more than out.cap_points nothing is written, *n_points
// holds the need and the call throws SFM_ERR_INVALID_ARG.
void fuse_device(sfm_ctx* ctx, const FuseProblem& F, const float* depth, const float* normal, const uint8_t* pixels,
                 const FuseOut& out, int64_t* n_points, int64_t* n_suppressed, double* seconds);
// depth maps, filter and fusion over one set of device buffers.  The maps are
// downloaded where their pointers are non-NULL.
struct DensifyMaps {
    float *depth, *normal, *cost, *depth_filtered;
    uint8_t* n_agree;
    int64_t* counts;
};
void densify_device(sfm_ctx* ctx, const DepthCall& call, bool init_given, const float* init_depth,
                    const float* init_normal, const DepthFilterParams& fprm, const FuseProblem& F, const uint8_t* pixels,
                    const FuseOut& out, const DensifyMaps& maps, sfm_densify_stats* st);
#endif

}  // namespace sfm
