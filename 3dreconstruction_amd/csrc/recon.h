// Incremental reconstruction (include/sfmcore.h, "Incremental reconstruction"):
// the resident tracks handle and what recon.cpp (host: checks, the host twins,
// the driver) and recon.hip (the round kernels) share.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"

namespace sfm {

// a gather's result: off[n_images + 1], and the rows (when asked for)
struct ReconGather {
    std::vector<int64_t> off;
    std::vector<double> X3, uv;
    std::vector<int64_t> obs;   // the old index of each row's observation
};
// a select's result: the compacted sub-problem and its maps to the old indices
struct ReconSelect {
    int64_t n_pt = 0, n_obs = 0;
    std::vector<int64_t> pt_offsets, pt_map, obs_map;
    std::vector<int32_t> obs_img;
    std::vector<double> obs_uv;
};

// What the handle derives from the tracks once, on the host, for the kernels:
// every observation's point, whether its point has another observation in the
// same image (only those need the visibility's look back), and the
// observations image by image in ascending order (the gather's work list).
struct ReconIndex {
    std::vector<int32_t> pt_off, obs_pt, img_off, img_obs;
    std::vector<uint8_t> dup;
};

#ifndef SFM_RECON_HOST_ONLY
struct ReconDevice;   // recon.hip: the device arrays
ReconDevice* recon_device_create(sfm_ctx* ctx, int32_t n_img, int32_t n_pt, int32_t n_obs, const ReconIndex& ix,
                                 const int32_t* obs_img, const double* obs_uv);
void recon_device_destroy(ReconDevice* d);
void recon_device_drop(ReconDevice* d, const int32_t* obs, int64_t n);
void recon_device_visibility(ReconDevice* d, const uint8_t* pt_ok, int32_t* count);
// seg_off[n_images + 1]: the work list's layout (image q's observations are
// items seg_off[q] .. seg_off[q + 1] - 1); seg_base[q] = img_off[images[q]]
void recon_device_gather(ReconDevice* d, const double* X, const uint8_t* pt_ok, int32_t n_images,
                         const int32_t* seg_off, const int32_t* seg_base, bool rows, ReconGather& out);
void recon_device_select(ReconDevice* d, const uint8_t* registered, const uint8_t* pt_ok, int32_t mode,
                         int32_t min_track_len, bool rows, ReconSelect& out);
#endif

}  // namespace sfm

struct sfm_recon_tracks {
    sfm_ctx* ctx = nullptr;   // null: the host twin
    int32_t n_img = 0;
    int64_t n_pt = 0, n_obs = 0;
    std::vector<int32_t> img_off;   // [n_img + 1] observations per image, summed (both kinds)
    // the host twin's copy of the tracks
    std::vector<int64_t> pt_off;
    std::vector<int32_t> obs_img;
    std::vector<double> obs_uv;
    std::vector<uint8_t> dead;
#ifndef SFM_RECON_HOST_ONLY
    sfm::ReconDevice* dev = nullptr;
#endif
};
