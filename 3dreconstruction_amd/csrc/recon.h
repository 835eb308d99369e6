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

// The argument checks of sfm_recon_tracks_create over a problem's tracks, and
// the index builder; inline, so that the track colouring (colorize.cpp) shares
// them in a host-only build without the driver's translation unit.
inline void recon_check_tracks(const char* who, const sfm_ba_problem* P) {
    SFM_REQUIRE(P, SFM_ERR_INVALID_ARG, "%s: null problem", who);
    SFM_REQUIRE(P->n_img >= 0 && P->n_pt >= 0 && P->n_obs >= 0, SFM_ERR_INVALID_ARG, "%s: negative count", who);
    SFM_REQUIRE(P->pt_offsets && (P->n_obs == 0 || (P->obs_img && P->obs_uv)), SFM_ERR_INVALID_ARG,
                "%s: incomplete problem", who);
    SFM_REQUIRE(P->pt_offsets[0] == 0 && P->pt_offsets[P->n_pt] == P->n_obs, SFM_ERR_INVALID_ARG,
                "%s: pt_offsets must run from 0 to n_obs", who);
    SFM_REQUIRE(P->n_obs < INT32_MAX && P->n_pt < INT32_MAX, SFM_ERR_UNSUPPORTED, "%s: 2^31 - 1 or more observations",
                who);
    for (int64_t p = 0; p < P->n_pt; ++p)
        SFM_REQUIRE(P->pt_offsets[p + 1] >= P->pt_offsets[p], SFM_ERR_INVALID_ARG,
                    "%s: pt_offsets not monotone at point %lld", who, (long long)p);
    for (int64_t o = 0; o < P->n_obs; ++o)
        SFM_REQUIRE(P->obs_img[o] >= 0 && P->obs_img[o] < P->n_img, SFM_ERR_INVALID_ARG,
                    "%s: observation %lld names image %d", who, (long long)o, P->obs_img[o]);
}

inline ReconIndex recon_build_index(const sfm_ba_problem& P, std::vector<int32_t>& img_off) {
    ReconIndex ix;
    const size_t N = (size_t)P.n_obs;
    ix.pt_off.resize((size_t)P.n_pt + 1);
    ix.obs_pt.resize(N);
    ix.dup.assign(N, 0);
    img_off.assign((size_t)P.n_img + 1, 0);
    std::vector<int64_t> first_at((size_t)P.n_img, -1);   // the point's first observation in the image ...
    std::vector<int64_t> first_of((size_t)P.n_img, -1);   // ... valid while this names the point
    for (int64_t p = 0; p <= P.n_pt; ++p) ix.pt_off[p] = (int32_t)P.pt_offsets[p];
    for (int64_t p = 0; p < P.n_pt; ++p)
        for (int64_t o = P.pt_offsets[p]; o < P.pt_offsets[p + 1]; ++o) {
            const int32_t im = P.obs_img[o];
            ix.obs_pt[o] = (int32_t)p;
            ++img_off[(size_t)im + 1];
            if (first_of[im] == p) {
                ix.dup[o] = 1;
                ix.dup[first_at[im]] = 1;
            } else {
                first_of[im] = p;
                first_at[im] = o;
            }
        }
    for (int32_t i = 0; i < P.n_img; ++i) img_off[(size_t)i + 1] += img_off[i];
    ix.img_off = img_off;
    ix.img_obs.resize(N);
    std::vector<int32_t> at(img_off.begin(), img_off.end() - 1);
    for (int64_t o = 0; o < P.n_obs; ++o) ix.img_obs[at[P.obs_img[o]]++] = (int32_t)o;
    return ix;
}

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
