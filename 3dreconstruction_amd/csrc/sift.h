// SIFT extraction: what sfm_sift (sift.cpp) hands the kernels
// of sift.hip.  The arithmetic is sift_point.h, shared with the host twin
// sfm_sift_host.  Every launch spans all images of the call: image `img` of a
// buffer starts at img * (elements of one image).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sift_point.h"

namespace sfm {

constexpr int kSiftTileX = 64, kSiftTileY = 16;   // outputs of one convolution workgroup

struct SiftOctave {
    sift::Levels lv;       // level i of image 0; image stride w * h
    int32_t w, h, S, n_img;
    double tp, te, sigma0, xper;
    const double* expn;    // [258]
    float* grad;           // [n_img][S][h][w][2] magnitude, angle of levels 1 .. S
    int32_t* rowcnt;       // [n_img][S * h] keypoints per (level, row)
    int32_t* rowbase;      // [n_img][S * h] exclusive scan of rowcnt
    int32_t* ktot;         // [n_img] keypoints of this octave
    sift::Keypoint* kps;   // [n_img][kcap] in (level, row, column) order of the extremum cell
    int32_t kcap;
    int32_t* nang;         // [n_img][kcap] orientations per keypoint
    double* angles;        // [n_img][kcap][4]
    int32_t* row;          // [n_img][kcap] output row of a keypoint's first feature
    int32_t* ftot;         // [n_img] features so far (running over the octaves)
    int32_t orientation, root_sift;
    int64_t cap;           // rows per image of xyso / desc
    float* xyso;           // [n_img][cap][4]
    uint8_t* desc;         // [n_img][cap][128]
};

void sift_launch_u8(const uint8_t* gray, float* out, int64_t n, hipStream_t s);
// dst(x, y) = src(2x, 2y): w x h from ws x hs
void sift_launch_decimate(const float* src, int ws, int hs, float* dst, int w, int h, int n_img, hipStream_t s);
// dst = rows(cols(src)) through tmp: the column pass, then the row pass (dst may be src)
void sift_launch_smooth(const float* src, float* tmp, float* dst, const float* taps, int W, int w, int h, int n_img,
                        hipStream_t s);
// rowcnt, then rowbase and ktot (count pass and scan)
void sift_launch_count(const SiftOctave& o, hipStream_t s);
// kps (needs kcap >= every ktot), grad, nang / angles, row and ftot, xyso / desc
void sift_launch_describe(const SiftOctave& o, int32_t kmax, hipStream_t s);

}  // namespace sfm
