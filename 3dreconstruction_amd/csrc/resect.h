// Camera resection: what sfm_resect (resect.cpp) hands the
// kernel of resect.hip.  The arithmetic is resect_pose.h, shared with the
// host twin sfm_resect_host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfm {

constexpr int kResectThreads = 256;      // one workgroup per image
constexpr int kResectMaxLdsSort = 8192;  // sort buffer in LDS up to this many slots

struct ResectArgs {
    const int64_t* off;        // [n_img + 1]
    const double* X;           // [3 n]
    const double* uv;          // [2 n]
    const int32_t* img_intr;   // [n_img]
    const double* intr;        // [iw * n_intr]
    int32_t iw;
    const double* cst;         // [n_img][4] logalpha0, the bound on the squared error, loge0, 0
    const uint32_t* rng;       // raw mt19937(default_seed) stream
    int64_t rng_n;
    double* bear;              // [3 n] bearings (scratch)
    uint8_t* ok;               // [n] 1: the bearing is finite (scratch)
    double* ltab;              // [n + n_img] log10(j), j = 0..n of each image (scratch)
    float* logc;               // [2 (n + n_img)] logcombi(k, n) | logcombi(3, k) per image (scratch)
    uint32_t* vidx;            // [n] the list samples draw from (scratch)
    uint32_t* binl;            // [n] best inliers so far (result)
    unsigned long long* gkey;  // sort keys of the images whose sort exceeds LDS, packed
    uint32_t* gval;
    const int64_t* goff;       // [n_img] slot offset of the image in gkey / gval, -1: LDS
    double* model;             // [n_img][24] the RANSAC model, the refined one (Rt each)
    double* stat;              // [n_img][6] min_nfa, squared threshold, n_inliers, iterations, status, 0
    int32_t* fail;             // set when an image exhausts the random stream
    int32_t max_iter, refine_iter;
    int32_t lds_slots;         // sort slots in dynamic LDS
};

// one launch of n_img workgroups on stream s
void resect_launch(const ResectArgs& a, int32_t camera_model, int64_t n_img, hipStream_t s);

}  // namespace sfm
