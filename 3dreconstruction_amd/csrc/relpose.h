// Relative pose: what sfm_relpose (relpose.cpp) hands the
// kernel of relpose.hip.  The arithmetic is relpose_pose.h, shared with the
// host twin sfm_relpose_host.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfm {

constexpr int kRelposeThreads = 256;      // one workgroup per pair
constexpr int kRelposeMaxLdsSort = 8192;  // sort buffer in LDS up to this many slots

struct RelposeArgs {
    const int64_t* off;        // [n_pairs + 1]
    const double* xy;          // [4 n] (x_I, y_I, x_J, y_J)
    const int32_t* pair_intr;  // [2 n_pairs]
    const double* intr;        // [iw * n_intr]
    int32_t iw;
    const double* cst;         // [n_pairs][4] logalpha0, the bound on the squared error, loge0, 0
    const uint32_t* rng;       // raw mt19937(default_seed) stream
    int64_t rng_n;
    double* bear;              // [6 n] bearings b_I, b_J (scratch)
    uint8_t* ok;               // [n] 1: both bearings are finite (scratch)
    double* ltab;              // [n + n_pairs] log10(j), j = 0..n of each pair (scratch)
    float* logc;               // [2 (n + n_pairs)] logcombi(k, n) | logcombi(5, k) per pair (scratch)
    uint32_t* vidx;            // [n] the list samples draw from; the front masks afterwards (scratch)
    uint32_t* binl;            // [n] best inliers so far (result)
    unsigned long long* gkey;  // sort keys of the pairs whose sort exceeds LDS, packed
    uint32_t* gval;
    const int64_t* goff;       // [n_pairs] slot offset of the pair in gkey / gval, -1: LDS
    double* model;             // [n_pairs][21] E, then the winning motion's R and t
    double* stat;              // [n_pairs][8] min_nfa, squared threshold, n_inliers, iterations, status,
                               //              n_front, angle_median, 0
    int32_t* fail;             // set when a pair exhausts the random stream
    int32_t max_iter;
    double front_ratio;
    int32_t lds_slots;         // sort slots in dynamic LDS
};

// one launch of n_pairs workgroups on stream s
void relpose_launch(const RelposeArgs& a, int32_t camera_model, int64_t n_pairs, hipStream_t s);

}  // namespace sfm
