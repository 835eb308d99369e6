// The incremental engine's choice of the initial pair among relative pose
// results (OpenMVG's AutomaticInitialPairChoice), defined once for the C++
// façade (include/sfm/relative_pose.hpp, best()) and the reconstruction driver
// (recon.cpp).  Plain C++ over the C-ABI structs: no other dependency.
#pragma once
#include <cstdint>

#include "../../include/sfmcore.h"

namespace sfm {

// Of the results that came out SFM_RELPOSE_OK with more than min_inliers
// inliers in front of both cameras (n_front, the inliers the angle is taken
// over) and an angle_median above min_angle_deg, the one with the largest
// angle_median (the first on a tie); -1 when there is none.
inline int64_t relpose_best(const sfm_relpose_result* results, int64_t n, int32_t min_inliers, double min_angle_deg) {
    int64_t b = -1;
    for (int64_t q = 0; q < n; ++q) {
        const sfm_relpose_result& r = results[q];
        if (r.status != SFM_RELPOSE_OK || !(r.n_front > min_inliers) || !(r.angle_median > min_angle_deg)) continue;
        if (b < 0 || r.angle_median > results[b].angle_median) b = q;
    }
    return b;
}

}  // namespace sfm
