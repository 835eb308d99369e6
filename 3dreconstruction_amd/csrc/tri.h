// N-view track triangulation: the device passes of tri.hip
// behind sfm_triangulate (tri.cpp).  The per-track algorithm is tri_point.h,
// shared with the host loop of sfm_triangulate_host; the kernel input
// (TrackInput, X and the maps null) and the point pass are track.h's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_types.h"
#include "common.h"
#include "track.h"

namespace sfm {

// counters, in sfm_tri_stats order
enum : int { kTcPtOk = 0, kTcPtShort, kTcPtAngle, kTcPtInfinite, kTcObsKept, kTcObsBad, kTcObsDepth, kTcObsResidual,
             kTcCount };

// Device results and scratch of one triangulation.
struct TriBuffers {
    DBuf<double> X;           // [3 * n_pt]
    DBuf<uint8_t> status;     // [n_pt]
    DBuf<uint8_t> keep_obs;   // [n_obs]
    DBuf<double> residual;    // [2 * n_obs]
    DBuf<double> gram;        // [10 * n_obs] scratch: C'C of each observation
    DBuf<double> ray;         // [3 * n_obs] scratch: R' b
    DBuf<uint8_t> bad;        // [n_obs] scratch: 1 for an observation without a finite bearing
    DBuf<uint8_t> code;       // [n_obs] scratch: the reject code at the final X
    DBuf<uint8_t> solved;     // [n_pt] scratch: what the solve pass left (kTriSolved ...)
    DBuf<unsigned long long> counts;   // [kTcCount]
    int64_t n_pt = 0, n_obs = 0;
    void alloc(int64_t n_pt_, int64_t n_obs_);
};

// The three passes on stream s (opts checked by the caller).
void tri_eval(const TrackInput& in, const sfm_tri_opts& o, TriBuffers& b, hipStream_t s);
// Results to the caller's arrays (each may be null); synchronises the stream.
void tri_download(TriBuffers& b, double* X, uint8_t* status, uint8_t* keep_obs, double* residual, sfm_tri_stats* stats,
                  hipStream_t s);

}  // namespace sfm
