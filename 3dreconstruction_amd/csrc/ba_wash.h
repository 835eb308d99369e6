// Post-BA outlier rejection ("wash"): per-observation residual
// and depth test, per-point survivor count and largest angle between the
// surviving rays (ba_wash.hip over the shared pieces of track.h), behind
// sfm_ba_wash (ba_wash.cpp: a TrackUpload of the caller's arrays, identity
// maps) and sfm_ba_plan_wash (ba_solver.cpp: a TrackInput over the plan's shard
// arrays, results scattered through its shard -> problem maps).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_types.h"
#include "common.h"
#include "track.h"

namespace sfm {

// counters, in sfm_ba_wash_stats order
enum : int { kWcObsDepth = 0, kWcObsResidual, kWcPtShort, kWcPtAngle, kWcObsKept, kWcPtKept, kWcCount };

// Device results (caller order) and scratch (kernel order) of one evaluation;
// a plan keeps them from its first wash on.
struct WashBuffers {
    DBuf<double> residual;    // [2 * n_obs]
    DBuf<double> max_angle;   // [n_pt]
    DBuf<uint8_t> keep_obs;   // [n_obs]
    DBuf<uint8_t> keep_pt;    // [n_pt]
    DBuf<uint8_t> code;       // [n_obs] scratch: reject code
    DBuf<double> ray;         // [3 * n_obs] scratch: R' P
    DBuf<int32_t> blk_pt;     // scratch: the point owning the first observation of each obs-pass workgroup
    DBuf<unsigned long long> counts;   // [kWcCount]
    int64_t n_pt = 0, n_obs = 0;
    void alloc(int64_t n_pt_, int64_t n_obs_);
};

// Both passes on stream s.  ev (two events) + ms[2]: the kernels' device
// times (observation pass, point pass) when ms is given; it synchronises.
void ba_wash_eval(const TrackInput& in, const sfm_ba_wash_opts& o, WashBuffers& b, hipStream_t s,
                  hipEvent_t* ev = nullptr, double* ms = nullptr);
// Results to the caller's arrays (each may be null); synchronises the stream.
void ba_wash_download(WashBuffers& b, double* residual, double* max_angle, uint8_t* keep_obs, uint8_t* keep_pt,
                      sfm_ba_wash_stats* stats, hipStream_t s);
// The options to use (null: the defaults), checked (SFM_ERR_INVALID_ARG).
sfm_ba_wash_opts wash_options(const sfm_ba_wash_opts* o);

}  // namespace sfm
