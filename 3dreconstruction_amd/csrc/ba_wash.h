// Post-BA outlier rejection ("wash"): per-observation residual
// and depth test, per-point survivor count and largest angle between the
// surviving rays (ba_wash.hip), behind sfm_ba_wash (ba_wash.cpp: caller-order
// arrays, identity maps) and sfm_ba_plan_wash (ba_solver.cpp: the plan's shard
// arrays, results scattered through its shard -> problem maps).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ba_types.h"
#include "common.h"

namespace sfm {

// reject code of an observation (obs pass -> point pass)
enum : uint8_t { kWashKeep = 0, kWashDepth = 1, kWashResidual = 2 };
// counters, in sfm_ba_wash_stats order
enum : int { kWcObsDepth = 0, kWcObsResidual, kWcPtShort, kWcPtAngle, kWcObsKept, kWcPtKept, kWcCount };

// lanes per point of the point pass's short form (a point of up to this many
// observations shares its wave with 64 / kWashGroup - 1 others); longer
// points take a whole wave each, in rounds of 64 observations
constexpr int kWashGroup = 16;

// What the two kernels read: observations grouped by point in "kernel order"
// (the caller's, or a plan's shard order) and the parameters.
struct WashInput {
    int32_t n_pt = 0, n_obs = 0, cam_model = 0, iw = 4;
    const int32_t* pt_off = nullptr;    // [n_pt + 1]
    const int32_t* obs_img = nullptr;   // [n_obs]
    const double* obs_uv = nullptr;     // [2 * n_obs]
    const int32_t* img_intr = nullptr;  // [n_img]
    const CamPre* cp = nullptr;         // [n_img]
    const double* intr = nullptr;       // [iw * n_intr]
    const double* X = nullptr;          // [3 * n_pt], kernel order
    // kernel order -> caller order (null: the identity)
    const int32_t* pt_map = nullptr;    // [n_pt]
    const int32_t* obs_map = nullptr;   // [n_obs]
};

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
void ba_wash_eval(const WashInput& in, const sfm_ba_wash_opts& o, WashBuffers& b, hipStream_t s,
                  hipEvent_t* ev = nullptr, double* ms = nullptr);
// Results to the caller's arrays (each may be null); synchronises the stream.
void ba_wash_download(WashBuffers& b, double* residual, double* max_angle, uint8_t* keep_obs, uint8_t* keep_pt,
                      sfm_ba_wash_stats* stats, hipStream_t s);
// The options to use (null: the defaults), checked (SFM_ERR_INVALID_ARG).
sfm_ba_wash_opts wash_options(const sfm_ba_wash_opts* o);

}  // namespace sfm
