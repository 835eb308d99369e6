// Post-BA outlier rejection for CDNA4 (gfx950), fp64: the filter OpenMVG's
// engine runs after every bundle adjustment (badTrackRejector:
// RemoveOutliers_PixelResidualError, then RemoveOutliers_AngleError) and the
// reference left as a hook (src/adjuster/BundleAdjuster.h:179-184, washPoint()).
//
//   obs pass    one lane per observation: project_residual and obs_verdict
//               (track.h) at the point's X -- P = R X + t, the unweighted
//               residual of the problem's camera model, the depth / residual
//               reject code -- and the ray R' P.
//               Streaming: reads image 4 B + measurement 16 B, writes residual
//               16 B + code 1 B + ray 24 B per observation (the cameras and
//               points it gathers are shared by neighbouring lanes).
//   point pass  track_point_kernel (track.h) with the WashPoint policy below:
//               survivors, the short-track rule and the largest angle between
//               two surviving rays, in one pass.
//
// Both write their results through kernel-order -> caller-order maps (a plan's
// shard order; null for arrays already in caller order).  The counters are
// integer block sums added with integer atomics: the same numbers every run.
#include "ba_wash.h"

namespace sfm {
namespace {

constexpr int kObsThreads = 256;
constexpr int kWin = kObsThreads + 2;   // pt_off window of an observation block: its points and their end

// blk_pt[b] = the point owning observation b * kObsThreads (one lane per point)
__global__ __launch_bounds__(256) void wash_block_point_kernel(const int32_t* __restrict__ pt_off, int32_t n_pt,
                                                              int32_t* __restrict__ blk_pt) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_pt) return;
    const int64_t a = pt_off[k], b = pt_off[k + 1];
    for (int64_t blk = (a + kObsThreads - 1) / kObsThreads; blk * kObsThreads < b; ++blk) blk_pt[blk] = (int32_t)k;
}

template <int CM>
__global__ __launch_bounds__(kObsThreads) void wash_obs_kernel(TrackInput in, ObsRule rule,
                                                               const int32_t* __restrict__ blk_pt,
                                                               double2* __restrict__ residual,
                                                               uint8_t* __restrict__ code, double* __restrict__ ray,
                                                               unsigned long long* __restrict__ counts) {
    __shared__ int32_t win[kWin];
    __shared__ unsigned cnt[2];
    const int tid = threadIdx.x;
    const int64_t s = (int64_t)blockIdx.x * kObsThreads + tid;
    const int32_t p0 = blk_pt[blockIdx.x];
    for (int i = tid; i < kWin; i += kObsThreads) win[i] = in.pt_off[min((int64_t)p0 + i, (int64_t)in.n_pt)];
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    uint8_t cd = kObsKeep;
    const bool live = s < in.n_obs;
    if (live) {
        // the observation's point: the last one of the window starting at or before s
        int lo = 0, hi = kWin - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (win[mid] <= s) lo = mid; else hi = mid - 1;
        }
        int32_t p = p0 + lo;
        if (lo == kWin - 1) {   // a run of points without observations longer than the window
            int32_t l = p, h = in.n_pt - 1;
            while (l < h) {
                const int32_t mid = l + (h - l + 1) / 2;
                if (in.pt_off[mid] <= s) l = mid; else h = mid - 1;
            }
            p = l;
        }
        const int32_t img = in.obs_img[s];
        const CamPre& cp = in.cp[img];
        const double* ib = in.intr + (int64_t)in.iw * in.img_intr[img];
        const double* Xp = in.X + 3 * (int64_t)p;
        const double X[3] = {Xp[0], Xp[1], Xp[2]};
        const double2 uv = reinterpret_cast<const double2*>(in.obs_uv)[s];
        double P[3], r0, r1;
        project_residual<CM>(cp, ib, X, uv.x, uv.y, P, r0, r1);
        cd = obs_verdict<CM>(rule, P, r0, r1);
        const int64_t so = in.obs_map ? in.obs_map[s] : s;
        residual[so] = make_double2(r0, r1);
        code[s] = cd;
        // the ray from the camera centre to the point in world axes, R' P
        double* d = ray + 3 * s;
#pragma unroll
        for (int j = 0; j < 3; ++j) d[j] = cp.R[j] * P[0] + cp.R[3 + j] * P[1] + cp.R[6 + j] * P[2];
    }
    const unsigned long long md = __ballot(cd == kObsDepth), mr = __ballot(cd == kObsResidual);
    if ((tid & 63) == 0) {
        if (md) atomicAdd(&cnt[0], (unsigned)__popcll(md));
        if (mr) atomicAdd(&cnt[1], (unsigned)__popcll(mr));
    }
    __syncthreads();
    if (tid < 2 && cnt[tid]) atomicAdd(&counts[tid == 0 ? kWcObsDepth : kWcObsResidual], (unsigned long long)cnt[tid]);
}

// The wash's side of the point pass (track.h): the verdict is the point rule
// alone; max_angle, keep_pt and keep_obs go out through the maps.
struct WashPoint {
    static constexpr int kCounts = 4;   // short, angle, points kept, observations kept
    __device__ static int slot(int t) {
        const int s[kCounts] = {kWcPtShort, kWcPtAngle, kWcPtKept, kWcObsKept};
        return s[t];
    }
    PointRule rule;
    double* __restrict__ max_angle;
    uint8_t* __restrict__ keep_obs;
    uint8_t* __restrict__ keep_pt;
    __device__ int verdict(int64_t, int survivors, double deg) const { return point_rule(rule, survivors, deg); }
    __device__ void point(const TrackInput& in, int64_t k, int v, double deg, unsigned (&c)[kCounts]) const {
        const int64_t pm = in.pt_map ? in.pt_map[k] : k;
        max_angle[pm] = deg;
        keep_pt[pm] = v == 0;
        c[0] += v == 1; c[1] += v == 2; c[2] += v == 0;
    }
    __device__ void obs(const TrackInput& in, int64_t s, bool keep, unsigned (&c)[kCounts]) const {
        keep_obs[in.obs_map ? in.obs_map[s] : s] = keep;
        c[3] += keep;
    }
};

}  // namespace

void WashBuffers::alloc(int64_t n_pt_, int64_t n_obs_) {
    n_pt = n_pt_;
    n_obs = n_obs_;
    residual.alloc(2 * (size_t)n_obs);
    max_angle.alloc((size_t)n_pt);
    keep_obs.alloc((size_t)n_obs);
    keep_pt.alloc((size_t)n_pt);
    code.alloc((size_t)n_obs);
    ray.alloc(3 * (size_t)n_obs);
    blk_pt.alloc(((size_t)n_obs + kObsThreads - 1) / kObsThreads);
    counts.alloc(kWcCount);
}

void ba_wash_eval(const TrackInput& in, const sfm_ba_wash_opts& o, WashBuffers& b, hipStream_t s, hipEvent_t* ev,
                  double* ms) {
    SFM_REQUIRE(b.n_pt == in.n_pt && b.n_obs == in.n_obs, SFM_ERR_INVALID_ARG, "internal: wash buffers of another size");
    b.counts.zero(s);
    const bool timed = ev && ms;
    auto lap = [&](double* out) {
        SFM_HIP(hipEventRecord(ev[1], s));
        SFM_HIP(hipEventSynchronize(ev[1]));
        float t = 0.f;
        SFM_HIP(hipEventElapsedTime(&t, ev[0], ev[1]));
        *out = t;
    };
    if (timed) {
        ms[0] = ms[1] = 0.0;
        SFM_HIP(hipEventRecord(ev[0], s));
    }
    if (in.n_obs > 0) {
        hipLaunchKernelGGL(wash_block_point_kernel, dim3((unsigned)((in.n_pt + 255) / 256)), dim3(256), 0, s, in.pt_off,
                           in.n_pt, b.blk_pt.p);
        SFM_HIP(hipGetLastError());
        const unsigned grid = (unsigned)(((int64_t)in.n_obs + kObsThreads - 1) / kObsThreads);
        SFM_BY_MODEL_ALL(in, hipLaunchKernelGGL(wash_obs_kernel<CM>, dim3(grid), dim3(kObsThreads), 0, s, in,
                                                ObsRule{o.max_residual_px, o.cheirality}, b.blk_pt.p,
                                                reinterpret_cast<double2*>(b.residual.p), b.code.p, b.ray.p,
                                                b.counts.p));
        SFM_HIP(hipGetLastError());
    }
    if (timed) {
        lap(&ms[0]);
        SFM_HIP(hipEventRecord(ev[0], s));
    }
    if (in.n_pt > 0)
        track_point_pass(in, WashPoint{PointRule{o.min_angle_deg, o.min_track_len}, b.max_angle.p, b.keep_obs.p,
                                       b.keep_pt.p},
                         b.code.p, b.ray.p, b.counts.p, s);
    if (timed) lap(&ms[1]);
}

void ba_wash_download(WashBuffers& b, double* residual, double* max_angle, uint8_t* keep_obs, uint8_t* keep_pt,
                      sfm_ba_wash_stats* stats, hipStream_t s) {
    const size_t no = (size_t)b.n_obs, np = (size_t)b.n_pt;
    if (residual && no) SFM_HIP(hipMemcpyAsync(residual, b.residual.p, 2 * no * sizeof(double), hipMemcpyDeviceToHost, s));
    if (max_angle && np) SFM_HIP(hipMemcpyAsync(max_angle, b.max_angle.p, np * sizeof(double), hipMemcpyDeviceToHost, s));
    if (keep_obs && no) SFM_HIP(hipMemcpyAsync(keep_obs, b.keep_obs.p, no, hipMemcpyDeviceToHost, s));
    if (keep_pt && np) SFM_HIP(hipMemcpyAsync(keep_pt, b.keep_pt.p, np, hipMemcpyDeviceToHost, s));
    unsigned long long c[kWcCount] = {0};
    if (stats) SFM_HIP(hipMemcpyAsync(c, b.counts.p, sizeof c, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    if (stats) {
        stats->n_obs_depth = (int64_t)c[kWcObsDepth];
        stats->n_obs_residual = (int64_t)c[kWcObsResidual];
        stats->n_pt_short = (int64_t)c[kWcPtShort];
        stats->n_pt_angle = (int64_t)c[kWcPtAngle];
        stats->n_obs_kept = (int64_t)c[kWcObsKept];
        stats->n_pt_kept = (int64_t)c[kWcPtKept];
    }
}

}  // namespace sfm
