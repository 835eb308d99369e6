// The dense depth maps on the device (gfx950): everything of a call resident
// (gray images, maps, views, pairs), one launch for the initial planes and one
// per colour pass, all images of the call in each (grid z is the image).
//
//   tile     a workgroup owns kDepthTileW x kDepthTileH pixels of the reference
//            image and stages them and their half_window halo in LDS as bytes
//            (at most 42 x 26); a lane owns one pixel of the active colour (the
//            launch of the initial planes runs both colours, grid y), so a
//            workgroup is 256 lanes.  Tile origins are even, so a pixel's
//            colour is that of its place in the tile.
//   pixel    depthmap_point.h's depth_init_pixel / depth_update_pixel: the
//            reference patch sums once, then every hypothesis against every
//            neighbour.  The neighbours stay 8-bit in global memory and are
//            read with plain loads through L2: a tile's footprint in a
//            neighbour is a neighbourhood of like size.  The maps are read and
//            written in place: a pass reads the other colour and writes its own.
//   counts   the pixels left at cost 2: per lane, summed over the wavefront by
//            shuffles, over the workgroup through LDS, then one atomic add per
//            workgroup (integer sums: the order does not matter).  The filter
//            counts candidates and kept pixels per image the same way.
#pragma clang fp contract(off)

#include <algorithm>

#include "depthmap.h"

namespace sfm {
namespace {

enum { kDepthModeInit = 0, kDepthModeInitGiven = 1, kDepthModePass = 2 };
constexpr int kDepthLanes = kDepthTileW * kDepthTileH / 2;
constexpr int kDepthLdsBytes = (kDepthTileW + 2 * kDepthMaxHalfWindow) * (kDepthTileH + 2 * kDepthMaxHalfWindow);

struct DepthLaunch {
    const DepthView* views;
    const DepthPair* pairs;
    const uint8_t* gray;
    float *depth, *normal, *cost;
    DepthParams prm;
    int32_t tiles_x, mode, it, colour;
};

__global__ __launch_bounds__(kDepthLanes) void depth_pass_kernel(DepthLaunch a) {
    static_assert(kDepthTileW % 2 == 0 && kDepthTileH % 2 == 0, "tile origins are even");
    __shared__ uint8_t tile[kDepthLdsBytes];
    const DepthView& V = a.views[blockIdx.z];
    if (!V.active) return;
    const int32_t x0 = (int32_t)(blockIdx.x % (unsigned)a.tiles_x) * kDepthTileW;
    const int32_t y0 = (int32_t)(blockIdx.x / (unsigned)a.tiles_x) * kDepthTileH;
    if (x0 >= V.w || y0 >= V.h) return;
    const int32_t r = a.prm.r, stride = kDepthTileW + 2 * r, rows = kDepthTileH + 2 * r;
    const uint8_t* src = a.gray + V.gray_off;
    for (int32_t k = threadIdx.x; k < stride * rows; k += kDepthLanes) {
        const int32_t gx = x0 - r + k % stride, gy = y0 - r + k / stride;
        tile[k] = gx >= 0 && gx < V.w && gy >= 0 && gy < V.h ? src[(int64_t)gy * V.w + gx] : (uint8_t)0;
    }
    __syncthreads();
    const int32_t colour = a.mode == kDepthModePass ? a.colour : (int32_t)blockIdx.y;
    const int32_t ly = threadIdx.x / (kDepthTileW / 2);
    const int32_t lx = 2 * (threadIdx.x % (kDepthTileW / 2)) + ((ly + colour) & 1);
    const int32_t px = x0 + lx, py = y0 + ly;
    if (px >= V.w || py >= V.h) return;
    float* depth = a.depth + V.map_off;
    float* normal = a.normal + 3 * V.map_off;
    float* cost = a.cost + V.map_off;
    if (!depth_estimated(V, r, px, py)) {
        if (a.mode != kDepthModePass) {
            const int64_t idx = (int64_t)py * V.w + px;
            depth[idx] = 0.0f;
            normal[3 * idx] = normal[3 * idx + 1] = normal[3 * idx + 2] = 0.0f;
            cost[idx] = kDepthWorstCost;
        }
        return;
    }
    const DepthRef ref{tile, stride, x0 - r, y0 - r};
    if (a.mode == kDepthModePass)
        depth_update_pixel(V, a.pairs, a.gray, ref, a.prm, a.it, (int32_t)blockIdx.z, px, py, depth, normal, cost);
    else
        depth_init_pixel(V, a.pairs, a.gray, ref, a.prm, a.mode == kDepthModeInitGiven, (int32_t)blockIdx.z, px, py, depth,
                         normal, cost);
}

// sums v over the workgroup (256 lanes); the result is valid in thread 0
__device__ inline unsigned block_sum(unsigned v, unsigned* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned t = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < 4; ++w) t += lds[w];
    __syncthreads();
    return t;
}

// the pixels at cost 2 (an image without maps is all 0)
__global__ __launch_bounds__(256) void depth_count_kernel(const float* cost, int64_t n, unsigned long long* count) {
    __shared__ unsigned lds[4];
    unsigned c = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256)
        c += cost[k] >= kDepthWorstCost;
    const unsigned t = block_sum(c, lds);
    if (threadIdx.x == 0 && t) atomicAdd(count, (unsigned long long)t);
}

struct FilterLaunch {
    const DepthView* views;
    const DepthPair* pairs;
    const float *depth, *cost;
    float* depth_out;
    uint8_t* n_agree;
    unsigned long long* counts;
    DepthFilterParams prm;
};

__global__ __launch_bounds__(256) void depth_filter_kernel(FilterLaunch a) {
    __shared__ unsigned lds[4];
    const DepthView& V = a.views[blockIdx.z];
    const int64_t n = (int64_t)V.w * V.h, at = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if ((int64_t)blockIdx.x * 256 >= n) return;
    unsigned cand = 0, kept = 0;
    if (at < n) {
        const int32_t px = (int32_t)(at % V.w), py = (int32_t)(at / V.w);
        const int32_t need = a.prm.min_consistent < V.nb1 - V.nb0 ? a.prm.min_consistent : V.nb1 - V.nb0;
        const int32_t g = depth_filter_pixel(V, a.pairs, a.prm, px, py, a.depth, a.cost);
        cand = g >= 0;
        kept = g >= 0 && g >= need;
        a.depth_out[V.map_off + at] = kept ? a.depth[V.map_off + at] : 0.0f;
        a.n_agree[V.map_off + at] = (uint8_t)(g > 0 ? g : 0);
    }
    const unsigned t_cand = block_sum(cand, lds), t_kept = block_sum(kept, lds);
    if (threadIdx.x == 0) {
        if (t_cand) atomicAdd(a.counts + 2 * blockIdx.z, (unsigned long long)t_cand);
        if (t_kept) atomicAdd(a.counts + 2 * blockIdx.z + 1, (unsigned long long)t_kept);
    }
}

}  // namespace

void depth_estimate_upload(hipStream_t s, const DepthProblem& P, bool init_given, const float* depth,
                           const float* normal, DepthResident& r) {
    const size_t n_map = (size_t)P.n_map;
    r.views.alloc(P.views.size());
    r.pairs.alloc(std::max<size_t>(P.pairs.size(), 1));
    r.gray.alloc(P.gray.size());
    r.depth.alloc(n_map);
    r.normal.alloc(3 * n_map);
    r.cost.alloc(n_map);
    r.count.alloc(1);
    r.views.upload(P.views.data(), P.views.size(), s);
    r.pairs.upload(P.pairs.data(), P.pairs.size(), s);
    r.gray.upload(P.gray.data(), P.gray.size(), s);
    if (init_given) {
        r.depth.upload(depth, n_map, s);
        r.normal.upload(normal, 3 * n_map, s);
    } else {
        r.depth.zero(s);
        r.normal.zero(s);
    }
    r.cost.zero(s);
    r.count.zero(s);
}

void depth_estimate_launch(hipStream_t s, const DepthProblem& P, const DepthParams& prm, bool init_given,
                           DepthResident& r) {
    DepthLaunch a;
    a.views = r.views.p;
    a.pairs = r.pairs.p;
    a.gray = r.gray.p;
    a.depth = r.depth.p;
    a.normal = r.normal.p;
    a.cost = r.cost.p;
    a.prm = prm;
    a.tiles_x = (P.max_w + kDepthTileW - 1) / kDepthTileW;
    const int32_t tiles_y = (P.max_h + kDepthTileH - 1) / kDepthTileH;
    a.mode = init_given ? kDepthModeInitGiven : kDepthModeInit;
    a.it = 0;
    a.colour = 0;
    const dim3 block(kDepthLanes);
    hipLaunchKernelGGL(depth_pass_kernel, dim3((unsigned)(a.tiles_x * tiles_y), 2, (unsigned)P.n_img), block, 0, s, a);
    a.mode = kDepthModePass;
    for (int32_t it = 0; it < prm.iterations; ++it)
        for (int32_t colour = 0; colour < 2; ++colour) {
            a.it = it;
            a.colour = colour;
            hipLaunchKernelGGL(depth_pass_kernel, dim3((unsigned)(a.tiles_x * tiles_y), 1, (unsigned)P.n_img), block, 0, s,
                               a);
        }
    const unsigned count_blocks = (unsigned)std::min<int64_t>((P.n_map + 255) / 256, 1024);
    hipLaunchKernelGGL(depth_count_kernel, dim3(count_blocks), dim3(256), 0, s, r.cost.p, P.n_map, r.count.p);
    SFM_HIP(hipGetLastError());
}

void depth_estimate_counts(const DepthProblem& P, const DepthParams& prm, unsigned long long at_worst,
                           int64_t* n_estimated, int64_t* n_invalid) {
    // the pixels outside the estimated area are at cost 2 by construction
    int64_t est = 0, border = 0;
    for (const DepthView& V : P.views) {
        if (!V.active) continue;
        const int64_t e = (int64_t)std::max(V.w - 2 * prm.r, 0) * std::max(V.h - 2 * prm.r, 0);
        est += e;
        border += (int64_t)V.w * V.h - e;
    }
    *n_estimated = est;
    *n_invalid = (int64_t)at_worst - border;
}

void depth_filter_launch(hipStream_t s, const DepthProblem& P, const DepthFilterParams& prm, DepthResident& r) {
    const size_t n_map = (size_t)P.n_map;
    r.filtered.alloc(n_map);
    r.agree.alloc(n_map);
    r.fcounts.alloc((size_t)2 * P.n_img);
    r.fcounts.zero(s);
    int64_t largest = 0;
    for (const DepthView& V : P.views) largest = std::max(largest, (int64_t)V.w * V.h);
    FilterLaunch a{r.views.p, r.pairs.p, r.depth.p, r.cost.p, r.filtered.p, r.agree.p, r.fcounts.p, prm};
    hipLaunchKernelGGL(depth_filter_kernel, dim3((unsigned)((largest + 255) / 256), 1, (unsigned)P.n_img), dim3(256), 0, s,
                       a);
    SFM_HIP(hipGetLastError());
}

void depthmap_device(sfm_ctx* ctx, const DepthProblem& P, const DepthParams& prm, bool init_given, float* depth,
                     float* normal, float* cost, int64_t* n_estimated, int64_t* n_invalid, double* seconds) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    const size_t n_map = (size_t)P.n_map;
    DepthResident r;
    StreamEvents<4> ev;
    ev.record(0, s);
    depth_estimate_upload(s, P, init_given, depth, normal, r);
    ev.record(1, s);
    depth_estimate_launch(s, P, prm, init_given, r);
    ev.record(2, s);
    unsigned long long at_worst = 0;
    SFM_HIP(hipMemcpyAsync(depth, r.depth.p, n_map * sizeof(float), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(normal, r.normal.p, 3 * n_map * sizeof(float), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(cost, r.cost.p, n_map * sizeof(float), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(&at_worst, r.count.p, sizeof at_worst, hipMemcpyDeviceToHost, s));
    ev.record(3, s);
    SFM_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < 3; ++p) seconds[p] = ev.between(p, p + 1);
    depth_estimate_counts(P, prm, at_worst, n_estimated, n_invalid);
}

void depthmap_filter_device(sfm_ctx* ctx, const DepthProblem& P, const DepthFilterParams& prm, const float* depth,
                            const float* cost, float* depth_out, uint8_t* n_agree, int64_t* counts, double* seconds) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    const size_t n_map = (size_t)P.n_map;
    DepthResident r;
    r.views.alloc(P.views.size());
    r.pairs.alloc(std::max<size_t>(P.pairs.size(), 1));
    r.depth.alloc(n_map);
    r.cost.alloc(n_map);
    StreamEvents<4> ev;
    ev.record(0, s);
    r.views.upload(P.views.data(), P.views.size(), s);
    r.pairs.upload(P.pairs.data(), P.pairs.size(), s);
    r.depth.upload(depth, n_map, s);
    r.cost.upload(cost, n_map, s);
    ev.record(1, s);
    depth_filter_launch(s, P, prm, r);
    ev.record(2, s);
    std::vector<unsigned long long> cnt((size_t)2 * P.n_img, 0);
    SFM_HIP(hipMemcpyAsync(depth_out, r.filtered.p, n_map * sizeof(float), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(n_agree, r.agree.p, n_map, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(cnt.data(), r.fcounts.p, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    ev.record(3, s);
    SFM_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < 3; ++p) seconds[p] = ev.between(p, p + 1);
    for (size_t k = 0; k < cnt.size(); ++k) counts[k] = (int64_t)cnt[k];
}

}  // namespace sfm
