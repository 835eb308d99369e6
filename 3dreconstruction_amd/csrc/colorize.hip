// The assignment of the track colouring on the device (gfx950): which view
// colours each point.  The counts are kept incrementally: a point that gets
// its colour takes 1 off every image it is seen in, so a round costs the
// chosen image's observation list and one reduction over the images, not a
// recount of every observation.
//
//   setup   one lane per point: view / obs / px start as "not coloured"; a
//           point to colour (pt_ok, a live observation) is flagged, adds 1 to
//           count[image] once per distinct image among its live observations
//           and 1 to the points left.  Integer atomics: the sums do not depend
//           on the order.
//   pick    one workgroup reduces count[0 .. n_img) to the largest count, the
//           lowest index on a tie, and leaves the view (-1 when no count is
//           positive) in device memory; a positive pick is appended to order.
//   colour  one lane per observation of the chosen image's list (the grid
//           covers the longest list; lanes past the chosen list leave).  A
//           live observation of a flagged point that is the first live one of
//           this image in its track owns the point: it writes view / obs / px,
//           clears the flag and takes the point off the counts.  A point has
//           one owner per round, so no two lanes write one point.
//
// Rounds are plain launches on the context's stream, kColorizeBatch at a time;
// the host reads the points left after each batch.  After the last round the
// pick leaves -1 and every colour lane leaves at once: an overrun changes
// nothing.  No kernel waits on another workgroup.
#include <algorithm>

#include "colorize.h"

namespace sfm {
namespace {

inline unsigned grid_of(int64_t n, int per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// the tracks and the masks as the kernels read them (pt_ok / keep null: all)
struct ColorView {
    const int32_t* pt_off;    // [n_pt + 1]
    const int32_t* obs_img;   // [n_obs]
    const int32_t* obs_pt;    // [n_obs]
    const uint8_t* dup;       // [n_obs] the point has another observation in this image
    const uint8_t* keep;      // [n_obs] or null
    __device__ bool live(int32_t o) const { return !keep || keep[o]; }
    // o is the first live observation of its image in the track of p
    __device__ bool first_in_image(int32_t p, int32_t o) const {
        if (!dup[o]) return true;
        const int32_t im = obs_img[o];
        for (int32_t q = pt_off[p]; q < o; ++q)
            if (live(q) && obs_img[q] == im) return false;
        return true;
    }
};

// the words the kernels share
enum { kCur = 0, kRounds = 1, kLeft = 2, kStateWords = 4 };

__global__ __launch_bounds__(kColorizeThreads) void colorize_setup_kernel(ColorView t, int32_t n_pt,
                                                                          const uint8_t* __restrict__ pt_ok,
                                                                          uint8_t* __restrict__ todo, int32_t* count,
                                                                          int32_t* state, int32_t* __restrict__ view,
                                                                          int32_t* __restrict__ obs,
                                                                          int32_t* __restrict__ px) {
    const int64_t p64 = (int64_t)blockIdx.x * kColorizeThreads + threadIdx.x;
    if (p64 >= n_pt) return;
    const int32_t p = (int32_t)p64;
    view[p] = -1;
    obs[p] = -1;
    px[2 * p64] = 0;
    px[2 * p64 + 1] = 0;
    bool any = false;
    if (!pt_ok || pt_ok[p])
        for (int32_t o = t.pt_off[p]; o < t.pt_off[p + 1]; ++o) {
            if (!t.live(o)) continue;
            any = true;
            if (t.first_in_image(p, o)) atomicAdd(&count[t.obs_img[o]], 1);
        }
    todo[p] = any;
    if (any) atomicAdd(&state[kLeft], 1);
}

__global__ __launch_bounds__(kColorizePickThreads) void colorize_pick_kernel(const int32_t* __restrict__ count,
                                                                             int32_t n_img, int32_t* state,
                                                                             int32_t* __restrict__ order) {
    __shared__ int32_t s_cnt[kColorizePickThreads / 64], s_idx[kColorizePickThreads / 64];
    // (count, index): a larger count wins, then a lower index
    int32_t bc = 0, bi = INT32_MAX;
    for (int32_t i = threadIdx.x; i < n_img; i += kColorizePickThreads) {   // ascending: `>` keeps the lowest index
        const int32_t c = count[i];
        if (c > bc) {
            bc = c;
            bi = i;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t oc = __shfl_down(bc, o), oi = __shfl_down(bi, o);
        if (oc > bc || (oc == bc && oi < bi)) {
            bc = oc;
            bi = oi;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_cnt[wave] = bc;
        s_idx[wave] = bi;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < kColorizePickThreads / 64; ++w)
        if (s_cnt[w] > bc || (s_cnt[w] == bc && s_idx[w] < bi)) {
            bc = s_cnt[w];
            bi = s_idx[w];
        }
    const int32_t r = state[kRounds];
    if (bc > 0 && r < n_img) {
        state[kCur] = bi;
        order[r] = bi;
        state[kRounds] = r + 1;
    } else {
        state[kCur] = -1;
    }
}

__global__ __launch_bounds__(kColorizeThreads) void colorize_colour_kernel(
    ColorView t, const int32_t* __restrict__ img_off, const int32_t* __restrict__ img_obs,
    const double* __restrict__ obs_uv, const int32_t* __restrict__ wh, uint8_t* todo, int32_t* count, int32_t* state,
    int32_t* __restrict__ view, int32_t* __restrict__ obs, int32_t* __restrict__ px) {
    const int32_t v = state[kCur];
    if (v < 0) return;
    const int64_t k = (int64_t)blockIdx.x * kColorizeThreads + threadIdx.x;
    const int32_t begin = img_off[v];
    if (k >= img_off[v + 1] - begin) return;
    const int32_t o = img_obs[begin + k];
    if (!t.live(o)) return;
    const int32_t p = t.obs_pt[o];
    // (another observation of p in v may read the flag while p's owner clears
    // it; that lane is not the first of v in the track and leaves either way)
    if (!todo[p] || !t.first_in_image(p, o)) return;
    view[p] = v;
    obs[p] = o;
    px[2 * (int64_t)p] = colorize_pixel(obs_uv[2 * (int64_t)o], wh[2 * v]);
    px[2 * (int64_t)p + 1] = colorize_pixel(obs_uv[2 * (int64_t)o + 1], wh[2 * v + 1]);
    todo[p] = 0;
    for (int32_t q = t.pt_off[p]; q < t.pt_off[p + 1]; ++q)
        if (t.live(q) && t.first_in_image(p, q)) atomicSub(&count[t.obs_img[q]], 1);
    atomicSub(&state[kLeft], 1);
}

}  // namespace

void colorize_device_assign(sfm_ctx* ctx, int32_t n_img, int32_t n_pt, int32_t n_obs, const ReconIndex& ix,
                            const int32_t* obs_img, const double* obs_uv, const int32_t* wh, const uint8_t* pt_ok,
                            const uint8_t* keep_obs, int32_t* view, int64_t* obs, int32_t* px, int32_t* order,
                            int32_t* n_rounds, int64_t* n_to_colour, int64_t* n_coloured, double* seconds) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    double t0 = seconds_now();
    const size_t N = (size_t)n_obs, NP = (size_t)n_pt, NI = (size_t)n_img;
    DBuf<int32_t> d_pt_off, d_obs_img, d_obs_pt, d_img_off, d_img_obs, d_wh, d_count, d_state, d_view, d_obs, d_px, d_order;
    DBuf<uint8_t> d_dup, d_ok, d_keep, d_todo;
    DBuf<double> d_uv;
    d_pt_off.alloc(NP + 1); d_pt_off.upload(ix.pt_off.data(), NP + 1, s);
    d_obs_img.alloc(N); d_obs_img.upload(obs_img, N, s);
    d_obs_pt.alloc(N); d_obs_pt.upload(ix.obs_pt.data(), N, s);
    d_img_off.alloc(NI + 1); d_img_off.upload(ix.img_off.data(), NI + 1, s);
    d_img_obs.alloc(N); d_img_obs.upload(ix.img_obs.data(), N, s);
    d_dup.alloc(N); d_dup.upload(ix.dup.data(), N, s);
    d_uv.alloc(2 * N); d_uv.upload(obs_uv, 2 * N, s);
    d_wh.alloc(2 * NI); d_wh.upload(wh, 2 * NI, s);
    if (pt_ok) { d_ok.alloc(NP); d_ok.upload(pt_ok, NP, s); }
    if (keep_obs) { d_keep.alloc(N); d_keep.upload(keep_obs, N, s); }
    d_todo.alloc(NP);
    d_count.alloc(NI); d_count.zero(s);
    d_state.alloc(kStateWords); d_state.zero(s);
    d_view.alloc(NP); d_obs.alloc(NP); d_px.alloc(2 * NP);
    d_order.alloc(NI);
    SFM_HIP(hipMemsetAsync(d_order.p, 0xFF, NI * sizeof(int32_t), s));   // -1: no round
    const ColorView t{d_pt_off.p, d_obs_img.p, d_obs_pt.p, d_dup.p, d_keep.p};
    hipLaunchKernelGGL(colorize_setup_kernel, dim3(grid_of(n_pt, kColorizeThreads)), dim3(kColorizeThreads), 0, s, t,
                       n_pt, d_ok.p, d_todo.p, d_count.p, d_state.p, d_view.p, d_obs.p, d_px.p);
    SFM_HIP(hipGetLastError());
    int32_t left = 0;
    SFM_HIP(hipMemcpyAsync(&left, d_state.p + kLeft, sizeof left, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    *n_to_colour = left;
    double t1 = seconds_now();
    seconds[0] = t1 - t0;

    // the colour kernel's grid: the longest per-image list
    int32_t longest = 0;
    for (int32_t i = 0; i < n_img; ++i) longest = std::max(longest, ix.img_off[(size_t)i + 1] - ix.img_off[i]);
    const unsigned colour_blocks = grid_of(longest, kColorizeThreads);
    // every positive round empties its view, so n_img rounds always suffice
    for (int32_t done = 0; left > 0 && done < n_img; done += kColorizeBatch) {
        for (int b = 0; b < kColorizeBatch; ++b) {
            hipLaunchKernelGGL(colorize_pick_kernel, dim3(1), dim3(kColorizePickThreads), 0, s, d_count.p, n_img,
                               d_state.p, d_order.p);
            hipLaunchKernelGGL(colorize_colour_kernel, dim3(colour_blocks), dim3(kColorizeThreads), 0, s, t,
                               d_img_off.p, d_img_obs.p, d_uv.p, d_wh.p, d_todo.p, d_count.p, d_state.p, d_view.p,
                               d_obs.p, d_px.p);
        }
        SFM_HIP(hipGetLastError());
        SFM_HIP(hipMemcpyAsync(&left, d_state.p + kLeft, sizeof left, hipMemcpyDeviceToHost, s));
        SFM_HIP(hipStreamSynchronize(s));
    }
    SFM_REQUIRE(left == 0, SFM_ERR_DEVICE, "sfm_colorize_assign: %d points left after %d rounds", left, n_img);
    const double t2 = seconds_now();
    seconds[1] = t2 - t1;

    std::vector<int32_t> obs32(NP);
    int32_t state[kStateWords];
    SFM_HIP(hipMemcpyAsync(view, d_view.p, NP * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(obs32.data(), d_obs.p, NP * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(px, d_px.p, 2 * NP * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(order, d_order.p, NI * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(state, d_state.p, sizeof state, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    for (size_t p = 0; p < NP; ++p) obs[p] = obs32[p];
    *n_rounds = state[kRounds];
    *n_coloured = *n_to_colour - state[kLeft];
    seconds[2] = seconds_now() - t2;
}

}  // namespace sfm
