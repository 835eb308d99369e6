// The round queries of the incremental reconstruction on the device (gfx950):
// the tracks stay resident, a round uploads its state (registered, pt_ok, X:
// image- and point-sized) and downloads compacted results.  Every output is
// integral or a gather, and every order comes from an exclusive scan, so the
// bytes equal the host twin's (recon.cpp).
//
//   visibility  one lane per observation (grid-stride): an alive observation
//               of a reconstructed point that is the first such of its point
//               in its image adds 1 to its image.  Integer atomics, first into
//               a per-workgroup LDS histogram (up to kVisLdsImages images),
//               then one global add per image and workgroup: the sums do not
//               depend on the order.
//   gather      the work list is the listed images' observations, image by
//               image (the handle's image-major index): flag = alive and
//               pt_ok, scan, scatter.  A lane finds its image by binary search
//               in the list's layout.
//   select      one lane per point decides whether the point qualifies (a
//               serial walk over its track, of any length); a scan over the
//               points numbers them, a scan over all observations of flag =
//               point qualifies, alive, image registered numbers the
//               observations: compaction in the old order.  A point's new
//               offset is the scan's value at its first observation.
//
// The scan is tracks.hip's: per-tile sums, one workgroup scans the tile sums,
// every tile applies.  Three launches, no kernel waits on another workgroup.
#include <algorithm>

#include "recon.h"

namespace sfm {
namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 4;
constexpr int kScanTile = kThreads * kScanItems;   // elements per scan tile: 1024
constexpr int kVisLdsImages = 4096;                // images of the LDS histogram (16 KiB)
constexpr int kVisMaxBlocks = 2048;

inline unsigned grid_of(int64_t n, int per_block = kThreads) { return (unsigned)((n + per_block - 1) / per_block); }

// the resident tracks as the kernels read them
struct ObsView {
    const int32_t* pt_off;    // [n_pt + 1]
    const int32_t* obs_img;   // [n_obs]
    const int32_t* obs_pt;    // [n_obs]
    const uint8_t* dup;       // [n_obs] the point has another observation in this image
    const uint8_t* dead;      // [n_obs]
};

// ---- visibility -------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void recon_visibility_kernel(ObsView v, int32_t n_obs, int32_t n_img,
                                                                    const uint8_t* __restrict__ pt_ok, int32_t* count,
                                                                    int use_lds) {
    __shared__ int32_t hist[kVisLdsImages];
    if (use_lds) {
        for (int32_t i = threadIdx.x; i < n_img; i += kThreads) hist[i] = 0;
        __syncthreads();
    }
    for (int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x; o < n_obs; o += (int64_t)gridDim.x * kThreads) {
        if (v.dead[o]) continue;
        const int32_t p = v.obs_pt[o];
        if (!pt_ok[p]) continue;
        const int32_t im = v.obs_img[o];
        bool seen = false;
        if (v.dup[o])   // an earlier alive observation of the point in this image counts instead
            for (int32_t q = v.pt_off[p]; q < o && !seen; ++q) seen = !v.dead[q] && v.obs_img[q] == im;
        if (seen) continue;
        if (use_lds) atomicAdd(&hist[im], 1);
        else atomicAdd(&count[im], 1);
    }
    if (use_lds) {
        __syncthreads();
        for (int32_t i = threadIdx.x; i < n_img; i += kThreads)
            if (hist[i]) atomicAdd(&count[i], hist[i]);
    }
}

// ---- the scan: exclusive count of the flags ------------------------------------
// exclusive prefix of `mine` over the workgroup's threads, and the total
__device__ __forceinline__ int32_t block_exclusive(int32_t mine, int32_t& total) {
    __shared__ int32_t wsum[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int32_t inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t c = __shfl_up(inc, o);
        if (lane >= o) inc += c;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int32_t base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) base += wsum[w];
        total += wsum[w];
    }
    __syncthreads();   // (wsum is written again by the next call)
    return base + inc - mine;
}

template <class Flag>
__device__ __forceinline__ void load_flags(const Flag& f, int32_t n, int64_t k0, int32_t (&x)[kScanItems]) {
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) x[t] = k0 + t < n ? f((int32_t)(k0 + t)) : 0;
}

// 1 of 3: every tile's count
template <class Flag>
__global__ __launch_bounds__(kThreads) void recon_scan_reduce_kernel(Flag f, int32_t n, int32_t* __restrict__ tile_sum) {
    int32_t x[kScanItems];
    load_flags(f, n, (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems, x);
    int32_t mine = 0;
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) mine += x[t];
    int32_t total;
    block_exclusive(mine, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// 2 of 3: the exclusive scan of the tile counts, in place, by one workgroup; *total_out = the grand total
__global__ __launch_bounds__(kThreads) void recon_scan_tiles_kernel(int32_t* tile_sum, int32_t n_tiles,
                                                                    int32_t* __restrict__ total_out) {
    int32_t carry = 0;
    for (int32_t base = 0; base < n_tiles; base += kThreads) {   // (uniform trip count)
        const int32_t k = base + threadIdx.x;
        const int32_t mine = k < n_tiles ? tile_sum[k] : 0;
        int32_t total;
        const int32_t ex = block_exclusive(mine, total);
        if (k < n_tiles) tile_sum[k] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// 3 of 3: emit(k, flag, the flags set before k) for every element
template <class Flag, class Emit>
__global__ __launch_bounds__(kThreads) void recon_scan_apply_kernel(Flag f, int32_t n,
                                                                    const int32_t* __restrict__ tile_sum, Emit emit) {
    const int64_t k0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int32_t x[kScanItems];
    load_flags(f, n, k0, x);
    int32_t mine = 0;
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) mine += x[t];
    int32_t total;
    int32_t at = tile_sum[blockIdx.x] + block_exclusive(mine, total);
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) {
        if (k0 + t < n) emit((int32_t)(k0 + t), x[t], at);
        at += x[t];
    }
}

// the first two launches, up to the total, which the host reads to size what the third fills
struct Scan {
    DBuf<int32_t> tiles, total;
    int32_t n = 0;
    template <class Flag>
    void sums(const Flag& f, int32_t count, hipStream_t s) {
        n = count;
        const int32_t n_tiles = (int32_t)grid_of(n, kScanTile);
        tiles.alloc((size_t)n_tiles);
        total.alloc(1);
        hipLaunchKernelGGL(recon_scan_reduce_kernel<Flag>, dim3(n_tiles), dim3(kThreads), 0, s, f, n, tiles.p);
        hipLaunchKernelGGL(recon_scan_tiles_kernel, dim3(1), dim3(kThreads), 0, s, tiles.p, n_tiles, total.p);
        SFM_HIP(hipGetLastError());
    }
    void fetch(int32_t* t, hipStream_t s) { SFM_HIP(hipMemcpyAsync(t, total.p, sizeof *t, hipMemcpyDeviceToHost, s)); }
    template <class Flag, class Emit>
    void apply(const Flag& f, const Emit& emit, hipStream_t s) {
        hipLaunchKernelGGL((recon_scan_apply_kernel<Flag, Emit>), dim3(grid_of(n, kScanTile)), dim3(kThreads), 0, s, f, n,
                           tiles.p, emit);
        SFM_HIP(hipGetLastError());
    }
};

// ---- gather -------------------------------------------------------------------
struct GatherFlag {
    int32_t n_seg;
    const int32_t* seg_off;    // [n_seg + 1]
    const int32_t* seg_base;   // [n_seg] where the image's observations start in img_obs
    const int32_t* img_obs;    // [n_obs] observations image by image, ascending
    const int32_t* obs_pt;
    const uint8_t* dead;
    const uint8_t* pt_ok;
    // item t's observation, and the listed image q it belongs to: the last q
    // with seg_off[q] <= t (images without observations share an offset with
    // the next image; the last of them is the one that has item t)
    __device__ int32_t obs_of(int32_t t, int32_t& q) const {
        int32_t lo = 0, hi = n_seg - 1;
        while (lo < hi) {
            const int32_t mid = (lo + hi + 1) >> 1;
            if (seg_off[mid] <= t) lo = mid;
            else hi = mid - 1;
        }
        q = lo;
        return img_obs[seg_base[lo] + (t - seg_off[lo])];
    }
    __device__ int32_t operator()(int32_t t) const {
        int32_t q;
        const int32_t o = obs_of(t, q);
        return !dead[o] && pt_ok[obs_pt[o]];
    }
};
struct GatherEmit {
    GatherFlag f;
    const double* X;        // [3 * n_pt]
    const double* obs_uv;   // [2 * n_obs]
    int32_t* off;           // [n_seg] (the images whose list starts before the end)
    double* X3;             // rows, or null
    double* uv;
    int32_t* obs;
    __device__ void operator()(int32_t t, int32_t flag, int32_t at) const {
        int32_t q;
        const int32_t o = f.obs_of(t, q);
        if (f.seg_off[q] == t)   // the first item of image q, and of the empty images listed just before it
            for (int32_t e = q; e >= 0 && f.seg_off[e] == t; --e) off[e] = at;
        if (flag && X3) {
            const int64_t p = f.obs_pt[o];
            for (int a = 0; a < 3; ++a) X3[3 * (int64_t)at + a] = X[3 * p + a];
            uv[2 * (int64_t)at] = obs_uv[2 * (int64_t)o];
            uv[2 * (int64_t)at + 1] = obs_uv[2 * (int64_t)o + 1];
            obs[at] = o;
        }
    }
};

// ---- select -------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void recon_select_points_kernel(ObsView v, int32_t n_pt,
                                                                       const uint8_t* __restrict__ registered,
                                                                       const uint8_t* __restrict__ pt_ok, int32_t mode,
                                                                       int32_t min_len, uint8_t* __restrict__ sel) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n_pt) return;
    const bool ok = pt_ok[p] != 0;
    if (ok != (mode == SFM_RECON_SOLVED)) {
        sel[p] = 0;
        return;
    }
    int32_t n = 0, first = -1;
    bool two = false;
    for (int32_t o = v.pt_off[p]; o < v.pt_off[p + 1]; ++o) {
        const int32_t im = v.obs_img[o];
        if (v.dead[o] || !registered[im]) continue;
        ++n;
        if (first < 0) first = im;
        else two |= im != first;
    }
    sel[p] = mode == SFM_RECON_SOLVED ? (n >= min_len) : two;
}

struct PointFlag {
    const uint8_t* sel;
    __device__ int32_t operator()(int32_t p) const { return sel[p]; }
};
struct PointEmit {
    int32_t* pt_idx;   // [n_pt] the new index of a selected point
    int32_t* pt_map;   // [n selected]
    __device__ void operator()(int32_t p, int32_t flag, int32_t at) const {
        if (flag) {
            pt_idx[p] = at;
            pt_map[at] = p;
        }
    }
};
struct ObsFlag {
    ObsView v;
    const uint8_t* sel;
    const uint8_t* registered;
    __device__ int32_t operator()(int32_t o) const {
        return sel[v.obs_pt[o]] && !v.dead[o] && registered[v.obs_img[o]];
    }
};
struct ObsEmit {
    ObsView v;
    const uint8_t* sel;
    const int32_t* pt_idx;
    const double* obs_uv;
    int32_t* pt_off_new;    // [n selected]
    int32_t* obs_map;       // [n kept]
    int32_t* obs_img_new;
    double* obs_uv_new;
    __device__ void operator()(int32_t o, int32_t flag, int32_t at) const {
        const int32_t p = v.obs_pt[o];
        if (sel[p] && o == v.pt_off[p]) pt_off_new[pt_idx[p]] = at;   // the kept observations before the point's first
        if (flag) {
            obs_map[at] = o;
            obs_img_new[at] = v.obs_img[o];
            obs_uv_new[2 * (int64_t)at] = obs_uv[2 * (int64_t)o];
            obs_uv_new[2 * (int64_t)at + 1] = obs_uv[2 * (int64_t)o + 1];
        }
    }
};

// ---- drop -----------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void recon_drop_kernel(const int32_t* __restrict__ obs, int32_t n,
                                                              uint8_t* __restrict__ dead) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < n) dead[obs[k]] = 1;   // (every writer stores the same byte)
}

template <class T>
void download(std::vector<T>& h, const DBuf<T>& d, size_t n, hipStream_t s) {
    h.resize(n);
    if (n) SFM_HIP(hipMemcpyAsync(h.data(), d.p, n * sizeof(T), hipMemcpyDeviceToHost, s));
}

}  // namespace

struct ReconDevice {
    sfm_ctx* ctx = nullptr;
    int32_t n_img = 0, n_pt = 0, n_obs = 0;
    DBuf<int32_t> pt_off, obs_img, obs_pt, img_obs;
    DBuf<uint8_t> dup, dead;
    DBuf<double> obs_uv;
    ObsView view() const { return ObsView{pt_off.p, obs_img.p, obs_pt.p, dup.p, dead.p}; }
};

ReconDevice* recon_device_create(sfm_ctx* ctx, int32_t n_img, int32_t n_pt, int32_t n_obs, const ReconIndex& ix,
                                 const int32_t* obs_img, const double* obs_uv) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    ReconDevice* d = new ReconDevice;
    try {
        d->ctx = ctx;
        d->n_img = n_img; d->n_pt = n_pt; d->n_obs = n_obs;
        const size_t N = (size_t)n_obs;
        d->pt_off.alloc((size_t)n_pt + 1); d->pt_off.upload(ix.pt_off.data(), (size_t)n_pt + 1, s);
        d->obs_img.alloc(N); d->obs_img.upload(obs_img, N, s);
        d->obs_pt.alloc(N); d->obs_pt.upload(ix.obs_pt.data(), N, s);
        d->img_obs.alloc(N); d->img_obs.upload(ix.img_obs.data(), N, s);
        d->dup.alloc(N); d->dup.upload(ix.dup.data(), N, s);
        d->obs_uv.alloc(2 * N); d->obs_uv.upload(obs_uv, 2 * N, s);
        d->dead.alloc(N); d->dead.zero(s);
        SFM_HIP(hipStreamSynchronize(s));   // (the index is the caller's temporary)
    } catch (...) {
        delete d;
        throw;
    }
    return d;
}

void recon_device_destroy(ReconDevice* d) {
    if (!d) return;
    CtxScope scope_(d->ctx);
    delete d;
}

void recon_device_drop(ReconDevice* d, const int32_t* obs, int64_t n) {
    if (n == 0) return;
    CtxScope scope_(d->ctx);
    hipStream_t s = d->ctx->stream;
    DBuf<int32_t> list;
    list.alloc((size_t)n); list.upload(obs, (size_t)n, s);
    hipLaunchKernelGGL(recon_drop_kernel, dim3(grid_of(n)), dim3(kThreads), 0, s, list.p, (int32_t)n, d->dead.p);
    SFM_HIP(hipGetLastError());
    SFM_HIP(hipStreamSynchronize(s));   // (obs is the caller's)
}

void recon_device_visibility(ReconDevice* d, const uint8_t* pt_ok, int32_t* count) {
    CtxScope scope_(d->ctx);
    hipStream_t s = d->ctx->stream;
    DBuf<uint8_t> ok;
    DBuf<int32_t> cnt;
    ok.alloc((size_t)d->n_pt); ok.upload(pt_ok, (size_t)d->n_pt, s);
    cnt.alloc((size_t)d->n_img); cnt.zero(s);
    if (d->n_obs) {
        const unsigned blocks = std::min<unsigned>(grid_of(d->n_obs), kVisMaxBlocks);
        hipLaunchKernelGGL(recon_visibility_kernel, dim3(blocks), dim3(kThreads), 0, s, d->view(), d->n_obs, d->n_img,
                           ok.p, cnt.p, d->n_img <= kVisLdsImages ? 1 : 0);
        SFM_HIP(hipGetLastError());
    }
    SFM_HIP(hipMemcpyAsync(count, cnt.p, (size_t)d->n_img * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
}

void recon_device_gather(ReconDevice* d, const double* X, const uint8_t* pt_ok, int32_t n_images,
                         const int32_t* seg_off, const int32_t* seg_base, bool rows, ReconGather& out) {
    out.off.assign((size_t)n_images + 1, 0);
    out.X3.clear();
    out.uv.clear();
    out.obs.clear();
    const int32_t T = n_images ? seg_off[n_images] : 0;
    if (T == 0) return;
    CtxScope scope_(d->ctx);
    hipStream_t s = d->ctx->stream;
    DBuf<uint8_t> ok;
    DBuf<int32_t> so, sb, off, rows_obs;
    DBuf<double> dX, X3, uv;
    ok.alloc((size_t)d->n_pt); ok.upload(pt_ok, (size_t)d->n_pt, s);
    so.alloc((size_t)n_images + 1); so.upload(seg_off, (size_t)n_images + 1, s);
    sb.alloc((size_t)n_images); sb.upload(seg_base, (size_t)n_images, s);
    off.alloc((size_t)n_images); off.zero(s);
    const GatherFlag f{n_images, so.p, sb.p, d->img_obs.p, d->obs_pt.p, d->dead.p, ok.p};
    Scan scan;
    scan.sums(f, T, s);
    int32_t total = 0;
    scan.fetch(&total, s);
    SFM_HIP(hipStreamSynchronize(s));
    if (rows && total) {
        dX.alloc(3 * (size_t)d->n_pt); dX.upload(X, 3 * (size_t)d->n_pt, s);
        X3.alloc(3 * (size_t)total);
        uv.alloc(2 * (size_t)total);
        rows_obs.alloc((size_t)total);
    }
    scan.apply(f, GatherEmit{f, dX.p, d->obs_uv.p, off.p, X3.p, uv.p, rows_obs.p}, s);
    std::vector<int32_t> off32, obs32;
    download(off32, off, (size_t)n_images, s);
    if (rows && total) {
        download(obs32, rows_obs, (size_t)total, s);
        download(out.X3, X3, 3 * (size_t)total, s);
        download(out.uv, uv, 2 * (size_t)total, s);
    }
    SFM_HIP(hipStreamSynchronize(s));
    // an image whose list starts at the end (no observations, last in the list) has no item to write its offset
    for (int32_t q = 0; q < n_images; ++q) out.off[q] = seg_off[q] == T ? total : off32[q];
    out.off[n_images] = total;
    out.obs.assign(obs32.begin(), obs32.end());
}

void recon_device_select(ReconDevice* d, const uint8_t* registered, const uint8_t* pt_ok, int32_t mode,
                         int32_t min_track_len, bool rows, ReconSelect& out) {
    out = ReconSelect{};
    out.pt_offsets.assign(1, 0);
    if (d->n_pt == 0 || d->n_obs == 0) return;
    CtxScope scope_(d->ctx);
    hipStream_t s = d->ctx->stream;
    DBuf<uint8_t> reg, ok, sel;
    reg.alloc((size_t)d->n_img); reg.upload(registered, (size_t)d->n_img, s);
    ok.alloc((size_t)d->n_pt); ok.upload(pt_ok, (size_t)d->n_pt, s);
    sel.alloc((size_t)d->n_pt);
    const ObsView v = d->view();
    hipLaunchKernelGGL(recon_select_points_kernel, dim3(grid_of(d->n_pt)), dim3(kThreads), 0, s, v, d->n_pt, reg.p, ok.p,
                       mode, min_track_len, sel.p);
    SFM_HIP(hipGetLastError());
    const PointFlag pf{sel.p};
    const ObsFlag of{v, sel.p, reg.p};
    Scan pts, obs;
    pts.sums(pf, d->n_pt, s);
    obs.sums(of, d->n_obs, s);
    int32_t n_pt = 0, n_obs = 0;
    pts.fetch(&n_pt, s);
    obs.fetch(&n_obs, s);
    SFM_HIP(hipStreamSynchronize(s));
    out.n_pt = n_pt;
    out.n_obs = n_obs;
    out.pt_offsets.assign((size_t)n_pt + 1, 0);
    out.pt_offsets[n_pt] = n_obs;
    if (!rows || n_pt == 0) return;
    DBuf<int32_t> pt_idx, pt_map, pt_off_new, obs_map, obs_img_new;
    DBuf<double> obs_uv_new;
    pt_idx.alloc((size_t)d->n_pt);
    pt_map.alloc((size_t)n_pt);
    pt_off_new.alloc((size_t)n_pt);
    obs_map.alloc((size_t)n_obs);
    obs_img_new.alloc((size_t)n_obs);
    obs_uv_new.alloc(2 * (size_t)n_obs);
    pts.apply(pf, PointEmit{pt_idx.p, pt_map.p}, s);
    obs.apply(of, ObsEmit{v, sel.p, pt_idx.p, d->obs_uv.p, pt_off_new.p, obs_map.p, obs_img_new.p, obs_uv_new.p}, s);
    std::vector<int32_t> off32, map32, omap32;
    download(off32, pt_off_new, (size_t)n_pt, s);
    download(map32, pt_map, (size_t)n_pt, s);
    download(omap32, obs_map, (size_t)n_obs, s);
    download(out.obs_img, obs_img_new, (size_t)n_obs, s);
    download(out.obs_uv, obs_uv_new, 2 * (size_t)n_obs, s);
    SFM_HIP(hipStreamSynchronize(s));
    out.pt_map.assign(map32.begin(), map32.end());
    out.obs_map.assign(omap32.begin(), omap32.end());
    for (int32_t k = 0; k < n_pt; ++k) out.pt_offsets[k] = off32[k];
}

}  // namespace sfm
