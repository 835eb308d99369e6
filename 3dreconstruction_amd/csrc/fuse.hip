// The depth-map fusion on the device (gfx950): the maps, the masks and the
// colour bytes of a call resident, three kernels, no atomics in the placement,
// so the cloud's order (image, y, x) does not depend on the schedule.
//
//   mark   grid y is the image; a workgroup of kFuseBlock = 256 lanes owns 256
//          consecutive pixels of the image's raster, so lane order is cloud
//          order.  A lane works out its pixel's agreement mask and fate
//          (fuse_point.h) and stores them (4 B + 1 B per pixel); the
//          workgroup's emitted count comes from the wavefronts' ballots
//          (wave64: 64 bits) and goes to block_count[image's first block +
//          block]; the suppressed pixels are summed the same way and added
//          with one integer atomic per workgroup (a count: order-free).
//   scan   dense_scan.h's kernel over one array: the exclusive int64 prefix
//          of block_count in (image, block) order; the total is read back
//          once, to check cap_points and to size the download.
//   emit   the same grid: a lane's rank is its block's base + the emitted
//          counts of the wavefronts before it (LDS) + the popcount of its
//          wavefront's ballot below it.  Emitting lanes gather their
//          contributors by walking the mask's set bits, average and store
//          with plain vector stores.
// sfm_densify runs depthmap.hip's passes and filter and these kernels over the
// same device buffers.
#pragma clang fp contract(off)

#include <algorithm>

#include "dense_scan.h"
#include "fuse.h"

namespace sfm {
namespace {

static_assert(kFuseBlock == kDenseBlock, "dense_scan.h's workgroup: four wavefronts of 64 lanes");

struct FuseLaunch {
    const FuseView* views;
    const FusePair* pairs;
    const float *depth, *normal;
    const uint8_t* pixels;
    uint32_t* mask;
    uint8_t* fate;
    int32_t* block_count;
    const int64_t* block_base;
    unsigned long long* n_suppressed;
    FuseParams prm;
    float *X, *N;
    uint8_t *rgb, *n_views;
    uint32_t* view_mask;
    int32_t *src_image, *src_pixel;
};

__global__ __launch_bounds__(kFuseBlock) void fuse_mark_kernel(FuseLaunch a) {
    __shared__ int32_t emitted[4], suppressed[4];
    const int32_t i = (int32_t)blockIdx.y;
    const FuseView& V = a.views[i];
    const int64_t n = (int64_t)V.w * V.h, at = (int64_t)blockIdx.x * kFuseBlock + threadIdx.x;
    if ((int64_t)blockIdx.x * kFuseBlock >= n) return;   // the whole workgroup
    int32_t fate = kFuseNone;
    if (at < n) {
        uint32_t mask;
        fate = fuse_pixel_fate(a.views, a.pairs, a.prm, i, (int32_t)(at % V.w), (int32_t)(at / V.w), a.depth, a.normal,
                               &mask);
        a.mask[V.map_off + at] = mask;
        a.fate[V.map_off + at] = (uint8_t)fate;
    }
    int32_t n_emitted, n_suppressed;
    block_ballot_rank(fate == kFuseEmitted, emitted, &n_emitted);
    block_ballot_rank(fate == kFuseSuppressed, suppressed, &n_suppressed);
    if (threadIdx.x == 0) {
        a.block_count[V.blk_off + blockIdx.x] = n_emitted;
        if (n_suppressed) atomicAdd(a.n_suppressed, (unsigned long long)n_suppressed);
    }
}

__global__ __launch_bounds__(kFuseBlock) void fuse_emit_kernel(FuseLaunch a) {
    __shared__ int32_t emitted[4];
    const int32_t i = (int32_t)blockIdx.y;
    const FuseView& V = a.views[i];
    const int64_t n = (int64_t)V.w * V.h, at = (int64_t)blockIdx.x * kFuseBlock + threadIdx.x;
    if ((int64_t)blockIdx.x * kFuseBlock >= n) return;   // the whole workgroup
    const bool emit = at < n && a.fate[V.map_off + at] == kFuseEmitted;
    int32_t n_emitted;
    const int32_t before = block_ballot_rank(emit, emitted, &n_emitted);
    if (!emit) return;
    const int64_t rank = a.block_base[V.blk_off + blockIdx.x] + before;
    const int32_t px = (int32_t)(at % V.w), py = (int32_t)(at / V.w);
    const uint32_t mask = a.mask[V.map_off + at];
    float X[3], N[3];
    uint8_t rgb[3] = {0, 0, 0};
    const int32_t m = fuse_pixel_point(a.views, a.pairs, a.prm, i, px, py, mask, a.depth, a.normal, a.pixels, X, N, rgb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        a.X[3 * rank + c] = X[c];
        if (a.N) a.N[3 * rank + c] = N[c];
        if (a.rgb) a.rgb[3 * rank + c] = rgb[c];
    }
    if (a.n_views) a.n_views[rank] = (uint8_t)m;
    if (a.view_mask) a.view_mask[rank] = mask;
    if (a.src_image) a.src_image[rank] = i;
    if (a.src_pixel) a.src_pixel[rank] = (int32_t)at;
}

// The device side of a fusion whose maps are resident.
struct FuseResident {
    DBuf<FuseView> views;
    DBuf<FusePair> pairs;
    DBuf<uint8_t> pool, fate;
    DBuf<uint32_t> mask;
    DBuf<int32_t> block_count;
    DBuf<int64_t> block_base;
    DBuf<unsigned long long> n_suppressed;
    // the cloud
    DBuf<float> X, N;
    DBuf<uint8_t> rgb, n_views;
    DBuf<uint32_t> view_mask;
    DBuf<int32_t> src_image, src_pixel;
    FuseLaunch a;
};

void fuse_upload(hipStream_t s, const FuseProblem& F, const uint8_t* pixels, FuseResident& r) {
    r.views.alloc(F.views.size());
    r.pairs.alloc(std::max<size_t>(F.pairs.size(), 1));
    r.pool.alloc((size_t)std::max<int64_t>(F.images.pool_hi - F.images.pool_lo, 1));
    r.mask.alloc((size_t)F.images.n_map);
    r.fate.alloc((size_t)F.images.n_map);
    r.block_count.alloc((size_t)F.n_blocks);
    r.block_base.alloc((size_t)F.n_blocks + 1);
    r.n_suppressed.alloc(1);
    r.views.upload(F.views.data(), F.views.size(), s);
    r.pairs.upload(F.pairs.data(), F.pairs.size(), s);
    if (pixels) r.pool.upload(pixels + F.images.pool_lo, (size_t)(F.images.pool_hi - F.images.pool_lo), s);
    r.n_suppressed.zero(s);
}

// mark and scan; the counts are read back (the stream is synchronised)
void fuse_mark(hipStream_t s, const FuseProblem& F, const float* d_depth, const float* d_normal, FuseResident& r,
               int64_t* n_points, int64_t* n_suppressed) {
    FuseLaunch& a = r.a;
    a = FuseLaunch{};
    a.views = r.views.p;
    a.pairs = r.pairs.p;
    a.depth = d_depth;
    a.normal = d_normal;
    a.pixels = r.pool.p;
    a.mask = r.mask.p;
    a.fate = r.fate.p;
    a.block_count = r.block_count.p;
    a.block_base = r.block_base.p;
    a.n_suppressed = r.n_suppressed.p;
    a.prm = F.prm;
    hipLaunchKernelGGL(fuse_mark_kernel, dim3((unsigned)F.max_blocks, (unsigned)F.images.n_img), dim3(kFuseBlock), 0, s, a);
    hipLaunchKernelGGL(dense_scan_kernel, dim3(1), dim3(kDenseBlock), 0, s, r.block_count.p, F.n_blocks, r.block_base.p);
    SFM_HIP(hipGetLastError());
    int64_t total = 0;
    unsigned long long supp = 0;
    SFM_HIP(hipMemcpyAsync(&total, r.block_base.p + F.n_blocks, sizeof total, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(&supp, r.n_suppressed.p, sizeof supp, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    *n_points = total;
    *n_suppressed = (int64_t)supp;
}

void fuse_emit(hipStream_t s, const FuseProblem& F, const FuseOut& out, int64_t n_points, FuseResident& r) {
    if (n_points == 0) return;
    const size_t n = (size_t)n_points;
    FuseLaunch& a = r.a;
    r.X.alloc(3 * n);
    a.X = r.X.p;
    if (out.N) r.N.alloc(3 * n), a.N = r.N.p;
    if (out.rgb && F.prm.use_color) r.rgb.alloc(3 * n), a.rgb = r.rgb.p;
    if (out.n_views) r.n_views.alloc(n), a.n_views = r.n_views.p;
    if (out.view_mask) r.view_mask.alloc(n), a.view_mask = r.view_mask.p;
    if (out.src_image) r.src_image.alloc(n), a.src_image = r.src_image.p;
    if (out.src_pixel) r.src_pixel.alloc(n), a.src_pixel = r.src_pixel.p;
    hipLaunchKernelGGL(fuse_emit_kernel, dim3((unsigned)F.max_blocks, (unsigned)F.images.n_img), dim3(kFuseBlock), 0, s, a);
    SFM_HIP(hipGetLastError());
}

void fuse_download(hipStream_t s, const FuseOut& out, int64_t n_points, const FuseResident& r) {
    if (n_points == 0) return;
    const size_t n = (size_t)n_points;
    SFM_HIP(hipMemcpyAsync(out.X, r.X.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (r.N.p) SFM_HIP(hipMemcpyAsync(out.N, r.N.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (r.rgb.p) SFM_HIP(hipMemcpyAsync(out.rgb, r.rgb.p, 3 * n, hipMemcpyDeviceToHost, s));
    if (r.n_views.p) SFM_HIP(hipMemcpyAsync(out.n_views, r.n_views.p, n, hipMemcpyDeviceToHost, s));
    if (r.view_mask.p) SFM_HIP(hipMemcpyAsync(out.view_mask, r.view_mask.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (r.src_image.p) SFM_HIP(hipMemcpyAsync(out.src_image, r.src_image.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (r.src_pixel.p) SFM_HIP(hipMemcpyAsync(out.src_pixel, r.src_pixel.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
}

void require_cap(const char* who, int64_t n_points, const FuseOut& out) {
    SFM_REQUIRE(n_points <= out.cap_points, SFM_ERR_INVALID_ARG, "%s: the cloud has %lld points, cap_points is %lld", who,
                (long long)n_points, (long long)out.cap_points);
}

}  // namespace

void fuse_device(sfm_ctx* ctx, const FuseProblem& F, const float* depth, const float* normal, const uint8_t* pixels,
                 const FuseOut& out, int64_t* n_points, int64_t* n_suppressed, double* seconds) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    const size_t n_map = (size_t)F.images.n_map;
    FuseResident r;
    DBuf<float> d_depth, d_normal;
    StreamEvents<6> ev;
    ev.record(0, s);
    d_depth.alloc(n_map);
    d_normal.alloc(3 * n_map);
    d_depth.upload(depth, n_map, s);
    d_normal.upload(normal, 3 * n_map, s);
    fuse_upload(s, F, pixels, r);
    ev.record(1, s);
    ev.record(2, s);
    fuse_mark(s, F, d_depth.p, d_normal.p, r, n_points, n_suppressed);
    require_cap("sfm_depthmap_fuse", *n_points, out);
    ev.record(3, s);
    fuse_emit(s, F, out, *n_points, r);
    ev.record(4, s);
    fuse_download(s, out, *n_points, r);
    ev.record(5, s);
    SFM_HIP(hipStreamSynchronize(s));
    seconds[0] = ev.between(0, 1);
    seconds[1] = ev.between(2, 3) + ev.between(3, 4);
    seconds[2] = ev.between(4, 5);
}

void densify_device(sfm_ctx* ctx, const DepthCall& call, bool init_given, const float* init_depth,
                    const float* init_normal, const DepthFilterParams& fprm, const FuseProblem& F, const uint8_t* pixels,
                    const FuseOut& out, const DensifyMaps& maps, sfm_densify_stats* st) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    const DepthProblem& P = call.P;
    const size_t n_map = (size_t)P.n_map;
    // the initial planes as sfm_depthmap uploads them: zero where an image gets no maps
    std::vector<float> h_depth, h_normal;
    if (init_given) {
        h_depth.assign(n_map, 0.0f);
        h_normal.assign(3 * n_map, 0.0f);
        depth_init_maps(P, init_depth, init_normal, h_depth.data(), h_normal.data(), nullptr);
    }
    DepthResident d;
    FuseResident r;
    StreamEvents<4> ev;
    ev.record(0, s);
    depth_estimate_upload(s, P, init_given, h_depth.data(), h_normal.data(), d);
    fuse_upload(s, F, pixels, r);
    ev.record(1, s);
    if (call.st.n_images > 0) depth_estimate_launch(s, P, call.prm, init_given, d);
    depth_filter_launch(s, P, fprm, d);
    fuse_mark(s, F, d.filtered.p, d.normal.p, r, &st->fuse.n_points, &st->fuse.n_suppressed);
    require_cap("sfm_densify", st->fuse.n_points, out);
    fuse_emit(s, F, out, st->fuse.n_points, r);
    ev.record(2, s);
    fuse_download(s, out, st->fuse.n_points, r);
    unsigned long long at_worst = 0;
    std::vector<unsigned long long> cnt((size_t)2 * P.n_img, 0);
    SFM_HIP(hipMemcpyAsync(&at_worst, d.count.p, sizeof at_worst, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(cnt.data(), d.fcounts.p, cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (maps.depth) SFM_HIP(hipMemcpyAsync(maps.depth, d.depth.p, n_map * sizeof(float), hipMemcpyDeviceToHost, s));
    if (maps.normal) SFM_HIP(hipMemcpyAsync(maps.normal, d.normal.p, 3 * n_map * sizeof(float), hipMemcpyDeviceToHost, s));
    if (maps.cost) SFM_HIP(hipMemcpyAsync(maps.cost, d.cost.p, n_map * sizeof(float), hipMemcpyDeviceToHost, s));
    if (maps.depth_filtered)
        SFM_HIP(hipMemcpyAsync(maps.depth_filtered, d.filtered.p, n_map * sizeof(float), hipMemcpyDeviceToHost, s));
    if (maps.n_agree) SFM_HIP(hipMemcpyAsync(maps.n_agree, d.agree.p, n_map, hipMemcpyDeviceToHost, s));
    ev.record(3, s);
    SFM_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < 3; ++p) st->seconds[p] = ev.between(p, p + 1);
    if (call.st.n_images > 0)
        depth_estimate_counts(P, call.prm, at_worst, &st->depthmap.n_estimated, &st->depthmap.n_invalid);
    for (int32_t i = 0; i < P.n_img; ++i) {
        st->filter.n_candidates += (int64_t)cnt[(size_t)2 * i];
        st->filter.n_kept += (int64_t)cnt[(size_t)2 * i + 1];
        if (maps.counts) {
            maps.counts[2 * i] = (int64_t)cnt[(size_t)2 * i];
            maps.counts[2 * i + 1] = (int64_t)cnt[(size_t)2 * i + 1];
        }
    }
}

}  // namespace sfm
