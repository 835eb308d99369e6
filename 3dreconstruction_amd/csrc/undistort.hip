// The undistortion on the device (gfx950): one launch per segment (the output
// rows [r0, r1) of one image), chunks streamed through two slots.
//
//   layout   device rows are pitched (undistort_pitch: whole groups of
//            kUndistortGroup pixels, padded to kUndistortPitchAlign bytes), the
//            caller's rows are not; 2-D copies between the two.
//   kernel   a workgroup is kUndistortTileH wavefronts, each on one output row;
//            a lane produces kUndistortGroup consecutive pixels of that row
//            (undistort_point.h, in double) and stores them as whole dwords:
//            one for a 1-channel image, three for a 3-channel one.  Pixels of
//            the last group past the image's width are stored as 0 into the
//            row's padding.  The source is read with plain global loads: the
//            footprint of a tile is a neighbourhood of the same size, and its
//            rows are shared between the lanes through L2.
//   counts   outside / low-weight pixels: per lane, summed over the wavefront
//            by shuffles, over the workgroup through LDS, then one 64-bit
//            atomic add per workgroup into the segment's word (outside in the
//            low half, low weight in the high half; a segment has fewer than
//            2^31 pixels).  Integer sums: the order does not matter.
//   chunks   slot c & 1 holds chunk c: pinned staging and device buffers for
//            input and output, and a stream.  The host stages chunk c's rows
//            into the slot's pinned input and enqueues upload, kernels and
//            download on the slot's stream; before a slot is reused its stream
//            is waited for and the finished rows go from the pinned output to
//            the caller's.  So chunk c + 1 uploads, and chunk c - 1 downloads,
//            while chunk c computes.
#pragma clang fp contract(off)

#include <algorithm>
#include <cstring>

#include "undistort.h"
#include "undistort_point.h"

namespace sfm {
namespace {

struct UndistortArgs {
    const uint8_t* src;           // source rows [s0, s0 + srows), pitched
    uint8_t* out;                 // output rows [r0, r1), pitched
    unsigned long long* count;    // the segment's counters
    double k[6];
    int64_t pitch;
    int32_t w, h, r0, r1, s0, srows, tiles_x;
    uint8_t fill[4];
};

template <int CH>
__global__ __launch_bounds__(64 * kUndistortTileH) void undistort_kernel(UndistortArgs a) {
    static_assert(kUndistortTileW == 64 * kUndistortGroup && kUndistortGroup == 4, "a lane stores CH dwords");
    __shared__ unsigned s_out[kUndistortTileH], s_low[kUndistortTileH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile_x = blockIdx.x % (unsigned)a.tiles_x, tile_y = blockIdx.x / (unsigned)a.tiles_x;
    const int64_t i0 = (tile_x * 64 + lane) * kUndistortGroup;
    const int64_t j = a.r0 + tile_y * kUndistortTileH + wave;
    unsigned n_out = 0, n_low = 0;
    if (i0 < a.w && j < a.r1) {
        uint8_t b[kUndistortGroup * CH];
#pragma unroll
        for (int p = 0; p < kUndistortGroup; ++p) {
            if (i0 + p < a.w) {
                const int st = undistort_pixel(a.k, a.w, a.h, CH, (int32_t)(i0 + p), (int32_t)j, a.src, a.pitch, a.s0,
                                               a.srows, a.fill, &b[p * CH]);
                n_out += st == kUndistortOutside;
                n_low += st == kUndistortLowWeight;
            } else {
#pragma unroll
                for (int c = 0; c < CH; ++c) b[p * CH + c] = 0;
            }
        }
        uint32_t* dst = reinterpret_cast<uint32_t*>(a.out + (j - a.r0) * a.pitch + i0 * CH);
#pragma unroll
        for (int q = 0; q < CH; ++q)
            dst[q] = (uint32_t)b[4 * q] | ((uint32_t)b[4 * q + 1] << 8) | ((uint32_t)b[4 * q + 2] << 16) |
                     ((uint32_t)b[4 * q + 3] << 24);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n_out += __shfl_down(n_out, o);
        n_low += __shfl_down(n_low, o);
    }
    if (lane == 0) {
        s_out[wave] = n_out;
        s_low[wave] = n_low;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long t_out = 0, t_low = 0;
    for (int w = 0; w < kUndistortTileH; ++w) {
        t_out += s_out[w];
        t_low += s_low[w];
    }
    if (t_out | t_low) atomicAdd(a.count, t_out | (t_low << 32));
}

// the second stream and the events of a call; waits for the stream before it goes
struct Streams {
    hipStream_t s[2] = {nullptr, nullptr};
    hipEvent_t ev[2][4] = {};
    ~Streams() {
        if (s[1]) {
            (void)hipStreamSynchronize(s[1]);
            (void)hipStreamDestroy(s[1]);
        }
        if (s[0]) (void)hipStreamSynchronize(s[0]);
        for (auto& slot : ev)
            for (hipEvent_t e : slot)
                if (e) (void)hipEventDestroy(e);
    }
};

struct Pinned {
    uint8_t* p = nullptr;
    ~Pinned() {
        if (p) pinned_free(p);
    }
    void alloc(size_t n) { p = static_cast<uint8_t*>(pinned_alloc(std::max<size_t>(n, 1))); }
};

// where the segments of a chunk lie in the slot's buffers
struct Layout {
    std::vector<int64_t> d_in, d_out, h_in, h_out;   // byte offsets per segment
    int64_t d_in_bytes = 0, d_out_bytes = 0, h_in_bytes = 0, h_out_bytes = 0;
};

Layout layout_of(const UndistortChunk& c, const int32_t* wh, const int32_t* channels) {
    Layout L;
    for (const UndistortSegment& g : c) {
        const int32_t w = wh[2 * g.img], ch = channels[g.img];
        const int64_t pitch = undistort_pitch(w, ch), row = (int64_t)w * ch;
        L.d_in.push_back(L.d_in_bytes);
        L.d_out.push_back(L.d_out_bytes);
        L.h_in.push_back(L.h_in_bytes);
        L.h_out.push_back(L.h_out_bytes);
        L.d_in_bytes += undistort_align_segment(pitch * (g.s1 - g.s0));
        L.d_out_bytes += undistort_align_segment(pitch * (g.r1 - g.r0));
        L.h_in_bytes += row * (g.s1 - g.s0);
        L.h_out_bytes += row * (g.r1 - g.r0);
    }
    return L;
}

}  // namespace

void undistort_device(sfm_ctx* ctx, const std::vector<UndistortChunk>& chunks, const int32_t* img_intr,
                      const double* intr, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                      const uint8_t* pixels, const uint8_t* fill, uint8_t* out, int64_t* n_outside,
                      int64_t* n_low_weight, double* seconds) {
    CtxScope scope_(ctx);
    std::vector<Layout> layouts;
    Layout cap;
    size_t cap_seg = 1;
    for (const UndistortChunk& c : chunks) {
        layouts.push_back(layout_of(c, wh, channels));
        const Layout& L = layouts.back();
        cap.d_in_bytes = std::max(cap.d_in_bytes, L.d_in_bytes);
        cap.d_out_bytes = std::max(cap.d_out_bytes, L.d_out_bytes);
        cap.h_in_bytes = std::max(cap.h_in_bytes, L.h_in_bytes);
        cap.h_out_bytes = std::max(cap.h_out_bytes, L.h_out_bytes);
        cap_seg = std::max(cap_seg, c.size());
    }
    const int n_slots = chunks.size() > 1 ? 2 : 1;
    // (declared before the streams: freed after the streams have been waited for)
    DBuf<uint8_t> d_in[2], d_out[2];
    DBuf<unsigned long long> d_cnt[2];
    Pinned h_in[2], h_out[2], h_cnt[2];
    Streams st;
    st.s[0] = ctx->stream;
    if (n_slots > 1) SFM_HIP(hipStreamCreateWithFlags(&st.s[1], hipStreamNonBlocking));
    for (int k = 0; k < n_slots; ++k) {
        d_in[k].alloc((size_t)std::max<int64_t>(cap.d_in_bytes, 1));
        d_out[k].alloc((size_t)std::max<int64_t>(cap.d_out_bytes, 1));
        d_cnt[k].alloc(cap_seg);
        h_in[k].alloc((size_t)cap.h_in_bytes);
        h_out[k].alloc((size_t)cap.h_out_bytes);
        h_cnt[k].alloc(cap_seg * sizeof(unsigned long long));
        for (hipEvent_t& e : st.ev[k]) SFM_HIP(hipEventCreate(&e));
    }
    // a poisoned or recycled block must not be in use by the context's stream any more
    SFM_HIP(hipStreamSynchronize(ctx->stream));

    int64_t held[2] = {-1, -1};   // the chunk in flight on each slot
    auto reap = [&](int k) {
        if (held[k] < 0) return;
        SFM_HIP(hipStreamSynchronize(st.s[k]));
        const UndistortChunk& c = chunks[(size_t)held[k]];
        const Layout& L = layouts[(size_t)held[k]];
        for (int p = 0; p < 3; ++p) {
            float ms = 0.f;
            SFM_HIP(hipEventElapsedTime(&ms, st.ev[k][p], st.ev[k][p + 1]));
            seconds[p] += ms * 1e-3;
        }
        const unsigned long long* cnt = reinterpret_cast<const unsigned long long*>(h_cnt[k].p);
        for (size_t g = 0; g < c.size(); ++g) {
            *n_outside += (int64_t)(cnt[g] & 0xFFFFFFFFull);
            *n_low_weight += (int64_t)(cnt[g] >> 32);
            const int64_t row = (int64_t)wh[2 * c[g].img] * channels[c[g].img];
            std::memcpy(out + img_off[c[g].img] + row * c[g].r0, h_out[k].p + L.h_out[g],
                        (size_t)(row * (c[g].r1 - c[g].r0)));
        }
        held[k] = -1;
    };

    for (size_t ci = 0; ci < chunks.size(); ++ci) {
        const int k = (int)(ci & 1) % n_slots;
        reap(k);
        const UndistortChunk& c = chunks[ci];
        const Layout& L = layouts[ci];
        hipStream_t s = st.s[k];
        for (size_t g = 0; g < c.size(); ++g) {
            const int64_t row = (int64_t)wh[2 * c[g].img] * channels[c[g].img];
            std::memcpy(h_in[k].p + L.h_in[g], pixels + img_off[c[g].img] + row * c[g].s0,
                        (size_t)(row * (c[g].s1 - c[g].s0)));
        }
        SFM_HIP(hipEventRecord(st.ev[k][0], s));
        SFM_HIP(hipMemsetAsync(d_cnt[k].p, 0, c.size() * sizeof(unsigned long long), s));
        for (size_t g = 0; g < c.size(); ++g) {
            const int32_t w = wh[2 * c[g].img], ch = channels[c[g].img], srows = c[g].s1 - c[g].s0;
            if (srows > 0)
                SFM_HIP(hipMemcpy2DAsync(d_in[k].p + L.d_in[g], (size_t)undistort_pitch(w, ch), h_in[k].p + L.h_in[g],
                                         (size_t)w * ch, (size_t)w * ch, (size_t)srows, hipMemcpyHostToDevice, s));
        }
        SFM_HIP(hipEventRecord(st.ev[k][1], s));
        for (size_t g = 0; g < c.size(); ++g) {
            const UndistortSegment& sg = c[g];
            const int32_t w = wh[2 * sg.img], h = wh[2 * sg.img + 1], ch = channels[sg.img];
            UndistortArgs a;
            a.src = d_in[k].p + L.d_in[g];
            a.out = d_out[k].p + L.d_out[g];
            a.count = d_cnt[k].p + g;
            std::memcpy(a.k, intr + 6 * (size_t)img_intr[sg.img], sizeof a.k);
            a.pitch = undistort_pitch(w, ch);
            a.w = w;
            a.h = h;
            a.r0 = sg.r0;
            a.r1 = sg.r1;
            a.s0 = sg.s0;
            a.srows = sg.s1 - sg.s0;
            a.tiles_x = (w + kUndistortTileW - 1) / kUndistortTileW;
            a.fill[0] = fill[0];
            a.fill[1] = fill[1];
            a.fill[2] = fill[2];
            a.fill[3] = 0;
            const int64_t tiles_y = ((int64_t)(sg.r1 - sg.r0) + kUndistortTileH - 1) / kUndistortTileH;
            const dim3 grid((unsigned)(a.tiles_x * tiles_y)), block(64 * kUndistortTileH);
            if (ch == 1)
                hipLaunchKernelGGL(undistort_kernel<1>, grid, block, 0, s, a);
            else
                hipLaunchKernelGGL(undistort_kernel<3>, grid, block, 0, s, a);
        }
        SFM_HIP(hipGetLastError());
        SFM_HIP(hipEventRecord(st.ev[k][2], s));
        for (size_t g = 0; g < c.size(); ++g) {
            const int32_t w = wh[2 * c[g].img], ch = channels[c[g].img];
            SFM_HIP(hipMemcpy2DAsync(h_out[k].p + L.h_out[g], (size_t)w * ch, d_out[k].p + L.d_out[g],
                                     (size_t)undistort_pitch(w, ch), (size_t)w * ch, (size_t)(c[g].r1 - c[g].r0),
                                     hipMemcpyDeviceToHost, s));
        }
        SFM_HIP(hipMemcpyAsync(h_cnt[k].p, d_cnt[k].p, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        SFM_HIP(hipEventRecord(st.ev[k][3], s));
        held[k] = (int64_t)ci;
    }
    // in chunk order (the counts are sums; the rows are disjoint)
    const int first = n_slots > 1 && held[1] >= 0 && held[1] < held[0] ? 1 : 0;
    reap(first);
    if (n_slots > 1) reap(1 - first);
}

}  // namespace sfm
