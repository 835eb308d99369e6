// Dense hand-off, undistortion, host side (include/sfmcore.h, "Dense
// hand-off"): the argument checks, the chunk plan, the host twin (threads over
// bands of rows), sfm_undistort over either, and the PNM writer.  The kernel
// and the chunked transfers are undistort.hip's.  SFM_UNDISTORT_HOST_ONLY
// leaves the device entry point out, so that the host twin builds with a plain
// host compiler (tests/cpp/undistort_test.cpp).
#pragma clang fp contract(off)

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "undistort.h"
#include "undistort_point.h"

using namespace sfm;

namespace {

// doubles per intrinsics block (sfm_ba_intr_width, which lives with the planner)
int intr_width(int32_t cm) { return cm == SFM_CAM_RADIAL3 ? 6 : (cm == SFM_CAM_PINHOLE || cm == SFM_CAM_SNAVELY ? 4 : 0); }

struct Images {
    int32_t camera_model, n_img, n_intr;
    const int32_t* img_intr;
    const double* intr;
    const int32_t* wh;
    const int32_t* channels;
    const int64_t* img_off;
    const uint8_t* pixels;
    bool loaded(int32_t i) const { return img_off[i] >= 0; }
    int64_t row_bytes(int32_t i) const { return (int64_t)wh[2 * i] * channels[i]; }
};

// every check; nothing has touched the device yet
void check(const char* who, const Images& m, const sfm_undistort_opts& o, const uint8_t* out) {
    const int iw = intr_width(m.camera_model);
    SFM_REQUIRE(iw > 0, SFM_ERR_INVALID_ARG, "%s: unknown camera_model %d", who, m.camera_model);
    SFM_REQUIRE(m.camera_model != SFM_CAM_SNAVELY, SFM_ERR_UNSUPPORTED,
                "%s: SFM_CAM_SNAVELY has no principal point, so no raster to resample", who);
    SFM_REQUIRE(m.n_img >= 0 && m.n_intr >= 0 && o.chunk_bytes >= 0, SFM_ERR_INVALID_ARG, "%s: negative count", who);
    SFM_REQUIRE(m.n_img == 0 || (m.img_intr && m.wh && m.channels && m.img_off), SFM_ERR_INVALID_ARG,
                "%s: null argument", who);
    SFM_REQUIRE(m.n_intr == 0 || m.intr, SFM_ERR_INVALID_ARG, "%s: null intr", who);
    for (int32_t i = 0; i < m.n_img; ++i) {
        const int32_t w = m.wh[2 * i], h = m.wh[2 * i + 1], b = m.img_intr[i];
        SFM_REQUIRE(w > 0 && h > 0, SFM_ERR_INVALID_ARG, "%s: image %d has a non-positive size", who, i);
        SFM_REQUIRE(b >= 0 && b < m.n_intr, SFM_ERR_INVALID_ARG, "%s: image %d names intrinsics block %d of %d", who, i,
                    b, m.n_intr);
        if (!m.loaded(i)) continue;
        SFM_REQUIRE(m.pixels && out, SFM_ERR_INVALID_ARG, "%s: null pixels", who);
        SFM_REQUIRE(m.channels[i] == 1 || m.channels[i] == 3, SFM_ERR_INVALID_ARG, "%s: image %d has %d channels", who,
                    i, m.channels[i]);
        SFM_REQUIRE((int64_t)w * h < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED, "%s: image %d has 2^31 or more pixels",
                    who, i);
        const double* k = m.intr + (size_t)iw * b;
        for (int a = 0; a < iw; ++a)
            SFM_REQUIRE(std::isfinite(k[a]), SFM_ERR_INVALID_ARG, "%s: intrinsics block %d is not finite", who, b);
        SFM_REQUIRE(m.camera_model != SFM_CAM_RADIAL3 || k[0] != 0.0, SFM_ERR_INVALID_ARG,
                    "%s: intrinsics block %d has f == 0", who, b);
    }
}

// The chunks of a RADIAL3 call.  Whole images are packed in index order while
// their pitched rows (input and output) fit the budget; an image that does not
// fit an empty chunk is cut into bands of output rows, a chunk each, every band
// with the source rows it samples, found by walking its pixels through
// undistort_source (the kernel's own arithmetic).
std::vector<UndistortChunk> plan_chunks(const char* who, const Images& m, int64_t budget) {
    std::vector<UndistortChunk> chunks;
    UndistortChunk cur;
    int64_t used = 0;
    auto flush = [&] {
        if (!cur.empty()) chunks.push_back(cur);
        cur.clear();
        used = 0;
    };
    for (int32_t i = 0; i < m.n_img; ++i) {
        if (!m.loaded(i)) continue;
        const int32_t w = m.wh[2 * i], h = m.wh[2 * i + 1];
        const int64_t pitch = undistort_pitch(w, m.channels[i]);
        const int64_t whole = 2 * undistort_align_segment(pitch * h);
        if (whole <= budget) {
            if (used + whole > budget) flush();
            cur.push_back(UndistortSegment{i, 0, h, 0, h});
            used += whole;
            continue;
        }
        flush();
        const double* k = m.intr + 6 * (size_t)m.img_intr[i];
        std::vector<int32_t> lo((size_t)h), hi((size_t)h);   // the source rows [lo, hi) of each output row
        for (int32_t j = 0; j < h; ++j) {
            int64_t a = h, b = 0;
            for (int32_t x = 0; x < w; ++x) {
                double sx, sy;
                if (!undistort_source(k, w, h, x, j, &sx, &sy)) continue;
                int64_t l, u;
                undistort_source_rows(sy, h, &l, &u);
                if (u > l) {
                    a = std::min(a, l);
                    b = std::max(b, u);
                }
            }
            lo[j] = (int32_t)(b > a ? a : 0);
            hi[j] = (int32_t)(b > a ? b : 0);
        }
        auto bytes = [&](int32_t rows, int32_t srows) {
            return undistort_align_segment(pitch * rows) + undistort_align_segment(pitch * srows);
        };
        for (int32_t r0 = 0; r0 < h;) {
            int32_t r1 = r0, s0 = 0, s1 = 0;
            while (r1 < h) {
                int32_t t0 = s0, t1 = s1;
                if (hi[r1] > lo[r1]) {
                    t0 = s1 > s0 ? std::min(s0, lo[r1]) : lo[r1];
                    t1 = s1 > s0 ? std::max(s1, hi[r1]) : hi[r1];
                }
                if (bytes(r1 + 1 - r0, t1 - t0) > budget) break;
                s0 = t0;
                s1 = t1;
                ++r1;
            }
            SFM_REQUIRE(r1 > r0, SFM_ERR_INVALID_ARG,
                        "%s: chunk_bytes %lld is too small for row %d of image %d and the source rows it samples", who,
                        (long long)budget, r0, i);
            chunks.push_back(UndistortChunk{UndistortSegment{i, r0, r1, s0, s1}});
            r0 = r1;
        }
    }
    flush();
    return chunks;
}

// The host twin: the loaded images cut into bands of rows, handed to up to 16
// threads; a pixel's bytes depend on nothing but the source, so neither the
// bytes nor the (summed) counts depend on the schedule.
void host_resample(const Images& m, const uint8_t* fill, uint8_t* out, int64_t* n_outside, int64_t* n_low) {
    constexpr int32_t kBand = 16;
    struct Item {
        int32_t img, r0, r1;
    };
    std::vector<Item> items;
    for (int32_t i = 0; i < m.n_img; ++i) {
        if (!m.loaded(i)) continue;
        for (int32_t r = 0; r < m.wh[2 * i + 1]; r += kBand)
            items.push_back(Item{i, r, std::min(r + kBand, m.wh[2 * i + 1])});
    }
    std::atomic<size_t> next{0};
    std::atomic<int64_t> outside{0}, low{0};
    auto work = [&] {
        int64_t c_out = 0, c_low = 0;
        for (size_t at; (at = next.fetch_add(1)) < items.size();) {
            const Item& it = items[at];
            const int32_t w = m.wh[2 * it.img], h = m.wh[2 * it.img + 1], ch = m.channels[it.img];
            const double* k = m.intr + 6 * (size_t)m.img_intr[it.img];
            const uint8_t* src = m.pixels + m.img_off[it.img];
            uint8_t* dst = out + m.img_off[it.img];
            for (int32_t j = it.r0; j < it.r1; ++j)
                for (int32_t i = 0; i < w; ++i) {
                    const int st = undistort_pixel(k, w, h, ch, i, j, src, (int64_t)w * ch, 0, h, fill,
                                                   dst + ((int64_t)j * w + i) * ch);
                    c_out += st == kUndistortOutside;
                    c_low += st == kUndistortLowWeight;
                }
        }
        outside += c_out;
        low += c_low;
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_threads = std::min<size_t>(std::min<size_t>(16, hw ? hw : 1), items.size());
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    *n_outside = outside;
    *n_low = low;
}

int undistort(const char* who, sfm_ctx* ctx, bool device, int32_t camera_model, int32_t n_img, int32_t n_intr,
              const int32_t* img_intr, const double* intr, const int32_t* wh, const int32_t* channels,
              const int64_t* img_off, const uint8_t* pixels, const sfm_undistort_opts* opts, uint8_t* out,
              sfm_undistort_stats* stats) {
    SFM_REQUIRE(!device || ctx, SFM_ERR_INVALID_ARG, "%s: null context", who);
    sfm_undistort_opts o;
    sfm_undistort_default_options(&o);
    if (opts) o = *opts;
    const Images m{camera_model, n_img, n_intr, img_intr, intr, wh, channels, img_off, pixels};
    check(who, m, o, out);
    sfm_undistort_stats st;
    std::memset(&st, 0, sizeof st);
    for (int32_t i = 0; i < n_img; ++i) st.n_images += m.loaded(i);
    if (camera_model == SFM_CAM_PINHOLE) {
        for (int32_t i = 0; i < n_img; ++i)
            if (m.loaded(i)) std::memcpy(out + img_off[i], pixels + img_off[i], (size_t)(m.row_bytes(i) * wh[2 * i + 1]));
        st.n_copied = st.n_images;
    } else if (st.n_images > 0) {
        const std::vector<UndistortChunk> chunks =
            plan_chunks(who, m, o.chunk_bytes > 0 ? o.chunk_bytes : kUndistortDefaultChunk);
        st.n_chunks = (int32_t)chunks.size();
        for (int32_t i = 0; i < n_img; ++i)
            if (m.loaded(i)) st.n_pixels += (int64_t)wh[2 * i] * wh[2 * i + 1];
        if (device) {
#ifndef SFM_UNDISTORT_HOST_ONLY
            undistort_device(ctx, chunks, img_intr, intr, wh, channels, img_off, pixels, o.fill, out, &st.n_outside,
                             &st.n_low_weight, st.seconds);
#endif
        } else {
            const double t0 = seconds_now();
            host_resample(m, o.fill, out, &st.n_outside, &st.n_low_weight);
            st.seconds[1] = seconds_now() - t0;
        }
    }
    if (stats) *stats = st;
    return SFM_OK;
}

}  // namespace

extern "C" void sfm_undistort_default_options(sfm_undistort_opts* opts) {
    if (opts) std::memset(opts, 0, sizeof *opts);
}

extern "C" int sfm_undistort_host(int32_t camera_model, int32_t n_img, int32_t n_intr, const int32_t* img_intr,
                                  const double* intr, const int32_t* wh, const int32_t* channels,
                                  const int64_t* img_off, const uint8_t* pixels, const sfm_undistort_opts* opts,
                                  uint8_t* out, sfm_undistort_stats* stats) {
    return guarded([&] {
        return undistort("sfm_undistort_host", nullptr, false, camera_model, n_img, n_intr, img_intr, intr, wh, channels,
                         img_off, pixels, opts, out, stats);
    });
}

extern "C" int sfm_undistort_write_pnm(const char* path, int32_t w, int32_t h, int32_t channels, const uint8_t* bytes) {
    return guarded([&] {
        const char* who = "sfm_undistort_write_pnm";
        SFM_REQUIRE(path && bytes && w > 0 && h > 0 && (channels == 1 || channels == 3), SFM_ERR_INVALID_ARG,
                    "%s: null argument, a non-positive size or %d channels", who, channels);
        std::FILE* f = std::fopen(path, "wb");
        SFM_REQUIRE(f, SFM_ERR_INVALID_ARG, "%s: cannot write %s", who, path);
        std::fprintf(f, "P%d\n%d %d\n255\n", channels == 1 ? 5 : 6, w, h);
        const size_t n = (size_t)w * h * channels;
        const bool wrote = std::fwrite(bytes, 1, n, f) == n;
        const bool good = (std::fclose(f) == 0) && wrote;
        SFM_REQUIRE(good, SFM_ERR_INVALID_ARG, "%s: writing %s failed", who, path);
        return SFM_OK;
    });
}

#ifndef SFM_UNDISTORT_HOST_ONLY
extern "C" int sfm_undistort(sfm_ctx* ctx, int32_t camera_model, int32_t n_img, int32_t n_intr,
                             const int32_t* img_intr, const double* intr, const int32_t* wh, const int32_t* channels,
                             const int64_t* img_off, const uint8_t* pixels, const sfm_undistort_opts* opts,
                             uint8_t* out, sfm_undistort_stats* stats) {
    return guarded([&] {
        return undistort("sfm_undistort", ctx, true, camera_model, n_img, n_intr, img_intr, intr, wh, channels, img_off,
                         pixels, opts, out, stats);
    });
}
#endif
