// The host preparation that the dense stages share (dense_views.h).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <thread>

#include "dense_views.h"

namespace sfm {

void dense_parallel_for(size_t n, const std::function<void(size_t)>& fn) {
    std::atomic<size_t> next{0};
    auto work = [&] {
        for (size_t at; (at = next.fetch_add(1)) < n;) fn(at);
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_threads = std::min<size_t>(std::min<size_t>(16, hw ? hw : 1), n);
    std::vector<std::thread> pool;
    for (size_t t = 1; t < n_threads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
}

void dense_KR(const double* K, const double* R, int32_t i, float* M) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const double* k = K + 9 * i + 3 * r;
            const double* rr = R + 9 * i + c;
            M[3 * r + c] = (float)(k[0] * rr[0] + k[1] * rr[3] + k[2] * rr[6]);
        }
}

void dense_C(const double* C, int32_t i, float* c) {
    for (int a = 0; a < 3; ++a) c[a] = (float)C[3 * i + a];
}

void dense_images_prepare(const char* who, int32_t n_img, const int32_t* wh, const int32_t* channels,
                          const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R, const double* C,
                          DenseImages& D, const std::function<void(int32_t)>& also) {
    D = DenseImages{};
    D.n_img = n_img;
    D.img.resize((size_t)std::max(n_img, 0));
    bool any = false;
    for (int32_t i = 0; i < n_img; ++i) {
        const int32_t w = wh[2 * i], h = wh[2 * i + 1];
        SFM_REQUIRE(w > 0 && h > 0, SFM_ERR_INVALID_ARG, "%s: image %d has a non-positive size", who, i);
        SFM_REQUIRE((int64_t)w * h < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED, "%s: image %d has 2^31 or more pixels", who, i);
        for (int a = 0; a < 9; ++a)
            SFM_REQUIRE(std::isfinite(K[9 * i + a]) && std::isfinite(R[9 * i + a]) && std::isfinite(C[3 * i + a % 3]),
                        SFM_ERR_INVALID_ARG, "%s: the camera of image %d is not finite", who, i);
        DenseImage& I = D.img[(size_t)i];
        const int64_t n = (int64_t)w * h;
        I = DenseImage{w, h, !pixels || img_off[i] >= 0, 0, D.n_map, 0};
        D.n_map += n;
        if (pixels && I.loaded) {
            SFM_REQUIRE(channels[i] == 1 || channels[i] == 3, SFM_ERR_INVALID_ARG, "%s: image %d has %d channels", who, i,
                        channels[i]);
            I.channels = channels[i];
            const int64_t lo = img_off[i], hi = img_off[i] + n * channels[i];
            D.pool_lo = any ? std::min(D.pool_lo, lo) : lo;
            D.pool_hi = any ? std::max(D.pool_hi, hi) : hi;
            any = true;
        }
        if (also) also(i);
    }
    for (int32_t i = 0; i < n_img; ++i)
        if (D.img[(size_t)i].channels) D.img[(size_t)i].pix_off = img_off[i] - D.pool_lo;
}

}  // namespace sfm
