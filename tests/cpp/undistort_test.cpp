// sfm_undistort_host, sfm_undistort_write_pnm, sfm_dense_scene_* and the façade
// of include/sfm/dense.hpp on the host backend, on small inputs whose results
// are known without a second implementation: zero distortion is the identity,
// PINHOLE is a byte copy, the result does not depend on the chunk budget, and a
// three-image scene worked out by hand.
//
// A stand-alone host program: the host paths of csrc/undistort.cpp and
// csrc/dense_scene.cpp are compiled in (no library, no HIP runtime), so it can
// be built with host sanitizers and run anywhere.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../3dreconstruction_amd/csrc/common.h"
#include "../../3dreconstruction_amd/include/sfm/dense.hpp"
namespace sfm {
static char g_err[512];
void set_error(const char* fmt, ...) {
    va_list a;
    va_start(a, fmt);
    std::vsnprintf(g_err, sizeof g_err, fmt, a);
    va_end(a);
}
}  // namespace sfm
extern "C" const char* sfm_last_error(void) { return sfm::g_err; }

using namespace sfm;

static int fails = 0;
#define EXPECT(c)                                                         \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c);     \
            ++fails;                                                      \
        }                                                                 \
    } while (0)

int main() {
    // three images at odd offsets: 67 x 41 rgb, 30 x 50 gray (not loaded), 64 x 48 gray; sentinels around them
    const int32_t wh[6] = {67, 41, 30, 50, 64, 48}, channels[3] = {3, 1, 1}, img_intr[3] = {0, 1, 1};
    const int64_t img_off[3] = {3, -1, 3 + 67 * 41 * 3 + 5};
    const size_t total = (size_t)img_off[2] + 64 * 48 + 7;
    std::vector<uint8_t> pool(total, 0xA5), out(total, 0x5A), again(total, 0x5A);
    uint32_t s = 12345;
    for (int i : {0, 2})
        for (int64_t b = 0; b < (int64_t)wh[2 * i] * wh[2 * i + 1] * channels[i]; ++b) {
            s = s * 1664525u + 1013904223u;
            pool[(size_t)(img_off[i] + b)] = (uint8_t)(s >> 24);
        }
    const double strong[12] = {60.0, 33.5, 20.5, 0.8, 0.0, 0.0, 70.0, 31.5, 23.5, 0.3, -0.2, 0.1};
    sfm_undistort_opts o;
    sfm_undistort_default_options(&o);
    EXPECT(o.chunk_bytes == 0 && o.fill[0] == 0 && o.fill[2] == 0);
    o.fill[0] = 200; o.fill[1] = 17; o.fill[2] = 96;
    sfm_undistort_stats st, st2;
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 3, 2, img_intr, strong, wh, channels, img_off, pool.data(), &o, out.data(),
                              &st) == SFM_OK);
    EXPECT(st.n_images == 2 && st.n_copied == 0 && st.n_pixels == 67 * 41 + 64 * 48 && st.n_chunks == 1);
    EXPECT(st.n_outside > 0 && st.n_low_weight > 0);
    EXPECT(out[0] == 0x5A && out[2] == 0x5A && out[(size_t)img_off[2] - 1] == 0x5A && out[total - 1] == 0x5A);
    EXPECT(out[3] == 200 && out[4] == 17 && out[5] == 96);   // pixel (0, 0) of image 0 maps outside
    // the same bytes and counts whatever the budget: bands of rows
    o.chunk_bytes = 4000;
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 3, 2, img_intr, strong, wh, channels, img_off, pool.data(), &o,
                              again.data(), &st2) == SFM_OK);
    EXPECT(again == out && st2.n_chunks > 2 && st2.n_outside == st.n_outside && st2.n_low_weight == st.n_low_weight);
    o.chunk_bytes = 64;
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 3, 2, img_intr, strong, wh, channels, img_off, pool.data(), &o,
                              again.data(), &st2) == SFM_ERR_INVALID_ARG);
    // black fill (the defaults): what exportUndistorted() below writes
    std::vector<uint8_t> black(total, 0x5A);
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 3, 2, img_intr, strong, wh, channels, img_off, pool.data(), nullptr,
                              black.data(), &st2) == SFM_OK);
    EXPECT(black != out && black[3] == 0 && st2.n_outside == st.n_outside);
    // zero distortion: the identity
    const double zero[12] = {61.37, 30.123, 22.987, 0.0, 0.0, 0.0, 55.5, 31.9, 24.2, 0.0, 0.0, 0.0};
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 3, 2, img_intr, zero, wh, channels, img_off, pool.data(), nullptr,
                              again.data(), &st2) == SFM_OK);
    for (int i : {0, 2})
        EXPECT(std::memcmp(&again[(size_t)img_off[i]], &pool[(size_t)img_off[i]],
                           (size_t)wh[2 * i] * wh[2 * i + 1] * channels[i]) == 0);
    EXPECT(st2.n_outside == 0 && st2.n_low_weight == 0);
    // PINHOLE: a copy; SNAVELY: unsupported; the checks
    const double pin[8] = {50, 50, 30, 20, 40, 40, 30, 20};
    std::fill(again.begin(), again.end(), 0x5A);
    EXPECT(sfm_undistort_host(SFM_CAM_PINHOLE, 3, 2, img_intr, pin, wh, channels, img_off, pool.data(), nullptr,
                              again.data(), &st2) == SFM_OK);
    EXPECT(st2.n_copied == 2 && st2.n_chunks == 0 && again[0] == 0x5A &&
           std::memcmp(&again[3], &pool[3], 67 * 41 * 3) == 0);
    EXPECT(sfm_undistort_host(SFM_CAM_SNAVELY, 3, 2, img_intr, pin, wh, channels, img_off, pool.data(), nullptr,
                              again.data(), &st2) == SFM_ERR_UNSUPPORTED);
    const int32_t bad_ch[3] = {2, 1, 1}, bad_ii[3] = {0, 1, 2};
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 3, 2, img_intr, strong, wh, bad_ch, img_off, pool.data(), nullptr,
                              again.data(), &st2) == SFM_ERR_INVALID_ARG);
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 3, 2, bad_ii, strong, wh, channels, img_off, pool.data(), nullptr,
                              again.data(), &st2) == SFM_ERR_INVALID_ARG);
    double nan_k[12];
    std::memcpy(nan_k, strong, sizeof strong);
    nan_k[4] = std::nan("");
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 3, 2, img_intr, nan_k, wh, channels, img_off, pool.data(), nullptr,
                              again.data(), &st2) == SFM_ERR_INVALID_ARG);
    EXPECT(sfm_undistort_host(SFM_CAM_RADIAL3, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                              nullptr, &st2) == SFM_OK && st2.n_images == 0);

    // the façade: two cameras, three images, four points
    auto world = std::make_shared<WorldStructure>();
    auto cam_a = std::make_shared<Camera>(60.0, 60.0, 33.5, 20.5), cam_b = std::make_shared<Camera>(70.0, 70.0, 31.5, 23.5);
    std::vector<Image::Ptr> imgs = {std::make_shared<Image>(cam_a), std::make_shared<Image>(cam_b),
                                    std::make_shared<Image>(cam_b)};
    imgs[1]->setPose({0.0, 0.0, 0.0, 1.0, 2.0, 3.0});
    imgs[2]->setPose({0.0, 0.0, 1.5707963267948966, 1.0, 0.0, 0.0});
    for (auto& im : imgs) world->addImage(im);
    const int seen[4][3] = {{1, 1, 1}, {1, 0, 1}, {0, 1, 0}, {0, 1, 1}};
    for (int p = 0; p < 4; ++p) {
        const auto idx = world->addPoint({1.0 + p, 2.0, 0.5}, std::vector<uint8_t>(128, 0));
        for (int i = 0; i < 3; ++i)
            if (seen[p][i]) world->addObservation(world->getPointFromIdx(idx), imgs[i], Point2d{1.0, 1.0});
    }
    DenseBuilder dense(world);
    DenseScene sc;
    EXPECT(dense.scene(imgs, {67, 41, 64, 48, 64, 48}, sc));
    EXPECT(sc.info.n_platforms == 2 && sc.info.n_images == 3 && sc.info.n_vertices == 3 && sc.info.n_short == 1);
    EXPECT(sc.image_platform == (std::vector<int32_t>{0, 1, 1}) && sc.image_pose == (std::vector<int32_t>{0, 0, 1}));
    EXPECT(sc.vert_off == (std::vector<int64_t>{0, 3, 5, 7}) && sc.vert_view == (std::vector<uint32_t>{0, 1, 2, 0, 2, 1, 2}));
    EXPECT(sc.vert_pt == (std::vector<int64_t>{0, 1, 3}) && sc.vert_X[3] == 2.0f && sc.K[2] == 33.5 && sc.K[9 + 4] == 70.0);
    EXPECT(sc.C[3] == -1.0 && sc.C[4] == -2.0 && sc.C[5] == -3.0);                            // R = I: C = -t
    EXPECT(std::fabs(sc.C[6]) < 1e-15 && std::fabs(sc.C[7] - 1.0) < 1e-15 && sc.C[8] == 0.0);   // a quarter turn about z
    EXPECT(!dense.scene(imgs, {67, 41, 64, 48, 64, 47}, sc));                                 // one camera, two sizes

    std::vector<ColorImage> pix = {ColorImage{&pool[(size_t)img_off[0]], 67, 41, 3}, ColorImage{nullptr, 64, 48, 1},
                                   ColorImage{&pool[(size_t)img_off[2]], 64, 48, 1}};
    const std::vector<double> k3 = {0.8, 0.0, 0.0, 0.3, -0.2, 0.1};
    EXPECT(dense.exportUndistorted(HostUndistortBackend{}, ".", imgs, {"undistort_test_a", "undistort_test_b", "undistort_test_c"},
                                   pix, &k3, &st2));
    EXPECT(st2.n_outside == st.n_outside && st2.n_low_weight == st.n_low_weight);
    for (const char* name : {"undistort_test_a.ppm", "undistort_test_c.pgm"}) {
        std::FILE* f = std::fopen(name, "rb");
        EXPECT(f != nullptr);
        if (!f) continue;
        std::vector<uint8_t> file(20000);
        file.resize(std::fread(file.data(), 1, file.size(), f));
        std::fclose(f);
        const bool rgb = name[15] == 'a';
        const std::string head = rgb ? "P6\n67 41\n255\n" : "P5\n64 48\n255\n";
        const size_t n = rgb ? 67 * 41 * 3 : 64 * 48;
        EXPECT(file.size() == head.size() + n && std::memcmp(file.data(), head.data(), head.size()) == 0 &&
               std::memcmp(file.data() + head.size(), &black[(size_t)img_off[rgb ? 0 : 2]], n) == 0);
        std::remove(name);
    }
    std::FILE* none = std::fopen("undistort_test_b.pgm", "rb");
    EXPECT(none == nullptr);
    if (none) std::fclose(none);
    EXPECT(sfm_undistort_write_pnm("no_such_dir/x.pgm", 2, 2, 1, pool.data()) == SFM_ERR_INVALID_ARG);
    if (fails) return 1;
    std::printf("undistort ok\n");
    return 0;
}
