// sfm_colorize_assign_host / sfm_colorize_sample / sfm_colorize_host and
// sfm::ColorizeTracks on the host backend (include/sfm/colorize.hpp) on a tiny
// scene worked out by hand: three images (two 3-channel, one gray, of
// different sizes), five points.
//
//   point 0: images 0, 1          point 3: image 2, twice (the first observation dead)
//   point 1: images 0, 1          point 4: image 1 (masked off by pt_ok)
//   point 2: images 1, 2
// Counts: image 0 sees 2, image 1 sees 3, image 2 sees 2.  Round 1 takes image 1
// (points 0, 1, 2), round 2 image 2 (point 3; image 0 is left with nothing).
//
// A stand-alone host program: csrc/colorize.cpp's host path is compiled in (no
// library, no HIP runtime), so it can be built with host sanitizers and run
// anywhere.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../../3dreconstruction_amd/csrc/common.h"
#include "../../3dreconstruction_amd/include/sfm/colorize.hpp"
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
    // images: 0 is 4 x 3 rgb, 1 is 5 x 2 rgb, 2 is 3 x 3 gray; pixel (x, y) of image i, channel c = 40 i + 10 y + x + 100 c
    const int32_t wh[6] = {4, 3, 5, 2, 3, 3}, channels[3] = {3, 3, 1};
    std::vector<uint8_t> pool;
    int64_t img_off[3];
    for (int i = 0; i < 3; ++i) {
        img_off[i] = (int64_t)pool.size();
        for (int y = 0; y < wh[2 * i + 1]; ++y)
            for (int x = 0; x < wh[2 * i]; ++x)
                for (int c = 0; c < channels[i]; ++c) pool.push_back((uint8_t)(40 * i + 10 * y + x + 100 * c));
    }
    const int64_t off[6] = {0, 2, 4, 6, 8, 9};
    const int32_t oi[9] = {0, 1, 0, 1, 1, 2, 2, 2, 1};
    //                      p0: im0, im1 | p1: im0, im1    | p2: im1, im2    | p3: im2 (dead), im2 | p4: im1
    const double uv[18] = {1.5, 1.5, 4.75, -3.0, 0.0, 0.0, 9.0, 0.99, 2.5, 1.0, 1.0, 1.0, 0.0, 0.0, 2.0, 2.9, 1.0, 1.0};
    const uint8_t keep[9] = {1, 1, 1, 1, 1, 1, 0, 1, 1}, ok[5] = {1, 1, 1, 1, 0};
    sfm_ba_problem P{};
    P.n_img = 3; P.n_pt = 5; P.n_obs = 9; P.pt_offsets = off; P.obs_img = oi; P.obs_uv = uv;
    int32_t view[5], px[10], order[3], n_rounds = -1;
    int64_t obs[5];
    sfm_colorize_stats st;
    EXPECT(sfm_colorize_assign_host(&P, wh, ok, keep, view, obs, px, order, &n_rounds, &st) == SFM_OK);
    EXPECT(n_rounds == 2 && order[0] == 1 && order[1] == 2 && order[2] == -1);
    EXPECT(st.n_to_colour == 4 && st.n_coloured == 4 && st.n_rounds == 2);
    const int32_t want_view[5] = {1, 1, 1, 2, -1};
    const int64_t want_obs[5] = {1, 3, 4, 7, -1};
    const int32_t want_px[10] = {4, 0, 4, 0, 2, 1, 2, 2, 0, 0};   // clamped, then truncated
    for (int p = 0; p < 5; ++p)
        EXPECT(view[p] == want_view[p] && obs[p] == want_obs[p] && px[2 * p] == want_px[2 * p] &&
               px[2 * p + 1] == want_px[2 * p + 1]);
    uint8_t rgb[15];
    EXPECT(sfm_colorize_sample(5, view, px, 3, wh, channels, img_off, pool.data(), rgb) == SFM_OK);
    const uint8_t want_rgb[15] = {44, 144, 244, 44, 144, 244, 52, 152, 252, 102, 102, 102, 0, 0, 0};
    EXPECT(std::memcmp(rgb, want_rgb, 15) == 0);
    // one call; image 0 colours nothing, but a point to colour is seen in it: it has to be loaded
    uint8_t rgb2[15];
    int32_t view2[5];
    EXPECT(sfm_colorize_host(&P, wh, ok, keep, channels, img_off, pool.data(), rgb2, view2, &st) == SFM_OK);
    EXPECT(std::memcmp(rgb2, want_rgb, 15) == 0 && std::memcmp(view2, want_view, sizeof view2) == 0);
    int64_t off_unloaded[3] = {-1, img_off[1], img_off[2]};
    EXPECT(sfm_colorize_host(&P, wh, ok, keep, channels, off_unloaded, pool.data(), rgb2, view2, &st) ==
           SFM_ERR_INVALID_ARG);
    EXPECT(sfm_colorize_sample(5, view, px, 3, wh, channels, off_unloaded, pool.data(), rgb2) == SFM_OK);   // not needed
    off_unloaded[0] = img_off[0];
    off_unloaded[2] = -1;
    EXPECT(sfm_colorize_sample(5, view, px, 3, wh, channels, off_unloaded, pool.data(), rgb2) == SFM_ERR_INVALID_ARG);
    // the checks
    const int32_t bad_wh[6] = {4, 3, 0, 2, 3, 3}, bad_ch[3] = {3, 2, 1};
    EXPECT(sfm_colorize_assign_host(&P, bad_wh, ok, keep, view, obs, px, order, &n_rounds, &st) == SFM_ERR_INVALID_ARG);
    EXPECT(sfm_colorize_host(&P, wh, ok, keep, bad_ch, img_off, pool.data(), rgb2, view2, &st) == SFM_ERR_INVALID_ARG);
    double uv_nan[18];
    std::memcpy(uv_nan, uv, sizeof uv);
    uv_nan[12] = std::nan("");   // a dead observation: not read
    P.obs_uv = uv_nan;
    EXPECT(sfm_colorize_assign_host(&P, wh, ok, keep, view, obs, px, order, &n_rounds, &st) == SFM_OK);
    uv_nan[14] = std::nan("");   // a live one
    EXPECT(sfm_colorize_assign_host(&P, wh, ok, keep, view, obs, px, order, &n_rounds, &st) == SFM_ERR_INVALID_ARG);
    P.obs_uv = uv;
    EXPECT(sfm_colorize_assign_host(nullptr, wh, ok, keep, view, obs, px, order, &n_rounds, &st) == SFM_ERR_INVALID_ARG);

    // the façade on the host backend: the same scene as a WorldStructure (no masks: every observation is live)
    auto world = std::make_shared<WorldStructure>();
    auto cam = std::make_shared<Camera>(100.0, 100.0, 2.0, 1.5);
    std::vector<Image::Ptr> imgs;
    std::vector<ColorImage> pix;
    for (int i = 0; i < 3; ++i) {
        imgs.push_back(std::make_shared<Image>(cam));
        world->addImage(imgs.back());
        pix.push_back(ColorImage{pool.data() + img_off[i], wh[2 * i], wh[2 * i + 1], channels[i]});
    }
    for (int p = 0; p < 5; ++p) {
        const auto idx = world->addPoint({0.0, 0.0, 0.0}, std::vector<uint8_t>(128, 0));
        for (int64_t o = off[p]; o < off[p + 1]; ++o)
            world->addObservation(world->getPointFromIdx(idx), imgs[oi[o]], Point2d{uv[2 * o], uv[2 * o + 1]});
    }
    std::vector<std::array<uint8_t, 3>> colors;
    EXPECT(ColorizeTracks(HostColorizeBackend{}, *world, imgs, pix, colors, nullptr, &st));
    // image 1 sees points 0, 1, 2, 4 and goes first; image 2 then colours point 3 at its first observation (0, 0)
    EXPECT(st.n_rounds == 2 && st.n_coloured == 5 && colors.size() == 5);
    EXPECT(colors[0][0] == 44 && colors[2][2] == 252 && colors[3][0] == 80 && colors[3][2] == 80 && colors[4][1] == 151);
    // every image here is seen by a point to colour: one that is not loaded fails the call
    pix[0].data = nullptr;
    EXPECT(!ColorizeTracks(HostColorizeBackend{}, *world, imgs, pix, colors));

    // the PLY writer: coloured and white
    const double X[15] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    const double extr[12] = {0, 0, 0, 1, 2, 3, 0, 0, 0, -1, 0, 0};
    const uint8_t reg[2] = {1, 0};
    const std::string path = "colorize_test_out.ply";
    for (int pass = 0; pass < 2; ++pass) {
        EXPECT(sfm_colorize_write_ply(path.c_str(), 5, X, ok, pass ? nullptr : want_rgb, 2, extr, reg) == SFM_OK);
        std::FILE* f = std::fopen(path.c_str(), "r");
        EXPECT(f != nullptr);
        if (!f) break;
        char buf[2048] = {0};
        const size_t n = std::fread(buf, 1, sizeof buf - 1, f);
        std::fclose(f);
        const std::string text(buf, n);
        EXPECT(text.find("element vertex 5\n") != std::string::npos);
        EXPECT(text.find(pass ? "1.0000000000000000 2.0000000000000000 3.0000000000000000 255 255 255\n"
                              : "1.0000000000000000 2.0000000000000000 3.0000000000000000 44 144 244\n") !=
               std::string::npos);
        EXPECT(text.find("-1.0000000000000000 -2.0000000000000000 -3.0000000000000000 0 255 0\n") != std::string::npos);
        EXPECT(text.find("13.0000000000000000") == std::string::npos);   // point 4 is masked off
    }
    std::remove(path.c_str());
    if (fails) return 1;
    std::printf("colorize ok\n");
    return 0;
}
