// sfm::Localizer (include/sfm/localizer.hpp) on the host backend over a small
// WorldStructure: six cameras on a circle around 60 points, exact pinhole
// observations, a few gross outlier observations.  Three of the images start
// from a garbage pose; after the resection they are at ground truth, the
// outliers are not among their inliers, and an image seeing three points keeps
// its pose (SFM_RESECT_FEW).  Then the checks of the [cpu] entry points.
//
// A stand-alone host program: csrc/resect.cpp's host path is compiled in (no
// library, no HIP runtime), so it can be built with host sanitizers and run
// anywhere.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>

#define SFM_RESECT_HOST_ONLY
#include "../../3dreconstruction_amd/csrc/resect.cpp"
#include "../../3dreconstruction_amd/include/sfm/localizer.hpp"
namespace sfm {
static char g_err[512];
void set_error(const char* fmt, ...) {
    va_list a;
    va_start(a, fmt);
    std::vsnprintf(g_err, sizeof g_err, fmt, a);
    va_end(a);
}
}  // namespace sfm
extern "C" int sfm_ba_intr_width(int32_t m) { return m == SFM_CAM_RADIAL3 ? 6 : (m == 0 || m == 1) ? 4 : 0; }
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
    auto world = std::make_shared<WorldStructure>();
    auto cam = std::make_shared<Camera>(2905.88, 2905.88, 1416.0, 1064.0);
    std::vector<Image::Ptr> imgs;
    std::vector<std::array<double, 6>> truth;
    for (int c = 0; c < 7; ++c) {
        const double a = 0.3 * c;
        double R[9];
        const double w[3] = {0.0, a, 0.0};
        rot::aa_to_matrix(w, R);
        const double C[3] = {10.0 * std::sin(a), 0.0, -10.0 * std::cos(a)};
        std::array<double, 6> pose{w[0], w[1], w[2], 0, 0, 0};
        for (int r = 0; r < 3; ++r) pose[3 + r] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
        auto im = std::make_shared<Image>(cam);
        im->setPose(pose);
        world->addImage(im);
        imgs.push_back(im);
        truth.push_back(pose);
    }
    uint64_t s = 2468;
    auto rnd = [&] {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) / 9007199254740992.0;
    };
    // image 6 sees three points only; the others see every point
    std::vector<std::vector<int>> outlier_at(7);
    for (int k = 0; k < 60; ++k) {
        const std::array<double, 3> X{4 * rnd() - 2, 4 * rnd() - 2, 4 * rnd() - 2};
        const auto idx = world->addPoint(X, std::vector<uint8_t>(128, 0));
        auto p = world->getPointFromIdx(idx);
        for (int c = 0; c < (k < 3 ? 7 : 6); ++c) {
            double R[9];
            rot::aa_to_matrix(truth[c].data(), R);
            double P[3];
            for (int r = 0; r < 3; ++r) P[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + truth[c][3 + r];
            Point2d uv{cam->fx * P[0] / P[2] + cam->cx, cam->fy * P[1] / P[2] + cam->cy};
            if (k % 7 == 5 && c % 2 == 1) {   // a gross outlier
                uv.x += 120.0 + k;
                uv.y -= 80.0;
                outlier_at[c].push_back(k);
            }
            world->addObservation(p, imgs[c], uv);
        }
    }
    const std::vector<Image::Ptr> lost{imgs[1], imgs[4], imgs[5], imgs[6]};
    for (const auto& im : lost) im->setPose({0.3, -0.2, 0.1, 1.0, 2.0, 3.0});
    HostLocalizer loc;
    loc.options().max_iterations = 128;
    const int64_t written = loc(world, lost, 2832, 2128);
    EXPECT(loc.lastError() == SFM_OK);
    EXPECT(written == 3);
    const int which[4] = {1, 4, 5, 6};
    double worst = 0;
    for (int q = 0; q < 3; ++q) {
        const sfm_resect_result& r = loc.results()[q];
        EXPECT(r.status == SFM_RESECT_OK && r.min_nfa < 0);
        EXPECT(r.n_inliers == 60 - (int)outlier_at[which[q]].size());
        for (int32_t k : loc.inliers()[q])
            for (int o : outlier_at[which[q]]) EXPECT(k != o);
        for (int a = 0; a < 6; ++a) worst = std::fmax(worst, std::fabs(lost[q]->pose()[a] - truth[which[q]][a]));
    }
    EXPECT(worst <= 1e-9);
    EXPECT(loc.results()[3].status == SFM_RESECT_FEW && lost[3]->pose()[3] == 1.0);
    std::printf("host: %lld poses written, max |pose - truth| %.3e\n", (long long)written, worst);

    // the [cpu] entry points
    sfm_resect_opts o;
    sfm_resect_default_options(&o);
    EXPECT(o.max_iterations == 4096 && o.refine_iterations == 10 && o.precision == 0.0);
    o.max_iterations = 0;
    sfm_resect_result res;
    int32_t inl[4];
    const int64_t off[2] = {0, 4};
    const double X[12] = {0, 0, 5, 1, 0, 5, 0, 1, 6, 1, 1, 7}, uv[8] = {0, 0, 1, 1, 2, 2, 3, 3};
    const int32_t ii[1] = {0}, wh[2] = {100, 100};
    const double in[4] = {100, 100, 50, 50};
    EXPECT(sfm_resect_host(SFM_CAM_PINHOLE, 1, off, X, uv, ii, in, 1, wh, &o, &res, inl) == SFM_ERR_INVALID_ARG);
    EXPECT(sfm_resect_host(SFM_CAM_PINHOLE, 1, off, X, uv, ii, in, 1, wh, nullptr, &res, inl) == SFM_OK);
    EXPECT(res.status == SFM_RESECT_NO_MODEL && res.n_inliers == 0);
    double Rt[4][12];
    int32_t nm = -1;
    const double b[9] = {0, 0, 1, 0.6, 0, 0.8, 0, 0.6, 0.8};
    const double line[9] = {0, 0, 1, 1, 1, 2, 2, 2, 3};
    EXPECT(sfm_resect_p3p(b, line, Rt, &nm) == SFM_OK && nm == 0);
    EXPECT(sfm_resect_p3p(nullptr, line, Rt, &nm) == SFM_ERR_INVALID_ARG);
    if (fails) return 1;
    std::printf("resect ok\n");
    return 0;
}
