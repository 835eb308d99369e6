// SIFT extraction, host side (include/sfmcore.h, "SIFT extraction"): the
// options, the argument checks and the tables both entry points share (the
// Gaussian taps of every level and the exp(-x) table are computed here, once,
// for both), the serial host twin (sfm_sift_host: sift.hip's kernels restated
// for one thread over the same sift_point.h statements) and the device entry
// point (sfm_sift: uploads, the launches of each octave, downloads).
// SFM_SIFT_HOST_ONLY leaves the device entry point out, so that the host path
// builds with a plain host compiler (tests/cpp/sift_test.cpp).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "sift.h"
#include "sift_point.h"

using namespace sfm;
using namespace sfm::sift;

extern "C" void sfm_sift_options_default(sfm_sift_options* o) {
    if (!o) return;
    // SIFT_Image_describer::Params as detectFeature() leaves them (NORMAL preset)
    o->n_octaves = 6;
    o->n_scales = 3;
    o->first_octave = 0;
    o->edge_threshold = 10.0f;
    o->peak_threshold = 0.04f;
    o->root_sift = 1;
    o->orientation = 1;
    o->reserved = 0;
}

namespace {

struct Plan {
    sfm_sift_options o;
    double tp = 0, te = 0, sigma0 = 0;
    // taps of set t at taps[off[t]], half-width W[t] (-1: no smoothing).  Set
    // 0 brings the input (nominal blur 0.5) to level 0 of the first octave;
    // set i >= 1 takes level i - 1 to level i, in every octave.
    std::vector<float> taps;
    std::vector<int> off, W;
    std::vector<double> expn;
};

void add_taps(Plan& p, double sd) {
    if (!(sd > 0)) {
        p.off.push_back((int)p.taps.size());
        p.W.push_back(-1);
        return;
    }
    const double c = std::ceil(4.0 * sd);
    SFM_REQUIRE(c <= kMaxHalf, SFM_ERR_UNSUPPORTED, "sfm_sift: a level needs a Gaussian of half-width %g (at most %d)", c,
                kMaxHalf);
    const int W = std::max((int)c, 1);
    p.off.push_back((int)p.taps.size());
    p.W.push_back(W);
    float acc = 0.f;
    const size_t at = p.taps.size();
    for (int j = 0; j <= 2 * W; ++j) {
        const float d = (float)(j - W) / (float)sd;
        const float g = (float)std::exp(-0.5 * (d * d));
        p.taps.push_back(g);
        acc += g;
    }
    for (int j = 0; j <= 2 * W; ++j) p.taps[at + j] /= acc;
}

Plan check_args(const char* who, const uint8_t* gray, int32_t n_img, int32_t w, int32_t h, const sfm_sift_options* opts,
                int64_t cap, const float* xyso, const uint8_t* desc, const int64_t* n_feat) {
    Plan p;
    if (opts) p.o = *opts; else sfm_sift_options_default(&p.o);
    const sfm_sift_options& o = p.o;
    SFM_REQUIRE(n_img >= 0 && cap >= 0, SFM_ERR_INVALID_ARG, "%s: negative count", who);
    SFM_REQUIRE(w > 0 && h > 0, SFM_ERR_INVALID_ARG, "%s: image size %d x %d", who, w, h);
    SFM_REQUIRE(o.n_octaves >= 0 && o.n_scales >= 1 && o.edge_threshold > 0.f && o.peak_threshold >= 0.f,
                SFM_ERR_INVALID_ARG, "%s: bad options", who);
    SFM_REQUIRE(o.first_octave == 0, SFM_ERR_UNSUPPORTED,
                "%s: first_octave %d (only 0: no up- or down-sampled first octave)", who, o.first_octave);
    SFM_REQUIRE(o.n_scales <= kMaxScales && o.n_octaves <= 30, SFM_ERR_UNSUPPORTED,
                "%s: at most %d scales per octave and 30 octaves", who, kMaxScales);
    SFM_REQUIRE((int64_t)w * h <= ((int64_t)1 << 28) && n_img <= 65535, SFM_ERR_UNSUPPORTED,
                "%s: at most 2^28 pixels per image and 65535 images per call", who);
    SFM_REQUIRE(n_img == 0 || (gray && n_feat), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    SFM_REQUIRE(n_img == 0 || cap == 0 || (xyso && desc), SFM_ERR_INVALID_ARG, "%s: null output with cap_per_img > 0",
                who);
    const int S = o.n_scales;
    p.tp = (double)(255 * o.peak_threshold / S);   // in float, as the describer hands it over
    p.te = (double)o.edge_threshold;
    const double sigmak = std::pow(2.0, 1.0 / S);
    p.sigma0 = 1.6 * sigmak;
    const double dsigma0 = p.sigma0 * std::sqrt(1.0 - 1.0 / (sigmak * sigmak));
    const double sa = p.sigma0 * std::pow(sigmak, -1.0), sb = 0.5;
    add_taps(p, sa > sb ? std::sqrt(sa * sa - sb * sb) : 0.0);
    for (int i = 1; i <= S + 2; ++i) add_taps(p, dsigma0 * std::pow(sigmak, (double)(i - 1)));
    p.expn.assign(kExpnSize + 2, 0.0);
    for (int k = 0; k <= kExpnSize; ++k) p.expn[k] = std::exp(-(double)k * (kExpnMax / kExpnSize));
    return p;
}

// octaves run while both sides hold a 3 x 3 neighbourhood (a smaller one has no
// cell to test)
inline bool octave_dims(int w, int h, int o, int& wo, int& ho) {
    wo = w >> o;
    ho = h >> o;
    return wo >= 3 && ho >= 3;
}

void host_smooth(const float* src, float* tmp, float* dst, const float* taps, int W, int w, int h) {
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            tmp[(size_t)y * w + x] = conv_acc(
                [&](int j) { return src[(size_t)std::min(std::max(y - W + j, 0), h - 1) * w + x]; }, taps, W);
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
            dst[(size_t)y * w + x] = conv_acc(
                [&](int j) { return tmp[(size_t)y * w + std::min(std::max(x - W + j, 0), w - 1)]; }, taps, W);
}

// one image; returns its feature count, adds its keypoints to *n_kp
int64_t host_image(const Plan& p, const uint8_t* gray, int w, int h, int64_t cap, float* xyso, uint8_t* desc,
                   int64_t* n_kp) {
    const int S = p.o.n_scales, nlev = S + 3;
    std::vector<std::vector<float>> L((size_t)nlev, std::vector<float>((size_t)w * h));
    std::vector<float> tmp((size_t)w * h), grad((size_t)S * 2 * w * h);
    std::vector<Keypoint> kps;
    int64_t n = 0;
    int wp = w, hp = h;
    for (int o = 0, wo, ho; o < p.o.n_octaves && octave_dims(w, h, o, wo, ho); ++o) {
        const double xper = (double)((int64_t)1 << o);
        if (o == 0) {
            for (size_t i = 0; i < (size_t)w * h; ++i) L[0][i] = (float)gray[i];
            if (p.W[0] >= 0) host_smooth(L[0].data(), tmp.data(), L[0].data(), &p.taps[p.off[0]], p.W[0], wo, ho);
        } else {
            for (int y = 0; y < ho; ++y)
                for (int x = 0; x < wo; ++x) L[0][(size_t)y * wo + x] = L[S][(size_t)(2 * y) * wp + 2 * x];
        }
        for (int i = 1; i < nlev; ++i)
            host_smooth(L[i - 1].data(), tmp.data(), L[i].data(), &p.taps[p.off[i]], p.W[i], wo, ho);
        Levels lv{};
        for (int i = 0; i < nlev; ++i) lv.L[i] = L[i].data();
        kps.clear();
        for (int k = 1; k <= S; ++k)
            for (int y = 1; y < ho - 1; ++y)
                for (int x = 1; x < wo - 1; ++x) {
                    Keypoint kp;
                    if (detect_cell(lv, wo, ho, S, x, y, k, p.tp, p.te, p.sigma0, xper, &kp)) kps.push_back(kp);
                }
        *n_kp += (int64_t)kps.size();
        if (!kps.empty()) {
            const size_t wh = (size_t)wo * ho;
            for (int k = 1; k <= S; ++k)
                for (int y = 0; y < ho; ++y)
                    for (int x = 0; x < wo; ++x) {
                        float* g = &grad[(size_t)(k - 1) * 2 * wh + 2 * ((size_t)y * wo + x)];
                        gradient(L[k].data(), wo, ho, x, y, g[0], g[1]);
                    }
            for (const Keypoint& kp : kps) {
                const float* g = &grad[(size_t)(kp.k - 1) * 2 * wh];
                double ang[4] = {0, 0, 0, 0};
                int na = 1;
                if (p.o.orientation) {
                    const OriWindow win = ori_window(kp, xper, wo, ho);
                    na = 0;
                    if (win.ok) {
                        // every bin's sum in row-major sample order: the kernel's lanes walk the same order
                        double hist[kOriBins] = {0};
                        for (int ys = win.y0; ys <= win.y1; ++ys)
                            for (int xs = win.x0; xs <= win.x1; ++xs) {
                                int bin;
                                double w0, w1;
                                if (!ori_sample(win, g, wo, p.expn.data(), xs, ys, bin, w0, w1)) continue;
                                hist[bin] += w0;
                                hist[(bin + 1) % kOriBins] += w1;
                            }
                        na = ori_peaks(hist, ang);
                    }
                }
                for (int a = 0; a < na; ++a, ++n) {
                    if (n >= cap) continue;
                    const DescWindow d = desc_window(kp, ang[a], xper, wo, ho);
                    float dd[128] = {0};
                    if (d.ok)
                        for (int dy = d.y0; dy <= d.y1; ++dy)
                            for (int dx = d.x0; dx <= d.x1; ++dx) {
                                const DescSample s = desc_sample(d, g, wo, p.expn.data(), dx, dy);
                                for (int bx = 0; bx < 2; ++bx)
                                    for (int by = 0; by < 2; ++by)
                                        for (int bt = 0; bt < 2; ++bt) {
                                            const int X = s.bx + bx, Y = s.by + by;
                                            if (X < -2 || X >= 2 || Y < -2 || Y >= 2) continue;
                                            dd[desc_index(X, Y, (s.bt + bt) & 7)] += desc_weight(s, bx, by, bt);
                                        }
                            }
                    desc_finish(dd, p.o.root_sift, desc + n * 128);
                    float* f = xyso + n * 4;
                    f[0] = kp.x; f[1] = kp.y; f[2] = kp.sigma; f[3] = (float)ang[a];
                }
            }
        }
        wp = wo;
        hp = ho;
    }
    (void)hp;
    return n;
}

void summarize(sfm_sift_summary* sm, int32_t n_img, int64_t cap, const int64_t* n_feat, int64_t n_kp, double ms) {
    if (!sm) return;
    std::memset(sm, 0, sizeof *sm);
    sm->n_images = n_img;
    sm->n_keypoints = n_kp;
    for (int32_t i = 0; i < n_img; ++i) {
        sm->n_features += n_feat[i];
        sm->n_written += std::min(n_feat[i], cap);
        sm->n_overflow += n_feat[i] > cap;
    }
    sm->kernel_ms = ms;
}

}  // namespace

extern "C" int sfm_sift_host(const uint8_t* gray, int32_t n_img, int32_t w, int32_t h, const sfm_sift_options* opts,
                             int64_t cap_per_img, float* xyso, uint8_t* desc, int64_t* n_feat,
                             sfm_sift_summary* summary) {
    return guarded([&] {
        const Plan p = check_args("sfm_sift_host", gray, n_img, w, h, opts, cap_per_img, xyso, desc, n_feat);
        int64_t n_kp = 0;
        for (int32_t i = 0; i < n_img; ++i)
            n_feat[i] = host_image(p, gray + (size_t)i * w * h, w, h, cap_per_img, xyso + (size_t)i * cap_per_img * 4,
                                   desc + (size_t)i * cap_per_img * 128, &n_kp);
        summarize(summary, n_img, cap_per_img, n_feat, n_kp, -1.0);
        return SFM_OK;
    });
}

#ifndef SFM_SIFT_HOST_ONLY
namespace {
// event pairs around each stretch of launches (SFM_CTX_TIME_KERNELS only)
struct Stopwatch {
    bool on;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    Stopwatch(bool on_, hipStream_t s_) : on(on_), s(s_) {}
    ~Stopwatch() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    void mark() {
        if (!on) return;
        hipEvent_t e;
        SFM_HIP(hipEventCreate(&e));
        ev.push_back(e);
        SFM_HIP(hipEventRecord(e, s));
    }
    double total() {   // after a synchronize
        double ms = 0;
        for (size_t i = 0; i + 1 < ev.size(); i += 2) {
            float t = 0.f;
            SFM_HIP(hipEventElapsedTime(&t, ev[i], ev[i + 1]));
            ms += t;
        }
        return ms;
    }
};
}  // namespace

extern "C" int sfm_sift(sfm_ctx* ctx, const uint8_t* gray, int32_t n_img, int32_t w, int32_t h,
                        const sfm_sift_options* opts, int64_t cap_per_img, float* xyso, uint8_t* desc, int64_t* n_feat,
                        sfm_sift_summary* summary) {
    return guarded([&] {
        SFM_REQUIRE(ctx, SFM_ERR_INVALID_ARG, "sfm_sift: null context");
        const Plan p = check_args("sfm_sift", gray, n_img, w, h, opts, cap_per_img, xyso, desc, n_feat);
        int wo, ho;
        if (n_img == 0 || p.o.n_octaves == 0 || !octave_dims(w, h, 0, wo, ho)) {
            for (int32_t i = 0; i < n_img; ++i) n_feat[i] = 0;
            summarize(summary, n_img, cap_per_img, n_feat, 0, -1.0);
            ctx->last_kernel_ms = -1.0;
            return SFM_OK;
        }
        const int S = p.o.n_scales, nlev = S + 3;
        const size_t wh = (size_t)w * h, all = wh * (size_t)n_img;
        CtxScope scope_(ctx);
        hipStream_t s = ctx->stream;
        PhaseTimer tm("sfm_sift");
        Stopwatch sw(ctx->time_kernels, s);
        DBuf<uint8_t> d_gray, d_desc;
        DBuf<float> d_lev[kMaxLevels], d_tmp, d_grad, d_taps, d_xyso;
        DBuf<double> d_expn, d_angles;
        DBuf<int32_t> d_rowcnt, d_rowbase, d_ktot, d_ftot, d_nang, d_row;
        DBuf<Keypoint> d_kps;
        d_gray.alloc(all); d_gray.upload(gray, all, s);
        d_taps.alloc(p.taps.size()); d_taps.upload(p.taps.data(), p.taps.size(), s);
        d_expn.alloc(p.expn.size()); d_expn.upload(p.expn.data(), p.expn.size(), s);
        for (int i = 0; i < nlev; ++i) d_lev[i].alloc(all);
        d_tmp.alloc(all);
        d_grad.alloc(all * 2 * S);
        d_rowcnt.alloc((size_t)n_img * S * h);
        d_rowbase.alloc((size_t)n_img * S * h);
        d_ktot.alloc(2 * (size_t)n_img);
        d_ftot.alloc(n_img); d_ftot.zero(s);
        d_xyso.alloc((size_t)n_img * cap_per_img * 4);
        d_desc.alloc((size_t)n_img * cap_per_img * 128);
        SiftOctave a{};
        for (int i = 0; i < nlev; ++i) a.lv.L[i] = d_lev[i].p;
        a.S = S; a.n_img = n_img; a.tp = p.tp; a.te = p.te; a.sigma0 = p.sigma0; a.expn = d_expn.p;
        a.grad = d_grad.p; a.rowcnt = d_rowcnt.p; a.rowbase = d_rowbase.p; a.ktot = d_ktot.p; a.ftot = d_ftot.p;
        a.orientation = p.o.orientation; a.root_sift = p.o.root_sift;
        a.cap = cap_per_img; a.xyso = d_xyso.p; a.desc = d_desc.p;
        if (sw.on) SFM_HIP(hipStreamSynchronize(s));   // the uploads are drained first
        tm.mark("upload");
        std::vector<int32_t> ktot(n_img);
        int64_t n_kp = 0;
        int wp = w, hp = h;
        for (int o = 0; o < p.o.n_octaves && octave_dims(w, h, o, wo, ho); ++o) {
            sw.mark();
            if (o == 0) {
                sift_launch_u8(d_gray.p, d_lev[0].p, (int64_t)all, s);
                if (p.W[0] >= 0)
                    sift_launch_smooth(d_lev[0].p, d_tmp.p, d_lev[0].p, d_taps.p + p.off[0], p.W[0], wo, ho, n_img, s);
            } else {
                sift_launch_decimate(d_lev[S].p, wp, hp, d_lev[0].p, wo, ho, n_img, s);
            }
            for (int i = 1; i < nlev; ++i)
                sift_launch_smooth(d_lev[i - 1].p, d_tmp.p, d_lev[i].p, d_taps.p + p.off[i], p.W[i], wo, ho, n_img, s);
            a.w = wo; a.h = ho; a.xper = (double)((int64_t)1 << o);
            sift_launch_count(a, s);
            sw.mark();
            SFM_HIP(hipMemcpyAsync(ktot.data(), d_ktot.p, sizeof(int32_t) * (size_t)n_img, hipMemcpyDeviceToHost, s));
            SFM_HIP(hipStreamSynchronize(s));
            int32_t kmax = 0;
            for (int32_t v : ktot) {
                kmax = std::max(kmax, v);
                n_kp += v;
            }
            if (kmax > 0) {
                if ((size_t)kmax * n_img > d_kps.n) {
                    d_kps.alloc((size_t)kmax * n_img);
                    d_nang.alloc((size_t)kmax * n_img);
                    d_row.alloc((size_t)kmax * n_img);
                    d_angles.alloc((size_t)kmax * n_img * 4);
                }
                a.kcap = kmax; a.kps = d_kps.p; a.nang = d_nang.p; a.row = d_row.p; a.angles = d_angles.p;
                sw.mark();
                sift_launch_describe(a, kmax, s);
                sw.mark();
            }
            wp = wo;
            hp = ho;
        }
        std::vector<int32_t> ftot(n_img);
        SFM_HIP(hipMemcpyAsync(ftot.data(), d_ftot.p, sizeof(int32_t) * (size_t)n_img, hipMemcpyDeviceToHost, s));
        SFM_HIP(hipStreamSynchronize(s));
        tm.mark("kernels");
        for (int32_t i = 0; i < n_img; ++i) {
            n_feat[i] = ftot[i];
            const size_t rows = (size_t)std::min<int64_t>(ftot[i], cap_per_img);
            if (!rows) continue;
            SFM_HIP(hipMemcpyAsync(xyso + (size_t)i * cap_per_img * 4, d_xyso.p + (size_t)i * cap_per_img * 4,
                                   rows * 4 * sizeof(float), hipMemcpyDeviceToHost, s));
            SFM_HIP(hipMemcpyAsync(desc + (size_t)i * cap_per_img * 128, d_desc.p + (size_t)i * cap_per_img * 128,
                                   rows * 128, hipMemcpyDeviceToHost, s));
        }
        SFM_HIP(hipStreamSynchronize(s));
        ctx->last_kernel_ms = sw.on ? sw.total() : -1.0;
        tm.mark("download");
        summarize(summary, n_img, cap_per_img, n_feat, n_kp, ctx->last_kernel_ms);
        return SFM_OK;
    });
}
#endif
