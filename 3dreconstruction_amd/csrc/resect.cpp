// Camera resection, host side (include/sfmcore.h, "Camera resection"): the
// options, the argument checks and a-contrario constants both entry points
// share, the serial host twin (sfm_resect_host: resect.hip's kernel restated
// for one thread over the same resect_pose.h statements), the minimal solver
// and the correspondence gather as [cpu] calls, and the device entry point
// (sfm_resect: uploads, one launch, downloads).  The rotation matrices become
// angle-axis vectors here, on the host, for both paths.
// SFM_RESECT_HOST_ONLY leaves the device entry point out, so that the host
// path builds with a plain host compiler (tests/cpp/resect_test.cpp).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "common.h"
#include "resect.h"
#include "resect_pose.h"
#include "rot_aa.h"

using namespace sfm;

extern "C" void sfm_resect_default_options(sfm_resect_opts* o) {
    if (!o) return;
    // SfM_Localizer::Localize as the incremental engine calls it: no upper
    // bound on the a-contrario threshold, 4096 iterations; RefinePose
    o->precision = 0.0;
    o->max_iterations = 4096;
    o->refine_iterations = 10;
}

namespace {

struct Checked {
    sfm_resect_opts o;
    int64_t n = 0;
    std::vector<double> cst;   // [n_img][4] logalpha0, the bound on the squared error, loge0, 0
};

Checked check_args(const char* who, int32_t cm, int64_t n_img, const int64_t* off, const double* X, const double* uv,
                   const int32_t* img_intr, const double* intr, int32_t n_intr, const int32_t* wh,
                   const sfm_resect_opts* opts, const sfm_resect_result* results, const int32_t* inliers) {
    Checked c;
    if (opts) c.o = *opts; else sfm_resect_default_options(&c.o);
    SFM_REQUIRE(sfm_ba_intr_width(cm) > 0, SFM_ERR_INVALID_ARG, "%s: unknown camera_model %d", who, cm);
    SFM_REQUIRE(n_img >= 0 && n_intr >= 0, SFM_ERR_INVALID_ARG, "%s: negative count", who);
    SFM_REQUIRE(c.o.max_iterations >= 1 && c.o.refine_iterations >= 0 && c.o.precision == c.o.precision,
                SFM_ERR_INVALID_ARG, "%s: bad options", who);
    if (n_img == 0) return c;
    SFM_REQUIRE(off && img_intr && wh && results, SFM_ERR_INVALID_ARG, "%s: null argument", who);
    SFM_REQUIRE(off[0] == 0, SFM_ERR_INVALID_ARG, "%s: off[0] must be 0", who);
    SFM_REQUIRE(n_img < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED, "%s: too many images", who);
    for (int64_t q = 0; q < n_img; ++q) {
        SFM_REQUIRE(off[q + 1] >= off[q], SFM_ERR_INVALID_ARG, "%s: off not monotone at %lld", who, (long long)q);
        SFM_REQUIRE(img_intr[q] >= 0 && img_intr[q] < n_intr, SFM_ERR_INVALID_ARG,
                    "%s: image %lld names intrinsics block %d of %d", who, (long long)q, img_intr[q], n_intr);
        SFM_REQUIRE(wh[2 * q] > 0 && wh[2 * q + 1] > 0, SFM_ERR_INVALID_ARG,
                    "%s: image %lld has a non-positive size", who, (long long)q);
    }
    c.n = off[n_img];
    SFM_REQUIRE(c.n < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED, "%s: too many correspondences", who);
    SFM_REQUIRE(intr && (c.n == 0 || (X && uv && inliers)), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    const bool bounded = c.o.precision > 0.0 && c.o.precision <= 1.7976931348623157e308;
    c.cst.resize(4 * (size_t)n_img);
    for (int64_t q = 0; q < n_img; ++q) {
        const int64_t np = off[q + 1] - off[q];
        c.cst[4 * q] = det_log10(3.14159265358979323846 / ((double)wh[2 * q] * (double)wh[2 * q + 1]));
        c.cst[4 * q + 1] = bounded ? c.o.precision * c.o.precision : 1.7976931348623157e308;
        c.cst[4 * q + 2] = det_log10((double)kP3PMaxModels * (double)(np > kP3PSample ? np - kP3PSample : 1));
        c.cst[4 * q + 3] = 0.0;
    }
    return c;
}

// results[] and inliers[] from what either path left per image: model[24]
// (the RANSAC Rt, the refined Rt), stat[6] and the image's binl
void write_results(int64_t n_img, const int64_t* off, const double* model, const double* stat, const uint32_t* binl,
                   sfm_resect_result* results, int32_t* inliers) {
    for (int64_t q = 0; q < n_img; ++q) {
        sfm_resect_result& r = results[q];
        std::memset(&r, 0, sizeof r);
        const double* s = stat + 6 * q;
        r.status = (int32_t)s[4];
        r.iterations = (int32_t)s[3];
        if (r.status == SFM_RESECT_FEW) continue;
        r.min_nfa = s[0];
        if (r.status != SFM_RESECT_OK) continue;
        r.error_max = std::sqrt(s[1]);
        r.n_inliers = (int32_t)s[2];
        const double* M = model + 24 * q;
        matrix_to_aa(M, r.pose_model);
        matrix_to_aa(M + 12, r.pose);
        for (int a = 0; a < 3; ++a) {
            r.pose_model[3 + a] = M[9 + a];
            r.pose[3 + a] = M[21 + a];
        }
        for (int64_t k = 0; k < r.n_inliers; ++k) inliers[off[q] + k] = (int32_t)binl[off[q] + k];
    }
}

// One image, serially: resect.hip's kernel for one thread.  False when the
// random stream ran out.
template <int CM>
bool host_image(int64_t n, const double* X, const double* uv, const double* in, const double* cst,
                const sfm_resect_opts& O, const std::vector<uint32_t>& rng, double* Mo, double* st, uint32_t* binl) {
    std::fill(Mo, Mo + 24, 0.0);
    std::fill(st, st + 6, 0.0);
    st[4] = (double)SFM_RESECT_FEW;
    if (n <= kP3PSample) return true;
    const double logalpha0 = cst[0], maxThr = cst[1], loge0 = cst[2];
    std::vector<double> bear(3 * (size_t)n), L((size_t)n + 1);
    std::vector<uint8_t> okf((size_t)n);
    std::vector<uint32_t> vidx;
    for (int64_t k = 0; k < n; ++k) {
        double b[3];
        okf[k] = tri_bearing<CM>(in, uv[2 * k], uv[2 * k + 1], b) ? 1 : 0;
        bear[3 * k] = b[0]; bear[3 * k + 1] = b[1]; bear[3 * k + 2] = b[2];
        if (okf[k]) vidx.push_back((uint32_t)k);
    }
    const int64_t nv = (int64_t)vidx.size();
    if (nv <= kP3PSample) return true;
    vidx.resize((size_t)n);
    for (int64_t j = 0; j <= n; ++j) L[j] = j == 0 ? 0.0 : det_log10((double)j);
    std::vector<float> logc_n((size_t)n + 1), logc_k((size_t)n + 1);
    for (int64_t k = 0; k <= n; ++k) {
        double r = 0.0;
        int64_t kk = k;
        if (!(kk >= n || kk <= 0)) {
            if (n - kk < kk) kk = n - kk;
            for (int64_t i = 1; i <= kk; ++i) r = r + (L[n - i + 1] - L[i]);
        }
        logc_n[k] = (float)r;
        double r3 = 0.0;
        int64_t k3 = kP3PSample;
        if (!(k3 >= k || k3 <= 0)) {
            if (k - k3 < k3) k3 = k - k3;
            for (int64_t i = 1; i <= k3; ++i) r3 = r3 + (L[k - i + 1] - L[i]);
        }
        logc_k[k] = (float)r3;
    }
    bool ac = false;
    double minNFA = resect_inf(), errorMax = resect_inf(), best[12] = {};
    int64_t nIterReserve = O.max_iterations / 10, nIter = O.max_iterations - nIterReserve, vsize = nv, ninl = 0;
    Stream rs{rng.data(), 0, (int64_t)rng.size()};
    std::vector<std::pair<unsigned long long, uint32_t>> srt;
    auto err = [&](const double* M, int64_t k) {
        return okf[k] ? resect_error<CM>(M, in, X + 3 * k, uv[2 * k], uv[2 * k + 1]) : resect_inf();
    };
    int64_t iter = 0;
    for (iter = 0; iter < nIter; ++iter) {
        uint32_t sample[kP3PSample];
        if (ac) {
            for (int i = 0; i < kP3PSample; ++i) {
                const uint32_t d = rs.uniform((uint32_t)i, (uint32_t)(vsize - 1));
                std::swap(vidx[i], vidx[d]);
                sample[i] = vidx[i];
            }
        } else {
            int ns = 0;
            while (ns < kP3PSample && !rs.over) {
                const uint32_t sm = vidx[rs.uniform(0u, (uint32_t)(nv - 1))];
                bool found = false;
                for (int j = 0; j < ns && !found; ++j) found = sample[j] == sm;
                if (!found) sample[ns++] = sm;
            }
        }
        if (rs.over) return false;
        bool upd = false;
        double sb[9], sX[9], models[kP3PMaxModels * 12], roots[4];
        for (int i = 0; i < kP3PSample; ++i)
            for (int j = 0; j < 3; ++j) {
                sb[3 * i + j] = bear[3 * (size_t)sample[i] + j];
                sX[3 * i + j] = X[3 * (size_t)sample[i] + j];
            }
        const int nm = p3p_solve(sb, sX, models, roots);
        for (int mi = 0; mi < nm; ++mi) {
            const double* M = models + 12 * mi;
            if (!ac) {
                int64_t c = 0;
                for (int64_t k = 0; k < n; ++k) c += err(M, k) <= maxThr;
                if ((double)c > 2.5 * kP3PSample) ac = true;
                if (!ac) continue;
            }
            srt.clear();
            for (int64_t k = 0; k < n; ++k) {
                const double e = err(M, k);
                if (e <= maxThr) srt.emplace_back(err_key(e), (uint32_t)k);
            }
            std::sort(srt.begin(), srt.end());
            const int64_t m = (int64_t)srt.size();
            double bn = resect_inf();
            int64_t bk = kP3PSample;
            for (int64_t k = kP3PSample + 1; k <= m; ++k) {
                const double nfa = resect_nfa(loge0, logalpha0, key_err(srt[k - 1].first), k, logc_n[k], logc_k[k]);
                if (nfa < bn) { bn = nfa; bk = k; }
            }
            if (bn < minNFA) {
                upd = true;
                minNFA = bn;
                ninl = bk;
                errorMax = key_err(srt[bk - 1].first);
                std::memcpy(best, M, sizeof best);
                for (int64_t k = 0; k < ninl; ++k) binl[k] = srt[k].second;
            }
        }
        if ((upd && minNFA < 0) || (iter + 1 == nIter && nIterReserve)) {
            if (ninl == 0) {
                nIter++;
                nIterReserve--;
            } else {
                for (int64_t k = 0; k < ninl; ++k) vidx[k] = binl[k];
                vsize = ninl;
                if (nIterReserve) {
                    nIter = iter + 1 + nIterReserve;
                    nIterReserve = 0;
                }
            }
        }
    }
    const bool keep = minNFA < 0 && ninl > 2 * kP3PSample + 1;
    st[0] = minNFA;
    st[1] = keep ? errorMax : 0.0;
    st[2] = keep ? (double)ninl : 0.0;
    st[3] = (double)iter;
    st[4] = (double)(keep ? SFM_RESECT_OK : SFM_RESECT_NO_MODEL);
    if (!keep) return true;
    std::memcpy(Mo, best, sizeof best);
    double Rt[12];
    std::memcpy(Rt, best, sizeof best);
    bool fitted = true;
    for (int it = 0; it < O.refine_iterations; ++it) {
        double S[27] = {}, H[42], d[6];
        for (int64_t t = 0; t < ninl; ++t) {
            const size_t k = binl[t];
            resect_normal_terms<CM>(Rt, in, X + 3 * k, uv[2 * k], uv[2 * k + 1], S);
        }
        if (!(resect_solve6(S, H, d) && resect_apply(Rt, d))) {
            fitted = false;
            break;
        }
        double n2 = 0.0;
        for (int z = 0; z < 6; ++z) n2 = n2 + d[z] * d[z];
        if (n2 < 1e-24) break;
    }
    std::memcpy(Mo + 12, fitted ? Rt : best, sizeof best);
    return true;
}

}  // namespace

extern "C" int sfm_resect_host(int32_t camera_model, int64_t n_img, const int64_t* off, const double* X,
                               const double* uv, const int32_t* img_intr, const double* intr, int32_t n_intr,
                               const int32_t* wh, const sfm_resect_opts* opts, sfm_resect_result* results,
                               int32_t* inliers) {
    return guarded([&] {
        const Checked c = check_args("sfm_resect_host", camera_model, n_img, off, X, uv, img_intr, intr, n_intr, wh,
                                     opts, results, inliers);
        if (n_img == 0) return SFM_OK;
        const int iw = sfm_ba_intr_width(camera_model);
        const auto& rng = rng_stream();
        std::vector<double> model(24 * (size_t)n_img), stat(6 * (size_t)n_img);
        std::vector<uint32_t> binl((size_t)std::max<int64_t>(c.n, 1));
        bool ok = true;
        for (int64_t q = 0; q < n_img; ++q) {
            const int64_t o0 = off[q], n = off[q + 1] - o0;
            const double* in = intr + (int64_t)iw * img_intr[q];
            auto run = [&](auto cm) {
                return host_image<decltype(cm)::value>(n, X + 3 * o0, uv + 2 * o0, in, &c.cst[4 * q], c.o, rng,
                                                       &model[24 * q], &stat[6 * q], binl.data() + o0);
            };
            if (camera_model == SFM_CAM_RADIAL3) ok = run(std::integral_constant<int, SFM_CAM_RADIAL3>{}) && ok;
            else if (camera_model == SFM_CAM_SNAVELY) ok = run(std::integral_constant<int, SFM_CAM_SNAVELY>{}) && ok;
            else ok = run(std::integral_constant<int, SFM_CAM_PINHOLE>{}) && ok;
        }
        SFM_REQUIRE(ok, SFM_ERR_UNSUPPORTED, "sfm_resect_host: an image drew more than %lld random numbers",
                    (long long)kRngWords);
        write_results(n_img, off, model.data(), stat.data(), binl.data(), results, inliers);
        return SFM_OK;
    });
}

extern "C" int sfm_resect_p3p(const double b[9], const double X[9], double Rt[4][12], int32_t* n) {
    return guarded([&] {
        SFM_REQUIRE(b && X && Rt && n, SFM_ERR_INVALID_ARG, "sfm_resect_p3p: null argument");
        double roots[4];
        *n = p3p_solve(b, X, &Rt[0][0], roots);
        return SFM_OK;
    });
}

extern "C" int sfm_resect_gather(const sfm_ba_problem* prob, const double* X, const uint8_t* pt_ok,
                                 const int32_t* images, int32_t n_images, int64_t* off, double* X3, double* uv) {
    return guarded([&] {
        SFM_REQUIRE(prob && pt_ok && off && n_images >= 0 && (n_images == 0 || images), SFM_ERR_INVALID_ARG,
                    "sfm_resect_gather: null argument");
        SFM_REQUIRE((X3 == nullptr) == (uv == nullptr) && (!X3 || X), SFM_ERR_INVALID_ARG,
                    "sfm_resect_gather: X3 and uv go together, and need X");
        SFM_REQUIRE(prob->n_img >= 0 && prob->n_pt >= 0 && prob->n_obs >= 0 &&
                        (prob->n_pt == 0 || prob->pt_offsets) && (prob->n_obs == 0 || (prob->obs_img && prob->obs_uv)),
                    SFM_ERR_INVALID_ARG, "sfm_resect_gather: incomplete problem");
        std::vector<int32_t> slot((size_t)std::max<int32_t>(prob->n_img, 1), -1);
        for (int32_t q = 0; q < n_images; ++q) {
            SFM_REQUIRE(images[q] >= 0 && images[q] < prob->n_img && slot[images[q]] < 0, SFM_ERR_INVALID_ARG,
                        "sfm_resect_gather: image %d is out of range or listed twice", images[q]);
            slot[images[q]] = q;
        }
        for (int32_t q = 0; q <= n_images; ++q) off[q] = 0;
        for (int pass = 0; pass < (X3 ? 2 : 1); ++pass) {
            std::vector<int64_t> at(off, off + n_images);   // (second pass: where each image's next one goes)
            for (int64_t p = 0; p < prob->n_pt; ++p) {
                if (!pt_ok[p]) continue;
                for (int64_t o = prob->pt_offsets[p]; o < prob->pt_offsets[p + 1]; ++o) {
                    const int32_t im = prob->obs_img[o];
                    SFM_REQUIRE(im >= 0 && im < prob->n_img, SFM_ERR_INVALID_ARG,
                                "sfm_resect_gather: observation %lld names image %d", (long long)o, im);
                    const int32_t q = slot[im];
                    if (q < 0) continue;
                    if (pass == 0) {
                        ++off[q + 1];
                    } else {
                        const int64_t k = at[q]++;
                        for (int a = 0; a < 3; ++a) X3[3 * k + a] = X[3 * p + a];
                        uv[2 * k] = prob->obs_uv[2 * o];
                        uv[2 * k + 1] = prob->obs_uv[2 * o + 1];
                    }
                }
            }
            if (pass == 0)
                for (int32_t q = 0; q < n_images; ++q) off[q + 1] += off[q];
        }
        return SFM_OK;
    });
}

#ifndef SFM_RESECT_HOST_ONLY
extern "C" int sfm_resect(sfm_ctx* ctx, int32_t camera_model, int64_t n_img, const int64_t* off, const double* X,
                          const double* uv, const int32_t* img_intr, const double* intr, int32_t n_intr,
                          const int32_t* wh, const sfm_resect_opts* opts, sfm_resect_result* results,
                          int32_t* inliers) {
    return guarded([&] {
        SFM_REQUIRE(ctx, SFM_ERR_INVALID_ARG, "sfm_resect: null context");
        const Checked c = check_args("sfm_resect", camera_model, n_img, off, X, uv, img_intr, intr, n_intr, wh, opts,
                                     results, inliers);
        if (n_img == 0) return SFM_OK;
        const int iw = sfm_ba_intr_width(camera_model);
        const int64_t n = c.n;
        const size_t n1 = (size_t)std::max<int64_t>(n, 1);
        CtxScope scope_(ctx);
        hipStream_t s = ctx->stream;
        PhaseTimer tm("sfm_resect");
        DBuf<int64_t> d_off, d_goff;
        DBuf<double> d_X, d_uv, d_intr, d_cst, d_bear, d_ltab, d_model, d_stat;
        DBuf<int32_t> d_img_intr, d_fail;
        DBuf<float> d_logc;
        DBuf<uint8_t> d_ok;
        DBuf<uint32_t> d_rng, d_vidx, d_binl, d_gval;
        DBuf<unsigned long long> d_gkey;
        d_off.alloc(n_img + 1); d_off.upload(off, n_img + 1, s);
        d_X.alloc(3 * n1); d_X.upload(X, 3 * (size_t)n, s);
        d_uv.alloc(2 * n1); d_uv.upload(uv, 2 * (size_t)n, s);
        d_img_intr.alloc(n_img); d_img_intr.upload(img_intr, n_img, s);
        d_intr.alloc((size_t)iw * n_intr); d_intr.upload(intr, (size_t)iw * n_intr, s);
        d_cst.alloc(c.cst.size()); d_cst.upload(c.cst.data(), c.cst.size(), s);
        const auto& rw = rng_stream();
        d_rng.alloc(rw.size()); d_rng.upload(rw.data(), rw.size(), s);
        d_bear.alloc(3 * n1);
        d_ok.alloc(n1);
        d_ltab.alloc((size_t)(n + n_img));
        d_logc.alloc(2 * (size_t)(n + n_img));
        d_vidx.alloc(n1);
        d_binl.alloc(n1);
        d_model.alloc(24 * (size_t)n_img);
        d_stat.alloc(6 * (size_t)n_img);
        d_fail.alloc(1);
        d_fail.zero(s);
        // sort buffers per image: next_pow2(n) slots, in LDS up to
        // kResectMaxLdsSort; only the images above that get global buffers,
        // packed by prefix sum
        std::vector<int64_t> goff((size_t)n_img, -1);
        int64_t lds_slots = 1, g_slots = 0;
        for (int64_t q = 0; q < n_img; ++q) {
            int64_t sl = 1;
            while (sl < off[q + 1] - off[q]) sl <<= 1;
            if (sl <= kResectMaxLdsSort) {
                lds_slots = std::max(lds_slots, sl);
            } else {
                goff[q] = g_slots;
                g_slots += sl;
            }
        }
        d_goff.alloc(goff.size()); d_goff.upload(goff.data(), goff.size(), s);
        if (g_slots) {
            d_gkey.alloc((size_t)g_slots);
            d_gval.alloc((size_t)g_slots);
        }
        ResectArgs a{};
        a.off = d_off.p; a.X = d_X.p; a.uv = d_uv.p; a.img_intr = d_img_intr.p; a.intr = d_intr.p; a.iw = iw;
        a.cst = d_cst.p; a.rng = d_rng.p; a.rng_n = (int64_t)rw.size();
        a.bear = d_bear.p; a.ok = d_ok.p; a.ltab = d_ltab.p; a.logc = d_logc.p; a.vidx = d_vidx.p; a.binl = d_binl.p;
        a.gkey = d_gkey.p; a.gval = d_gval.p; a.goff = d_goff.p; a.model = d_model.p; a.stat = d_stat.p;
        a.fail = d_fail.p; a.max_iter = c.o.max_iterations; a.refine_iter = c.o.refine_iterations;
        a.lds_slots = (int32_t)lds_slots;
        // the kernel alone (sfm_ctx_last_kernel_ms, SFM_CTX_TIME_KERNELS only):
        // the uploads are drained first
        const bool timed = ctx->time_kernels;
        hipEvent_t* ev = timed ? ctx_events(ctx) : nullptr;
        if (timed) {
            SFM_HIP(hipStreamSynchronize(s));
            SFM_HIP(hipEventRecord(ev[0], s));
        }
        tm.mark("upload");
        resect_launch(a, camera_model, n_img, s);
        if (timed) SFM_HIP(hipEventRecord(ev[1], s));
        std::vector<double> model(24 * (size_t)n_img), stat(6 * (size_t)n_img);
        std::vector<uint32_t> binl(n1);
        int32_t fail = 0;
        SFM_HIP(hipMemcpyAsync(model.data(), d_model.p, model.size() * 8, hipMemcpyDeviceToHost, s));
        SFM_HIP(hipMemcpyAsync(stat.data(), d_stat.p, stat.size() * 8, hipMemcpyDeviceToHost, s));
        if (n) SFM_HIP(hipMemcpyAsync(binl.data(), d_binl.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
        SFM_HIP(hipMemcpyAsync(&fail, d_fail.p, 4, hipMemcpyDeviceToHost, s));
        SFM_HIP(hipStreamSynchronize(s));
        ctx->last_kernel_ms = -1.0;
        if (timed) {
            float ms = 0.f;
            SFM_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
            ctx->last_kernel_ms = ms;
        }
        tm.mark("kernel+download");
        SFM_REQUIRE(!fail, SFM_ERR_UNSUPPORTED, "sfm_resect: an image drew more than %lld random numbers",
                    (long long)kRngWords);
        write_results(n_img, off, model.data(), stat.data(), binl.data(), results, inliers);
        return SFM_OK;
    });
}
#endif
