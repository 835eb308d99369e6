// Relative pose, host side (include/sfmcore.h, "Relative pose"): the options,
// the argument checks and a-contrario constants both entry points share, the
// serial host twin (sfm_relpose_host: relpose.hip's kernel restated for one
// thread over the same relpose_pose.h statements), the minimal solver as a
// [cpu] call, and the device entry point (sfm_relpose: uploads, one launch,
// downloads).  The rotation becomes an angle-axis vector here, on the host,
// for both paths.
// SFM_RELPOSE_HOST_ONLY leaves the device entry point out, so that the host
// path builds with a plain host compiler (tests/cpp/relpose_test.cpp).
#pragma clang fp contract(off)

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "common.h"
#include "relpose.h"
#include "relpose_pose.h"
#include "rot_aa.h"

using namespace sfm;

extern "C" void sfm_relpose_default_options(sfm_relpose_opts* o) {
    if (!o) return;
    // robustRelativePose as the incremental engine's initial-pair search calls
    // it: 4 px upper bound, 4096 iterations; RelativePoseFromEssential's ratio
    o->precision = 4.0;
    o->max_iterations = 4096;
    o->reserved = 0;
    o->front_ratio = 0.7;
}

namespace {

struct Checked {
    sfm_relpose_opts o;
    int64_t n = 0;
    std::vector<double> cst;   // [n_pairs][4] logalpha0, the bound on the squared error, loge0, 0
};

Checked check_args(const char* who, int32_t cm, int64_t n_pairs, const int64_t* off, const double* xy,
                   const int32_t* pair_intr, const double* intr, int32_t n_intr, const int32_t* wh,
                   const sfm_relpose_opts* opts, const sfm_relpose_result* results, const int32_t* inliers) {
    Checked c;
    if (opts) c.o = *opts; else sfm_relpose_default_options(&c.o);
    SFM_REQUIRE(sfm_ba_intr_width(cm) > 0, SFM_ERR_INVALID_ARG, "%s: unknown camera_model %d", who, cm);
    SFM_REQUIRE(n_pairs >= 0 && n_intr >= 0, SFM_ERR_INVALID_ARG, "%s: negative count", who);
    SFM_REQUIRE(c.o.max_iterations >= 1 && c.o.precision == c.o.precision && c.o.front_ratio == c.o.front_ratio,
                SFM_ERR_INVALID_ARG, "%s: bad options", who);
    if (n_pairs == 0) return c;
    SFM_REQUIRE(off && pair_intr && wh && results, SFM_ERR_INVALID_ARG, "%s: null argument", who);
    SFM_REQUIRE(off[0] == 0, SFM_ERR_INVALID_ARG, "%s: off[0] must be 0", who);
    SFM_REQUIRE(n_pairs < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED, "%s: too many pairs", who);
    for (int64_t q = 0; q < n_pairs; ++q) {
        SFM_REQUIRE(off[q + 1] >= off[q], SFM_ERR_INVALID_ARG, "%s: off not monotone at %lld", who, (long long)q);
        for (int s = 0; s < 2; ++s) {
            SFM_REQUIRE(pair_intr[2 * q + s] >= 0 && pair_intr[2 * q + s] < n_intr, SFM_ERR_INVALID_ARG,
                        "%s: pair %lld names intrinsics block %d of %d", who, (long long)q, pair_intr[2 * q + s], n_intr);
            SFM_REQUIRE(wh[4 * q + 2 * s] > 0 && wh[4 * q + 2 * s + 1] > 0, SFM_ERR_INVALID_ARG,
                        "%s: pair %lld has a non-positive image size", who, (long long)q);
        }
    }
    c.n = off[n_pairs];
    SFM_REQUIRE(c.n < ((int64_t)1 << 31), SFM_ERR_UNSUPPORTED, "%s: too many correspondences", who);
    SFM_REQUIRE(intr && (c.n == 0 || (xy && inliers)), SFM_ERR_INVALID_ARG, "%s: null argument", who);
    const bool bounded = c.o.precision > 0.0 && c.o.precision <= 1.7976931348623157e308;
    c.cst.resize(4 * (size_t)n_pairs);
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int64_t np = off[q + 1] - off[q];
        const double w = (double)wh[4 * q + 2], h = (double)wh[4 * q + 3];
        c.cst[4 * q] = det_log10(2.0 * std::sqrt(w * w + h * h) / (w * h));
        c.cst[4 * q + 1] = bounded ? c.o.precision * c.o.precision : 1.7976931348623157e308;
        c.cst[4 * q + 2] = det_log10((double)kE5MaxModels * (double)(np > kE5Sample ? np - kE5Sample : 1));
        c.cst[4 * q + 3] = 0.0;
    }
    return c;
}

// results[] and inliers[] from what either path left per pair: model[21] (E,
// the winning motion's R and t), stat[8] and the pair's binl
void write_results(int64_t n_pairs, const int64_t* off, const double* model, const double* stat,
                   const uint32_t* binl, sfm_relpose_result* results, int32_t* inliers) {
    for (int64_t q = 0; q < n_pairs; ++q) {
        sfm_relpose_result& r = results[q];
        std::memset(&r, 0, sizeof r);
        const double* s = stat + 8 * q;
        r.status = (int32_t)s[4];
        r.iterations = (int32_t)s[3];
        if (r.status == SFM_RELPOSE_FEW) continue;
        r.min_nfa = s[0];
        if (r.status == SFM_RELPOSE_NO_MODEL) continue;
        r.error_max = std::sqrt(s[1]);
        r.n_inliers = (int32_t)s[2];
        const double* M = model + 21 * q;
        for (int a = 0; a < 9; ++a) r.E[a] = M[a];
        for (int64_t k = 0; k < r.n_inliers; ++k) inliers[off[q] + k] = (int32_t)binl[off[q] + k];
        if (r.status != SFM_RELPOSE_OK) continue;
        matrix_to_aa(M + 9, r.pose);
        for (int a = 0; a < 3; ++a) r.pose[3 + a] = M[18 + a];
        r.n_front = (int32_t)s[5];
        r.angle_median = s[6];
    }
}

// One pair, serially: relpose.hip's kernel for one thread.  False when the
// random stream ran out.
template <int CM>
bool host_pair(int64_t n, const double* xy, const double* inI, const double* inJ, const double* cst,
               const sfm_relpose_opts& O, const std::vector<uint32_t>& rng, double* Mo, double* st, uint32_t* binl) {
    std::fill(Mo, Mo + 21, 0.0);
    std::fill(st, st + 8, 0.0);
    st[4] = (double)SFM_RELPOSE_FEW;
    if (n <= kE5Sample) return true;
    const double logalpha0 = cst[0], maxThr = cst[1], loge0 = cst[2];
    std::vector<double> bear(6 * (size_t)n), L((size_t)n + 1);
    std::vector<uint8_t> okf((size_t)n);
    std::vector<uint32_t> vidx;
    for (int64_t k = 0; k < n; ++k) {
        double bi[3], bj[3];
        const bool oi = tri_bearing<CM>(inI, xy[4 * k], xy[4 * k + 1], bi);
        const bool oj = tri_bearing<CM>(inJ, xy[4 * k + 2], xy[4 * k + 3], bj);
        for (int j = 0; j < 3; ++j) {
            bear[6 * k + j] = bi[j];
            bear[6 * k + 3 + j] = bj[j];
        }
        okf[k] = oi && oj ? 1 : 0;
        if (okf[k]) vidx.push_back((uint32_t)k);
    }
    const int64_t nv = (int64_t)vidx.size();
    if (nv <= kE5Sample) return true;
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
        double r5 = 0.0;
        int64_t k5 = kE5Sample;
        if (!(k5 >= k || k5 <= 0)) {
            if (k - k5 < k5) k5 = k - k5;
            for (int64_t i = 1; i <= k5; ++i) r5 = r5 + (L[k - i + 1] - L[i]);
        }
        logc_k[k] = (float)r5;
    }
    bool ac = false;
    double minNFA = relpose_inf(), errorMax = relpose_inf(), best[9] = {};
    int64_t nIterReserve = O.max_iterations / 10, nIter = O.max_iterations - nIterReserve, vsize = nv, ninl = 0;
    Stream rs{rng.data(), 0, (int64_t)rng.size()};
    std::vector<std::pair<unsigned long long, uint32_t>> srt;
    auto err = [&](const double* M, int64_t k) {
        return okf[k] ? relpose_error<CM>(M, inJ, &bear[6 * k], &bear[6 * k + 3]) : relpose_inf();
    };
    E5Work work;
    int64_t iter = 0;
    for (iter = 0; iter < nIter; ++iter) {
        uint32_t sample[kE5Sample];
        if (ac) {
            for (int i = 0; i < kE5Sample; ++i) {
                const uint32_t d = rs.uniform((uint32_t)i, (uint32_t)(vsize - 1));
                std::swap(vidx[i], vidx[d]);
                sample[i] = vidx[i];
            }
        } else {
            int ns = 0;
            while (ns < kE5Sample && !rs.over) {
                const uint32_t sm = vidx[rs.uniform(0u, (uint32_t)(nv - 1))];
                bool found = false;
                for (int j = 0; j < ns && !found; ++j) found = sample[j] == sm;
                if (!found) sample[ns++] = sm;
            }
        }
        if (rs.over) return false;
        bool upd = false;
        double sI[15], sJ[15], models[kE5MaxModels * 9];
        for (int i = 0; i < kE5Sample; ++i)
            for (int j = 0; j < 3; ++j) {
                sI[3 * i + j] = bear[6 * (size_t)sample[i] + j];
                sJ[3 * i + j] = bear[6 * (size_t)sample[i] + 3 + j];
            }
        const int nm = e5_solve(sI, sJ, models, work);
        for (int mi = 0; mi < nm; ++mi) {
            const double* M = models + 9 * mi;
            if (!ac) {
                int64_t c = 0;
                for (int64_t k = 0; k < n; ++k) c += err(M, k) <= maxThr;
                if ((double)c > 2.5 * kE5Sample) ac = true;
                if (!ac) continue;
            }
            srt.clear();
            for (int64_t k = 0; k < n; ++k) {
                const double e = err(M, k);
                if (e <= maxThr) srt.emplace_back(err_key(e), (uint32_t)k);
            }
            std::sort(srt.begin(), srt.end());
            const int64_t m = (int64_t)srt.size();
            double bn = relpose_inf();
            int64_t bk = kE5Sample;
            for (int64_t k = kE5Sample + 1; k <= m; ++k) {
                const double nfa = relpose_nfa(loge0, logalpha0, key_err(srt[k - 1].first), k, logc_n[k], logc_k[k]);
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
    const bool keep = minNFA < 0 && ninl > 2 * kE5Sample + 2;
    st[0] = minNFA;
    st[1] = keep ? errorMax : 0.0;
    st[2] = keep ? (double)ninl : 0.0;
    st[3] = (double)iter;
    st[4] = (double)(keep ? SFM_RELPOSE_AMBIGUOUS : SFM_RELPOSE_NO_MODEL);
    if (!keep) return true;
    std::memcpy(Mo, best, sizeof best);
    double Ra[9], Rb[9], t[3];
    if (!relpose_motions(best, Ra, Rb, t)) return true;
    int64_t cnt[4] = {0, 0, 0, 0};
    std::vector<uint32_t> mask((size_t)ninl);
    for (int64_t i = 0; i < ninl; ++i) {
        const size_t k = binl[i];
        mask[i] = relpose_front_mask<CM>(Ra, Rb, t, &bear[6 * k], &bear[6 * k + 3]);
        for (int m = 0; m < 4; ++m) cnt[m] += (mask[i] >> m) & 1u;
    }
    const int win = relpose_vote(cnt, O.front_ratio);
    if (win < 0) return true;
    const double* R = win < 2 ? Ra : Rb;
    srt.clear();
    for (int64_t i = 0; i < ninl; ++i) {
        if (!((mask[i] >> win) & 1u)) continue;
        const size_t k = binl[i];
        srt.emplace_back(err_key(relpose_angle_key(R, &bear[6 * k], &bear[6 * k + 3])), (uint32_t)k);
    }
    std::sort(srt.begin(), srt.end());
    const size_t km = srt[srt.size() / 2].second;
    st[4] = (double)SFM_RELPOSE_OK;
    st[5] = (double)cnt[win];
    st[6] = relpose_angle_deg(R, &bear[6 * km], &bear[6 * km + 3]);
    for (int a = 0; a < 9; ++a) Mo[9 + a] = R[a];
    for (int a = 0; a < 3; ++a) Mo[18 + a] = (win & 1) ? -t[a] : t[a];
    return true;
}

}  // namespace

extern "C" int sfm_relpose_host(int32_t camera_model, int64_t n_pairs, const int64_t* off, const double* xy,
                                const int32_t* pair_intr, const double* intr, int32_t n_intr, const int32_t* wh,
                                const sfm_relpose_opts* opts, sfm_relpose_result* results, int32_t* inliers) {
    return guarded([&] {
        const Checked c = check_args("sfm_relpose_host", camera_model, n_pairs, off, xy, pair_intr, intr, n_intr, wh,
                                     opts, results, inliers);
        if (n_pairs == 0) return SFM_OK;
        const int iw = sfm_ba_intr_width(camera_model);
        const auto& rng = rng_stream();
        std::vector<double> model(21 * (size_t)n_pairs), stat(8 * (size_t)n_pairs);
        std::vector<uint32_t> binl((size_t)std::max<int64_t>(c.n, 1));
        bool ok = true;
        for (int64_t q = 0; q < n_pairs; ++q) {
            const int64_t o0 = off[q], n = off[q + 1] - o0;
            const double* inI = intr + (int64_t)iw * pair_intr[2 * q];
            const double* inJ = intr + (int64_t)iw * pair_intr[2 * q + 1];
            auto run = [&](auto cm) {
                return host_pair<decltype(cm)::value>(n, xy + 4 * o0, inI, inJ, &c.cst[4 * q], c.o, rng, &model[21 * q],
                                                      &stat[8 * q], binl.data() + o0);
            };
            if (camera_model == SFM_CAM_RADIAL3) ok = run(std::integral_constant<int, SFM_CAM_RADIAL3>{}) && ok;
            else if (camera_model == SFM_CAM_SNAVELY) ok = run(std::integral_constant<int, SFM_CAM_SNAVELY>{}) && ok;
            else ok = run(std::integral_constant<int, SFM_CAM_PINHOLE>{}) && ok;
        }
        SFM_REQUIRE(ok, SFM_ERR_UNSUPPORTED, "sfm_relpose_host: a pair drew more than %lld random numbers",
                    (long long)kRngWords);
        write_results(n_pairs, off, model.data(), stat.data(), binl.data(), results, inliers);
        return SFM_OK;
    });
}

extern "C" int sfm_relpose_5pt(const double bI[15], const double bJ[15], double E[10][9], int32_t* n) {
    return guarded([&] {
        SFM_REQUIRE(bI && bJ && E && n, SFM_ERR_INVALID_ARG, "sfm_relpose_5pt: null argument");
        E5Work work;
        *n = e5_solve(bI, bJ, &E[0][0], work);
        return SFM_OK;
    });
}

#ifndef SFM_RELPOSE_HOST_ONLY
extern "C" int sfm_relpose(sfm_ctx* ctx, int32_t camera_model, int64_t n_pairs, const int64_t* off, const double* xy,
                           const int32_t* pair_intr, const double* intr, int32_t n_intr, const int32_t* wh,
                           const sfm_relpose_opts* opts, sfm_relpose_result* results, int32_t* inliers) {
    return guarded([&] {
        SFM_REQUIRE(ctx, SFM_ERR_INVALID_ARG, "sfm_relpose: null context");
        const Checked c = check_args("sfm_relpose", camera_model, n_pairs, off, xy, pair_intr, intr, n_intr, wh, opts,
                                     results, inliers);
        if (n_pairs == 0) return SFM_OK;
        const int iw = sfm_ba_intr_width(camera_model);
        const int64_t n = c.n;
        const size_t n1 = (size_t)std::max<int64_t>(n, 1);
        CtxScope scope_(ctx);
        hipStream_t s = ctx->stream;
        PhaseTimer tm("sfm_relpose");
        DBuf<int64_t> d_off, d_goff;
        DBuf<double> d_xy, d_intr, d_cst, d_bear, d_ltab, d_model, d_stat;
        DBuf<int32_t> d_pair_intr, d_fail;
        DBuf<float> d_logc;
        DBuf<uint8_t> d_ok;
        DBuf<uint32_t> d_rng, d_vidx, d_binl, d_gval;
        DBuf<unsigned long long> d_gkey;
        d_off.alloc(n_pairs + 1); d_off.upload(off, n_pairs + 1, s);
        d_xy.alloc(4 * n1); d_xy.upload(xy, 4 * (size_t)n, s);
        d_pair_intr.alloc(2 * n_pairs); d_pair_intr.upload(pair_intr, 2 * n_pairs, s);
        d_intr.alloc((size_t)iw * n_intr); d_intr.upload(intr, (size_t)iw * n_intr, s);
        d_cst.alloc(c.cst.size()); d_cst.upload(c.cst.data(), c.cst.size(), s);
        const auto& rw = rng_stream();
        d_rng.alloc(rw.size()); d_rng.upload(rw.data(), rw.size(), s);
        d_bear.alloc(6 * n1);
        d_ok.alloc(n1);
        d_ltab.alloc((size_t)(n + n_pairs));
        d_logc.alloc(2 * (size_t)(n + n_pairs));
        d_vidx.alloc(n1);
        d_binl.alloc(n1);
        d_model.alloc(21 * (size_t)n_pairs);
        d_stat.alloc(8 * (size_t)n_pairs);
        d_fail.alloc(1);
        d_fail.zero(s);
        // sort buffers per pair: next_pow2(n) slots, in LDS up to
        // kRelposeMaxLdsSort; only the pairs above that get global buffers,
        // packed by prefix sum
        std::vector<int64_t> goff((size_t)n_pairs, -1);
        int64_t lds_slots = 1, g_slots = 0;
        for (int64_t q = 0; q < n_pairs; ++q) {
            int64_t sl = 1;
            while (sl < off[q + 1] - off[q]) sl <<= 1;
            if (sl <= kRelposeMaxLdsSort) {
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
        RelposeArgs a{};
        a.off = d_off.p; a.xy = d_xy.p; a.pair_intr = d_pair_intr.p; a.intr = d_intr.p; a.iw = iw;
        a.cst = d_cst.p; a.rng = d_rng.p; a.rng_n = (int64_t)rw.size();
        a.bear = d_bear.p; a.ok = d_ok.p; a.ltab = d_ltab.p; a.logc = d_logc.p; a.vidx = d_vidx.p; a.binl = d_binl.p;
        a.gkey = d_gkey.p; a.gval = d_gval.p; a.goff = d_goff.p; a.model = d_model.p; a.stat = d_stat.p;
        a.fail = d_fail.p; a.max_iter = c.o.max_iterations; a.front_ratio = c.o.front_ratio;
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
        relpose_launch(a, camera_model, n_pairs, s);
        if (timed) SFM_HIP(hipEventRecord(ev[1], s));
        std::vector<double> model(21 * (size_t)n_pairs), stat(8 * (size_t)n_pairs);
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
        SFM_REQUIRE(!fail, SFM_ERR_UNSUPPORTED, "sfm_relpose: a pair drew more than %lld random numbers",
                    (long long)kRngWords);
        write_results(n_pairs, off, model.data(), stat.data(), binl.data(), results, inliers);
        return SFM_OK;
    });
}
#endif
