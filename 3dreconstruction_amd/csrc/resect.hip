// Camera resection on gfx950 (include/sfmcore.h, "Camera resection"; DESIGN.md
// §5e): OpenMVG's a-contrario RANSAC over a P3P solver and the Gauss-Newton
// refit of the pose on its inliers, one independent problem per image.
//
// Layout and work split, as the F-matrix filter's (fmat.hip): one 256-thread
// workgroup per image.  The sampling and the P3P solve are a short serial
// chain (lane 0); every model's error pass, the compaction of the errors
// under the bound, their (error, index) bitonic sort in LDS (global memory
// above 8192 slots) and the NFA scan over the sorted prefix are spread over
// the 256 threads.  The refit runs in the same launch: each thread sums the
// 21 + 6 normal-equation terms of its inliers, the sums are reduced in a fixed
// order (shuffles within a wave, then the waves in index order through LDS),
// lane 0 solves the 6x6 system and updates the pose.  No floating-point
// atomics, no wait on another workgroup: two runs give the same bits.
//
// The arithmetic is resect_pose.h, shared with the host twin (resect.cpp), and
// compiled without FMA contraction in both.
#pragma clang fp contract(off)
// 1 / depth by division, as the host's (track.h, depth_rcp): the search then
// computes the host twin's bits; only the order of the refit's sums differs
#define SFM_DEPTH_RCP_DIVIDES

#include <hip/hip_runtime.h>

#include "common.h"
#include "resect.h"
#include "resect_pose.h"

namespace sfm {
namespace {

constexpr int kRT = kResectThreads;
constexpr int kRW = kRT / 64;   // waves

template <int CM>
__global__ __launch_bounds__(kRT) void resect_ac_kernel(ResectArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t o0 = a.off[q], n = a.off[q + 1] - o0;
    double* Mo = a.model + 24 * (size_t)q;
    double* st = a.stat + 6 * (size_t)q;
    if (n <= kP3PSample) {
        if (tid < 24) Mo[tid] = 0.0;
        if (tid < 6) st[tid] = tid == 4 ? (double)SFM_RESECT_FEW : 0.0;
        return;
    }
    const double* X = a.X + 3 * o0;
    const double* uv = a.uv + 2 * o0;
    const double* in = a.intr + (int64_t)a.iw * a.img_intr[q];
    const double logalpha0 = a.cst[4 * q], maxThr = a.cst[4 * q + 1], loge0 = a.cst[4 * q + 2];
    double* bear = a.bear + 3 * o0;
    uint8_t* okf = a.ok + o0;
    double* L = a.ltab + o0 + q;                 // [n + 1]
    float* logc_n = a.logc + 2 * (o0 + q);       // [n + 1]
    float* logc_k = logc_n + (n + 1);            // [n + 1]
    uint32_t* vidx = a.vidx + o0;
    uint32_t* binl = a.binl + o0;
    const int64_t go = a.goff[q];
    const bool lds_sort = go < 0;
    unsigned long long* keys = lds_sort ? reinterpret_cast<unsigned long long*>(smem) : a.gkey + go;
    uint32_t* vals = lds_sort ? reinterpret_cast<uint32_t*>(smem + 8 * (size_t)a.lds_slots) : a.gval + go;

    __shared__ double s_models[kP3PMaxModels * 12], s_best[12], s_roots[4];
    __shared__ double s_red[kRW];
    __shared__ int s_redk[kRW];
    __shared__ int s_wc[kRW];
    __shared__ int s_nm, s_m, s_cnt, s_ac, s_upd, s_copy, s_stop;
    __shared__ uint32_t s_sample[kP3PSample];
    __shared__ int64_t s_nIter, s_nIterReserve, s_vsize, s_ninl;
    __shared__ double s_minNFA, s_errorMax;
    __shared__ double s_S[kRW][27], s_H[42], s_d[6], s_Rt[12];
    __shared__ int s_fit;

    // ---- prologue: bearings, log10 table, the sampling list, logcombi tables --
    for (int64_t k = tid; k < n; k += kRT) {
        double b[3];
        const bool ok = tri_bearing<CM>(in, uv[2 * k], uv[2 * k + 1], b);
        bear[3 * k] = b[0]; bear[3 * k + 1] = b[1]; bear[3 * k + 2] = b[2];
        okf[k] = ok ? 1 : 0;
    }
    for (int64_t j = tid; j <= n; j += kRT) L[j] = j == 0 ? 0.0 : det_log10((double)j);
    __syncthreads();
    // the correspondences with a bearing, in order (ballot prefix per wave,
    // the waves' counts through LDS)
    int64_t nv = 0;
    for (int64_t b0 = 0; b0 < n; b0 += kRT) {
        const int64_t k = b0 + tid;
        const bool f = k < n && okf[k] != 0;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) s_wc[wave] = __popcll(bal);
        __syncthreads();
        int64_t at = nv;
        for (int w = 0; w < kRW; ++w) {
            if (w < wave) at += s_wc[w];
            nv += s_wc[w];
        }
        if (f) vidx[at + __popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)k;
        __syncthreads();
    }
    if (nv <= kP3PSample) {   // (uniform)
        if (tid < 24) Mo[tid] = 0.0;
        if (tid < 6) st[tid] = tid == 4 ? (double)SFM_RESECT_FEW : 0.0;
        return;
    }
    for (int64_t k = tid; k <= n; k += kRT) {
        // logcombi(k, n) and logcombi(3, k): OpenMVG's loop, log10 from the table
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
    if (tid == 0) {
        s_ac = 0;
        s_minNFA = resect_inf();
        s_errorMax = resect_inf();
        s_nIterReserve = a.max_iter / 10;
        s_nIter = a.max_iter - s_nIterReserve;
        s_vsize = nv;
        s_ninl = 0;
        s_stop = 0;
    }
    if (tid < 12) s_best[tid] = 0.0;
    __syncthreads();
    Stream rs{a.rng, 0, a.rng_n};
    int64_t iter = 0;
    for (iter = 0; iter < s_nIter; ++iter) {
        // ---- sampling and the P3P solve (lane 0) ------------------------------
        if (tid == 0) {
            if (s_ac) {
                for (int i = 0; i < kP3PSample; ++i) {
                    const uint32_t d = rs.uniform((uint32_t)i, (uint32_t)(s_vsize - 1));
                    const uint32_t t = vidx[i];
                    vidx[i] = vidx[d];
                    vidx[d] = t;
                    s_sample[i] = vidx[i];
                }
            } else {
                int ns = 0;
                while (ns < kP3PSample && !rs.over) {
                    const uint32_t sm = vidx[rs.uniform(0u, (uint32_t)(nv - 1))];
                    bool found = false;
                    for (int j = 0; j < ns && !found; ++j) found = s_sample[j] == sm;
                    if (!found) s_sample[ns++] = sm;
                }
            }
            s_stop = rs.over ? 1 : 0;
            if (rs.over) a.fail[0] = 1;
            s_upd = 0;
            int nm = 0;
            if (!rs.over) {
                double sb[9], sX[9];
#pragma unroll
                for (int i = 0; i < kP3PSample; ++i) {
                    const size_t k = s_sample[i];
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        sb[3 * i + j] = bear[3 * k + j];
                        sX[3 * i + j] = X[3 * k + j];
                    }
                }
                nm = p3p_solve(sb, sX, s_models, s_roots);
            }
            s_nm = nm;
        }
        __syncthreads();
        if (s_stop) break;
        const int nm = s_nm;
        for (int mi = 0; mi < nm; ++mi) {
            double M[12];
#pragma unroll
            for (int z = 0; z < 12; ++z) M[z] = s_models[12 * mi + z];
            if (!s_ac) {   // does the model explain > 2.5 * 3 errors under the bound?
                int c = 0;
                for (int64_t k = tid; k < n; k += kRT) {
                    const double e = okf[k] ? resect_error<CM>(M, in, X + 3 * k, uv[2 * k], uv[2 * k + 1])
                                            : resect_inf();
                    c += e <= maxThr;
                }
                for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
                if (tid == 0) s_cnt = 0;
                __syncthreads();
                if (lane == 0) atomicAdd(&s_cnt, c);
                __syncthreads();
                if (tid == 0 && (double)s_cnt > 2.5 * kP3PSample) s_ac = 1;
                __syncthreads();
                if (!s_ac) continue;
            }
            // errors under the bound -> (error, index) keys
            if (tid == 0) s_m = 0;
            __syncthreads();
            for (int64_t k = tid; k < n; k += kRT) {
                const double e = okf[k] ? resect_error<CM>(M, in, X + 3 * k, uv[2 * k], uv[2 * k + 1])
                                        : resect_inf();
                if (e <= maxThr) {
                    const int slot = atomicAdd(&s_m, 1);
                    keys[slot] = err_key(e);
                    vals[slot] = (uint32_t)k;
                }
            }
            __syncthreads();
            const int m = s_m;
            int P2 = 1;
            while (P2 < m) P2 <<= 1;
            for (int k = m + tid; k < P2; k += kRT) {
                keys[k] = ~0ull;
                vals[k] = 0xFFFFFFFFu;
            }
            __syncthreads();
            // bitonic sort of (key, val) ascending
            for (int size = 2; size <= P2; size <<= 1) {
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int t = tid; t < P2 / 2; t += kRT) {
                        const int lo = 2 * t - (t & (stride - 1));
                        const int hi = lo + stride;
                        const bool asc = (lo & size) == 0;
                        const unsigned long long kl = keys[lo], kh = keys[hi];
                        const uint32_t vl = vals[lo], vh = vals[hi];
                        const bool gt = kl > kh || (kl == kh && vl > vh);
                        if (gt == asc) {
                            keys[lo] = kh; keys[hi] = kl;
                            vals[lo] = vh; vals[hi] = vl;
                        }
                    }
                    __syncthreads();
                }
            }
            // bestNFA over the sorted prefix: k = 4 .. m
            double bn = resect_inf();
            int bk = kP3PSample;
            for (int k = kP3PSample + 1 + tid; k <= m; k += kRT) {
                const double nfa = resect_nfa(loge0, logalpha0, key_err(keys[k - 1]), k, logc_n[k], logc_k[k]);
                if (nfa < bn) { bn = nfa; bk = k; }
            }
            for (int d = 32; d >= 1; d >>= 1) {
                const double on = __shfl_xor(bn, d);
                const int ok = __shfl_xor(bk, d);
                if (on < bn || (on == bn && ok < bk)) { bn = on; bk = ok; }
            }
            if (lane == 0) { s_red[wave] = bn; s_redk[wave] = bk; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < kRW; ++w)
                    if (s_red[w] < bn || (s_red[w] == bn && s_redk[w] < bk)) { bn = s_red[w]; bk = s_redk[w]; }
                s_copy = 0;
                if (bn < s_minNFA) {
                    s_upd = 1;
                    s_copy = 1;
                    s_minNFA = bn;
                    s_ninl = bk;
                    s_errorMax = key_err(keys[bk - 1]);
                    for (int z = 0; z < 12; ++z) s_best[z] = M[z];
                }
            }
            __syncthreads();
            if (s_copy)
                for (int64_t k = tid; k < s_ninl; k += kRT) binl[k] = vals[k];
            __syncthreads();
        }
        // focused sampling: draw among the best inliers so far
        if (tid == 0) {
            s_copy = 0;
            if ((s_upd && s_minNFA < 0) || (iter + 1 == s_nIter && s_nIterReserve)) {
                if (s_ninl == 0) {
                    s_nIter++;
                    s_nIterReserve--;
                } else {
                    s_copy = 1;
                    s_vsize = s_ninl;
                    if (s_nIterReserve) {
                        s_nIter = iter + 1 + s_nIterReserve;
                        s_nIterReserve = 0;
                    }
                }
            }
        }
        __syncthreads();
        if (s_copy)
            for (int64_t k = tid; k < s_ninl; k += kRT) vidx[k] = binl[k];
        __syncthreads();
    }
    const bool keep = s_minNFA < 0 && s_ninl > 2 * kP3PSample + 1;   // > 2.5 * 3
    const int64_t ninl = s_ninl;
    if (tid == 0) {
        st[0] = s_minNFA;
        st[1] = keep ? s_errorMax : 0.0;
        st[2] = keep ? (double)ninl : 0.0;
        st[3] = (double)iter;
        st[4] = (double)(keep ? SFM_RESECT_OK : SFM_RESECT_NO_MODEL);
        st[5] = 0.0;
    }
    if (tid < 12) {
        Mo[tid] = keep ? s_best[tid] : 0.0;
        s_Rt[tid] = s_best[tid];
    }
    __syncthreads();
    // ---- the refit over the inliers (binl, in sorted order) --------------------
    bool fitted = true;
    if (keep) {
        for (int it = 0; it < a.refine_iter; ++it) {
            double M[12], S[27];
#pragma unroll
            for (int z = 0; z < 12; ++z) M[z] = s_Rt[z];
#pragma unroll
            for (int z = 0; z < 27; ++z) S[z] = 0.0;
            for (int64_t t = tid; t < ninl; t += kRT) {
                const size_t k = binl[t];
                resect_normal_terms<CM>(M, in, X + 3 * k, uv[2 * k], uv[2 * k + 1], S);
            }
#pragma unroll
            for (int z = 0; z < 27; ++z) {
                double v = S[z];
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
                if (lane == 0) s_S[wave][z] = v;
            }
            __syncthreads();
            if (tid == 0) {
                for (int z = 0; z < 27; ++z) {
                    double v = s_S[0][z];
                    for (int w = 1; w < kRW; ++w) v = v + s_S[w][z];
                    s_S[0][z] = v;
                }
                int fit = 2;   // 0: go on, 1: converged, 2: failed
                if (resect_solve6(s_S[0], s_H, s_d) && resect_apply(s_Rt, s_d)) {
                    double n2 = 0.0;
                    for (int z = 0; z < 6; ++z) n2 = n2 + s_d[z] * s_d[z];
                    fit = n2 < 1e-24 ? 1 : 0;
                }
                s_fit = fit;
            }
            __syncthreads();
            const int fit = s_fit;
            if (fit == 2) fitted = false;
            if (fit != 0) break;
        }
    }
    if (tid < 12) Mo[12 + tid] = !keep ? 0.0 : fitted ? s_Rt[tid] : s_best[tid];
}

}  // namespace

void resect_launch(const ResectArgs& a, int32_t camera_model, int64_t n_img, hipStream_t s) {
    const size_t lds = 12 * (size_t)a.lds_slots;
    auto go = [&](auto kernel) {
        set_dyn_lds((const void*)kernel, 12 * (size_t)kResectMaxLdsSort);
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_img), dim3(kRT), lds, s, a);
        SFM_HIP(hipGetLastError());
    };
    if (camera_model == SFM_CAM_RADIAL3) go(resect_ac_kernel<SFM_CAM_RADIAL3>);
    else if (camera_model == SFM_CAM_SNAVELY) go(resect_ac_kernel<SFM_CAM_SNAVELY>);
    else go(resect_ac_kernel<SFM_CAM_PINHOLE>);
}

}  // namespace sfm
