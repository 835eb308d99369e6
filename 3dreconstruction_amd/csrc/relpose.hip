// Relative pose on gfx950 (include/sfmcore.h, "Relative pose"):
// OpenMVG's a-contrario RANSAC over a five-point essential-matrix solver, the
// cheirality vote over the four motions of the kept E and the median ray
// angle of its front inliers, one independent problem per image pair.
//
// Layout, as the resection's (resect.hip): one 256-thread workgroup per pair.
// Lane 0 draws the sample.  The five-point solve is spread over the workgroup
// through LDS: the 5x9 and the 10x20 Gauss-Jordan eliminations hold one matrix
// entry per lane with two barriers per pivot step, the ten constraint rows are
// built one per lane, the Sturm sequence of the degree-10 polynomial is
// evaluated at one grid point per lane, and each real root is refined and
// turned into a model by a lane of its own.  Every model's error pass, the
// compaction of the errors under the bound, their (error, index) bitonic sort
// in LDS (global memory above 8192 slots) and the NFA scan are spread over the
// 256 threads.  Every number comes from the operation sequence the serial host
// twin (relpose.cpp) runs over the same relpose_pose.h statements, compiled
// without FMA contraction in both; the reductions are over integers or total
// orders.  No floating-point atomics, no wait on another workgroup: two runs
// give the same bits.
#pragma clang fp contract(off)

#include <hip/hip_runtime.h>

#include "common.h"
#include "relpose.h"
#include "relpose_pose.h"

namespace sfm {
namespace {

constexpr int kRT = kRelposeThreads;
constexpr int kRW = kRT / 64;   // waves
static_assert(kE5Grid == kRT, "one Sturm evaluation per lane");

// what the workgroup's five-point solve keeps in LDS
struct E5Shared {
    double sb[30];   // the sample's bearings: b_I[15], b_J[15]
    double A5[45], basis[36], eet[60], A[200], Bz[45], poly[kE5Poly], sc[kE5Poly * kE5Poly], B;
    double models[kE5MaxModels * 9];
    int sdeg[kE5Poly], cnt[kE5Grid], mok[kE5MaxModels], ns, nm;
};

// e5_gauss_jordan with entry (tid / C, tid % C) per lane: every lane finds the
// pivot of step c from LDS, computes its entry's new value from the old
// matrix, and the matrix is replaced between two barriers.  Uniform result;
// ends on a barrier when true.
template <int R, int C, bool FULL>
__device__ bool gj_lds(double* A, int tid, double thr, int* pc) {
    const int r = tid / C, k = tid % C;
    const bool act = tid < R * C;
    uint32_t used = 0;
    for (int c = 0; c < R; ++c) {
        int piv, pk;
        if (!e5_pivot<R, C, FULL>(A, c, used, thr, piv, pk)) return false;
        used |= 1u << pk;
        pc[c] = pk;
        double nv = 0.0;
        if (act) {
            const int src = r == c ? piv : r == piv ? c : r;   // the row that sits at r after the swap
            const double p = A[piv * C + k] / A[piv * C + pk];
            if (r == c) {
                nv = p;
            } else {
                const double f = A[src * C + pk];
                nv = A[src * C + k] - f * p;
            }
        }
        __syncthreads();
        if (act) A[r * C + k] = nv;
        __syncthreads();
    }
    return true;
}

// e5_solve over the workgroup: the sample's bearings are in S.sb; the models
// come out in S.models, their number (uniform) is returned.  Starts and ends
// with every lane past a barrier.
__device__ int e5_solve_wg(E5Shared& S, int tid) {
    if (tid < 45) S.A5[tid] = e5_epipolar_entry(S.sb, S.sb + 15, tid / 9, tid % 9);
    __syncthreads();
    int pc[10];
    if (!gj_lds<5, 9, true>(S.A5, tid, kE5NullPivot, pc)) return 0;
    if (tid < 4) e5_basis_vector(S.A5, pc, tid, S.basis + 9 * tid);
    __syncthreads();
    if (tid < 6) {
        const int i = tid < 3 ? 0 : tid < 5 ? 1 : 2, k = tid < 3 ? tid : tid < 5 ? tid - 2 : 2;
        e5_eet(S.basis, i, k, S.eet + 10 * tid);
    } else if (tid == 6) {
        e5_row_det(S.basis, S.A);
    }
    __syncthreads();
    if (tid < 9) e5_row_trace(S.eet, S.basis, tid / 3, tid % 3, S.A + 20 * (1 + tid));
    __syncthreads();
    if (!gj_lds<10, 20, false>(S.A, tid, kE5ElimPivot, pc)) return 0;
    if (tid == 0) {
        e5_bz(S.A, S.Bz);
        e5_poly10(S.Bz, S.poly);
        S.ns = e5_sturm(S.poly, S.sc, S.sdeg, &S.B);
    }
    __syncthreads();
    const int ns = S.ns;
    if (ns == 0) return 0;
    S.cnt[tid] = e5_sturm_count(S.sc, S.sdeg, ns, e5_grid(S.B, tid));
    __syncthreads();
    int nr = S.cnt[0] - S.cnt[kE5Grid - 1];
    if (nr > kE5MaxModels) nr = kE5MaxModels;
    if (tid < kE5MaxModels) {
        bool ok = false;
        if (tid < nr) {
            const double z = e5_root(S.sc, S.sdeg, ns, S.cnt, S.B, tid);
            ok = e5_model(S.Bz, S.basis, z, S.models + 9 * tid);
        }
        S.mok[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {   // the valid models, in root order
        int nm = 0;
        for (int j = 0; j < kE5MaxModels; ++j) {
            if (!S.mok[j]) continue;
            if (nm != j)
                for (int z = 0; z < 9; ++z) S.models[9 * nm + z] = S.models[9 * j + z];
            ++nm;
        }
        S.nm = nm;
    }
    __syncthreads();
    return S.nm;
}

// bitonic sort of the m (key, val) pairs ascending, padded to a power of two;
// starts and ends on a barrier
__device__ void sort_pairs(unsigned long long* keys, uint32_t* vals, int m, int tid) {
    int P2 = 1;
    while (P2 < m) P2 <<= 1;
    for (int k = m + tid; k < P2; k += kRT) {
        keys[k] = ~0ull;
        vals[k] = 0xFFFFFFFFu;
    }
    __syncthreads();
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
}

template <int CM>
__global__ __launch_bounds__(kRT) void relpose_ac_kernel(RelposeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t o0 = a.off[q], n = a.off[q + 1] - o0;
    double* Mo = a.model + 21 * (size_t)q;
    double* st = a.stat + 8 * (size_t)q;
    if (n <= kE5Sample) {
        if (tid < 21) Mo[tid] = 0.0;
        if (tid < 8) st[tid] = tid == 4 ? (double)SFM_RELPOSE_FEW : 0.0;
        return;
    }
    const double* xy = a.xy + 4 * o0;
    const double* inI = a.intr + (int64_t)a.iw * a.pair_intr[2 * q];
    const double* inJ = a.intr + (int64_t)a.iw * a.pair_intr[2 * q + 1];
    const double logalpha0 = a.cst[4 * q], maxThr = a.cst[4 * q + 1], loge0 = a.cst[4 * q + 2];
    double* bear = a.bear + 6 * o0;
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

    __shared__ E5Shared S;
    __shared__ double s_best[9], s_Ra[9], s_Rb[9], s_t[3];
    __shared__ double s_red[kRW];
    __shared__ int s_redk[kRW];
    __shared__ int s_wc[kRW][4];
    __shared__ int s_m, s_cnt, s_ac, s_upd, s_copy, s_stop, s_mot, s_win;
    __shared__ uint32_t s_sample[kE5Sample];
    __shared__ int64_t s_nIter, s_nIterReserve, s_vsize, s_ninl, s_nfront;
    __shared__ double s_minNFA, s_errorMax, s_angle;

    // ---- prologue: bearings, log10 table, the sampling list, logcombi tables --
    for (int64_t k = tid; k < n; k += kRT) {
        double bi[3], bj[3];
        const bool oi = tri_bearing<CM>(inI, xy[4 * k], xy[4 * k + 1], bi);
        const bool oj = tri_bearing<CM>(inJ, xy[4 * k + 2], xy[4 * k + 3], bj);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            bear[6 * k + j] = bi[j];
            bear[6 * k + 3 + j] = bj[j];
        }
        okf[k] = oi && oj ? 1 : 0;
    }
    for (int64_t j = tid; j <= n; j += kRT) L[j] = j == 0 ? 0.0 : det_log10((double)j);
    __syncthreads();
    // the correspondences with both bearings, in order (ballot prefix per wave,
    // the waves' counts through LDS)
    int64_t nv = 0;
    for (int64_t b0 = 0; b0 < n; b0 += kRT) {
        const int64_t k = b0 + tid;
        const bool f = k < n && okf[k] != 0;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) s_wc[wave][0] = __popcll(bal);
        __syncthreads();
        int64_t at = nv;
        for (int w = 0; w < kRW; ++w) {
            if (w < wave) at += s_wc[w][0];
            nv += s_wc[w][0];
        }
        if (f) vidx[at + __popcll(bal & ((1ull << lane) - 1ull))] = (uint32_t)k;
        __syncthreads();
    }
    if (nv <= kE5Sample) {   // (uniform)
        if (tid < 21) Mo[tid] = 0.0;
        if (tid < 8) st[tid] = tid == 4 ? (double)SFM_RELPOSE_FEW : 0.0;
        return;
    }
    for (int64_t k = tid; k <= n; k += kRT) {
        // logcombi(k, n) and logcombi(5, k): OpenMVG's loop, log10 from the table
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
    if (tid == 0) {
        s_ac = 0;
        s_minNFA = relpose_inf();
        s_errorMax = relpose_inf();
        s_nIterReserve = a.max_iter / 10;
        s_nIter = a.max_iter - s_nIterReserve;
        s_vsize = nv;
        s_ninl = 0;
        s_stop = 0;
    }
    if (tid < 9) s_best[tid] = 0.0;
    __syncthreads();
    Stream rs{a.rng, 0, a.rng_n};
    int64_t iter = 0;
    for (iter = 0; iter < s_nIter; ++iter) {
        // ---- sampling (lane 0), the five-point solve (the workgroup) ----------
        if (tid == 0) {
            if (s_ac) {
                for (int i = 0; i < kE5Sample; ++i) {
                    const uint32_t d = rs.uniform((uint32_t)i, (uint32_t)(s_vsize - 1));
                    const uint32_t t = vidx[i];
                    vidx[i] = vidx[d];
                    vidx[d] = t;
                    s_sample[i] = vidx[i];
                }
            } else {
                int ns = 0;
                while (ns < kE5Sample && !rs.over) {
                    const uint32_t sm = vidx[rs.uniform(0u, (uint32_t)(nv - 1))];
                    bool found = false;
                    for (int j = 0; j < ns && !found; ++j) found = s_sample[j] == sm;
                    if (!found) s_sample[ns++] = sm;
                }
            }
            s_stop = rs.over ? 1 : 0;
            if (rs.over) a.fail[0] = 1;
            s_upd = 0;
            if (!rs.over)
                for (int i = 0; i < kE5Sample; ++i) {
                    const size_t k = s_sample[i];
                    for (int j = 0; j < 3; ++j) {
                        S.sb[3 * i + j] = bear[6 * k + j];
                        S.sb[15 + 3 * i + j] = bear[6 * k + 3 + j];
                    }
                }
        }
        __syncthreads();
        if (s_stop) break;
        const int nm = e5_solve_wg(S, tid);
        for (int mi = 0; mi < nm; ++mi) {
            double M[9];
#pragma unroll
            for (int z = 0; z < 9; ++z) M[z] = S.models[9 * mi + z];
            if (!s_ac) {   // does the model explain > 2.5 * 5 errors under the bound?
                int c = 0;
                for (int64_t k = tid; k < n; k += kRT) {
                    const double e = okf[k] ? relpose_error<CM>(M, inJ, bear + 6 * k, bear + 6 * k + 3) : relpose_inf();
                    c += e <= maxThr;
                }
                for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d);
                if (tid == 0) s_cnt = 0;
                __syncthreads();
                if (lane == 0) atomicAdd(&s_cnt, c);
                __syncthreads();
                if (tid == 0 && (double)s_cnt > 2.5 * kE5Sample) s_ac = 1;
                __syncthreads();
                if (!s_ac) continue;
            }
            // errors under the bound -> (error, index) keys
            if (tid == 0) s_m = 0;
            __syncthreads();
            for (int64_t k = tid; k < n; k += kRT) {
                const double e = okf[k] ? relpose_error<CM>(M, inJ, bear + 6 * k, bear + 6 * k + 3) : relpose_inf();
                if (e <= maxThr) {
                    const int slot = atomicAdd(&s_m, 1);
                    keys[slot] = err_key(e);
                    vals[slot] = (uint32_t)k;
                }
            }
            __syncthreads();
            const int m = s_m;
            sort_pairs(keys, vals, m, tid);
            // bestNFA over the sorted prefix: k = 6 .. m
            double bn = relpose_inf();
            int bk = kE5Sample;
            for (int k = kE5Sample + 1 + tid; k <= m; k += kRT) {
                const double nfa = relpose_nfa(loge0, logalpha0, key_err(keys[k - 1]), k, logc_n[k], logc_k[k]);
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
                    for (int z = 0; z < 9; ++z) s_best[z] = M[z];
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
    const bool keep = s_minNFA < 0 && s_ninl > 2 * kE5Sample + 2;   // > 2.5 * 5
    const int64_t ninl = s_ninl;
    // ---- the motion: Horn's four, the cheirality vote, the median ray angle ----
    if (tid == 0) {
        s_mot = keep && relpose_motions(s_best, s_Ra, s_Rb, s_t) ? 1 : 0;
        s_win = -1;
        s_nfront = 0;
        s_angle = 0.0;
    }
    __syncthreads();
    if (s_mot) {   // (uniform)
        int c4[4] = {0, 0, 0, 0};
        for (int64_t t = tid; t < ninl; t += kRT) {
            const size_t k = binl[t];
            const uint32_t msk = relpose_front_mask<CM>(s_Ra, s_Rb, s_t, bear + 6 * k, bear + 6 * k + 3);
            vidx[t] = msk;
#pragma unroll
            for (int mm = 0; mm < 4; ++mm) c4[mm] += (int)((msk >> mm) & 1u);
        }
#pragma unroll
        for (int mm = 0; mm < 4; ++mm) {
            int v = c4[mm];
            for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
            if (lane == 0) s_wc[wave][mm] = v;
        }
        __syncthreads();
        if (tid == 0) {
            int64_t cnt[4];
            for (int mm = 0; mm < 4; ++mm) {
                cnt[mm] = 0;
                for (int w = 0; w < kRW; ++w) cnt[mm] += s_wc[w][mm];
            }
            const int win = relpose_vote(cnt, a.front_ratio);
            s_win = win;
            s_nfront = win >= 0 ? cnt[win] : 0;
            s_m = 0;
        }
        __syncthreads();
        const int win = s_win;
        if (win >= 0) {
            const double* R = win < 2 ? s_Ra : s_Rb;
            for (int64_t t = tid; t < ninl; t += kRT) {
                if (!((vidx[t] >> win) & 1u)) continue;
                const size_t k = binl[t];
                const int slot = atomicAdd(&s_m, 1);
                keys[slot] = err_key(relpose_angle_key(R, bear + 6 * k, bear + 6 * k + 3));
                vals[slot] = (uint32_t)k;
            }
            __syncthreads();
            const int m = s_m;
            sort_pairs(keys, vals, m, tid);
            if (tid == 0) {
                const size_t k = vals[m / 2];
                s_angle = relpose_angle_deg(R, bear + 6 * k, bear + 6 * k + 3);
            }
            __syncthreads();
        }
    }
    const int win = s_win;
    if (tid == 0) {
        st[0] = s_minNFA;
        st[1] = keep ? s_errorMax : 0.0;
        st[2] = keep ? (double)ninl : 0.0;
        st[3] = (double)iter;
        st[4] = (double)(!keep ? SFM_RELPOSE_NO_MODEL : win >= 0 ? SFM_RELPOSE_OK : SFM_RELPOSE_AMBIGUOUS);
        st[5] = (double)s_nfront;
        st[6] = s_angle;
        st[7] = 0.0;
    }
    if (tid < 9) {
        Mo[tid] = keep ? s_best[tid] : 0.0;
        Mo[9 + tid] = win < 0 ? 0.0 : win < 2 ? s_Ra[tid] : s_Rb[tid];
    }
    if (tid < 3) Mo[18 + tid] = win < 0 ? 0.0 : (win & 1) ? -s_t[tid] : s_t[tid];
}

}  // namespace

void relpose_launch(const RelposeArgs& a, int32_t camera_model, int64_t n_pairs, hipStream_t s) {
    const size_t lds = 12 * (size_t)a.lds_slots;
    auto go = [&](auto kernel) {
        set_dyn_lds((const void*)kernel, 12 * (size_t)kRelposeMaxLdsSort);
        hipLaunchKernelGGL(kernel, dim3((unsigned)n_pairs), dim3(kRT), lds, s, a);
        SFM_HIP(hipGetLastError());
    };
    if (camera_model == SFM_CAM_RADIAL3) go(relpose_ac_kernel<SFM_CAM_RADIAL3>);
    else if (camera_model == SFM_CAM_SNAVELY) go(relpose_ac_kernel<SFM_CAM_SNAVELY>);
    else go(relpose_ac_kernel<SFM_CAM_PINHOLE>);
}

}  // namespace sfm
