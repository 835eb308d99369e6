// BA after the reduce: the one-workgroup RCS solve, candidate cameras, per
// point back substitution (chunk and general points), finalize / publish.
#include "ba_device.h"
namespace sfm {
namespace {
// RCS solve: block-banded (6x6 blocks, half-bandwidth D) Cholesky with a dense
// intrinsics arrow, over a circular window of D+1 block rows.
__device__ __forceinline__ double lm2(const DevProblem& P, int64_t col, double radius) {
    const double lm = sqrt(clampd(P.cnF[col], P.min_diag, P.max_diag) / radius);
    return lm * lm;
}

__device__ bool chol_inplace(double* A, int n, int ld) {  // lower, serial
    bool ok = true;
    for (int j = 0; j < n; ++j) {
        double s = A[j * ld + j];
        for (int k = 0; k < j; ++k) s -= A[j * ld + k] * A[j * ld + k];
        if (!(s > 0.0)) ok = false;
        const double d = sqrt(s);
        A[j * ld + j] = d;
        const double id = 1.0 / d;
        for (int i = j + 1; i < n; ++i) {
            double t = A[i * ld + j];
            for (int k = 0; k < j; ++k) t -= A[i * ld + k] * A[j * ld + k];
            A[i * ld + j] = t * id;
        }
    }
    return ok;
}

__global__ __launch_bounds__(256) void solve_kernel(DevProblem P, double radius, int use_lds) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int ncam = P.ncam, nintr = P.nintr, D = P.D, Dp = D + 1;
    const int tid = threadIdx.x;
    // LDS: [fail (2 doubles) | YW (Dp x 6) | window if it fits]; else window in HBM
    double* failp = lds;
    double* YW = lds + 2;                                   // [Dp][6], always LDS
    double* W = use_lds ? lds + 2 + (size_t)Dp * 6 : P.Wglobal;
    double* WA = W + (size_t)Dp * Dp * 36;                // [nintr][Dp][24]
    double* WC = WA + (size_t)nintr * Dp * 24;             // [4nintr][4nintr]
    double* WR = WC + (size_t)16 * nintr * nintr;          // [Dp][6]
    double* WRA = WR + (size_t)Dp * 6;                     // [4nintr]
    int fail_local = 0;
    const int na4 = 4 * nintr;

    auto Wb = [&](int i, int d) { return W + ((size_t)(i % Dp) * Dp + d) * 36; };
    auto WAb = [&](int k, int j) { return WA + ((size_t)k * Dp + (j % Dp)) * 24; };

    auto load_row = [&](int i) {
        const int dm = min(D, i);
        for (int e = tid; e < (dm + 1) * 36; e += 256) {
            const int d = e / 36, q = e % 36;
            double v = P.Sband[((size_t)i * Dp + d) * 36 + q];
            if (d == 0 && q % 7 == 0) v += lm2(P, 6LL * i + q / 7, radius);
            Wb(i, d)[q] = v;
        }
        for (int e = tid; e < nintr * 24; e += 256) {
            const int k = e / 24, q = e % 24;
            WAb(k, i)[q] = P.Sarrow[((size_t)k * ncam + i) * 24 + q];
        }
        if (tid < 6) WR[(i % Dp) * 6 + tid] = P.rhs[6LL * i + tid];
    };
    // corner (dense 4nintr x 4nintr from 4x4 blocks) and arrow rhs
    for (int e = tid; e < na4 * na4; e += 256) {
        const int rr = e / na4, cc = e % na4;
        double v = P.Scorner[(((size_t)(rr / 4) * nintr + cc / 4) * 16) + (rr % 4) * 4 + cc % 4];
        if (rr == cc) v += lm2(P, P.nb + rr, radius);
        WC[e] = v;
    }
    if (tid < na4) WRA[tid] = P.rhs[P.nb + tid];
    for (int i = 0; i < min(Dp, ncam); ++i) load_row(i);
    __syncthreads();

    for (int j = 0; j < ncam; ++j) {
        const int dm = min(D, ncam - 1 - j);
        // (a) factor the diagonal block; forward-substitute its rhs
        if (tid == 0) {
            double* Ljj = Wb(j, 0);
            if (!chol_inplace(Ljj, 6, 6)) fail_local = 1;
            double* z = WR + (j % Dp) * 6;
            for (int r = 0; r < 6; ++r) {
                double s = z[r];
                for (int k = 0; k < r; ++k) s -= Ljj[r * 6 + k] * z[k];
                z[r] = s / Ljj[r * 6 + r];
            }
        }
        __syncthreads();
        // (b) TRSM: rows of blocks (j+d, j) and arrow rows: X L_jj' = S
        {
            const double* Ljj = Wb(j, 0);
            const int nrows = 6 * dm + na4;
            for (int t = tid; t < nrows; t += 256) {
                double* row;
                if (t < 6 * dm) row = Wb(j + t / 6 + 1, t / 6 + 1) + (t % 6) * 6;
                else row = WAb((t - 6 * dm) / 4, j) + ((t - 6 * dm) % 4) * 6;
                for (int cc = 0; cc < 6; ++cc) {
                    double s = row[cc];
                    for (int m = 0; m < cc; ++m) s -= row[m] * Ljj[cc * 6 + m];
                    row[cc] = s / Ljj[cc * 6 + cc];
                }
            }
        }
        __syncthreads();
        // (c) trailing updates + rhs updates + write column j out
        {
            const double* z = WR + (j % Dp) * 6;
            const int npair = dm * (dm + 1) / 2;
            const int nb_el = npair * 36, na_el = nintr * dm * 24, nc_el = na4 * na4;
            const int nr_el = 6 * dm + na4;
            const int total = nb_el + na_el + nc_el + nr_el;
            for (int t = tid; t < total; t += 256) {
                if (t < nb_el) {
                    const int q = t / 36, e = t % 36, r = e / 6, cc = e % 6;
                    int di = (int)((1.0 + sqrt(1.0 + 8.0 * q)) * 0.5);
                    while (di * (di - 1) / 2 > q) --di;
                    while ((di + 1) * di / 2 <= q) ++di;
                    const int dk = q - di * (di - 1) / 2 + 1;
                    const double* Li = Wb(j + di, di) + r * 6;
                    const double* Lk = Wb(j + dk, dk) + cc * 6;
                    double s = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) s += Li[m] * Lk[m];
                    Wb(j + di, di - dk)[e] -= s;
                } else if (t < nb_el + na_el) {
                    const int u = t - nb_el, k = u / (dm * 24), rem = u % (dm * 24);
                    const int dk = rem / 24 + 1, e = rem % 24, r = e / 6, cc = e % 6;
                    const double* La = WAb(k, j) + r * 6;
                    const double* Lk = Wb(j + dk, dk) + cc * 6;
                    double s = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) s += La[m] * Lk[m];
                    WAb(k, j + dk)[e] -= s;
                } else if (t < nb_el + na_el + nc_el) {
                    const int u = t - nb_el - na_el, rr = u / na4, cc = u % na4;
                    const double* La = WAb(rr / 4, j) + (rr % 4) * 6;
                    const double* Lb = WAb(cc / 4, j) + (cc % 4) * 6;
                    double s = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; ++m) s += La[m] * Lb[m];
                    WC[u] -= s;
                } else {
                    const int u = t - nb_el - na_el - nc_el;
                    if (u < 6 * dm) {
                        const int di = u / 6 + 1, r = u % 6;
                        const double* Li = Wb(j + di, di) + r * 6;
                        double s = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; ++m) s += Li[m] * z[m];
                        WR[((j + di) % Dp) * 6 + r] -= s;
                    } else {
                        const int a = u - 6 * dm;
                        const double* La = WAb(a / 4, j) + (a % 4) * 6;
                        double s = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; ++m) s += La[m] * z[m];
                        WRA[a] -= s;
                    }
                }
            }
            for (int e = tid; e < (dm + 1) * 36; e += 256)
                P.Lcol[((size_t)j * Dp + e / 36) * 36 + e % 36] = Wb(j + e / 36, e / 36)[e % 36];
            for (int e = tid; e < nintr * 24; e += 256)
                P.Larrow[((size_t)j * nintr + e / 24) * 24 + e % 24] = WAb(e / 24, j)[e % 24];
            if (tid < 6) P.zF[6LL * j + tid] = z[tid];
        }
        __syncthreads();
        // (d) slide the window: block row j+Dp takes row j's slot
        if (j + Dp < ncam) load_row(j + Dp);
        __syncthreads();
    }
    // corner: factor, forward, backward
    if (tid == 0) {
        if (na4 > 0 && !chol_inplace(WC, na4, na4)) fail_local = 1;
        for (int r = 0; r < na4; ++r) {
            double s = WRA[r];
            for (int k = 0; k < r; ++k) s -= WC[r * na4 + k] * WRA[k];
            WRA[r] = s / WC[r * na4 + r];
        }
        for (int r = na4 - 1; r >= 0; --r) {
            double s = WRA[r];
            for (int k = r + 1; k < na4; ++k) s -= WC[k * na4 + r] * WRA[k];
            WRA[r] = s / WC[r * na4 + r];
            P.yF[P.nb + r] = WRA[r];
        }
    }
    __syncthreads();
    // back substitution over the band (wave 0)
    if (tid < 64) {
        const int lane = tid;
        for (int j = ncam - 1; j >= 0; --j) {
            const int dm = min(D, ncam - 1 - j);
            double s[6] = {0, 0, 0, 0, 0, 0};
            const int nterm = 6 * dm + na4;
            for (int t = lane; t < nterm; t += 64) {
                const double* Lrow;  // row (c) of the block: L[c][0..5]
                double yv;
                if (t < 6 * dm) {
                    const int d = t / 6 + 1, cc = t % 6;
                    Lrow = P.Lcol + ((size_t)j * Dp + d) * 36 + cc * 6;
                    yv = YW[((j + d) % Dp) * 6 + cc];
                } else {
                    const int a = t - 6 * dm;
                    Lrow = P.Larrow + ((size_t)j * nintr + a / 4) * 24 + (a % 4) * 6;
                    yv = WRA[a];
                }
#pragma unroll
                for (int r = 0; r < 6; ++r) s[r] += Lrow[r] * yv;
            }
            wave_sum(s);
            if (lane == 0) {
                const double* Ljj = P.Lcol + ((size_t)j * Dp) * 36;
                double y[6];
                for (int r = 5; r >= 0; --r) {
                    double v = P.zF[6LL * j + r] - s[r];
                    for (int k = r + 1; k < 6; ++k) v -= Ljj[k * 6 + r] * y[k];
                    y[r] = v / Ljj[r * 6 + r];
                }
                for (int r = 0; r < 6; ++r) {
                    YW[(j % Dp) * 6 + r] = y[r];
                    P.yF[6LL * j + r] = y[r];
                }
            }
            __builtin_amdgcn_s_waitcnt(0);
            __builtin_amdgcn_wave_barrier();
        }
    }
    __syncthreads();
    (void)failp;
    if (tid == 0) P.scal[kScSolveFail] = fail_local ? 1.0 : 0.0;
}

// Candidate parameters: one thread per image / intrinsic block.  Active
// columns take x - yF*scaleF (Ceres' x + delta in the unscaled frame),
// inactive (constant) blocks are copied; the candidate CamPre is built inline.
// Per-workgroup partials of |x|^2, |delta|^2 and max|g| over the F columns go
// to part_f and are summed in fixed order by finalize_kernel.
__global__ __launch_bounds__(kCandThreads) void cand_kernel(DevProblem P,
                                                            const double* __restrict__ extr,
                                                            const double* __restrict__ intr,
                                                            double* __restrict__ cand_extr,
                                                            double* __restrict__ cand_intr,
                                                            CamPre* __restrict__ cand_cp) {
    const int t = blockIdx.x * kCandThreads + threadIdx.x;
    CandAcc ca;
    auto col = [&](double x, int64_t c) { return cand_col(x, P.yF[c], P.scaleF[c], P.bF[c], ca); };
    if (t < P.n_img) {
        const int c0 = P.img_colc[t];
        double e[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double x = extr[6 * (size_t)t + a];
            e[a] = c0 >= 0 ? col(x, (int64_t)c0 + a) : x;
            cand_extr[6 * (size_t)t + a] = e[a];
        }
        cand_cp[t] = make_campre(e);
    } else if (t < P.n_img + P.n_intr) {
        const int q = t - P.n_img;
        const int c0 = P.intr_col[q];
        // SNAVELY: the 4th double is not a parameter (not moved, not in the norms)
        const int iw = P.iw, na = P.cam_model == SFM_CAM_SNAVELY ? 3 : iw;
        for (int a = 0; a < iw; ++a) {
            const double x = intr[iw * (size_t)q + a];
            cand_intr[iw * (size_t)q + a] = (c0 >= 0 && a < na) ? col(x, (int64_t)c0 + a) : x;
        }
    }
    double v[2] = {ca.x2, ca.d2};
    wave_sum(v);
    const double gm = wave_max(ca.gm);
    constexpr int kW = kCandThreads / 64;
    __shared__ double red[kW][3];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[wave][0] = v[0]; red[wave][1] = v[1]; red[wave][2] = gm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double r[3] = {0.0, 0.0, 0.0};
        for (int w = 0; w < kW; ++w) { r[0] += red[w][0]; r[1] += red[w][1]; r[2] = fmax(r[2], red[w][2]); }
        for (int k = 0; k < 3; ++k) P.part_f[3 * (size_t)blockIdx.x + k] = r[k];
    }
}

// per-point back substitution, model cost change, candidate cost
// One workgroup per Schur chunk, SPLIT threads per point (adjacent lanes, each
// taking every SPLIT-th observation; their sums are combined with xor
// shuffles, identical in every lane of the group), at most kStepThreads
// threads.  A landmark shard at N = 8 has short chunks (~30 points, so that
// the Schur pass keeps dividing by N): one thread per point would leave three
// quarters of a 128-thread workgroup idle and each lane a chain of 20
// linearisations.  The chunk's current and candidate cameras, intrinsics, column scales
// and y_F are staged in LDS once, so the per-observation work gathers only the
// measurement.
constexpr int kStepThreads = 256;
template <int CM, int SPLIT>
__global__ __launch_bounds__(kStepThreads) void step_kernel(DevProblem P, const CamPre* __restrict__ cps,
                                                         const double* __restrict__ intr,
                                                         const CamPre* __restrict__ cps_c,
                                                         const double* __restrict__ intr_c,
                                                         const double* __restrict__ X,
                                                         double* __restrict__ Xc, double radius) {
    constexpr int IW = kIW<CM>;
    __shared__ CamPre scp[kCamSlots], scc[kCamSlots];
    __shared__ double csy[kCamSlots][6];        // camera scaleF * yF (0 for a constant image)
    __shared__ double isy[kIntrSlots][3 * IW];  // intrinsics | candidate | scaleF * yF
    const int c = blockIdx.x, tid = threadIdx.x;
    const double inv_radius = 1.0 / radius;   // as schur_kernel
    const ChunkDesc& cd = P.chunks[c];
    {
        constexpr int kCpW = sizeof(CamPre) / 8;
        for (int e = tid; e < cd.n_cams * kCpW; e += blockDim.x) {
            const int t = e / kCpW, w = e - t * kCpW;
            reinterpret_cast<double*>(&scp[t])[w] = reinterpret_cast<const double*>(&cps[cd.cam_img[t]])[w];
            reinterpret_cast<double*>(&scc[t])[w] = reinterpret_cast<const double*>(&cps_c[cd.cam_img[t]])[w];
        }
        for (int e = tid; e < cd.n_cams * 6; e += blockDim.x) {
            const int t = e / 6, k = e - 6 * t, col = cd.cam_col[t];
            csy[t][k] = col >= 0 ? P.scaleF[col + k] * P.yF[col + k] : 0.0;
        }

        if (tid < IW * cd.n_intr) {
            const int t = tid / IW, k = tid - IW * t, col = cd.intr_col[t];
            isy[t][k] = intr[IW * cd.intr_id[t] + k];
            isy[t][IW + k] = intr_c[IW * cd.intr_id[t] + k];
            isy[t][2 * IW + k] = P.scaleF[col + k] * P.yF[col + k];
        }
    }
    __syncthreads();
    const int p = cd.pt_begin + tid / SPLIT, sub = tid % SPLIT;
    double acc[3] = {0.0, 0.0, 0.0};  // model acc, candidate cost, step norm^2
    double bad = 0.0, cbad = 0.0;     // non-finite step / non-finite candidate residual
    if (p < cd.pt_end) {
        const double Xp[3] = {X[3 * (size_t)p], X[3 * (size_t)p + 1], X[3 * (size_t)p + 2]};
        const double sE[3] = {P.scaleE[3 * (size_t)p], P.scaleE[3 * (size_t)p + 1], P.scaleE[3 * (size_t)p + 2]};
        // One linearisation per observation at x gathers everything the step
        // needs: with j = J_E rows scaled by sE and q = J_F y_F (this row),
        //   V = sum j j',  b = sum j (f - q) = bf - bq,
        // and the model change sum m (f + m/2), m = -(q + j y_E), expands to
        //   -(sum q f + y_E . bf) + (sum q^2 + 2 y_E . bq + y_E' V y_E) / 2.
        double V[6] = {0, 0, 0, 0, 0, 0}, bf[3] = {0, 0, 0}, bq[3] = {0, 0, 0};
        double sqf = 0.0, sqq = 0.0;
        const int o0 = P.pt_off[p] + sub, o1 = P.pt_off[p + 1];
        // the next observation's (slot, uv) is loaded while this one is linearised
        int nslot = o0 < o1 ? P.obs_slot[o0] : 0;
        double2 nuv = o0 < o1 ? reinterpret_cast<const double2*>(P.obs_uv)[o0] : double2{0.0, 0.0};
        for (int o = o0; o < o1; o += SPLIT) {
            const int slot = nslot, cs = slot & 255, is = (slot >> 8) & 255;
            const double2 uv = nuv;
            if (o + SPLIT < o1) {
                nslot = P.obs_slot[o + SPLIT];
                nuv = reinterpret_cast<const double2*>(P.obs_uv)[o + SPLIT];
            }
            LinT<CM> L;
            linearize<CM, true, true, true>(scp[cs], &isy[is][0], Xp, uv.x, uv.y, P.huber_a, L);
            // (a ChunkDesc read: an LDS copy of the flag measured 8 % slower,
            // 94.8 -> 102.5 us at C4, profiles/r03/q_final/step_ab.txt)
            const bool cam = crow_valid(cd, cs);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                double q = 0.0;  // (J_F y_F) for this row
                if (cam)
#pragma unroll
                    for (int a = 0; a < 6; ++a) q += L.Jc[r][a] * csy[cs][a];
#pragma unroll
                for (int a = 0; a < IW; ++a) q += L.Ji[r][a] * isy[is][2 * IW + a];
                const double j0 = L.Jx[r][0] * sE[0], j1 = L.Jx[r][1] * sE[1], j2 = L.Jx[r][2] * sE[2];
                const double fr = L.f[r];
                V[0] += j0 * j0; V[1] += j1 * j0; V[2] += j1 * j1;
                V[3] += j2 * j0; V[4] += j2 * j1; V[5] += j2 * j2;
                bf[0] += j0 * fr; bf[1] += j1 * fr; bf[2] += j2 * fr;
                bq[0] += j0 * q; bq[1] += j1 * q; bq[2] += j2 * q;
                sqf += q * fr;
                sqq += q * q;
            }
        }
        if constexpr (SPLIT > 1) {
            // the group's partial sums (xor butterfly: the same value in every lane)
#pragma unroll
            for (int m = 1; m < SPLIT; m <<= 1) {
#pragma unroll
                for (int k = 0; k < 6; ++k) V[k] += __shfl_xor(V[k], m);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    bf[k] += __shfl_xor(bf[k], m);
                    bq[k] += __shfl_xor(bq[k], m);
                }
                sqf += __shfl_xor(sqf, m);
                sqq += __shfl_xor(sqq, m);
            }
        }
        const double V0[6] = {V[0], V[1], V[2], V[3], V[4], V[5]};
        const double b[3] = {bf[0] - bq[0], bf[1] - bq[1], bf[2] - bq[2]};
        const int di[3] = {0, 2, 5};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            V[di[a]] += point_d2(P, V[di[a]], inv_radius);
        }
        // y_E = (V + D^2)^-1 (g_E - W' y_F) via Cholesky
        const double l00 = sqrt(V[0]), l10 = V[1] / l00, l20 = V[3] / l00;
        const double l11 = sqrt(V[2] - l10 * l10), l21 = (V[4] - l20 * l10) / l11;
        const double l22 = sqrt(V[5] - l20 * l20 - l21 * l21);
        const double z0 = b[0] / l00, z1 = (b[1] - l10 * z0) / l11, z2 = (b[2] - l20 * z0 - l21 * z1) / l22;
        const double y2 = z2 / l22, y1 = (z1 - l21 * y2) / l11, y0 = (z0 - l10 * y1 - l20 * y2) / l00;
        const double yE[3] = {y0, y1, y2};
        double xc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xc[a] = Xp[a] + (-yE[a]) * sE[a];
            const double d = Xp[a] - xc[a];
            acc[2] += d * d;
            if (sub == 0) Xc[3 * (size_t)p + a] = xc[a];
            if (!isfinite(xc[a])) bad = 1.0;
        }
        {
            const double ybf = yE[0] * bf[0] + yE[1] * bf[1] + yE[2] * bf[2];
            const double ybq = yE[0] * bq[0] + yE[1] * bq[1] + yE[2] * bq[2];
            const double Vy0 = V0[0] * yE[0] + V0[1] * yE[1] + V0[3] * yE[2];
            const double Vy1 = V0[1] * yE[0] + V0[2] * yE[1] + V0[4] * yE[2];
            const double Vy2 = V0[3] * yE[0] + V0[4] * yE[1] + V0[5] * yE[2];
            const double yVy = yE[0] * Vy0 + yE[1] * Vy1 + yE[2] * Vy2;
            acc[0] = -(sqf + ybf) + 0.5 * (sqq + 2.0 * ybq + yVy);
        }
        if (sub != 0) acc[0] = acc[2] = 0.0;   // one lane of the group carries the point's terms
        // candidate residuals at (x_c, candidate cameras / intrinsics)
        nslot = o0 < o1 ? P.obs_slot[o0] : 0;
        nuv = o0 < o1 ? reinterpret_cast<const double2*>(P.obs_uv)[o0] : double2{0.0, 0.0};
        for (int o = o0; o < o1; o += SPLIT) {
            const int slot = nslot, cs = slot & 255, is = (slot >> 8) & 255;
            const double2 uv = nuv;
            if (o + SPLIT < o1) {
                nslot = P.obs_slot[o + SPLIT];
                nuv = reinterpret_cast<const double2*>(P.obs_uv)[o + SPLIT];
            }
            LinT<CM> C;
            linearize<CM, false, false, false>(scc[cs], &isy[is][IW], xc, uv.x, uv.y, P.huber_a, C);
            acc[1] += C.half_rho;
            if (!C.ok) cbad = 1.0;
        }
        if (!isfinite(acc[0])) bad = 1.0;
    }
    wave_sum(acc);
    bad = wave_max(bad);
    cbad = wave_max(cbad);
    __shared__ double red[kStepThreads / 64][kPartT];
    const int wave = tid >> 6, lane = tid & 63, nw = blockDim.x >> 6;
    if (lane == 0) {
        red[wave][0] = acc[0]; red[wave][1] = acc[1]; red[wave][2] = acc[2];
        red[wave][3] = bad; red[wave][4] = cbad;
    }
    __syncthreads();
    if (tid < kPartT) {
        double v = red[0][tid];
        for (int w = 1; w < nw; ++w) v = tid < 3 ? v + red[w][tid] : fmax(v, red[w][tid]);
        P.part_t[kPartT * (size_t)c + tid] = v;
    }
}

// Step for general points: one thread per point, the same arithmetic as
// step_kernel with cameras and column scales read from global memory.
template <int CM>
__global__ __launch_bounds__(kGStepThreads) void step_general_kernel(
    DevProblem P, const CamPre* __restrict__ cps, const double* __restrict__ intr, const CamPre* __restrict__ cps_c,
    const double* __restrict__ intr_c, const double* __restrict__ X, double* __restrict__ Xc, double radius) {
    constexpr int IW = kIW<CM>;
    const int tid = threadIdx.x, g = blockIdx.x * kGStepThreads + tid;
    const double inv_radius = 1.0 / radius;
    double acc[3] = {0.0, 0.0, 0.0};
    double bad = 0.0, cbad = 0.0;
    if (g < P.n_gpt) {
        const int p = P.n_cpt + g;
        const double Xp[3] = {X[3 * (size_t)p], X[3 * (size_t)p + 1], X[3 * (size_t)p + 2]};
        const double sE[3] = {P.scaleE[3 * (size_t)p], P.scaleE[3 * (size_t)p + 1], P.scaleE[3 * (size_t)p + 2]};
        double V[6] = {0, 0, 0, 0, 0, 0}, bf[3] = {0, 0, 0}, bq[3] = {0, 0, 0};
        double sqf = 0.0, sqq = 0.0;
        const int o0 = P.pt_off[p], o1 = P.pt_off[p + 1];
        for (int o = o0; o < o1; ++o) {
            const int img = P.obs_img[o];
            const double2 uv = reinterpret_cast<const double2*>(P.obs_uv)[o];
            const int colc = P.img_colc[img], coli = P.img_coli[img];
            LinT<CM> L;
            linearize<CM, true, true, true>(cps[img], intr + IW * (size_t)P.img_intr[img], Xp, uv.x, uv.y, P.huber_a, L);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                double q = 0.0;
                if (colc >= 0)
#pragma unroll
                    for (int a = 0; a < 6; ++a) q += L.Jc[r][a] * (P.scaleF[colc + a] * P.yF[colc + a]);
                const int ni = CM == SFM_CAM_SNAVELY ? 3 : IW;
#pragma unroll
                for (int a = 0; a < IW; ++a)
                    if (a < ni) q += L.Ji[r][a] * (P.scaleF[coli + a] * P.yF[coli + a]);
                const double j0 = L.Jx[r][0] * sE[0], j1 = L.Jx[r][1] * sE[1], j2 = L.Jx[r][2] * sE[2];
                const double fr = L.f[r];
                V[0] += j0 * j0; V[1] += j1 * j0; V[2] += j1 * j1;
                V[3] += j2 * j0; V[4] += j2 * j1; V[5] += j2 * j2;
                bf[0] += j0 * fr; bf[1] += j1 * fr; bf[2] += j2 * fr;
                bq[0] += j0 * q; bq[1] += j1 * q; bq[2] += j2 * q;
                sqf += q * fr;
                sqq += q * q;
            }
        }
        const double V0[6] = {V[0], V[1], V[2], V[3], V[4], V[5]};
        const double b[3] = {bf[0] - bq[0], bf[1] - bq[1], bf[2] - bq[2]};
        const int di[3] = {0, 2, 5};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            V[di[a]] += point_d2(P, V[di[a]], inv_radius);
        }
        const double l00 = sqrt(V[0]), l10 = V[1] / l00, l20 = V[3] / l00;
        const double l11 = sqrt(V[2] - l10 * l10), l21 = (V[4] - l20 * l10) / l11;
        const double l22 = sqrt(V[5] - l20 * l20 - l21 * l21);
        const double z0 = b[0] / l00, z1 = (b[1] - l10 * z0) / l11, z2 = (b[2] - l20 * z0 - l21 * z1) / l22;
        const double y2 = z2 / l22, y1 = (z1 - l21 * y2) / l11, y0 = (z0 - l10 * y1 - l20 * y2) / l00;
        const double yE[3] = {y0, y1, y2};
        double xc[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            xc[a] = Xp[a] + (-yE[a]) * sE[a];
            const double d = Xp[a] - xc[a];
            acc[2] += d * d;
            Xc[3 * (size_t)p + a] = xc[a];
            if (!isfinite(xc[a])) bad = 1.0;
        }
        {
            const double ybf = yE[0] * bf[0] + yE[1] * bf[1] + yE[2] * bf[2];
            const double ybq = yE[0] * bq[0] + yE[1] * bq[1] + yE[2] * bq[2];
            const double Vy0 = V0[0] * yE[0] + V0[1] * yE[1] + V0[3] * yE[2];
            const double Vy1 = V0[1] * yE[0] + V0[2] * yE[1] + V0[4] * yE[2];
            const double Vy2 = V0[3] * yE[0] + V0[4] * yE[1] + V0[5] * yE[2];
            const double yVy = yE[0] * Vy0 + yE[1] * Vy1 + yE[2] * Vy2;
            acc[0] = -(sqf + ybf) + 0.5 * (sqq + 2.0 * ybq + yVy);
        }
        for (int o = o0; o < o1; ++o) {
            const int img = P.obs_img[o];
            const double2 uv = reinterpret_cast<const double2*>(P.obs_uv)[o];
            LinT<CM> C;
            linearize<CM, false, false, false>(cps_c[img], intr_c + IW * (size_t)P.img_intr[img], xc, uv.x, uv.y,
                                               P.huber_a, C);
            acc[1] += C.half_rho;
            if (!C.ok) cbad = 1.0;
        }
        if (!isfinite(acc[0])) bad = 1.0;
    }
    wave_sum(acc);
    bad = wave_max(bad);
    cbad = wave_max(cbad);
    constexpr int kW = kGStepThreads / 64;
    __shared__ double red[kW][kPartT];
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0) {
        red[wave][0] = acc[0]; red[wave][1] = acc[1]; red[wave][2] = acc[2];
        red[wave][3] = bad; red[wave][4] = cbad;
    }
    __syncthreads();
    if (tid < kPartT) {
        double v = red[0][tid];
        for (int w = 1; w < kW; ++w) v = tid < 3 ? v + red[w][tid] : fmax(v, red[w][tid]);
        P.part_t[kPartT * (size_t)(P.n_chunk + blockIdx.x) + tid] = v;
    }
}

// fixed-order reduction of the per-block partials, in kFinBlocks
// workgroups: workgroup g sums elements g * kFinThreads + t, stepping by
// kFinBlocks * kFinThreads (every thread's loads in flight together), stores
// its 12 partials write-through and takes a ticket; the last to arrive adds
// the partials in workgroup order and publishes (Guideline 16, counter form).
// One 1024-thread workgroup walking every list took 12-13 us at C4 (a chain
// of dependent loads per thread); the sums are now in a different (still
// fixed) order.
// The host's accept decision for this iteration's step (ba_solver.cpp
// run_plan, "this iteration": an invalid step, the parameter and function
// tolerance tests, then the relative decrease), restated on the scalars just
// combined, same operations in the same order -- so the speculative Gram pass
// at the candidate (ba_image_gram with gate) runs exactly when the host will
// accept.  The host still checks the flag against its own decision (and runs
// or redoes the pass on a mismatch), so no result depends on this copy.
__device__ __forceinline__ bool lm_spec_accept(const double* sc, const DevProblem& P) {
    const double model_change = -sc[kScModelAcc];
    const bool finite = sc[kScSolveFail] == 0.0 && sc[kScStepBad] == 0.0 && isfinite(model_change);
    if (!(finite && model_change > 0.0)) return false;
    const double x_cost = sc[kScCost];
    const double cand_cost = sc[kScCandBad] != 0.0 ? DBL_MAX : sc[kScCandCost];
    const double x_norm = sqrt(sc[kScXnorm2E] + sc[kScXnorm2F]);
    const double step_norm = sqrt(sc[kScStepnorm2E] + sc[kScStepnorm2F]);
    if (step_norm <= P.lm_ptol * (x_norm + P.lm_ptol)) return false;
    if (fabs(x_cost - cand_cost) <= P.lm_ftol * x_cost) return false;
    const double rel = cand_cost >= DBL_MAX ? -DBL_MAX : (x_cost - cand_cost) / model_change;
    return rel > P.lm_min_rel;
}

constexpr int kFinThreads = 256, kFinBlocks = 16;
__global__ __launch_bounds__(kFinThreads) void finalize_kernel(DevProblem P, int n_step_blocks,
                                                               unsigned long long seq) {
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    double m[5] = {0, 0, 0, 0, 0};
    // the four lists in one loop, so every list's loads are in flight together
    const int nf = P.n_fblk, nu = P.n_img * P.gram_seg, ns = P.n_chunk + P.n_gpt, nt = n_step_blocks;
    const int nmax = max(max(nf, nu), max(ns, nt));
    constexpr int kStride = kFinBlocks * kFinThreads;
#pragma unroll 2
    for (int i = blockIdx.x * kFinThreads + threadIdx.x; i < nmax; i += kStride) {
        // loads from clamped indices (unconditional, so the compiler issues
        // them all before the first use), accumulated only where in range
        const bool bf = i < nf, bu = i < nu, bs = i < ns, bt = i < nt;
        const int jf = bf ? i : 0, ju = bu ? i : 0, js = bs ? i : 0, jt = bt ? i : 0;
        // (an empty list may have no buffer: its loads are skipped, uniformly)
        double f0 = 0.0, f1 = 0.0, f2 = 0.0, u0 = 0.0, u1 = 0.0, s0 = 0.0, s1 = 0.0;
        double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0, t4 = 0.0;
        if (nf > 0) { f0 = P.part_f[3 * jf]; f1 = P.part_f[3 * jf + 1]; f2 = P.part_f[3 * jf + 2]; }
        if (nu > 0) { u0 = P.part_u[2 * ju]; u1 = P.part_u[2 * ju + 1]; }
        if (ns > 0) { s0 = P.part_s[2 * js]; s1 = P.part_s[2 * js + 1]; }
        if (nt > 0) {
            t0 = P.part_t[kPartT * jt]; t1 = P.part_t[kPartT * jt + 1]; t2 = P.part_t[kPartT * jt + 2];
            t3 = P.part_t[kPartT * jt + 3]; t4 = P.part_t[kPartT * jt + 4];
        }
        if (bf) { s[5] += f0; s[6] += f1; m[4] = fmax(m[4], f2); }
        if (bu) { s[0] += u0; m[0] = fmax(m[0], u1); }
        if (bs) { s[1] += s0; m[1] = fmax(m[1], s1); }
        if (bt) { s[2] += t0; s[3] += t1; s[4] += t2; m[2] = fmax(m[2], t4); m[3] = fmax(m[3], t3); }
    }
    wave_sum(s);
#pragma unroll
    for (int k = 0; k < 5; ++k) m[k] = wave_max(m[k]);
    constexpr int kW = kFinThreads / 64;
    __shared__ double red[kW][12];
    __shared__ int last;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        for (int k = 0; k < 7; ++k) red[wave][k] = s[k];
        for (int k = 0; k < 5; ++k) red[wave][7 + k] = m[k];
    }
    __syncthreads();
    if (threadIdx.x < 12) {   // one thread per scalar, waves in order
        const int k = threadIdx.x;
        double t = red[0][k];
        for (int w = 1; w < kW; ++w) t = k < 7 ? t + red[w][k] : fmax(t, red[w][k]);
        st_wt64(P.fin_part + 12 * blockIdx.x + k, t);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
        last = __hip_atomic_fetch_add((gu32_t*)P.fin_count, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
               (unsigned)(kFinBlocks - 1);
    __syncthreads();
    if (!last) return;
    if (threadIdx.x < 12) {   // the workgroups' partials in workgroup order
        const int k = threadIdx.x;
        double t = ld_wt64(P.fin_part + k);
        for (int g = 1; g < kFinBlocks; ++g) {
            const double v = ld_wt64(P.fin_part + 12 * g + k);
            t = k < 7 ? t + v : fmax(t, v);
        }
        constexpr int kSlot[12] = {kScCost, kScXnorm2E, kScModelAcc, kScCandCost, kScStepnorm2E, kScXnorm2F,
                                   kScStepnorm2F, kScBadX, kScGmaxE, kScCandBad, kScStepBad, kScGmaxF};
        P.scal[kSlot[k]] = t;
        if (P.scal_host) P.scal_host[kSlot[k]] = t;
    }
    if (threadIdx.x == 0)   // ready for the next launch (stream order)
        __hip_atomic_store((gu32_t*)P.fin_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (P.scal_host) {
        // publish to host-mapped memory: every scalar, a system-scope fence,
        // then the sequence word the host polls (no blit, no stream sync)
        if (threadIdx.x == 12) P.scal_host[kScSolveFail] = P.scal[kScSolveFail];
        __syncthreads();   // every slot of P.scal is written
        if (threadIdx.x == 0) {
            const double acc = (P.spec_force || lm_spec_accept(P.scal, P)) ? 1.0 : 0.0;
            P.scal[kScAccept] = acc;
            P.scal_host[kScAccept] = acc;
        }
        if (threadIdx.x < 13) __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(reinterpret_cast<unsigned long long*>(P.scal_host + kScCount), seq,
                               __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if (threadIdx.x == 0) {
        P.scal[kScAccept] = 0.0;   // a rank's partial scalars: decided after the combine
    }
}

// world > 1 over RCCL: the all-gathered per-rank scalars [world][kScMaxEnd]
// combined in rank order (sums, maxima; the replicated slots are this rank's)
// and published to host-mapped memory like finalize_kernel does at one rank,
// so the host polls a sequence word instead of copying and synchronising
__global__ void publish_gathered_kernel(DevProblem P, const double* __restrict__ g, int world,
                                        double* __restrict__ scal, double* __restrict__ host,
                                        unsigned long long seq) {
    const int k = threadIdx.x;
    if (k < kScCount && k != kScAccept) {
        double v = k < kScMaxEnd ? g[k] : scal[k];
        if (k < kScMaxEnd)
            for (int r = 1; r < world; ++r) {
                const double w = g[(size_t)r * kScMaxEnd + k];
                v = k < kScSumEnd ? v + w : fmax(v, w);
            }
        scal[k] = v;
        host[k] = v;
    }
    __syncthreads();   // the combined scalars: the accept decision (as finalize_kernel at one rank)
    if (k == 0) {
        const double acc = (P.spec_force || lm_spec_accept(scal, P)) ? 1.0 : 0.0;
        scal[kScAccept] = acc;
        host[kScAccept] = acc;
    }
    if (k < kScCount) __threadfence_system();
    __syncthreads();
    if (k == 0)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(host + kScCount), seq, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

}  // namespace

size_t solve_window_doubles(const DevProblem& P) {
    const size_t Dp = P.D + 1;
    return Dp * Dp * 36 + (size_t)P.nintr * Dp * 24 + 16 * (size_t)P.nintr * P.nintr + Dp * 6 +
           4 * (size_t)P.nintr;
}

size_t solve_lds_bytes(const DevProblem& P, bool* use_lds) {
    const size_t small = (2 + (size_t)(P.D + 1) * 6) * sizeof(double);
    const size_t full = small + solve_window_doubles(P) * sizeof(double);
    *use_lds = full <= 150 * 1024;
    return *use_lds ? full : small;
}

void ba_solve(const DevProblem& P, double radius, hipStream_t s) {
    bool lds = false;
    const size_t bytes = solve_lds_bytes(P, &lds);
    SFM_REQUIRE(bytes <= 160 * 1024, SFM_ERR_UNSUPPORTED, "RCS band too wide (D=%d)", P.D);
    if (bytes > 64 * 1024) set_dyn_lds((const void*)solve_kernel, bytes);
    hipLaunchKernelGGL(solve_kernel, dim3(1), dim3(256), bytes, s, P, radius, lds ? 1 : 0);
    SFM_HIP(hipGetLastError());
}

int ba_cand_blocks(const DevProblem& P) {
    return std::max(1, (P.n_img + P.n_intr + kCandThreads - 1) / kCandThreads);
}
void ba_cand(const DevProblem& P, const double* extr, const double* intr, double* cand_extr,
             double* cand_intr, CamPre* cand_cp, hipStream_t s) {
    hipLaunchKernelGGL(cand_kernel, dim3(P.n_fblk), dim3(kCandThreads), 0, s, P, extr, intr,
                       cand_extr, cand_intr, cand_cp);
    SFM_HIP(hipGetLastError());
}

int ba_step_blocks(const DevProblem& P) { return P.n_chunk + (P.n_gpt + kGStepThreads - 1) / kGStepThreads; }

void ba_step(const DevProblem& P, const CamPre* cp, const double* intr, const CamPre* cp_cand,
             const double* intr_cand, const double* X, double* X_cand, double radius, hipStream_t s) {
    if (P.n_chunk > 0) {
        const int split = P.step_split;
        const int threads = std::min(kStepThreads, (P.chunk_pts_max * split + 63) / 64 * 64);
        SFM_REQUIRE(P.chunk_pts_max * split <= threads, SFM_ERR_UNSUPPORTED, "step kernel: chunk exceeds the workgroup");
        auto go = [&](auto tag) {
            constexpr int SP = decltype(tag)::value;
            SFM_BY_MODEL_ALL(P, hipLaunchKernelGGL((step_kernel<CM, SP>), dim3(P.n_chunk), dim3(threads), 0, s, P,
                                                   cp, intr, cp_cand, intr_cand, X, X_cand, radius));
        };
        if (split == 8) go(std::integral_constant<int, 8>{});
        else if (split == 4) go(std::integral_constant<int, 4>{});
        else if (split == 2) go(std::integral_constant<int, 2>{});
        else go(std::integral_constant<int, 1>{});
        SFM_HIP(hipGetLastError());
    }
    if (P.n_gpt > 0) {
        const int nb = (P.n_gpt + kGStepThreads - 1) / kGStepThreads;
        SFM_BY_MODEL_ALL(P, hipLaunchKernelGGL(step_general_kernel<CM>, dim3(nb), dim3(kGStepThreads), 0, s, P, cp, intr,
                                           cp_cand, intr_cand, X, X_cand, radius));
        SFM_HIP(hipGetLastError());
    }
}

void ba_finalize(const DevProblem& P, hipStream_t s, unsigned long long seq) {
    hipLaunchKernelGGL(finalize_kernel, dim3(kFinBlocks), dim3(kFinThreads), 0, s, P, ba_step_blocks(P), seq);
    SFM_HIP(hipGetLastError());
}

void ba_publish_gathered(const DevProblem& P, const double* gathered, int world, double* scal, double* scal_host,
                         hipStream_t s, unsigned long long seq) {
    hipLaunchKernelGGL(publish_gathered_kernel, dim3(1), dim3(64), 0, s, P, gathered, world, scal, scal_host, seq);
    SFM_HIP(hipGetLastError());
}

}  // namespace sfm
