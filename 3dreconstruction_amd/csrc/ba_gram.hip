// BA camera side: per-camera precompute, the per-image Gram blocks (U, b,
// cost) and their rescale, Jacobi column scales, fills / copies.
#include "ba_device.h"
namespace sfm {
namespace {
// per-camera precompute (make_campre: ba_cand.h)
__global__ void campre_kernel(const double* __restrict__ extr, int n, CamPre* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double e[6];
    for (int a = 0; a < 6; ++a) e[a] = extr[6 * (size_t)i + a];
    out[i] = make_campre(e);
}

// per-image Gram blocks: U = J_F' J_F (10x10), b = J_F' f, cost
// P.gram_seg (<= kGramSeg) workgroups per image, one observation per lane per step.  Each lane
// keeps its own running sums of the 62 structurally nonzero entries of
// [J_c | J_i | f]' [J_c | J_i | f] (J_i row 0 = [x s, 0, s, 0], row 1 =
// [0, y s, 0, s]) plus the cost on the VALU -- 90 FMAs per observation, no
// LDS staging -- and the wave then reduce-scatters the 64 sums (permlane32 /
// permlane16 swaps, then xor shuffles) so lane l ends with entry l; the four
// waves add in fixed order.
namespace gram {
// F columns of an image block: pose 6 | intrinsics kIW; index FW is f
template <int CM>
constexpr int FW = 6 + kIW<CM>;
// structurally nonzero entries of [J_c | J_i | f] rows 0 / 1 (index 0..FW)
// PINHOLE: J_i row 0 = [x s, 0, s, 0], row 1 = [0, y s, 0, s];
// SNAVELY: J_i rows = [d, f r2, f r2^2, 0] p_r s (column 9 is never a parameter);
// RADIAL3: J_i row 0 = [x c, 1, 0, f x r2, f x r4, f x r6] s, row 1 the same
//          with y and (0, 1) at the principal point
template <int CM>
constexpr bool in0(int i) {
    return CM == SFM_CAM_RADIAL3 ? i != 8 : CM == SFM_CAM_SNAVELY ? i != 9 : (i < 6 || i == 6 || i == 8 || i == 10);
}
template <int CM>
constexpr bool in1(int i) {
    return CM == SFM_CAM_RADIAL3 ? i != 7 : CM == SFM_CAM_SNAVELY ? i != 9 : (i < 6 || i == 7 || i == 9 || i == 10);
}
struct Slots {
    int i[128], j[128], id[13][13], n;
};
template <int CM>
constexpr Slots make_slots() {
    Slots t{};
    t.n = 0;
    for (int a = 0; a < 13; ++a)
        for (int b = 0; b < 13; ++b) t.id[a][b] = -1;
    for (int a = 0; a <= FW<CM>; ++a)
        for (int b = 0; b <= a; ++b)
            if ((in0<CM>(a) && in0<CM>(b)) || (in1<CM>(a) && in1<CM>(b))) {
                t.i[t.n] = a; t.j[t.n] = b;
                t.id[a][b] = t.id[b][a] = t.n;
                ++t.n;
            }
    return t;
}
template <int CM>
struct SlotTable {
    static constexpr Slots kS = make_slots<CM>();
    static constexpr int kCost = kS.n;   // slot of the cost; later slots stay zero
    static constexpr int kPasses = (kS.n + 1 + 63) / 64;   // 64 register sums per lane and pass
};
static_assert(SlotTable<SFM_CAM_PINHOLE>::kS.n == 62, "image Gram: 62 nonzero entries (pinhole)");
static_assert(SlotTable<SFM_CAM_SNAVELY>::kS.n == 55, "image Gram: 55 nonzero entries (Snavely)");
static_assert(SlotTable<SFM_CAM_RADIAL3>::kS.n == 90 && SlotTable<SFM_CAM_RADIAL3>::kPasses == 2,
              "image Gram: 90 nonzero entries in two passes (RADIAL3)");

__device__ __forceinline__ unsigned lo32(double v) { return (unsigned)__double_as_longlong(v); }
__device__ __forceinline__ unsigned hi32(double v) { return (unsigned)(__double_as_longlong(v) >> 32); }
__device__ __forceinline__ double mk(unsigned lo, unsigned hi) {
    return __longlong_as_double(((long long)hi << 32) | lo);
}
// v[j] + partner's v[j] in the lanes that keep j, v[j+H] + partner's in the others
template <int H>
__device__ __forceinline__ void swap_add(double (&v)[64]) {
#pragma unroll
    for (int k = 0; k < H; ++k) {
        const double a = v[k], b = v[k + H];
        double na, nb;
        if (H == 32) {
            const auto l = __builtin_amdgcn_permlane32_swap(lo32(a), lo32(b), false, false);
            const auto h = __builtin_amdgcn_permlane32_swap(hi32(a), hi32(b), false, false);
            na = mk(l[0], h[0]); nb = mk(l[1], h[1]);
        } else {
            const auto l = __builtin_amdgcn_permlane16_swap(lo32(a), lo32(b), false, false);
            const auto h = __builtin_amdgcn_permlane16_swap(hi32(a), hi32(b), false, false);
            na = mk(l[0], h[0]); nb = mk(l[1], h[1]);
        }
        v[k] = na + nb;
    }
}
template <int M>
__device__ __forceinline__ void xor_add(double (&v)[64], int lane) {
    const bool up = (lane & M) != 0;
#pragma unroll
    for (int k = 0; k < M; ++k) {
        const double send = up ? v[k] : v[k + M], keep = up ? v[k + M] : v[k];
        v[k] = keep + __shfl_xor(send, M);
    }
}
// after the call lane l holds the wave sum of v[l] in v[0]
__device__ __forceinline__ void reduce_scatter64(double (&v)[64], int lane) {
    swap_add<32>(v);   // lanes 0-31: entries 0..31, lanes 32-63: 32..63 (in v[0..31])
    swap_add<16>(v);   // row r (16 lanes): entries 16 r + (0..15)
    xor_add<8>(v, lane);
    xor_add<4>(v, lane);
    xor_add<2>(v, lane);
    xor_add<1>(v, lane);
}
}  // namespace gram

// PASS: which 64 slots this launch sums (RADIAL3's 91 sums take two passes,
// each re-linearising the image's observations; the other models one).
template <int CM, int PASS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void image_gram_kernel(DevProblem P, const CamPre* __restrict__ cps,
                                                         const double* __restrict__ intr,
                                                         const double* __restrict__ X,
                                                         const double* __restrict__ gate) {
    if (gate && *gate == 0.0) return;   // speculative pass, step not accepted (uniform)
    using kT = gram::SlotTable<CM>;
    constexpr int IW = kIW<CM>, FW = gram::FW<CM>, S0 = 64 * PASS;
    constexpr bool kHasCost = kT::kCost >= S0 && kT::kCost < S0 + 64;
    // workgroup -> (image with observations, slice); outputs at b = img * ns + seg
    const int ns = P.gram_seg, gi = blockIdx.x / ns, seg = blockIdx.x - ns * gi, img = P.gram_img[gi];
    const int b = img * ns + seg;
    const int a0 = P.img_obs_ptr[img], n = P.img_obs_ptr[img + 1] - a0;
    const int o0 = a0 + (int)((int64_t)n * seg / ns), o1 = a0 + (int)((int64_t)n * (seg + 1) / ns);
    const int colc = P.img_colc[img], coli = P.img_coli[img];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __shared__ CamPre scp;
    __shared__ double sin_[IW], ssc[FW];
    __shared__ double part[4][64], badw[4];
    if (threadIdx.x < sizeof(CamPre) / 8)
        reinterpret_cast<double*>(&scp)[threadIdx.x] = reinterpret_cast<const double*>(&cps[img])[threadIdx.x];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + IW)
        sin_[threadIdx.x - 64] = intr[IW * (size_t)P.img_intr[img] + threadIdx.x - 64];
    if (threadIdx.x >= 96 && threadIdx.x < 96 + FW) {
        const int a = threadIdx.x - 96;
        ssc[a] = a < 6 ? (colc >= 0 ? P.scaleF[colc + a] : 0.0) : P.scaleF[coli + a - 6];
    }
    __syncthreads();
    double g[64];
#pragma unroll
    for (int k = 0; k < 64; ++k) g[k] = 0.0;
    double bad = 0.0;
    // software pipeline: point ids / measurements two iterations ahead, the
    // point itself one iteration ahead
    auto fetch_ids = [&](int base, int& p, double2& uv) {
        const int q = base + lane;
        p = q < o1 ? P.img_pt[q] : -1;
        uv = q < o1 ? reinterpret_cast<const double2*>(P.img_uv)[q] : double2{0.0, 0.0};
    };
    auto fetch_x = [&](int p, double (&x)[3]) {
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] = p >= 0 ? X[3 * (size_t)p + a] : 0.0;
    };
    // one observation's contribution (lane's running sums, observation order)
    auto process = [&](int p_cur, const double2& uv, const double (&Xp)[3]) {
    // re-read the staged camera from LDS each step instead of keeping its
    // 28 doubles live across the loop (register budget of 2 waves/SIMD)
    asm volatile("" ::: "memory");
    if (p_cur >= 0) {
        LinT<CM> L;
        linearize<CM, true, true, false>(scp, sin_, Xp, uv.x, uv.y, P.huber_a, L);
        if constexpr (kHasCost) g[kT::kCost - S0] += L.half_rho;
        bad = fmax(bad, L.ok ? 0.0 : 1.0);
        // unscaled rows; the per-image column scales are applied to the sums
        auto r = [&](int q, int i) -> double {
            return i < 6 ? L.Jc[q][i] : i < FW ? L.Ji[q][i - 6] : L.f[q];
        };
#pragma unroll
        for (int s = 0; s < 64; ++s) {
            if (S0 + s >= kT::kS.n) break;
            const int i = kT::kS.i[S0 + s], j = kT::kS.j[S0 + s];
            if (gram::in0<CM>(i) && gram::in0<CM>(j)) g[s] = fma(r(0, i), r(0, j), g[s]);
            if (gram::in1<CM>(i) && gram::in1<CM>(j)) g[s] = fma(r(1, i), r(1, j), g[s]);
        }
    }
    };
    // three stages: the point gather (random rows of X) two iterations ahead
    int p_c, p_n, p_nn;
    double2 uv_c, uv_n, uv_nn;
    double x_c[3], x_n[3];
    fetch_ids(o0 + 64 * wave, p_c, uv_c);
    fetch_ids(o0 + 64 * wave + 256, p_n, uv_n);
    fetch_ids(o0 + 64 * wave + 512, p_nn, uv_nn);
    fetch_x(p_c, x_c);
    fetch_x(p_n, x_n);
    for (int base = o0 + 64 * wave; base < o1; base += 256) {
        const int p_cur = p_c;
        const double2 uv = uv_c;
        const double Xp[3] = {x_c[0], x_c[1], x_c[2]};
        p_c = p_n; uv_c = uv_n;
        x_c[0] = x_n[0]; x_c[1] = x_n[1]; x_c[2] = x_n[2];
        p_n = p_nn; uv_n = uv_nn;
        fetch_x(p_n, x_n);
        fetch_ids(base + 768, p_nn, uv_nn);
        process(p_cur, uv, Xp);
    }
    gram::reduce_scatter64(g, lane);
    bad = wave_max(bad);
    part[wave][lane] = g[0];
    if (lane == 0) badw[wave] = bad;
    __syncthreads();
    // slot s of this pass (S0 <= s < S0 + 64) summed over the four waves
    auto tot = [&](int s) { return ((part[0][s - S0] + part[1][s - S0]) + part[2][s - S0]) + part[3][s - S0]; };
    auto mine = [&](int s) { return s >= S0 && s < S0 + 64; };
    if (threadIdx.x < FW * FW) {
        const int i = threadIdx.x / FW, j = threadIdx.x % FW, s = kT::kS.id[i][j];
        if (s >= 0 ? mine(s) : PASS == 0) {
            const double u = s >= 0 ? ssc[i] * ssc[j] * tot(s) : 0.0;
            P.U[(size_t)b * (FW * FW) + threadIdx.x] = u;
            if (i == j) P.Ucn[(size_t)b * FW + i] = u;
        }
    }
    if (threadIdx.x >= 160 && threadIdx.x < 160 + FW) {
        const int i = threadIdx.x - 160, s = kT::kS.id[FW][i];
        if (mine(s)) P.Ub[(size_t)b * FW + i] = ssc[i] * tot(s);
    }
    if (kHasCost && threadIdx.x == 192) {
        P.part_u[2 * (size_t)b] = tot(kT::kCost);
        P.part_u[2 * (size_t)b + 1] = fmax(fmax(badw[0], badw[1]), fmax(badw[2], badw[3]));
    }
}

// Iteration 0 after the Jacobi scales are known: the image Gram pass applies
// the per-image column scales to its sums (u = (s_i s_j) * sum), so the
// scaled blocks follow from the unit-scale pass's exactly, without a second
// linearisation of every observation (bit-identical to re-running the pass).
template <int CM>
__global__ __launch_bounds__(128) void gram_rescale_kernel(DevProblem P) {
    using kT = gram::SlotTable<CM>;
    constexpr int FW = gram::FW<CM>;
    const int gi = blockIdx.x / P.gram_seg, img = P.gram_img[gi];
    const int b = img * P.gram_seg + (blockIdx.x - gi * P.gram_seg);
    const int colc = P.img_colc[img], coli = P.img_coli[img];
    __shared__ double ssc[FW];
    if (threadIdx.x < FW) {
        const int a = threadIdx.x;
        ssc[a] = a < 6 ? (colc >= 0 ? P.scaleF[colc + a] : 0.0) : P.scaleF[coli + a - 6];
    }
    __syncthreads();
    for (int e = threadIdx.x; e < FW * FW; e += 128) {
        const int i = e / FW, j = e % FW, s = kT::kS.id[i][j];
        const double u = s >= 0 ? ssc[i] * ssc[j] * P.U[(size_t)b * (FW * FW) + e] : 0.0;
        P.U[(size_t)b * (FW * FW) + e] = u;
        if (i == j) P.Ucn[(size_t)b * FW + i] = u;
    }
    if (threadIdx.x < FW) {
        const int i = threadIdx.x;
        P.Ub[(size_t)b * FW + i] = ssc[i] * P.Ub[(size_t)b * FW + i];
    }
}

__global__ void fill_kernel(double* p, int64_t n, double v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// up to kSegs copies (src) or fills (src null: value v) in one launch, grid-stride
__global__ void segs_kernel(SegList L) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < L.n; ++k) {
        const Seg& g = L.seg[k];
        for (int64_t j = i; j < g.n; j += stride) g.dst[j] = g.src ? g.src[j] : g.v;
    }
}

__global__ void fscale_kernel(DevProblem P) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < P.nF) P.scaleF[c] = 1.0 / (1.0 + sqrt(P.cnF[c]));
}

}  // namespace

void ba_campre(const double* extr, int n_img, CamPre* out, hipStream_t s) {
    if (n_img <= 0) return;
    hipLaunchKernelGGL(campre_kernel, dim3((n_img + 127) / 128), dim3(128), 0, s, extr, n_img, out);
    SFM_HIP(hipGetLastError());
}

void ba_image_gram(const DevProblem& P, const CamPre* cp, const double* intr, const double* X,
                   hipStream_t s, const double* gate) {
    if (P.n_gram_img <= 0) return;
    SFM_BY_MODEL_ALL(P, {
        hipLaunchKernelGGL((image_gram_kernel<CM, 0>), dim3(P.n_gram_img * P.gram_seg), dim3(256), 0, s, P, cp, intr,
                           X, gate);
        if constexpr (gram::SlotTable<CM>::kPasses > 1)
            hipLaunchKernelGGL((image_gram_kernel<CM, 1>), dim3(P.n_gram_img * P.gram_seg), dim3(256), 0, s, P, cp,
                               intr, X, gate);
    });
    SFM_HIP(hipGetLastError());
}

void ba_gram_rescale(const DevProblem& P, hipStream_t s) {
    if (P.n_gram_img <= 0) return;
    SFM_BY_MODEL_ALL(P, hipLaunchKernelGGL(gram_rescale_kernel<CM>, dim3(P.n_gram_img * P.gram_seg), dim3(128), 0, s, P));
    SFM_HIP(hipGetLastError());
}

void ba_fill(double* p, int64_t n, double v, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, n, v);
    SFM_HIP(hipGetLastError());
}

void ba_segs(const SegList& L, hipStream_t s) {
    int64_t nmax = 0;
    for (int k = 0; k < L.n; ++k) nmax = std::max(nmax, L.seg[k].n);
    if (nmax <= 0) return;
    const unsigned g = (unsigned)std::min<int64_t>((nmax + 255) / 256, 2048);
    hipLaunchKernelGGL(segs_kernel, dim3(g), dim3(256), 0, s, L);
    SFM_HIP(hipGetLastError());
}

void ba_fscale(const DevProblem& P, hipStream_t s) {
    if (P.nF <= 0) return;
    hipLaunchKernelGGL(fscale_kernel, dim3((unsigned)((P.nF + 255) / 256)), dim3(256), 0, s, P);
    SFM_HIP(hipGetLastError());
}

}  // namespace sfm
