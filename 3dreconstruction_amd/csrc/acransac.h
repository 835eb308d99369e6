// What the two a-contrario RANSAC kernels (fmat.hip: the F-matrix filter,
// resect.hip: camera resection) and the resection's serial host twin
// (resect.cpp) share: the exact-operation log10 and cube root, the cubic
// solver, the restatement of libstdc++'s uniform_int_distribution over a raw
// mt19937 stream, the sort key of an error, and the host's copy of that stream.
// Everything is the arithmetic of oracle/fmat_oracle.cpp: the same operation
// sequences, meant to be compiled without FMA contraction (the including file
// sets `#pragma clang fp contract(off)` first).  Builds with a plain host
// compiler too.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

namespace sfm {
namespace {

#if !defined(__HIPCC__)   // a plain host compiler
using std::fabs;
using std::frexp;
using std::ldexp;
using std::sqrt;
#endif

constexpr int64_t kRngWords = 1 << 18;   // raw mt19937 outputs a problem may draw

// ---- exact-operation math, identical to oracle/fmat_oracle.cpp ---------------
__host__ __device__ double det_log10(double x) {
    int e = 0;
    double m = frexp(x, &e);
    if (m < 0.70710678118654752440) {
        m = m * 2.0;
        e = e - 1;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double s2 = s * s;
    double p = 1.0 / 23.0;
    p = p * s2 + 1.0 / 21.0;
    p = p * s2 + 1.0 / 19.0;
    p = p * s2 + 1.0 / 17.0;
    p = p * s2 + 1.0 / 15.0;
    p = p * s2 + 1.0 / 13.0;
    p = p * s2 + 1.0 / 11.0;
    p = p * s2 + 1.0 / 9.0;
    p = p * s2 + 1.0 / 7.0;
    p = p * s2 + 1.0 / 5.0;
    p = p * s2 + 1.0 / 3.0;
    p = p * s2 + 1.0;
    const double ln = (double)e * 0.69314718055994530942 + 2.0 * s * p;
    return ln * 0.43429448190325182765;
}

__host__ __device__ double det_cbrt(double v) {
    int e = 0;
    double m = frexp(v, &e);
    int r = e % 3;
    if (r < 0) r += 3;
    m = ldexp(m, r);
    e = e - r;
    double y = 1.0;
    for (int it = 0; it < 8; ++it) y = y - (y * y * y - m) / (3.0 * y * y);
    return ldexp(y, e / 3);
}

__host__ __device__ __forceinline__ double dep_cubic(double t, double q3, double r2) { return (t * t - q3) * t + r2; }

__host__ __device__ double bisect(double lo, double hi, double q3, double r2, bool up) {
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        const double g = dep_cubic(mid, q3, r2);
        if ((g < 0.0) == up) lo = mid;
        else hi = mid;
    }
    return 0.5 * (lo + hi);
}

// real roots of P[0] + P[1] x + P[2] x^2 + P[3] x^3 (1 or 3, ascending when 3);
// 0 when P[0] == 0 (the 7-point caller's rule)
[[maybe_unused]] __host__ __device__ int solve_cubic(const double P[4], double roots[3]) {
    if (P[0] == 0.0) return 0;
    const double a = P[2] / P[3], b = P[1] / P[3], c = P[0] / P[3];
    const double q = a * a - 3.0 * b;
    const double r = 2.0 * a * a * a - 9.0 * a * b + 27.0 * c;
    const double Q = q / 9.0;
    const double R = r / 54.0;
    const double Q3 = Q * Q * Q;
    const double R2 = R * R;
    const double CR2 = 729.0 * r * r;
    const double CQ3 = 2916.0 * q * q * q;
    const double a3 = a / 3.0;
    if (R == 0.0 && Q == 0.0) {
        roots[0] = roots[1] = roots[2] = -a3;
        return 3;
    }
    if (CR2 == CQ3) {
        const double sQ = sqrt(Q);
        if (R > 0.0) {
            roots[0] = -2.0 * sQ - a3;
            roots[1] = sQ - a3;
            roots[2] = sQ - a3;
        } else {
            roots[0] = -sQ - a3;
            roots[1] = -sQ - a3;
            roots[2] = 2.0 * sQ - a3;
        }
        return 3;
    }
    if (CR2 < CQ3) {
        const double sQ = sqrt(Q);
        const double q3 = 3.0 * Q, r2 = 2.0 * R;
        roots[0] = bisect(-2.0 * sQ, -sQ, q3, r2, true) - a3;
        roots[1] = bisect(-sQ, sQ, q3, r2, false) - a3;
        roots[2] = bisect(sQ, 2.0 * sQ, q3, r2, true) - a3;
        return 3;
    }
    const double sgnR = R >= 0.0 ? 1.0 : -1.0;
    const double A = -sgnR * det_cbrt(fabs(R) + sqrt(R2 - Q3));
    roots[0] = A + Q / A - a3;
    return 1;
}

// libstdc++ uniform_int_distribution<uint32_t>(lo, hi) over mt19937 (32-bit
// outputs): Lemire's nearly-divisionless downscaling with a 64-bit product
struct Stream {
    const uint32_t* w;
    int64_t pos, cap;
    bool over = false;
    __host__ __device__ uint32_t next() {
        if (pos >= cap) { over = true; return 0u; }
        return w[pos++];
    }
    __host__ __device__ uint32_t uniform(uint32_t lo, uint32_t hi) {
        const uint32_t urange = hi - lo;
        if (urange == 0xFFFFFFFFu) return lo + next();
        const uint32_t range = urange + 1u;
        uint64_t product = (uint64_t)next() * (uint64_t)range;
        uint32_t low = (uint32_t)product;
        if (low < range) {
            const uint32_t threshold = (0u - range) % range;
            while (low < threshold && !over) {
                product = (uint64_t)next() * (uint64_t)range;
                low = (uint32_t)product;
            }
        }
        return lo + (uint32_t)(product >> 32);
    }
};

__host__ __device__ __forceinline__ unsigned long long err_key(double r) {
    // non-negative doubles order as their bit patterns; NaN never reaches the
    // threshold (filtered before)
#if defined(__HIP_DEVICE_COMPILE__)
    return (unsigned long long)__double_as_longlong(r);
#else
    unsigned long long k;
    std::memcpy(&k, &r, sizeof k);
    return k;
#endif
}
__host__ __device__ __forceinline__ double key_err(unsigned long long k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)k);
#else
    double r;
    std::memcpy(&r, &k, sizeof r);
    return r;
#endif
}

// raw mt19937(default_seed) outputs, generated once per process
inline const std::vector<uint32_t>& rng_stream() {
    static const std::vector<uint32_t> w = [] {
        std::vector<uint32_t> v((size_t)kRngWords);
        std::mt19937 g(std::mt19937::default_seed);
        for (auto& x : v) x = (uint32_t)g();
        return v;
    }();
    return w;
}

}  // namespace
}  // namespace sfm
