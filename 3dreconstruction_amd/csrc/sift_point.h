// SIFT extraction (include/sfmcore.h, "SIFT extraction"): the
// arithmetic written once for the device kernels (sift.hip) and the serial
// host twin (sift.cpp, sfm_sift_host).  Lowe's detector and descriptor with
// VLFeat's parameters and its table/bit-trick replacements for exp, sqrt and
// atan2, each restated here as plain + - * / so that host and device run the
// same statements and neither depends on a math library: the square root by
// the reciprocal-root bit estimate and two Newton steps, the arc tangent by a
// cubic in (x - |y|) / (x + |y|), exp(-x) by a 256-step table with linear
// interpolation (the table is built on the host), 2^t and sin/cos by short
// Taylor sums.  Every function is a pure function of its arguments; which
// thread calls it, and in which order the callers add what it returns, is the
// callers' business and is spelled out where the two callers meet.
#pragma once
#include <cstdint>
#include <cstring>

#include "common.h"

namespace sfm {
namespace sift {

constexpr int kMaxScales = 8;                 // S
constexpr int kMaxLevels = kMaxScales + 3;    // s = -1 .. S+1
constexpr int kMaxHalf = 32;                  // Gaussian half-width the convolution tiles hold
constexpr int kOriBins = 36;
constexpr int kExpnSize = 256;                // exp(-x) table: x in [0, 25]
constexpr double kExpnMax = 25.0;
constexpr double kPi = 3.141592653589793;
constexpr float kEpsF = 1.19209290E-07F;
constexpr double kEpsD = 2.220446049250313e-16;

// the levels of one octave of one image (level i is s = i - 1), row-major w x h
struct Levels {
    const float* L[kMaxLevels];
};
// a refined keypoint: full-resolution x, y, sigma and the level it was found in
struct Keypoint {
    float x, y, sigma;
    int32_t k;
};

// ---- the small helpers --------------------------------------------------------

__host__ __device__ inline float bits_to_float(int32_t i) {
    float f;
    memcpy(&f, &i, 4);
    return f;
}
__host__ __device__ inline int32_t float_to_bits(float f) {
    int32_t i;
    memcpy(&i, &f, 4);
    return i;
}
__host__ __device__ inline float absf(float x) { return x < 0.f ? -x : x; }
__host__ __device__ inline double absd(double x) { return x < 0.0 ? -x : x; }

// floor to an integer by truncation and one correction
__host__ __device__ inline int floor_f(float x) {
    const int xi = (int)x;
    return (x >= 0.f || (float)xi == x) ? xi : xi - 1;
}
__host__ __device__ inline int floor_d(double x) {
    const int xi = (int)x;
    return (x >= 0.0 || (double)xi == x) ? xi : xi - 1;
}

// x^(-1/2): the shifted-exponent estimate and two Newton steps, in float
__host__ __device__ inline float fast_rsqrt(float x) {
    const float xh = 0.5f * x;
    float y = bits_to_float(0x5f3759df - (float_to_bits(x) >> 1));
    y = y * (1.5f - xh * y * y);
    y = y * (1.5f - xh * y * y);
    return y;
}
__host__ __device__ inline float fast_sqrt(float x) { return ((double)x < 1e-8) ? 0.f : x * fast_rsqrt(x); }

// atan2(y, x) by the cubic pi/4 - 0.9675 r + 0.1821 r^3 in the octant ratio r
__host__ __device__ inline float fast_atan2(float y, float x) {
    const float c3 = 0.1821f, c1 = 0.9675f;
    const float ay = absf(y) + kEpsF;
    float r, a;
    if (x >= 0.f) {
        r = (x - ay) / (x + ay);
        a = (float)(kPi / 4);
    } else {
        r = (x + ay) / (ay - x);
        a = (float)(3 * kPi / 4);
    }
    a += (c3 * r * r - c1) * r;
    return y < 0.f ? -a : a;
}

// into [0, 2 pi] by whole turns (the arguments here are within two turns)
__host__ __device__ inline float mod_2pi(float x) {
    const float t = (float)(2 * kPi);
    for (int i = 0; i < 4 && x > t; ++i) x -= t;
    for (int i = 0; i < 4 && x < 0.f; ++i) x += t;
    return x;
}

// exp(-x), x >= 0, from the table tab[k] = exp(-25 k / 256), k <= 257
__host__ __device__ inline double fast_expn(const double* tab, double x) {
    if (x > kExpnMax) return 0.0;
    x *= kExpnSize / kExpnMax;
    const int i = floor_d(x);
    const double r = x - i;
    const double a = tab[i], b = tab[i + 1];
    return a + r * (b - a);
}

// 2^t for moderate t: 2^floor(t) by doubling, the rest as sqrt(2) exp(u ln 2),
// |u| <= 1/2, by its Taylor sum to the 14th power (below 1e-17)
__host__ __device__ inline double exp2_small(double t) {
    const int n = floor_d(t);
    const double u = ((t - n) - 0.5) * 0.6931471805599453;
    double p = 1.0;
    for (int k = 14; k >= 1; --k) p = 1.0 + p * u / k;
    p *= 1.4142135623730951;
    for (int i = 0; i < n; ++i) p *= 2.0;
    for (int i = 0; i > n; --i) p *= 0.5;
    return p;
}

// sin and cos of an angle of a few turns: the nearest multiple of pi/2 taken
// off, Taylor sums to the 17th / 16th power on what is left (below 1e-17)
__host__ __device__ inline void sincos_small(double a, double& s, double& c) {
    const int q = floor_d(a / (kPi / 2) + 0.5);
    const double r = a - q * (kPi / 2), r2 = r * r;
    double ps = 1.0, pc = 1.0;
    for (int k = 8; k >= 1; --k) {
        ps = 1.0 - ps * r2 / ((2 * k) * (2 * k + 1));
        pc = 1.0 - pc * r2 / ((2 * k - 1) * (2 * k));
    }
    ps *= r;
    switch (q & 3) {
        case 0: s = ps; c = pc; break;
        case 1: s = pc; c = -ps; break;
        case 2: s = -ps; c = -pc; break;
        default: s = -pc; c = ps; break;
    }
}

// ---- scale space ---------------------------------------------------------------

// one output of a 1-D Gaussian of half-width W: the 2W+1 products added in tap
// order in float; ld(j) is the input at offset j - W, the border continued
template <class Load>
__host__ __device__ inline float conv_acc(Load ld, const float* taps, int W) {
    float acc = 0.f;
    for (int j = 0; j <= 2 * W; ++j) acc += ld(j) * taps[j];
    return acc;
}

__host__ __device__ inline float dog(const Levels& lv, int k, int64_t i) { return lv.L[k + 1][i] - lv.L[k][i]; }

// ---- detection -------------------------------------------------------------------

// Cell (x, y) of DoG level k (1 <= k <= S, 1 <= x <= w-2, 1 <= y <= h-2): a
// strict 3x3x3 extremum at or beyond 0.8 tp, refined by up to five steps of
// the quadratic fit (the cell moves by one when the offset passes 0.6 and the
// move stays inside), then the contrast, edge, offset and border tests.
__host__ __device__ inline bool detect_cell(const Levels& lv, int w, int h, int S, int x, int y, int k, double tp,
                                            double te, double sigma0, double xper, Keypoint* out) {
    const int64_t yo = w;
    {
        const int64_t c = (int64_t)y * w + x;
        const float v = dog(lv, k, c);
        const bool up = (double)v >= 0.8 * tp, dn = (double)v <= -0.8 * tp;
        if (!up && !dn) return false;
        bool is_max = up, is_min = dn;
        for (int dk = -1; dk <= 1; ++dk)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!dk && !dy && !dx) continue;
                    const float n = dog(lv, k + dk, c + dy * yo + dx);
                    is_max = is_max && v > n;
                    is_min = is_min && v < n;
                }
        if (!is_max && !is_min) return false;
    }
    double Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dss = 0, Dxy = 0;
    double b[3] = {0, 0, 0};
    float centre = 0.f;
    int dx = 0, dy = 0;
    for (int iter = 0; iter < 5; ++iter) {
        x += dx;
        y += dy;
        const int64_t c = (int64_t)y * w + x;
#define SIFT_AT(ax, ay, ak) dog(lv, k + (ak), c + (ay) * yo + (ax))
        centre = SIFT_AT(0, 0, 0);
        Dx = 0.5 * (SIFT_AT(1, 0, 0) - SIFT_AT(-1, 0, 0));
        Dy = 0.5 * (SIFT_AT(0, 1, 0) - SIFT_AT(0, -1, 0));
        Ds = 0.5 * (SIFT_AT(0, 0, 1) - SIFT_AT(0, 0, -1));
        Dxx = (SIFT_AT(1, 0, 0) + SIFT_AT(-1, 0, 0)) - 2.0 * centre;
        Dyy = (SIFT_AT(0, 1, 0) + SIFT_AT(0, -1, 0)) - 2.0 * centre;
        Dss = (SIFT_AT(0, 0, 1) + SIFT_AT(0, 0, -1)) - 2.0 * centre;
        Dxy = 0.25 * (SIFT_AT(1, 1, 0) + SIFT_AT(-1, -1, 0) - SIFT_AT(-1, 1, 0) - SIFT_AT(1, -1, 0));
        const double Dxs = 0.25 * (SIFT_AT(1, 0, 1) + SIFT_AT(-1, 0, -1) - SIFT_AT(-1, 0, 1) - SIFT_AT(1, 0, -1));
        const double Dys = 0.25 * (SIFT_AT(0, 1, 1) + SIFT_AT(0, -1, -1) - SIFT_AT(0, -1, 1) - SIFT_AT(0, 1, -1));
#undef SIFT_AT
        // H d = -g by Gauss-Jordan with the largest pivot of each column; a
        // pivot below 1e-10 gives the zero offset.  A[r][c], rows r.
        double A[3][3] = {{Dxx, Dxy, Dxs}, {Dxy, Dyy, Dys}, {Dxs, Dys, Dss}};
        b[0] = -Dx; b[1] = -Dy; b[2] = -Ds;
        for (int j = 0; j < 3; ++j) {
            double pv = 0, pa = 0;
            int pi = -1;
            for (int i = j; i < 3; ++i) {
                const double a = A[i][j], aa = absd(a);
                if (aa > pa) { pv = a; pa = aa; pi = i; }
            }
            if (pa < (double)1e-10f) {
                b[0] = b[1] = b[2] = 0;
                break;
            }
            for (int c2 = j; c2 < 3; ++c2) {
                const double t = A[pi][c2];
                A[pi][c2] = A[j][c2];
                A[j][c2] = t / pv;
            }
            const double t = b[j];
            b[j] = b[pi];
            b[pi] = t;
            b[j] /= pv;
            for (int i = j + 1; i < 3; ++i) {
                const double f = A[i][j];
                for (int c2 = j; c2 < 3; ++c2) A[i][c2] -= f * A[j][c2];
                b[i] -= f * b[j];
            }
        }
        for (int i = 2; i > 0; --i) {
            const double f = b[i];
            for (int r = i - 1; r >= 0; --r) b[r] -= f * A[r][i];
        }
        dx = ((b[0] > 0.6 && x < w - 2) ? 1 : 0) + ((b[0] < -0.6 && x > 1) ? -1 : 0);
        dy = ((b[1] > 0.6 && y < h - 2) ? 1 : 0) + ((b[1] < -0.6 && y > 1) ? -1 : 0);
        if (dx == 0 && dy == 0) break;
    }
    const double val = centre + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2]);
    const double score = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
    const double xn = x + b[0], yn = y + b[1], sn = (k - 1) + b[2];
    const bool good = absd(val) > tp && score < (te + 1) * (te + 1) / te && score >= 0 && absd(b[0]) < 1.5 &&
                      absd(b[1]) < 1.5 && absd(b[2]) < 1.5 && xn >= 0 && xn <= w - 1 && yn >= 0 && yn <= h - 1 &&
                      sn >= -1 && sn <= S + 1;
    if (!good) return false;
    out->x = (float)(xn * xper);
    out->y = (float)(yn * xper);
    out->sigma = (float)(sigma0 * exp2_small(sn / S) * xper);
    out->k = k;
    return true;
}

// ---- gradient --------------------------------------------------------------------

// magnitude and angle in [0, 2 pi] of level L at (x, y): central differences,
// one-sided at the border
__host__ __device__ inline void gradient(const float* L, int w, int h, int x, int y, float& mod, float& ang) {
    const int64_t c = (int64_t)y * w + x;
    const float gx = x == 0 ? L[c + 1] - L[c] : x == w - 1 ? L[c] - L[c - 1] : 0.5f * (L[c + 1] - L[c - 1]);
    const float gy = y == 0 ? L[c + w] - L[c] : y == h - 1 ? L[c] - L[c - w] : 0.5f * (L[c + w] - L[c - w]);
    mod = fast_sqrt(gx * gx + gy * gy);
    ang = mod_2pi((float)((double)fast_atan2(gy, gx) + 2 * kPi));
}

// ---- orientation -----------------------------------------------------------------

// the window of a keypoint in its octave: centre, the clipped square of
// samples and the Gaussian's 2 sigma_w^2
struct OriWindow {
    double x, y, two_s2;
    int xi, yi, W, x0, x1, y0, y1;   // samples xi + x0 .. xi + x1, yi + y0 .. yi + y1
    bool ok;
};
__host__ __device__ inline OriWindow ori_window(const Keypoint& kp, double xper, int w, int h) {
    OriWindow o;
    o.x = kp.x / xper;
    o.y = kp.y / xper;
    const double sw = 1.5 * (kp.sigma / xper);
    o.two_s2 = 2 * sw * sw;
    o.xi = (int)(o.x + 0.5);
    o.yi = (int)(o.y + 0.5);
    const int W = floor_d(3.0 * sw);
    o.W = W > 1 ? W : 1;
    o.ok = !(o.xi < 0 || o.xi > w - 1 || o.yi < 0 || o.yi > h - 1);
    o.x0 = -o.W > -o.xi ? -o.W : -o.xi;
    o.x1 = o.W < w - 1 - o.xi ? o.W : w - 1 - o.xi;
    o.y0 = -o.W > -o.yi ? -o.W : -o.yi;
    o.y1 = o.W < h - 1 - o.yi ? o.W : h - 1 - o.yi;
    return o;
}
// sample (xs, ys) of the window: false outside the disc; else the two
// neighbouring bins (bin, bin + 1 mod 36) and what each receives
__host__ __device__ inline bool ori_sample(const OriWindow& o, const float* grad, int w, const double* expn, int xs,
                                           int ys, int& bin, double& w0, double& w1) {
    const double dx = (double)(o.xi + xs) - o.x, dy = (double)(o.yi + ys) - o.y;
    const double r2 = dx * dx + dy * dy;
    if (r2 >= o.W * o.W + 0.6) return false;
    const double wgt = fast_expn(expn, r2 / o.two_s2);
    const float* g = grad + 2 * ((int64_t)(o.yi + ys) * w + (o.xi + xs));
    const double mod = g[0], ang = g[1];
    const double fbin = kOriBins * ang / (2 * kPi);
    const int b = floor_d(fbin - 0.5);
    const double rbin = fbin - b - 0.5;
    bin = (b + kOriBins) % kOriBins;
    w0 = (1 - rbin) * mod * wgt;
    w1 = rbin * mod * wgt;
    return true;
}
// the histogram, in place: six passes of the circular 3-box, then the peaks at
// or above 0.8 of the largest, refined by the parabola through their
// neighbours, in bin order, four at most
__host__ __device__ inline int ori_peaks(double* hist, double* angles) {
    for (int it = 0; it < 6; ++it) {
        double prev = hist[kOriBins - 1];
        const double first = hist[0];
        for (int i = 0; i < kOriBins - 1; ++i) {
            const double nh = (prev + hist[i] + hist[i + 1]) / 3.0;
            prev = hist[i];
            hist[i] = nh;
        }
        hist[kOriBins - 1] = (prev + hist[kOriBins - 1] + first) / 3.0;
    }
    double maxh = 0;
    for (int i = 0; i < kOriBins; ++i) maxh = maxh > hist[i] ? maxh : hist[i];
    int n = 0;
    for (int i = 0; i < kOriBins && n < 4; ++i) {
        const double h0 = hist[i], hm = hist[(i + kOriBins - 1) % kOriBins], hp = hist[(i + 1) % kOriBins];
        if (h0 > 0.8 * maxh && h0 > hm && h0 > hp) {
            const double di = -0.5 * (hp - hm) / (hp + hm - 2 * h0);
            angles[n++] = 2 * kPi * (i + di + 0.5) / kOriBins;
        }
    }
    return n;
}

// ---- descriptor ------------------------------------------------------------------

struct DescWindow {
    double x, y, st, ct, sbp, angle;
    int xi, yi, x0, x1, y0, y1;
    bool ok;
};
__host__ __device__ inline DescWindow desc_window(const Keypoint& kp, double angle, double xper, int w, int h) {
    DescWindow d;
    d.x = kp.x / xper;
    d.y = kp.y / xper;
    d.angle = angle;
    d.xi = (int)(d.x + 0.5);
    d.yi = (int)(d.y + 0.5);
    sincos_small(angle, d.st, d.ct);
    d.sbp = 3.0 * (kp.sigma / xper) + kEpsD;
    const int W = floor_d(1.4142135623730951 * d.sbp * 5 / 2.0 + 0.5);
    d.ok = !(d.xi < 0 || d.xi >= w || d.yi < 0 || d.yi >= h - 1);
    d.x0 = -W > 1 - d.xi ? -W : 1 - d.xi;
    d.x1 = W < w - d.xi - 2 ? W : w - d.xi - 2;
    d.y0 = -W > 1 - d.yi ? -W : 1 - d.yi;
    d.y1 = W < h - d.yi - 2 ? W : h - d.yi - 2;
    return d;
}
// one sample in the keypoint's frame: the lower corner of the 2x2x2 bins it
// spreads over, its offsets from that corner, and window x magnitude
struct DescSample {
    int bx, by, bt;
    float rx, ry, rt, wm;
};
__host__ __device__ inline DescSample desc_sample(const DescWindow& d, const float* grad, int w, const double* expn,
                                                  int dxi, int dyi) {
    const float* g = grad + 2 * ((int64_t)(d.yi + dyi) * w + (d.xi + dxi));
    const float mod = g[0], ang = g[1];
    const float theta = mod_2pi((float)(ang - d.angle));
    const float dx = (float)(d.xi + dxi - d.x), dy = (float)(d.yi + dyi - d.y);
    const float nx = (float)((d.ct * dx + d.st * dy) / d.sbp);
    const float ny = (float)((-d.st * dx + d.ct * dy) / d.sbp);
    const float nt = (float)((8 * theta) / (2 * kPi));
    const float win = (float)fast_expn(expn, (nx * nx + ny * ny) / 8.0);
    DescSample s;
    s.bx = floor_f((float)(nx - 0.5));
    s.by = floor_f((float)(ny - 0.5));
    s.bt = floor_f(nt);
    s.rx = (float)(nx - (s.bx + 0.5));
    s.ry = (float)(ny - (s.by + 0.5));
    s.rt = nt - s.bt;
    s.wm = win * mod;
    return s;
}
// what the sample gives the bin (dbx, dby, dbt) in {0, 1}^3 above its corner
__host__ __device__ inline float desc_weight(const DescSample& s, int dbx, int dby, int dbt) {
    return s.wm * absf(1 - dbx - s.rx) * absf(1 - dby - s.ry) * absf(1 - dbt - s.rt);
}
// spatial bins run -2 .. 1; descriptor index of (bx, by, bt)
__host__ __device__ inline int desc_index(int bx, int by, int bt) { return (by + 2) * 32 + (bx + 2) * 8 + bt; }

__host__ __device__ inline void desc_normalize(float* d) {
    float n = 0.f;
    for (int i = 0; i < 128; ++i) n += d[i] * d[i];
    n = fast_sqrt(n) + kEpsF;
    for (int i = 0; i < 128; ++i) d[i] /= n;
}
// the accumulated histogram d[128] (changed in place) to bytes: unit length,
// clamp at 0.2, unit length again; then the square root of the L1-normalised
// entries times 512 (RootSIFT), or the entries times 512; the integer part's
// low byte is kept
__host__ __device__ inline void desc_finish(float* d, int root_sift, uint8_t* out) {
    desc_normalize(d);
    for (int i = 0; i < 128; ++i)
        if ((double)d[i] > 0.2) d[i] = (float)0.2;
    desc_normalize(d);
    if (root_sift) {
        float sum = 0.f;
        for (int i = 0; i < 128; ++i) sum += d[i];
        for (int i = 0; i < 128; ++i) {
            const float v = 512.f * __builtin_sqrtf(d[i] / sum);
            out[i] = v == v ? (uint8_t)(int)v : (uint8_t)0;
        }
    } else {
        for (int i = 0; i < 128; ++i) {
            const float v = 512.f * d[i];
            out[i] = v == v ? (uint8_t)(int)v : (uint8_t)0;
        }
    }
}

}  // namespace sift
}  // namespace sfm
