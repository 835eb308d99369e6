// One output pixel of the undistortion (include/sfmcore.h, "Dense hand-off"):
// the arithmetic of the contract, once, for the kernel (undistort.hip) and the
// host twin (undistort.cpp).  Every operation is a single IEEE operation in the
// stated order; the two translation units that include this switch contraction
// off (#pragma clang fp contract(off) at their top), so no multiply-add is
// fused on either side and the bytes agree.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SFM_UNDISTORT_HD __host__ __device__
#else
#define SFM_UNDISTORT_HD
#endif

namespace sfm {

// what became of an output pixel
enum { kUndistortSampled = 0, kUndistortOutside = 1, kUndistortLowWeight = 2 };

// The source position (x, y) of the output pixel (i, j) under k = {f, ppx,
// ppy, k1, k2, k3}; true when it is inside the w x h image (NaN is not).
SFM_UNDISTORT_HD inline bool undistort_source(const double* k, int32_t w, int32_t h, int32_t i, int32_t j, double* x,
                                              double* y) {
    const double f = k[0], ppx = k[1], ppy = k[2];
    const double px = ((double)i - ppx) / f, py = ((double)j - ppy) / f;
    const double r2 = px * px + py * py, r4 = r2 * r2, r6 = r4 * r2;
    const double c = 1.0 + k[3] * r2 + k[4] * r4 + k[5] * r6;
    *x = f * (px * c) + ppx;
    *y = f * (py * c) + ppy;
    return *x > -1.0 && *x < (double)w && *y > -1.0 && *y < (double)h;
}

// The two source rows an inside position reads, cut to the image: [*lo, *hi)
// (empty when both fall outside).  The band planner's view of undistort_pixel.
SFM_UNDISTORT_HD inline void undistort_source_rows(double y, int32_t h, int64_t* lo, int64_t* hi) {
    const int64_t gy = (int64_t)floorf((float)y);
    *lo = gy < 0 ? 0 : gy;
    *hi = gy + 2 > h ? h : gy + 2;
    if (*hi < *lo) *hi = *lo;
}

// The output pixel (i, j): px[0 .. ch).  src holds the source rows
// [row0, row0 + rows) of the image, `stride` bytes apart (the host twin: the
// whole image, stride w * ch; the kernel: the band its chunk holds, pitched);
// a row outside what is held is skipped like a row outside the image, which a
// correct plan never meets.
SFM_UNDISTORT_HD inline int undistort_pixel(const double* k, int32_t w, int32_t h, int32_t ch, int32_t i, int32_t j,
                                            const uint8_t* src, int64_t stride, int64_t row0, int64_t rows,
                                            const uint8_t* fill, uint8_t* px) {
    double x, y;
    if (!undistort_source(k, w, h, i, j, &x, &y)) {
        for (int32_t c = 0; c < ch; ++c) px[c] = fill[c];
        return kUndistortOutside;
    }
    const float xf = (float)x, yf = (float)y;
    const float gxf = floorf(xf), gyf = floorf(yf);
    const double dx = (double)xf - (double)gxf, dy = (double)yf - (double)gyf;
    const int64_t gx = (int64_t)gxf, gy = (int64_t)gyf;
    const double wxs[2] = {1.0 - dx, dx}, wys[2] = {1.0 - dy, dy};
    double res[3] = {0.0, 0.0, 0.0}, total = 0.0;
    for (int a = 0; a < 2; ++a) {
        const int64_t yy = gy + a;
        if (yy < 0 || yy >= h || yy < row0 || yy >= row0 + rows) continue;
        const uint8_t* row = src + (yy - row0) * stride;
        for (int b = 0; b < 2; ++b) {
            const int64_t xx = gx + b;
            if (xx < 0 || xx >= w) continue;
            const double wgt = wxs[b] * wys[a];
            for (int32_t c = 0; c < ch; ++c) res[c] += (double)row[xx * ch + c] * wgt;
            total += wgt;
        }
    }
    if (total <= 0.2) {
        for (int32_t c = 0; c < ch; ++c) px[c] = 0;
        return kUndistortLowWeight;
    }
    for (int32_t c = 0; c < ch; ++c) {
        double r = res[c];
        if (total != 1.0) r /= total;
        px[c] = (uint8_t)(r + 0.5);
    }
    return kUndistortSampled;
}

}  // namespace sfm
