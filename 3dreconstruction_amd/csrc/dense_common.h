// The point arithmetic that the dense stages share, once, for their kernels and
// host twins.  Floats are single IEEE operations in the stated order, and every
// translation unit that includes this switches contraction off (#pragma clang fp
// contract(off) at its top), so device and host agree by bytes.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SFM_HD __host__ __device__
#else
#define SFM_HD
#endif

namespace sfm {

SFM_HD inline float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// M [x y 1]
SFM_HD inline void mul_pixel(const float* M, float x, float y, float* o) {
    o[0] = (M[0] * x + M[1] * y) + M[2];
    o[1] = (M[3] * x + M[4] * y) + M[5];
    o[2] = (M[6] * x + M[7] * y) + M[8];
}

// h = M (X - C); x = h0 / h2, y = h1 / h2, z = h2.  The caller tests z > 0.  (The pairs of the depth
// maps and of the fusion project with d A [p 1] + b, another order: they share only nearest_pixel.)
SFM_HD inline void project_point(const float* M, const float* C, const float* X, float* x, float* y, float* z) {
    const float q[3] = {X[0] - C[0], X[1] - C[1], X[2] - C[2]};
    const float h0 = dot3(M, q), h1 = dot3(M + 3, q);
    *z = dot3(M + 6, q);
    *x = h0 / *z;
    *y = h1 / *z;
}

// the raster index of the pixel nearest to (x, y) in a w x h image, or -1 (also for a NaN)
SFM_HD inline int64_t nearest_pixel(float x, float y, int32_t w, int32_t h) {
    const float fx = floorf(x + 0.5f), fy = floorf(y + 0.5f);
    if (!(fx >= 0.0f && fx <= (float)(w - 1) && fy >= 0.0f && fy <= (float)(h - 1))) return -1;
    return (int64_t)(int32_t)fy * w + (int32_t)fx;
}

// The bilinear read of a byte image at (x, y), 0 <= x <= w - 1 and 0 <= y <= h - 1,
// unrounded; the neighbours beyond the last column and row are clamped.  Pixel
// (px, py)'s byte is img[(py * w + px) * stride_px + channel_off].
SFM_HD inline float bilinear_u8(const uint8_t* img, int32_t w, int32_t h, int32_t stride_px, int32_t channel_off, float x,
                                float y) {
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int32_t x0 = (int32_t)x0f, y0 = (int32_t)y0f;
    const int32_t x1 = x0 + 1 > w - 1 ? w - 1 : x0 + 1, y1 = y0 + 1 > h - 1 ? h - 1 : y0 + 1;
    const uint8_t *p00 = img + ((int64_t)y0 * w + x0) * stride_px, *p10 = img + ((int64_t)y0 * w + x1) * stride_px;
    const uint8_t *p01 = img + ((int64_t)y1 * w + x0) * stride_px, *p11 = img + ((int64_t)y1 * w + x1) * stride_px;
    const float g00 = (float)p00[channel_off], g10 = (float)p10[channel_off];
    const float g01 = (float)p01[channel_off], g11 = (float)p11[channel_off];
    const float top = g00 + fx * (g10 - g00), bot = g01 + fx * (g11 - g01);
    return top + fy * (bot - top);
}

// s += the colour of the pixel at p; a gray byte counts for all three
SFM_HD inline void add_color(const uint8_t* p, int32_t channels, uint32_t* s) {
    if (channels == 3) {   // (a branch, not selects: fuse_emit_kernel keeps 64 registers with it)
        s[0] += p[0], s[1] += p[1], s[2] += p[2];
    } else {
        s[0] += p[0], s[1] += p[0], s[2] += p[0];
    }
}
// the mean of m bytes whose sum is `sum`, rounded half up
SFM_HD inline uint8_t mean_u8(uint32_t sum, uint32_t m) { return (uint8_t)((2u * sum + m) / (2u * m)); }

}  // namespace sfm
