// One pixel of the depth-map fusion (include/sfmcore.h, "Dense fusion"): the
// arithmetic of the contract, once, for the kernels (fuse.hip) and the host
// twin (fuse.cpp).  Everything is float; every operation is a single IEEE
// operation in the stated order, and the two translation units that include
// this switch contraction off (#pragma clang fp contract(off) at their top), so
// the bytes agree.  The colours are integer sums.
#pragma once
#include <cmath>
#include <cstdint>

#include "dense_common.h"

namespace sfm {

constexpr int kFuseMaxPairs = 32;
// a workgroup of the fusion kernels: this many consecutive pixels of an image's raster
constexpr int kFuseBlock = 256;
enum { kFuseNone = 0, kFuseEmitted = 1, kFuseSuppressed = 2 };

// An image of the call: Ki = K^-1, R and C rounded from double once, its fusion
// pairs pairs[p0 .. p1), its maps, its colour bytes, its first block.
struct FuseView {
    float Ki[9], R[9], C[3];
    int32_t w, h, p0, p1;
    int32_t channels, loaded;     // channels 0: no colours; !loaded: its depth counts as 0
    int32_t pad[2];
    int64_t map_off, pix_off;     // pixels into the maps; bytes into the colour pool
    int64_t blk_off;              // blocks of kFuseBlock pixels before this image's
};
// A fusion pair (image i, other image j): A and b as DepthPair's.
struct FusePair {
    float A[9], b[3];
    int32_t view, pad;
};
struct FuseParams {
    float rel_tol, min_normal_cos;
    int32_t use_normal, use_color;
};

SFM_HD inline float fuse_depth_at(const FuseView& V, const float* depth, int64_t idx) {
    return V.loaded ? depth[V.map_off + idx] : 0.0f;
}
// N = R' n
SFM_HD inline void fuse_world_normal(const FuseView& V, const float* normal, int64_t idx, float* N) {
    const float* n = normal + 3 * (V.map_off + idx);
    for (int c = 0; c < 3; ++c) N[c] = (V.R[c] * n[0] + V.R[3 + c] * n[1]) + V.R[6 + c] * n[2];
}
// Xw = R' (d * (Ki [p 1])) + C
SFM_HD inline void fuse_world_point(const FuseView& V, int32_t px, int32_t py, float d, float* X) {
    float ray[3];
    mul_pixel(V.Ki, (float)px, (float)py, ray);
    const float c0 = d * ray[0], c1 = d * ray[1], c2 = d * ray[2];
    for (int c = 0; c < 3; ++c) X[c] = ((V.R[c] * c0 + V.R[3 + c] * c1) + V.R[6 + c] * c2) + V.C[c];
}

// Pixel p of the reference at depth d against the pair Q whose image is J: the
// pixel q of J it falls on (its raster index, or -1) and its depth z there.
SFM_HD inline int64_t fuse_project(const FusePair& Q, const FuseView& J, int32_t px, int32_t py, float d, float* z) {
    float ap[3];
    mul_pixel(Q.A, (float)px, (float)py, ap);
    const float h0 = d * ap[0] + Q.b[0], h1 = d * ap[1] + Q.b[1], h2 = d * ap[2] + Q.b[2];
    *z = h2;
    const int64_t q = nearest_pixel(h0 / h2, h1 / h2, J.w, J.h);
    return h2 > 0.0f ? q : -1;
}

// Does pair Q agree with pixel idx of V at depth d?  qidx: the pixel of J.
SFM_HD inline bool fuse_agrees(const FuseView* views, const FuseView& V, const FusePair& Q, const FuseParams& prm,
                               int32_t px, int32_t py, int64_t idx, float d, const float* depth,
                               const float* normal, int64_t* qidx) {
    const FuseView& J = views[Q.view];
    float z;
    const int64_t q = fuse_project(Q, J, px, py, d, &z);
    *qidx = q;
    if (q < 0) return false;
    const float dj = fuse_depth_at(J, depth, q);
    if (!(dj > 0.0f && fabsf(z - dj) <= prm.rel_tol * z)) return false;
    if (prm.use_normal) {
        float Ni[3], Nj[3];
        fuse_world_normal(V, normal, idx, Ni);
        fuse_world_normal(J, normal, q, Nj);
        if (!(dot3(Ni, Nj) >= prm.min_normal_cos)) return false;
    }
    return true;
}

// The agreement mask and the fate of pixel (px, py) of image i.
SFM_HD inline int32_t fuse_pixel_fate(const FuseView* views, const FusePair* pairs, const FuseParams& prm, int32_t i,
                                      int32_t px, int32_t py, const float* depth, const float* normal,
                                      uint32_t* mask_out) {
    const FuseView& V = views[i];
    const int64_t idx = (int64_t)py * V.w + px;
    const float d = fuse_depth_at(V, depth, idx);
    uint32_t mask = 0;
    bool lower = false;
    if (d > 0.0f)
        for (int32_t k = V.p0; k < V.p1; ++k) {
            int64_t q;
            if (fuse_agrees(views, V, pairs[k], prm, px, py, idx, d, depth, normal, &q)) {
                mask |= 1u << (k - V.p0);
                lower = lower || pairs[k].view < i;
            }
        }
    *mask_out = mask;
    return !(d > 0.0f) ? kFuseNone : (lower ? kFuseSuppressed : kFuseEmitted);
}

// The fused point of an emitted pixel from its agreement mask; returns m.
// rgb is written only when prm.use_color.
SFM_HD inline int32_t fuse_pixel_point(const FuseView* views, const FusePair* pairs, const FuseParams& prm, int32_t i,
                                       int32_t px, int32_t py, uint32_t mask, const float* depth,
                                       const float* normal, const uint8_t* pixels, float* X, float* N,
                                       uint8_t* rgb) {
    const FuseView& V = views[i];
    const int64_t idx = (int64_t)py * V.w + px;
    const float d = fuse_depth_at(V, depth, idx);
    float own[3], sx[3], sn[3];
    uint32_t col[3] = {0, 0, 0};
    fuse_world_point(V, px, py, d, sx);
    fuse_world_normal(V, normal, idx, own);
    sn[0] = own[0];
    sn[1] = own[1];
    sn[2] = own[2];
    if (prm.use_color) add_color(pixels + V.pix_off + idx * V.channels, V.channels, col);
    int32_t m = 1;
    for (uint32_t rest = mask; rest; rest &= rest - 1) {
        const int32_t k = __builtin_ctz(rest);
        const FusePair& Q = pairs[V.p0 + k];
        const FuseView& J = views[Q.view];
        float z, xj[3], nj[3];
        const int64_t q = fuse_project(Q, J, px, py, d, &z);
        const int32_t qx = (int32_t)(q % J.w), qy = (int32_t)(q / J.w);
        fuse_world_point(J, qx, qy, fuse_depth_at(J, depth, q), xj);
        fuse_world_normal(J, normal, q, nj);
        for (int c = 0; c < 3; ++c) {
            sx[c] = sx[c] + xj[c];
            sn[c] = sn[c] + nj[c];
        }
        if (prm.use_color) add_color(pixels + J.pix_off + q * J.channels, J.channels, col);
        ++m;
    }
    const float fm = (float)m;
    for (int c = 0; c < 3; ++c) X[c] = sx[c] / fm;
    const float len = sqrtf((sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2]);
    for (int c = 0; c < 3; ++c) N[c] = len > 0.0f ? sn[c] / len : own[c];
    if (prm.use_color)
        for (int c = 0; c < 3; ++c) rgb[c] = mean_u8(col[c], (uint32_t)m);
    return m;
}

}  // namespace sfm
