// One pixel of the dense depth maps (include/sfmcore.h, "Dense depth maps"):
// the arithmetic of the contract, once, for the kernels (depthmap.hip) and the
// host twins (depthmap.cpp).  Everything is float; every operation is a single
// IEEE operation (+ - * / sqrtf floorf) in the stated order, and the two
// translation units that include this switch contraction off (#pragma clang fp
// contract(off) at their top), so no multiply-add is fused on either side and
// the bytes agree.  No pow, acos or sin: their device and host versions differ.
#pragma once
#include <cmath>
#include <cstdint>

#include "dense_common.h"

namespace sfm {

constexpr int kDepthMaxNeighbors = 8;
constexpr int kDepthMaxHalfWindow = 5;
constexpr int kDepthMaxIterations = 16;
constexpr float kDepthWorstCost = 2.0f;
// draws of a pixel: 0..2 the initial plane, then kDepthDrawsPerIteration per iteration
constexpr int kDepthDrawsInit = 3;
constexpr int kDepthDrawsPerIteration = 7;

// An image of the call.  Ki = K^-1 (worked out in double, rounded), the depth
// range and its inverses (imin = 1.0f / dmax, imax = 1.0f / dmin, in float),
// its neighbours pairs[nb0 .. nb1), its gray bytes and its maps.
struct DepthView {
    float Ki[9];
    float dmin, dmax, imin, imax;
    int32_t w, h, nb0, nb1;
    int32_t active, pad;          // loaded, with neighbours: it gets depth maps
    int64_t gray_off, map_off;    // bytes into the gray pool; pixels into the maps
};
// A (reference, neighbour) pair: A = K_j R_j R_r' K_r^-1 and b = K_j R_j (C_r - C_j),
// worked out in double and rounded; the neighbour's size, gray bytes and maps.
struct DepthPair {
    float A[9], b[3];
    int32_t view, w, h, loaded;
    int64_t gray_off, map_off;
};
struct DepthParams {
    int32_t r, iterations, n_best, pad;
    uint64_t seed;
};
struct DepthFilterParams {
    float max_cost, rel_tol;
    int32_t min_consistent, pad;
};
// the reference image's bytes around a pixel: pixel (x, y) is p[(y - oy) * stride + (x - ox)]
// (the host twin: the image; the kernel: the tile and its halo in LDS)
struct DepthRef {
    const uint8_t* p;
    int32_t stride, ox, oy;
    SFM_HD float at(int32_t x, int32_t y) const { return (float)p[(y - oy) * stride + (x - ox)]; }
};

SFM_HD inline uint64_t depth_mix64(uint64_t z) {   // synth_rng.h's mix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// synth_rng.h's entity_seed(seed, image, pixel)
SFM_HD inline uint64_t depth_pixel_seed(uint64_t seed, uint64_t img, uint64_t idx) {
    return depth_mix64(depth_mix64(seed ^ (img * 0xD1B54A32D192ED03ULL)) + idx * 0x9E3779B97F4A7C15ULL);
}
// draw k of a pixel, in [0, 1)
SFM_HD inline float depth_uniform(uint64_t base, uint32_t k) {
    return (float)(depth_mix64(base + (uint64_t)k * 0x9E3779B97F4A7C15ULL) >> 40) * 0x1.0p-24f;
}

// n . (d ray): the plane's offset along its normal
SFM_HD inline float depth_plane_offset(const float* n, float d, const float* ray) {
    const float X[3] = {d * ray[0], d * ray[1], d * ray[2]};
    return dot3(n, X);
}
SFM_HD inline void depth_face_camera(float* n, const float* ray) {
    if (dot3(n, ray) > 0.0f) {
        n[0] = -n[0];
        n[1] = -n[1];
        n[2] = -n[2];
    }
}
SFM_HD inline void depth_normalize(float* v) {
    const float len = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] = v[0] / len;
    v[1] = v[1] / len;
    v[2] = v[2] / len;
}

// Σa and Σaa of the reference patch (integers below 2^24: exact in any order)
SFM_HD inline void depth_ref_sums(const DepthRef& ref, int32_t px, int32_t py, int32_t r, float* sa, float* saa) {
    float s = 0.0f, ss = 0.0f;
    for (int32_t dy = -r; dy <= r; ++dy)
        for (int32_t dx = -r; dx <= r; ++dx) {
            const float a = ref.at(px + dx, py + dy);
            s += a;
            ss += a * a;
        }
    *sa = s;
    *saa = ss;
}

// The cost of the plane (offset t = n . (d ray(p)), normal n) at pixel p against one neighbour.
SFM_HD inline float depth_pair_cost(const DepthView& V, const DepthPair& Q, const uint8_t* gray, const DepthRef& ref,
                                    int32_t px, int32_t py, int32_t r, float t, const float* n, float sa,
                                    float saa) {
    const uint8_t* img = gray + Q.gray_off;
    const int32_t side = 2 * r + 1;
    const float N = (float)(side * side);
    const float va = saa - (sa * sa) / N;
    if (!(va >= N) || !Q.loaded) return kDepthWorstCost;
    const float xmax = (float)(Q.w - 1), ymax = (float)(Q.h - 1);
    float sb = 0.0f, sbb = 0.0f, sab = 0.0f;
    for (int32_t dy = -r; dy <= r; ++dy)
        for (int32_t dx = -r; dx <= r; ++dx) {
            const float qx = (float)(px + dx), qy = (float)(py + dy);
            float rq[3], aq[3];
            mul_pixel(V.Ki, qx, qy, rq);
            const float z = t / dot3(n, rq);
            mul_pixel(Q.A, qx, qy, aq);
            const float h0 = z * aq[0] + Q.b[0], h1 = z * aq[1] + Q.b[1], h2 = z * aq[2] + Q.b[2];
            const float x = h0 / h2, y = h1 / h2;
            if (!(z > 0.0f && h2 > 0.0f && x >= 0.0f && x <= xmax && y >= 0.0f && y <= ymax)) return kDepthWorstCost;
            const float b = bilinear_u8(img, Q.w, Q.h, 1, 0, x, y);
            const float a = ref.at(px + dx, py + dy);
            sb += b;
            sbb += b * b;
            sab += a * b;
        }
    const float vb = sbb - (sb * sb) / N, cov = sab - (sa * sb) / N;
    if (!(vb >= N)) return kDepthWorstCost;
    float c = cov / sqrtf(va * vb);
    if (c < -1.0f) c = -1.0f;
    if (c > 1.0f) c = 1.0f;
    return 1.0f - c;
}

// The cost of the plane (d, n) at pixel p: the neighbours' costs ascending, the
// first min(n_best, n_nb) averaged (summed in that order, then divided).
SFM_HD inline float depth_cost(const DepthView& V, const DepthPair* pairs, const uint8_t* gray, const DepthRef& ref,
                               int32_t px, int32_t py, const float* rp, const DepthParams& prm, float d,
                               const float* n, float sa, float saa) {
    const float t = depth_plane_offset(n, d, rp);
    float s[kDepthMaxNeighbors];
#pragma unroll
    for (int k = 0; k < kDepthMaxNeighbors; ++k) s[k] = 3.0f;
    for (int32_t q = V.nb0; q < V.nb1; ++q) {
        float c = depth_pair_cost(V, pairs[q], gray, ref, px, py, prm.r, t, n, sa, saa);
#pragma unroll
        for (int k = 0; k < kDepthMaxNeighbors; ++k)
            if (c < s[k]) {
                const float o = s[k];
                s[k] = c;
                c = o;
            }
    }
    const int32_t n_nb = V.nb1 - V.nb0, m = prm.n_best < n_nb ? prm.n_best : n_nb;
    float sum = 0.0f;
#pragma unroll
    for (int k = 0; k < kDepthMaxNeighbors; ++k)
        if (k < m) sum += s[k];
    return sum / (float)m;
}

// the random plane of draws u[0..3): inverse depth uniform, normal towards the camera
SFM_HD inline void depth_random_plane(const DepthView& V, const float* rp, const float* u, float* d, float* n) {
    const float inv = V.imin + u[0] * (V.imax - V.imin);
    *d = 1.0f / inv;
    n[0] = 2.0f * u[1] - 1.0f;
    n[1] = 2.0f * u[2] - 1.0f;
    n[2] = -1.0f;
    depth_normalize(n);
    depth_face_camera(n, rp);
}

// the plane (d, n) perturbed by delta with the draws u[0..4)
SFM_HD inline void depth_perturbed_plane(const DepthView& V, const float* rp, float delta, const float* u, float d,
                                         const float* n, float* d2, float* n2) {
    float inv = 1.0f / d + (delta * (2.0f * u[0] - 1.0f)) * (V.imax - V.imin);
    if (inv < V.imin) inv = V.imin;
    if (inv > V.imax) inv = V.imax;
    *d2 = 1.0f / inv;
    for (int c = 0; c < 3; ++c) n2[c] = n[c] + delta * (2.0f * u[1 + c] - 1.0f);
    depth_normalize(n2);
    depth_face_camera(n2, rp);
}

SFM_HD inline bool depth_estimated(const DepthView& V, int32_t r, int32_t x, int32_t y) {
    return x >= r && x < V.w - r && y >= r && y < V.h - r;
}

// The initial plane of pixel p of image i and its cost.  depth / normal / cost
// are the image's maps; with init_given the plane is read from them.
SFM_HD inline void depth_init_pixel(const DepthView& V, const DepthPair* pairs, const uint8_t* gray,
                                    const DepthRef& ref, const DepthParams& prm, bool init_given, int32_t i,
                                    int32_t px, int32_t py, float* depth, float* normal, float* cost) {
    const int64_t idx = (int64_t)py * V.w + px;
    float rp[3], sa, saa, d, n[3];
    mul_pixel(V.Ki, (float)px, (float)py, rp);
    depth_ref_sums(ref, px, py, prm.r, &sa, &saa);
    if (init_given) {
        d = depth[idx];
        for (int c = 0; c < 3; ++c) n[c] = normal[3 * idx + c];
    } else {
        const uint64_t base = depth_pixel_seed(prm.seed, (uint64_t)i, (uint64_t)idx);
        const float u[3] = {depth_uniform(base, 0), depth_uniform(base, 1), depth_uniform(base, 2)};
        depth_random_plane(V, rp, u, &d, n);
        depth[idx] = d;
        for (int c = 0; c < 3; ++c) normal[3 * idx + c] = n[c];
    }
    cost[idx] = depth_cost(V, pairs, gray, ref, px, py, rp, prm, d, n, sa, saa);
}

// Iteration `it` at the active pixel p of image i: propagation from the eight
// neighbours of the other colour, a perturbed plane, a fresh random plane; each
// taken when strictly cheaper.  Reads planes of the other colour only and
// writes its own.
SFM_HD inline void depth_update_pixel(const DepthView& V, const DepthPair* pairs, const uint8_t* gray,
                                      const DepthRef& ref, const DepthParams& prm, int32_t it, int32_t i,
                                      int32_t px, int32_t py, float* depth, float* normal, float* cost) {
    const int64_t idx = (int64_t)py * V.w + px;
    float rp[3], sa, saa;
    mul_pixel(V.Ki, (float)px, (float)py, rp);
    depth_ref_sums(ref, px, py, prm.r, &sa, &saa);
    float d = depth[idx], n[3] = {normal[3 * idx], normal[3 * idx + 1], normal[3 * idx + 2]}, c = cost[idx];
    const int32_t ox[8] = {-1, 1, 0, 0, -5, 5, 0, 0}, oy[8] = {0, 0, -1, 1, 0, 0, -5, 5};
    for (int k = 0; k < 8; ++k) {
        const int32_t sx = px + ox[k], sy = py + oy[k];
        if (!depth_estimated(V, prm.r, sx, sy)) continue;
        const int64_t sidx = (int64_t)sy * V.w + sx;
        const float ns[3] = {normal[3 * sidx], normal[3 * sidx + 1], normal[3 * sidx + 2]};
        float rs[3];
        mul_pixel(V.Ki, (float)sx, (float)sy, rs);
        const float dp = depth_plane_offset(ns, depth[sidx], rs) / dot3(ns, rp);
        if (!(dp >= V.dmin && dp <= V.dmax)) continue;
        const float cc = depth_cost(V, pairs, gray, ref, px, py, rp, prm, dp, ns, sa, saa);
        if (cc < c) {
            c = cc;
            d = dp;
            n[0] = ns[0];
            n[1] = ns[1];
            n[2] = ns[2];
        }
    }
    const uint64_t base = depth_pixel_seed(prm.seed, (uint64_t)i, (uint64_t)idx);
    const uint32_t k0 = (uint32_t)(kDepthDrawsInit + kDepthDrawsPerIteration * it);
    float u[kDepthDrawsPerIteration];
    for (int k = 0; k < kDepthDrawsPerIteration; ++k) u[k] = depth_uniform(base, k0 + (uint32_t)k);
    const float delta = 0.1f / (float)(1 << it);
    float d2, n2[3];
    depth_perturbed_plane(V, rp, delta, u, d, n, &d2, n2);
    float cc = depth_cost(V, pairs, gray, ref, px, py, rp, prm, d2, n2, sa, saa);
    if (cc < c) {
        c = cc;
        d = d2;
        n[0] = n2[0];
        n[1] = n2[1];
        n[2] = n2[2];
    }
    depth_random_plane(V, rp, u + 4, &d2, n2);
    cc = depth_cost(V, pairs, gray, ref, px, py, rp, prm, d2, n2, sa, saa);
    if (cc < c) {
        c = cc;
        d = d2;
        n[0] = n2[0];
        n[1] = n2[1];
        n[2] = n2[2];
    }
    depth[idx] = d;
    normal[3 * idx] = n[0];
    normal[3 * idx + 1] = n[1];
    normal[3 * idx + 2] = n[2];
    cost[idx] = c;
}

// The consistency filter at pixel p: how many neighbours agree (-1: the pixel
// is no candidate).  depth / cost are the maps of all images.
SFM_HD inline int32_t depth_filter_pixel(const DepthView& V, const DepthPair* pairs, const DepthFilterParams& prm,
                                         int32_t px, int32_t py, const float* depth, const float* cost) {
    const int64_t idx = V.map_off + (int64_t)py * V.w + px;
    const float d = depth[idx];
    if (!(d > 0.0f && cost[idx] <= prm.max_cost)) return -1;
    int32_t agree = 0;
    for (int32_t q = V.nb0; q < V.nb1; ++q) {
        const DepthPair& Q = pairs[q];
        float ap[3];
        mul_pixel(Q.A, (float)px, (float)py, ap);
        const float h0 = d * ap[0] + Q.b[0], h1 = d * ap[1] + Q.b[1], z = d * ap[2] + Q.b[2];
        const int64_t at = nearest_pixel(h0 / z, h1 / z, Q.w, Q.h);
        if (!(z > 0.0f) || at < 0) continue;
        const float dj = depth[Q.map_off + at];
        if (dj > 0.0f && fabsf(z - dj) <= prm.rel_tol * z) ++agree;
    }
    return agree;
}

}  // namespace sfm
