// One face, one pixel and one texel of the mesh texturing (include/sfmcore.h,
// "Mesh texture"): the arithmetic of the contract, once, for the kernels
// (texture.hip) and the host twins (texture.cpp).  Floats are single IEEE
// operations in the stated order, and the two translation units that include
// this switch contraction off (#pragma clang fp contract(off) at their top), so
// the bytes agree.  Coverage is exact: sub-pixel integers and int64 edge
// functions.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "dense_common.h"

namespace sfm {

// a workgroup of every texturing kernel
constexpr int kTexBlock = 256;
// a face whose clipped bounding box has more pixels than this is drawn by a whole wavefront
constexpr int kTexLargeBox = 256;
// consecutive texels of an atlas row that one lane of the bake writes
constexpr int kTexRun = 4;
// sub-pixel positions a pixel
constexpr int kTexSub = 16;
constexpr int kTexMinCell = 4;
constexpr int kTexMaxCell = 64;
constexpr int kTexDefaultCell = 8;
constexpr int kTexMaxAtlas = 32768;
// a projection beyond this many pixels is not drawable
constexpr float kTexMaxCoord = 1048576.0f;

// An image of the call: M = K R and C, worked out in double and rounded once.
struct TexView {
    float M[9], C[3];
    int32_t w, h, channels, loaded;   // !loaded: skipped entirely
    int64_t pix_off;                  // bytes into the colour pool
};

// the atlas of a call
struct TexAtlas {
    int32_t s, cols, W, H;
};

SFM_HD inline int64_t tex_floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
SFM_HD inline int64_t tex_ceil_div(int64_t a, int64_t b) { return -tex_floor_div(-a, b); }

// ---- a face in a view (steps a, b) ----------------------------------------------------
struct TexFace {
    int64_t X[3], Y[3];   // sub-pixel corners, counter-clockwise (A2 > 0) after the exchange
    float w[3];           // 1.0f / z of those corners
    int64_t A2;           // twice the area, after the exchange; 0: covers nothing
    int32_t px0, px1, py0, py1;   // the bounding box clipped to the image, inclusive; empty when px0 > px1 or py0 > py1
    bool inside, front;   // the unrounded projections lie in the image; the face looks at the camera
    SFM_HD int64_t box() const {
        return A2 > 0 && px0 <= px1 && py0 <= py1 ? (int64_t)(px1 - px0 + 1) * (py1 - py0 + 1) : 0;
    }
};

// false: the face is not drawable in the view
SFM_HD inline bool tex_face_setup(const TexView& v, const float* V, const int32_t* tri, int64_t f, TexFace& F) {
    float x[3], y[3], z[3];
    const float* P[3];
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        P[k] = V + 3 * (int64_t)tri[3 * f + k];
        project_point(v.M, v.C, P[k], &x[k], &y[k], &z[k]);
        ok = ok && z[k] > 0.0f && fabsf(x[k]) <= kTexMaxCoord && fabsf(y[k]) <= kTexMaxCoord;
    }
    if (!ok) return false;
    F.inside = true;
    for (int k = 0; k < 3; ++k) {
        F.X[k] = (int64_t)floorf(x[k] * 16.0f + 0.5f);
        F.Y[k] = (int64_t)floorf(y[k] * 16.0f + 0.5f);
        F.w[k] = 1.0f / z[k];
        F.inside = F.inside && x[k] >= 0.0f && x[k] <= (float)(v.w - 1) && y[k] >= 0.0f && y[k] <= (float)(v.h - 1);
    }
    const float e1[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
    const float e2[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    const float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float t[3] = {v.C[0] - P[0][0], v.C[1] - P[0][1], v.C[2] - P[0][2]};
    F.front = dot3(n, t) > 0.0f;
    F.A2 = (F.X[1] - F.X[0]) * (F.Y[2] - F.Y[0]) - (F.X[2] - F.X[0]) * (F.Y[1] - F.Y[0]);
    if (F.A2 < 0) {
        const int64_t tx = F.X[1], ty = F.Y[1];
        const float tw = F.w[1];
        F.X[1] = F.X[2], F.Y[1] = F.Y[2], F.w[1] = F.w[2];
        F.X[2] = tx, F.Y[2] = ty, F.w[2] = tw;
        F.A2 = -F.A2;
    }
    int64_t lox = F.X[0], hix = F.X[0], loy = F.Y[0], hiy = F.Y[0];
    for (int k = 1; k < 3; ++k) {
        lox = F.X[k] < lox ? F.X[k] : lox;
        hix = F.X[k] > hix ? F.X[k] : hix;
        loy = F.Y[k] < loy ? F.Y[k] : loy;
        hiy = F.Y[k] > hiy ? F.Y[k] : hiy;
    }
    const int64_t a0 = tex_ceil_div(lox, kTexSub), a1 = tex_floor_div(hix, kTexSub);
    const int64_t b0 = tex_ceil_div(loy, kTexSub), b1 = tex_floor_div(hiy, kTexSub);
    F.px0 = (int32_t)(a0 > 0 ? a0 : 0);
    F.px1 = (int32_t)(a1 < v.w - 1 ? a1 : v.w - 1);
    F.py0 = (int32_t)(b0 > 0 ? b0 : 0);
    F.py1 = (int32_t)(b1 < v.h - 1 ? b1 : v.h - 1);
    return true;
}

// Is the centre of pixel (px, py) covered?  *key: ((uint64)bits(d) << 32) | face.
SFM_HD inline bool tex_pixel(const TexFace& F, uint32_t face, int32_t px, int32_t py, uint64_t* key) {
    const int64_t Px = (int64_t)kTexSub * px, Py = (int64_t)kTexSub * py;
    int64_t E[3];
    for (int k = 0; k < 3; ++k) {
        const int a = (k + 1) % 3, b = (k + 2) % 3;
        const int64_t dx = F.X[b] - F.X[a], dy = F.Y[b] - F.Y[a];
        E[k] = dx * (Py - F.Y[a]) - dy * (Px - F.X[a]);
        if (!(E[k] > 0 || (E[k] == 0 && (dy > 0 || (dy == 0 && dx > 0))))) return false;
    }
    const float num = ((float)E[0] * F.w[0] + (float)E[1] * F.w[1]) + (float)E[2] * F.w[2];
    const float d = (float)F.A2 / num;
    uint32_t bits;
    memcpy(&bits, &d, sizeof bits);
    *key = ((uint64_t)bits << 32) | face;
    return true;
}

// step d for one (face, view): the running best of the face
SFM_HD inline void tex_score(const TexFace& F, bool drawable, int64_t covered, int64_t won, int32_t view,
                             int32_t* best_view, int32_t* best_pixels) {
    if (drawable && F.front && F.inside && covered >= 1 && won == covered && covered > (int64_t)*best_pixels) {
        *best_view = view;
        *best_pixels = (int32_t)covered;
    }
}

// ---- the atlas ------------------------------------------------------------------------
// the corner k of face f in texel units from the atlas's origin
SFM_HD inline void tex_corner(const TexAtlas& A, int64_t f, int k, float* cx, float* cy) {
    const int64_t sq = f / 2;
    const float ox = (float)((int32_t)(sq % A.cols) * A.s), oy = (float)((int32_t)(sq / A.cols) * A.s);
    const float s = (float)A.s;
    float x, y;
    if (f % 2 == 0) {
        x = k == 1 ? s - 2.5f : 0.5f;
        y = k == 2 ? s - 2.5f : 0.5f;
    } else {
        x = k == 1 ? 2.5f : s - 0.5f;
        y = k == 2 ? 2.5f : s - 0.5f;
    }
    *cx = ox + x;
    *cy = oy + y;
}
SFM_HD inline void tex_uv(const TexAtlas& A, int64_t f, float* uv) {
    for (int k = 0; k < 3; ++k) {
        float cx, cy;
        tex_corner(A, f, k, &cx, &cy);
        uv[2 * k] = cx / (float)A.W;
        uv[2 * k + 1] = 1.0f - cy / (float)A.H;
    }
}

SFM_HD inline uint8_t tex_round(float v) { return (uint8_t)floorf(v + 0.5f); }
// a texel as r | g << 8 | b << 16 (registers on the device; the host twin unpacks)
SFM_HD inline uint32_t tex_pack(const uint8_t* c) { return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16; }
SFM_HD inline void tex_unpack(uint32_t rgb, uint8_t* c) {
    c[0] = (uint8_t)rgb, c[1] = (uint8_t)(rgb >> 8), c[2] = (uint8_t)(rgb >> 16);
}

// the face of texel (tx, ty), or -1, and its barycentric weights
SFM_HD inline int64_t tex_texel_face(const TexAtlas& A, int64_t n_triangles, int32_t tx, int32_t ty, float* l1, float* l2) {
    const int32_t a = tx % A.s, b = ty % A.s;
    const int64_t sq = (int64_t)(ty / A.s) * A.cols + tx / A.s;
    const int half = a + b <= A.s - 2 ? 0 : 1;
    const int64_t f = 2 * sq + half;
    if (f >= n_triangles) return -1;
    const float den = (float)(A.s - 3);
    *l1 = (float)(half ? A.s - 1 - a : a) / den;
    *l2 = (float)(half ? A.s - 1 - b : b) / den;
    return f;
}

// a texel of a face textured from view v
SFM_HD inline uint32_t tex_sample(const TexView& v, const uint8_t* pixels, const float* V, const int32_t* tri, int64_t f,
                                  float l1, float l2, uint32_t fill) {
    const float *P0 = V + 3 * (int64_t)tri[3 * f], *P1 = V + 3 * (int64_t)tri[3 * f + 1], *P2 = V + 3 * (int64_t)tri[3 * f + 2];
    float X[3], px, py, z;
    for (int c = 0; c < 3; ++c) X[c] = (P0[c] + l1 * (P1[c] - P0[c])) + l2 * (P2[c] - P0[c]);
    project_point(v.M, v.C, X, &px, &py, &z);
    if (!(z > 0.0f)) return fill;
    const float x = fminf(fmaxf(px, 0.0f), (float)(v.w - 1)), y = fminf(fmaxf(py, 0.0f), (float)(v.h - 1));
    uint32_t rgb = 0;
    for (int c = 0; c < 3; ++c)
        rgb |= (uint32_t)tex_round(bilinear_u8(pixels + v.pix_off, v.w, v.h, v.channels, v.channels == 3 ? c : 0, x, y)) << (8 * c);
    return rgb;
}

// a texel of a face without a view: the vertex colours, or the fill
SFM_HD inline uint32_t tex_fallback(const uint8_t* vertex_rgb, const int32_t* tri, int64_t f, float l1, float l2,
                                    uint32_t fill) {
    if (!vertex_rgb) return fill;
    const uint8_t *c0 = vertex_rgb + 3 * (int64_t)tri[3 * f], *c1 = vertex_rgb + 3 * (int64_t)tri[3 * f + 1],
                  *c2 = vertex_rgb + 3 * (int64_t)tri[3 * f + 2];
    uint32_t rgb = 0;
    for (int c = 0; c < 3; ++c) {
        const float a = (float)c0[c];
        const float val = (a + l1 * ((float)c1[c] - a)) + l2 * ((float)c2[c] - a);
        rgb |= (uint32_t)tex_round(fminf(fmaxf(val, 0.0f), 255.0f)) << (8 * c);
    }
    return rgb;
}

}  // namespace sfm
