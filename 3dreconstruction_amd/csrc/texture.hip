// Mesh texturing on the device (gfx950): the mesh, one identity buffer and the
// texture of a call resident.  Per view, in index order:
//
//   raster     one lane per face: the face is projected (three vertices, the
//              view's constants read at a uniform index, so they stay in scalar
//              registers) and every covered pixel of its clipped bounding box
//              takes a 64-bit atomic minimum of (depth bits, face).  The
//              minimum does not depend on the order of arrival, so the buffer
//              is the same on every run.  A face whose box has more than
//              kTexLargeBox pixels is appended to a list instead (its order is
//              never seen outside) and drawn by
//   raster big one wavefront per listed face, lanes striding over the box, in a
//              fixed grid of wavefronts that loop over the list, so no lane
//              ever walks a whole image and no count is read back.
//   score      the same two walks, reading the buffer: covered and won per
//              face (a wavefront's come from shuffles), then the running
//              (covered, view) of the face.
// Then one kernel counts the textured faces and their pixels (integer atomics),
// and
//   bake       one lane per run of kTexRun consecutive texels of an atlas row;
//              square, half and face follow from the texel index alone.  The
//              views of a wavefront's faces are taken one at a time
//              (readfirstlane), so the view's constants are scalar here too.
//              Full, aligned runs are stored as three dwords.
//   uv         one lane per face.
#pragma clang fp contract(off)

#include <algorithm>

#include "texture.h"

namespace sfm {
namespace {

static_assert(kTexBlock == 256 && kTexRun == 4, "four wavefronts of 64 lanes; a run is three dwords");
constexpr int kTexBigGroups = 256;   // workgroups of the kernels that walk the list of big faces

enum { kNotDrawable = 0, kTextured = 1, kSumPixels = 2, kBigCount = 3, kCounters = 4 };

struct ViewLaunch {
    const TexView* views;
    const float* V;
    const int32_t* tri;
    unsigned long long* id;         // [max_pixels]
    int32_t *face_view, *face_pixels;
    int32_t* big;                   // [n_triangles]
    unsigned long long* counters;   // [kCounters]
    int64_t n_triangles;
    int32_t view;
};

template <bool kScore>
__device__ inline void walk_pixel(const ViewLaunch& a, const TexView& v, const TexFace& F, uint32_t f, int32_t px, int32_t py,
                                  int32_t& covered, int32_t& won) {
    uint64_t key;
    if (!tex_pixel(F, f, px, py, &key)) return;
    unsigned long long* at = a.id + ((int64_t)py * v.w + px);
    if (kScore) {
        ++covered;
        won += (uint32_t)*at == f;
    } else {
        atomicMin(at, (unsigned long long)key);
    }
}

template <bool kScore>
__global__ __launch_bounds__(kTexBlock) void tex_face_kernel(ViewLaunch a) {
    const TexView& v = a.views[a.view];
    const int64_t f = (int64_t)blockIdx.x * kTexBlock + threadIdx.x;
    bool refused = false;
    if (f < a.n_triangles) {
        TexFace F;
        if (!tex_face_setup(v, a.V, a.tri, f, F)) {
            refused = true;
        } else {
            const int64_t box = F.box();
            if (box > kTexLargeBox) {
                if (!kScore) a.big[atomicAdd(&a.counters[kBigCount], 1ull)] = (int32_t)f;
            } else if (box > 0) {
                int32_t covered = 0, won = 0;
                for (int32_t py = F.py0; py <= F.py1; ++py)
                    for (int32_t px = F.px0; px <= F.px1; ++px) walk_pixel<kScore>(a, v, F, (uint32_t)f, px, py, covered, won);
                if (kScore) {
                    int32_t bv = a.face_view[f], bp = a.face_pixels[f];
                    tex_score(F, true, covered, won, a.view, &bv, &bp);
                    a.face_view[f] = bv;
                    a.face_pixels[f] = bp;
                }
            }
        }
    }
    if (!kScore) {
        const unsigned long long r = __ballot(refused);
        if ((threadIdx.x & 63) == 0 && r) atomicAdd(&a.counters[kNotDrawable], (unsigned long long)__popcll(r));
    }
}

template <bool kScore>
__global__ __launch_bounds__(kTexBlock) void tex_big_kernel(ViewLaunch a) {
    const TexView& v = a.views[a.view];
    const int64_t n = (int64_t)a.counters[kBigCount];
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t at = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); at < n; at += (int64_t)gridDim.x * 4) {
        const int64_t f = a.big[at];
        TexFace F;
        tex_face_setup(v, a.V, a.tri, f, F);   // drawable, or it would not be listed
        const int32_t bw = F.px1 - F.px0 + 1;
        const int64_t box = F.box();
        int32_t covered = 0, won = 0;
        for (int64_t p = lane; p < box; p += 64)
            walk_pixel<kScore>(a, v, F, (uint32_t)f, F.px0 + (int32_t)(p % bw), F.py0 + (int32_t)(p / bw), covered, won);
        if (kScore) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                covered += __shfl_down(covered, o);
                won += __shfl_down(won, o);
            }
            if (lane == 0) {
                int32_t bv = a.face_view[f], bp = a.face_pixels[f];
                tex_score(F, true, covered, won, a.view, &bv, &bp);
                a.face_view[f] = bv;
                a.face_pixels[f] = bp;
            }
        }
    }
}

__global__ __launch_bounds__(kTexBlock) void tex_count_kernel(ViewLaunch a) {
    const int64_t f = (int64_t)blockIdx.x * kTexBlock + threadIdx.x;
    const bool in = f < a.n_triangles;
    const unsigned long long t = __ballot(in && a.face_view[f] >= 0);
    long long px = in ? a.face_pixels[f] : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) px += __shfl_down(px, o);
    if ((threadIdx.x & 63) == 0 && t) {
        atomicAdd(&a.counters[kTextured], (unsigned long long)__popcll(t));
        atomicAdd(&a.counters[kSumPixels], (unsigned long long)px);
    }
}

struct BakeLaunch {
    const TexView* views;
    const uint8_t* pixels;
    const float* V;
    const uint8_t* vrgb;   // NULL: fill
    const int32_t *tri, *face_view;
    uint8_t* texture;
    float* uv;
    int64_t n_triangles, n_runs;
    TexAtlas A;
    int32_t runs_per_row;
    uint32_t fill;   // r | g << 8 | b << 16
};

__global__ __launch_bounds__(kTexBlock) void tex_bake_kernel(BakeLaunch a) {
    const int64_t run = (int64_t)blockIdx.x * kTexBlock + threadIdx.x;
    if (run >= a.n_runs) return;
    const int32_t ty = (int32_t)(run / a.runs_per_row), tx0 = (int32_t)(run % a.runs_per_row) * kTexRun;
    uint32_t t[kTexRun];
#pragma unroll
    for (int k = 0; k < kTexRun; ++k) {
        const int32_t tx = tx0 + k;
        uint32_t rgb = a.fill;
        if (tx < a.A.W) {
            float l1 = 0.0f, l2 = 0.0f;
            const int64_t f = tex_texel_face(a.A, a.n_triangles, tx, ty, &l1, &l2);
            const int32_t view = f >= 0 ? a.face_view[f] : -2;
            if (view == -1) rgb = tex_fallback(a.vrgb, a.tri, f, l1, l2, a.fill);
            bool todo = view >= 0;
            while (todo) {
                const int32_t u = __builtin_amdgcn_readfirstlane(view);   // uniform: the view's constants are scalar loads
                if (view == u) {
                    rgb = tex_sample(a.views[u], a.pixels, a.V, a.tri, f, l1, l2, a.fill);
                    todo = false;
                }
            }
        }
        t[k] = rgb;
    }
    // four texels of 24 bits are three dwords
    const uint32_t word[3] = {t[0] | t[1] << 24, t[1] >> 8 | t[2] << 16, t[2] >> 16 | t[3] << 8};
    const int64_t off = 3 * ((int64_t)ty * a.A.W + tx0);
    if (tx0 + kTexRun <= a.A.W && (off & 3) == 0) {
        uint32_t* o = reinterpret_cast<uint32_t*>(a.texture + off);
        o[0] = word[0];
        o[1] = word[1];
        o[2] = word[2];
    } else {
        const int32_t n = 3 * (a.A.W - tx0 < kTexRun ? a.A.W - tx0 : kTexRun);
#pragma unroll
        for (int byte = 0; byte < 3 * kTexRun; ++byte)
            if (byte < n) a.texture[off + byte] = (uint8_t)(word[byte >> 2] >> (8 * (byte & 3)));
    }
}

__global__ __launch_bounds__(kTexBlock) void tex_uv_kernel(BakeLaunch a) {
    const int64_t f = (int64_t)blockIdx.x * kTexBlock + threadIdx.x;
    if (f >= a.n_triangles) return;
    float uv[6];
    tex_uv(a.A, f, uv);
#pragma unroll
    for (int k = 0; k < 6; ++k) a.uv[6 * f + k] = uv[k];
}

// the mesh and the views of a call on the device
struct Resident {
    DBuf<TexView> views;
    DBuf<float> V;
    DBuf<int32_t> tri, face_view, face_pixels, big;
    DBuf<unsigned long long> id, counters;
    DBuf<uint8_t> pool, vrgb, texture;
    DBuf<float> uv;
};

unsigned blocks(int64_t n) { return (unsigned)((n + kTexBlock - 1) / kTexBlock); }

void upload_mesh(hipStream_t s, const TexProblem& P, const float* V, const int32_t* tri, Resident& r) {
    r.views.alloc(std::max<size_t>(P.views.size(), 1));
    r.views.upload(P.views.data(), P.views.size(), s);
    r.V.alloc(3 * (size_t)P.n_vertices);
    r.V.upload(V, 3 * (size_t)P.n_vertices, s);
    r.tri.alloc(3 * (size_t)P.n_triangles);
    r.tri.upload(tri, 3 * (size_t)P.n_triangles, s);
    r.face_view.alloc((size_t)P.n_triangles);
}

void upload_images(hipStream_t s, const TexProblem& P, const uint8_t* pixels, const uint8_t* vertex_rgb, Resident& r) {
    r.pool.alloc((size_t)std::max<int64_t>(P.images.pool_hi - P.images.pool_lo, 1));
    if (pixels) r.pool.upload(pixels + P.images.pool_lo, (size_t)(P.images.pool_hi - P.images.pool_lo), s);
    if (vertex_rgb) {
        r.vrgb.alloc(3 * (size_t)P.n_vertices);
        r.vrgb.upload(vertex_rgb, 3 * (size_t)P.n_vertices, s);
    }
    r.texture.alloc(3 * (size_t)P.atlas.W * P.atlas.H);
    r.uv.alloc(6 * (size_t)P.n_triangles);
}

void launch_views(hipStream_t s, const TexProblem& P, Resident& r) {
    const size_t n = (size_t)P.n_triangles;
    r.face_pixels.alloc(n);
    r.big.alloc(n);
    r.id.alloc((size_t)std::max<int64_t>(P.max_pixels, 1));
    r.counters.alloc(kCounters);
    r.counters.zero(s);
    r.face_pixels.zero(s);
    SFM_HIP(hipMemsetAsync(r.face_view.p, 0xFF, n * sizeof(int32_t), s));   // -1
    ViewLaunch a{};
    a.views = r.views.p;
    a.V = r.V.p;
    a.tri = r.tri.p;
    a.id = r.id.p;
    a.face_view = r.face_view.p;
    a.face_pixels = r.face_pixels.p;
    a.big = r.big.p;
    a.counters = r.counters.p;
    a.n_triangles = P.n_triangles;
    const dim3 faces(blocks(P.n_triangles)), big(kTexBigGroups), wg(kTexBlock);
    for (int32_t v = 0; v < P.images.n_img; ++v) {
        const TexView& T = P.views[(size_t)v];
        if (!T.loaded) continue;
        a.view = v;
        SFM_HIP(hipMemsetAsync(r.id.p, 0xFF, (size_t)T.w * T.h * sizeof(unsigned long long), s));
        SFM_HIP(hipMemsetAsync(r.counters.p + kBigCount, 0, sizeof(unsigned long long), s));
        hipLaunchKernelGGL(tex_face_kernel<false>, faces, wg, 0, s, a);
        hipLaunchKernelGGL(tex_big_kernel<false>, big, wg, 0, s, a);
        hipLaunchKernelGGL(tex_face_kernel<true>, faces, wg, 0, s, a);
        hipLaunchKernelGGL(tex_big_kernel<true>, big, wg, 0, s, a);
    }
    hipLaunchKernelGGL(tex_count_kernel, faces, wg, 0, s, a);
    SFM_HIP(hipGetLastError());
}

void launch_bake(hipStream_t s, const TexProblem& P, Resident& r) {
    BakeLaunch a{};
    a.views = r.views.p;
    a.pixels = r.pool.p;
    a.V = r.V.p;
    a.vrgb = r.vrgb.p;
    a.tri = r.tri.p;
    a.face_view = r.face_view.p;
    a.texture = r.texture.p;
    a.uv = r.uv.p;
    a.n_triangles = P.n_triangles;
    a.A = P.atlas;
    a.runs_per_row = (P.atlas.W + kTexRun - 1) / kTexRun;
    a.n_runs = (int64_t)a.runs_per_row * P.atlas.H;
    a.fill = tex_pack(P.fill);
    hipLaunchKernelGGL(tex_bake_kernel, dim3(blocks(a.n_runs)), dim3(kTexBlock), 0, s, a);
    hipLaunchKernelGGL(tex_uv_kernel, dim3(blocks(P.n_triangles)), dim3(kTexBlock), 0, s, a);
    SFM_HIP(hipGetLastError());
}

// after the stream is synchronised
void read_counts(hipStream_t s, const TexProblem& P, const Resident& r, sfm_mesh_face_views_stats* st) {
    unsigned long long c[kCounters] = {};
    SFM_HIP(hipMemcpyAsync(c, r.counters.p, sizeof c, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    st->n_not_drawable = (int64_t)c[kNotDrawable];
    st->n_textured = (int64_t)c[kTextured];
    st->sum_pixels = (int64_t)c[kSumPixels];
    st->n_untextured = P.n_triangles - st->n_textured;
}

void download_views(hipStream_t s, const TexProblem& P, const Resident& r, int32_t* face_view, int32_t* face_pixels) {
    const size_t bytes = (size_t)P.n_triangles * sizeof(int32_t);
    if (face_view) SFM_HIP(hipMemcpyAsync(face_view, r.face_view.p, bytes, hipMemcpyDeviceToHost, s));
    if (face_pixels) SFM_HIP(hipMemcpyAsync(face_pixels, r.face_pixels.p, bytes, hipMemcpyDeviceToHost, s));
}

void download_bake(hipStream_t s, const TexProblem& P, const Resident& r, uint8_t* texture, float* uv) {
    SFM_HIP(hipMemcpyAsync(texture, r.texture.p, 3 * (size_t)P.atlas.W * P.atlas.H, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipMemcpyAsync(uv, r.uv.p, 6 * (size_t)P.n_triangles * sizeof(float), hipMemcpyDeviceToHost, s));
}

}  // namespace

void tex_face_views_device(sfm_ctx* ctx, const TexProblem& P, const float* V, const int32_t* tri, int32_t* face_view,
                           int32_t* face_pixels, sfm_mesh_face_views_stats* st) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    Resident r;
    StreamEvents<4> ev;
    ev.record(0, s);
    upload_mesh(s, P, V, tri, r);
    ev.record(1, s);
    launch_views(s, P, r);
    ev.record(2, s);
    download_views(s, P, r, face_view, face_pixels);
    ev.record(3, s);
    read_counts(s, P, r, st);
    for (int p = 0; p < 3; ++p) st->seconds[p] = ev.between(p, p + 1);
}

void tex_bake_device(sfm_ctx* ctx, const TexProblem& P, const uint8_t* pixels, const float* V, const uint8_t* vertex_rgb,
                     const int32_t* tri, const int32_t* face_view, uint8_t* texture, float* uv, sfm_mesh_bake_stats* st) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    Resident r;
    StreamEvents<4> ev;
    ev.record(0, s);
    upload_mesh(s, P, V, tri, r);
    upload_images(s, P, pixels, vertex_rgb, r);
    r.face_view.upload(face_view, (size_t)P.n_triangles, s);
    ev.record(1, s);
    launch_bake(s, P, r);
    ev.record(2, s);
    download_bake(s, P, r, texture, uv);
    ev.record(3, s);
    SFM_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < 3; ++p) st->seconds[p] = ev.between(p, p + 1);
}

void tex_texture_device(sfm_ctx* ctx, const TexProblem& P, const uint8_t* pixels, const float* V, const uint8_t* vertex_rgb,
                        const int32_t* tri, int32_t* face_view, int32_t* face_pixels, uint8_t* texture, float* uv,
                        sfm_mesh_texture_stats* st) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    Resident r;
    StreamEvents<4> ev;
    ev.record(0, s);
    upload_mesh(s, P, V, tri, r);
    upload_images(s, P, pixels, vertex_rgb, r);
    ev.record(1, s);
    launch_views(s, P, r);
    launch_bake(s, P, r);
    ev.record(2, s);
    download_views(s, P, r, face_view, face_pixels);
    download_bake(s, P, r, texture, uv);
    ev.record(3, s);
    read_counts(s, P, r, &st->views);
    for (int p = 0; p < 3; ++p) st->seconds[p] = ev.between(p, p + 1);
}

}  // namespace sfm
