// The mesh stage on the device (gfx950): the depth maps and the volume of a
// call resident, five kernels, no atomics anywhere, so the order of the
// vertices (owner's raster index, slot) and of the triangles (cell raster,
// tetrahedron, triangle) does not depend on the schedule.
//
//   integrate  one lane per lattice point; a workgroup of 256 lanes owns 64
//              points along x by 4 along y (grid z is k), so neighbouring
//              lanes read neighbouring depth pixels.  The image loop is
//              uniform over the workgroup and the per-image constants are read
//              at a uniform index (scalar registers).  A lane keeps its sum,
//              count and colour sums in registers and stores 9 bytes; the
//              workgroup's observed count goes to obs_count[workgroup]
//              (ballots, LDS), summed by the scan kernel.
//   mark       one lane per lattice point, 256 consecutive raster indices per
//              workgroup: the 7-bit mask of the owned edges that carry a
//              vertex and the triangle count of the point's own cell (0 .. 12),
//              a byte each; the workgroup's totals (vertices, triangles,
//              degenerate triangles) come from a wavefront reduction
//              (shuffles, then LDS) and go to three block_count arrays.
//   scan       dense_scan.h's kernel, one workgroup per array: the exclusive
//              int64 prefix of its block counts; the totals are read back
//              once, to check the caps and to size the download.
//   vertex     a lane's rank is its block's base + the prefix inside the
//              workgroup over the lanes' popcounts; writes vert_base[point]
//              and the point's vertices.
//   triangle   the same ranking over the triangle counts; the index of an
//              edge's vertex is vert_base[owner] + popcount(mask[owner] below
//              the slot).
#pragma clang fp contract(off)

#include <algorithm>

#include "dense_scan.h"
#include "mesh.h"

namespace sfm {
namespace {

static_assert(kMeshBlock == kDenseBlock && kMeshTileX * kMeshTileY == kMeshBlock, "dense_scan.h's workgroup");

struct TsdfLaunch {
    const MeshView* views;
    const float* depth;
    const uint8_t* pixels;   // NULL: no colours
    float* tsdf;
    uint8_t *weight, *rgb, *has_rgb;
    int32_t* obs_count;
    MeshGrid g;
    float trunc;
    int32_t n_img;
};

__global__ __launch_bounds__(kMeshBlock) void tsdf_integrate_kernel(TsdfLaunch a) {
    __shared__ int32_t seen[4];
    const int32_t i = (int32_t)(blockIdx.x * kMeshTileX + (threadIdx.x & (kMeshTileX - 1)));
    const int32_t j = (int32_t)(blockIdx.y * kMeshTileY + (threadIdx.x >> 6));
    const int32_t k = (int32_t)blockIdx.z;
    int32_t wgt = 0;
    if (i < a.g.nx && j < a.g.ny) {
        const int64_t at = mesh_raster(a.g, i, j, k);
        float t;
        uint8_t c[3] = {0, 0, 0}, has = 0;
        wgt = mesh_integrate_point(a.views, a.n_img, a.g, a.trunc, a.depth, a.pixels, i, j, k, &t, c, &has);
        a.tsdf[at] = t;
        a.weight[at] = (uint8_t)wgt;
        if (a.pixels) {
            a.rgb[3 * at] = c[0];
            a.rgb[3 * at + 1] = c[1];
            a.rgb[3 * at + 2] = c[2];
            a.has_rgb[at] = has;
        }
    }
    int32_t n_seen;
    block_ballot_rank(wgt > 0, seen, &n_seen);
    if (threadIdx.x == 0) a.obs_count[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = n_seen;
}

struct MeshLaunch {
    const float* tsdf;
    const uint8_t *weight, *rgb, *has_rgb;   // rgb NULL: no colours
    uint8_t *mask, *ntri;
    int32_t* block_count;        // [3][n_blocks]: vertices, triangles, degenerate triangles
    const int64_t* block_base;   // [3][n_blocks + 1]
    int32_t* vert_base;
    float* V;
    uint8_t* vrgb;
    int32_t* tri;
    MeshGrid g;
    int64_t n_vox, n_blocks;
    int32_t min_weight;
};

__global__ __launch_bounds__(kMeshBlock) void mesh_mark_kernel(MeshLaunch a) {
    __shared__ int32_t wave_sum[3][4];
    const int64_t at = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    int32_t nv = 0, nt = 0, nd = 0;
    if (at < a.n_vox) {
        const int32_t i = (int32_t)(at % a.g.nx), j = (int32_t)((at / a.g.nx) % a.g.ny), k = (int32_t)(at / ((int64_t)a.g.nx * a.g.ny));
        const uint32_t m = mesh_point_marks(a.g, a.tsdf, a.weight, a.min_weight, i, j, k, &nt, &nd);
        a.mask[at] = (uint8_t)m;
        a.ntri[at] = (uint8_t)nt;
        nv = __popc(m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nv += __shfl_down(nv, o);
        nt += __shfl_down(nt, o);
        nd += __shfl_down(nd, o);
    }
    if ((threadIdx.x & 63) == 0) {
        wave_sum[0][threadIdx.x >> 6] = nv;
        wave_sum[1][threadIdx.x >> 6] = nt;
        wave_sum[2][threadIdx.x >> 6] = nd;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        a.block_count[threadIdx.x * a.n_blocks + blockIdx.x] =
            (wave_sum[threadIdx.x][0] + wave_sum[threadIdx.x][1]) + (wave_sum[threadIdx.x][2] + wave_sum[threadIdx.x][3]);
}

__global__ __launch_bounds__(kMeshBlock) void mesh_vertex_kernel(MeshLaunch a) {
    __shared__ int32_t wave_sum[4];
    const int64_t at = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    const uint32_t m = at < a.n_vox ? a.mask[at] : 0u;
    int32_t all;
    int64_t rank = a.block_base[blockIdx.x] + block_exclusive(__popc(m), wave_sum, &all);
    if (at >= a.n_vox) return;
    a.vert_base[at] = (int32_t)rank;
    if (!m) return;
    const int32_t i = (int32_t)(at % a.g.nx), j = (int32_t)((at / a.g.nx) % a.g.ny), k = (int32_t)(at / ((int64_t)a.g.nx * a.g.ny));
    for (int s = 0; s < 7; ++s)
        if ((m >> s) & 1u) {
            float X[3];
            uint8_t c[3] = {0, 0, 0};
            mesh_edge_vertex(a.g, a.tsdf, a.rgb, a.has_rgb, i, j, k, s, X, c);
            a.V[3 * rank] = X[0];
            a.V[3 * rank + 1] = X[1];
            a.V[3 * rank + 2] = X[2];
            if (a.vrgb) {
                a.vrgb[3 * rank] = c[0];
                a.vrgb[3 * rank + 1] = c[1];
                a.vrgb[3 * rank + 2] = c[2];
            }
            ++rank;
        }
}

__global__ __launch_bounds__(kMeshBlock) void mesh_triangle_kernel(MeshLaunch a) {
    __shared__ int32_t wave_sum[4];
    const int64_t at = (int64_t)blockIdx.x * kMeshBlock + threadIdx.x;
    const int32_t nt = at < a.n_vox ? (int32_t)a.ntri[at] : 0;
    int32_t all;
    const int64_t rank = a.block_base[a.n_blocks + 1 + blockIdx.x] + block_exclusive(nt, wave_sum, &all);
    if (!nt) return;
    const int32_t i = (int32_t)(at % a.g.nx), j = (int32_t)((at / a.g.nx) % a.g.ny), k = (int32_t)(at / ((int64_t)a.g.nx * a.g.ny));
    mesh_cell_triangles(a.g, a.tsdf, a.vert_base, a.mask, i, j, k, a.tri + 3 * rank);
}

// the volume of a call on the device
struct Volume {
    DBuf<float> tsdf;
    DBuf<uint8_t> weight, rgb, has_rgb;
};
struct TsdfResident {
    DBuf<MeshView> views;
    DBuf<float> depth;
    DBuf<uint8_t> pool;
    DBuf<int32_t> obs_count;
    DBuf<int64_t> obs_base;
    int64_t n_groups = 0;
};
struct MeshResident {
    DBuf<uint8_t> mask, ntri;
    DBuf<int32_t> block_count, vert_base;
    DBuf<int64_t> block_base;
    DBuf<float> V;
    DBuf<uint8_t> vrgb;
    DBuf<int32_t> tri;
    MeshLaunch a;
};

void tsdf_upload(hipStream_t s, const MeshProblem& P, const float* depth, const uint8_t* pixels, TsdfResident& r,
                 Volume& vol) {
    const size_t n = (size_t)P.n_vox;
    r.views.alloc(std::max<size_t>(P.views.size(), 1));
    r.depth.alloc((size_t)std::max<int64_t>(P.images.n_map, 1));
    r.views.upload(P.views.data(), P.views.size(), s);
    r.depth.upload(depth, (size_t)P.images.n_map, s);
    if (pixels) {
        r.pool.alloc((size_t)std::max<int64_t>(P.images.pool_hi - P.images.pool_lo, 1));
        r.pool.upload(pixels + P.images.pool_lo, (size_t)(P.images.pool_hi - P.images.pool_lo), s);
        vol.rgb.alloc(3 * n);
        vol.has_rgb.alloc(n);
    }
    vol.tsdf.alloc(n);
    vol.weight.alloc(n);
}

void tsdf_launch(hipStream_t s, const MeshProblem& P, TsdfResident& r, Volume& vol) {
    const dim3 grid((unsigned)((P.g.nx + kMeshTileX - 1) / kMeshTileX), (unsigned)((P.g.ny + kMeshTileY - 1) / kMeshTileY),
                    (unsigned)P.g.nz);
    r.n_groups = (int64_t)grid.x * grid.y * grid.z;
    r.obs_count.alloc((size_t)r.n_groups);
    r.obs_base.alloc((size_t)r.n_groups + 1);
    TsdfLaunch a{};
    a.views = r.views.p;
    a.depth = r.depth.p;
    a.pixels = r.pool.p;
    a.tsdf = vol.tsdf.p;
    a.weight = vol.weight.p;
    a.rgb = vol.rgb.p;
    a.has_rgb = vol.has_rgb.p;
    a.obs_count = r.obs_count.p;
    a.g = P.g;
    a.trunc = P.trunc;
    a.n_img = P.images.n_img;
    hipLaunchKernelGGL(tsdf_integrate_kernel, grid, dim3(kMeshBlock), 0, s, a);
    hipLaunchKernelGGL(dense_scan_kernel, dim3(1), dim3(kDenseBlock), 0, s, r.obs_count.p, r.n_groups, r.obs_base.p);
    SFM_HIP(hipGetLastError());
}

void volume_download(hipStream_t s, int64_t n_vox, const Volume& vol, float* tsdf, uint8_t* weight, uint8_t* rgb,
                     uint8_t* has_rgb) {
    const size_t n = (size_t)n_vox;
    if (tsdf) SFM_HIP(hipMemcpyAsync(tsdf, vol.tsdf.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    if (weight) SFM_HIP(hipMemcpyAsync(weight, vol.weight.p, n, hipMemcpyDeviceToHost, s));
    if (rgb && vol.rgb.p) SFM_HIP(hipMemcpyAsync(rgb, vol.rgb.p, 3 * n, hipMemcpyDeviceToHost, s));
    if (has_rgb && vol.has_rgb.p) SFM_HIP(hipMemcpyAsync(has_rgb, vol.has_rgb.p, n, hipMemcpyDeviceToHost, s));
}

// mark and scan; the totals are read back (the stream is synchronised)
void mesh_mark(hipStream_t s, const MeshGrid& g, int64_t n_vox, int32_t min_weight, const float* tsdf,
               const uint8_t* weight, const uint8_t* rgb, const uint8_t* has_rgb, MeshResident& r, sfm_mesh_stats* st) {
    const size_t n = (size_t)n_vox;
    const int64_t nb = mesh_blocks(n_vox);
    r.mask.alloc(n);
    r.ntri.alloc(n);
    r.vert_base.alloc(n);
    r.block_count.alloc((size_t)(3 * nb));
    r.block_base.alloc((size_t)(3 * (nb + 1)));
    MeshLaunch& a = r.a;
    a = MeshLaunch{};
    a.tsdf = tsdf;
    a.weight = weight;
    a.rgb = rgb;
    a.has_rgb = has_rgb;
    a.mask = r.mask.p;
    a.ntri = r.ntri.p;
    a.block_count = r.block_count.p;
    a.block_base = r.block_base.p;
    a.vert_base = r.vert_base.p;
    a.g = g;
    a.n_vox = n_vox;
    a.n_blocks = nb;
    a.min_weight = min_weight;
    hipLaunchKernelGGL(mesh_mark_kernel, dim3((unsigned)nb), dim3(kMeshBlock), 0, s, a);
    hipLaunchKernelGGL(dense_scan_kernel, dim3(3), dim3(kDenseBlock), 0, s, r.block_count.p, nb, r.block_base.p);
    SFM_HIP(hipGetLastError());
    int64_t totals[3] = {0, 0, 0};
    for (int q = 0; q < 3; ++q)
        SFM_HIP(hipMemcpyAsync(&totals[q], r.block_base.p + q * (nb + 1) + nb, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    st->n_vertices = totals[0];
    st->n_triangles = totals[1];
    st->n_degenerate = totals[2];
}

void mesh_emit(hipStream_t s, const MeshOut& out, const sfm_mesh_stats& st, MeshResident& r) {
    MeshLaunch& a = r.a;
    if (st.n_vertices == 0) return;   // no vertex: no triangle either
    r.V.alloc(3 * (size_t)st.n_vertices);
    a.V = r.V.p;
    if (a.rgb && out.rgb) r.vrgb.alloc(3 * (size_t)st.n_vertices), a.vrgb = r.vrgb.p;
    r.tri.alloc(3 * (size_t)std::max<int64_t>(st.n_triangles, 1));
    a.tri = r.tri.p;
    hipLaunchKernelGGL(mesh_vertex_kernel, dim3((unsigned)a.n_blocks), dim3(kMeshBlock), 0, s, a);
    hipLaunchKernelGGL(mesh_triangle_kernel, dim3((unsigned)a.n_blocks), dim3(kMeshBlock), 0, s, a);
    SFM_HIP(hipGetLastError());
}

void mesh_download(hipStream_t s, const MeshOut& out, const sfm_mesh_stats& st, const MeshResident& r) {
    if (st.n_vertices == 0) return;
    SFM_HIP(hipMemcpyAsync(out.V, r.V.p, 3 * (size_t)st.n_vertices * sizeof(float), hipMemcpyDeviceToHost, s));
    if (r.vrgb.p) SFM_HIP(hipMemcpyAsync(out.rgb, r.vrgb.p, 3 * (size_t)st.n_vertices, hipMemcpyDeviceToHost, s));
    if (st.n_triangles)
        SFM_HIP(hipMemcpyAsync(out.tri, r.tri.p, 3 * (size_t)st.n_triangles * sizeof(int32_t), hipMemcpyDeviceToHost, s));
}

int64_t read_observed(hipStream_t s, const TsdfResident& r) {
    int64_t n = 0;
    SFM_HIP(hipMemcpyAsync(&n, r.obs_base.p + r.n_groups, sizeof n, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    return n;
}

}  // namespace

void tsdf_device(sfm_ctx* ctx, const MeshProblem& P, const float* depth, const uint8_t* pixels, float* tsdf,
                 uint8_t* weight, uint8_t* rgb, uint8_t* has_rgb, int64_t* n_observed, double* seconds) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    TsdfResident r;
    Volume vol;
    StreamEvents<4> ev;
    ev.record(0, s);
    tsdf_upload(s, P, depth, pixels, r, vol);
    ev.record(1, s);
    tsdf_launch(s, P, r, vol);
    ev.record(2, s);
    volume_download(s, P.n_vox, vol, tsdf, weight, rgb, has_rgb);
    ev.record(3, s);
    *n_observed = read_observed(s, r);
    for (int p = 0; p < 3; ++p) seconds[p] = ev.between(p, p + 1);
}

void mesh_extract_device(sfm_ctx* ctx, const MeshGrid& g, int32_t min_weight, const float* tsdf, const uint8_t* weight,
                         const uint8_t* rgb, const uint8_t* has_rgb, const MeshOut& out, sfm_mesh_stats* st) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    const int64_t n_vox = (int64_t)g.nx * g.ny * g.nz;
    const size_t n = (size_t)n_vox;
    Volume vol;
    MeshResident r;
    StreamEvents<4> ev;
    ev.record(0, s);
    vol.tsdf.alloc(n);
    vol.weight.alloc(n);
    vol.tsdf.upload(tsdf, n, s);
    vol.weight.upload(weight, n, s);
    if (rgb) {
        vol.rgb.alloc(3 * n);
        vol.has_rgb.alloc(n);
        vol.rgb.upload(rgb, 3 * n, s);
        vol.has_rgb.upload(has_rgb, n, s);
    }
    ev.record(1, s);
    mesh_mark(s, g, n_vox, min_weight, vol.tsdf.p, vol.weight.p, vol.rgb.p, vol.has_rgb.p, r, st);
    mesh_require_indexable("sfm_mesh_extract", st->n_vertices);
    mesh_require_caps("sfm_mesh_extract", *st, out);
    mesh_emit(s, out, *st, r);
    ev.record(2, s);
    mesh_download(s, out, *st, r);
    ev.record(3, s);
    SFM_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < 3; ++p) st->seconds[p] = ev.between(p, p + 1);
}

void mesh_reconstruct_device(sfm_ctx* ctx, const MeshProblem& P, const float* depth, const uint8_t* pixels,
                             int32_t min_weight, const MeshOut& out, float* tsdf, uint8_t* weight,
                             sfm_mesh_reconstruct_stats* st) {
    CtxScope scope_(ctx);
    hipStream_t s = ctx->stream;
    TsdfResident t;
    Volume vol;
    MeshResident r;
    StreamEvents<4> ev;
    ev.record(0, s);
    tsdf_upload(s, P, depth, pixels, t, vol);
    ev.record(1, s);
    tsdf_launch(s, P, t, vol);
    mesh_mark(s, P.g, P.n_vox, min_weight, vol.tsdf.p, vol.weight.p, vol.rgb.p, vol.has_rgb.p, r, &st->mesh);
    st->tsdf.n_observed = read_observed(s, t);
    mesh_require_indexable("sfm_mesh_reconstruct", st->mesh.n_vertices);
    mesh_require_caps("sfm_mesh_reconstruct", st->mesh, out);
    mesh_emit(s, out, st->mesh, r);
    ev.record(2, s);
    mesh_download(s, out, st->mesh, r);
    volume_download(s, P.n_vox, vol, tsdf, weight, nullptr, nullptr);
    ev.record(3, s);
    SFM_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < 3; ++p) st->seconds[p] = ev.between(p, p + 1);
}

}  // namespace sfm
