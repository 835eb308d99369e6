// Track building on the device (gfx950): connected components of the match
// graph by lock-free hooking, then the per-component verdicts and the tracks
// in canonical order.  Every result is integral and a function of the edge
// set alone, so the output equals the host twin's (tracks.cpp) bit for bit.
//
//   init        parent[v] = v
//   union       one lane per edge: CAS the larger root under the smaller, so
//               a component's final root is its smallest node, whatever the
//               order the edges were taken in; flags the nodes it touches
//   label       label[v] = root(v) for the touched nodes, size[root] += 1
//   scan        exclusive scan over the nodes of (is a root, size): the
//               component's index (roots in node order = track order, nodes
//               being image-major) and its slab offset; three launches
//   gather      the members into their component's slab, in arrival order
//   component   a 16-lane group per component of <= 16 members, else a wave in
//               rounds of 64: each member's image (binary search), its rank =
//               the members with a smaller id, a conflict = another member of
//               its image, all pairs by shuffles; the member goes to
//               sorted[rank]; the verdict (kept, conflict, short)
//   scan        the same scan over the components of (kept, kept length)
//   write       pt_offsets, obs_img, obs_feat, obs_uv of the kept components
//
// No kernel waits on another workgroup: the only retry loop is the union's
// CAS, which fails only when another lane's CAS on the same word succeeded.
#include <climits>

#include "tracks.h"

namespace sfm {
namespace {

constexpr int kThreads = 256;
constexpr int kScanItems = 4;
constexpr int kScanTile = kThreads * kScanItems;   // elements per scan tile: 1024
constexpr int kGroup = 16;                         // lanes of the short form of the component pass
constexpr int kCompPerWave = 64 / kGroup;

inline unsigned grid_of(int64_t n, int per_block = kThreads) { return (unsigned)((n + per_block - 1) / per_block); }

// ---- union-find -------------------------------------------------------------
// parent[x] <= x always, and only a root (parent[x] == x) is ever hooked, by a
// CAS: the pointers form a forest at every moment and a node that stopped being
// a root never becomes one again.  Any value a lane reads from parent[x], however
// stale, is a node of x's component, so reads need no ordering: a stale "root"
// costs a failed CAS, whose return value is current.

__device__ __forceinline__ int32_t load_parent(const int32_t* parent, int32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x as far as this lane sees, halving the path on the way (the
// stored value is an ancestor below x of a node that is no root: harmless to
// every other lane)
__device__ __forceinline__ int32_t find_halving(int32_t* parent, int32_t x) {
    int32_t p = load_parent(parent, x);
    while (p != x) {
        const int32_t g = load_parent(parent, p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

__global__ __launch_bounds__(kThreads) void tracks_init_kernel(int32_t n, int32_t* __restrict__ parent) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v < n) parent[v] = (int32_t)v;
}

__global__ __launch_bounds__(kThreads) void tracks_union_kernel(int32_t n_edges, const int32_t* __restrict__ eu,
                                                                const int32_t* __restrict__ ev, int32_t* parent,
                                                                uint8_t* touched) {
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k >= n_edges) return;
    int32_t u = eu[k], v = ev[k];
    touched[u] = 1;   // (every writer stores the same byte)
    touched[v] = 1;
    u = find_halving(parent, u);
    v = find_halving(parent, v);
    while (u != v) {
        if (u < v) {
            const int32_t t = u;
            u = v;
            v = t;
        }
        const int32_t old = atomicCAS(parent + u, u, v);   // the larger root under the smaller
        if (old == u) break;
        // another lane hooked u first: on from where it points now (old < u, so
        // this lane's u falls with every failure and the loop ends)
        u = find_halving(parent, old);
        v = find_halving(parent, v);
    }
}

// the forest is final here: plain loads
__global__ __launch_bounds__(kThreads) void tracks_label_kernel(int32_t n, const int32_t* __restrict__ parent,
                                                                const uint8_t* __restrict__ touched,
                                                                int32_t* __restrict__ label, int32_t* size) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    if (!touched[v]) {
        label[v] = -1;
        return;
    }
    int32_t r = (int32_t)v;
    for (int32_t p = parent[r]; p != r; p = parent[r]) r = p;
    label[v] = r;
    atomicAdd(size + r, 1);
}

// ---- the scan: (count of positive values, sum of values) ------------------------
struct Duo {
    int32_t c, s;
};
__device__ __forceinline__ Duo operator+(Duo a, Duo b) { return Duo{a.c + b.c, a.s + b.s}; }

// exclusive prefix of `mine` over the workgroup's threads, and the total
__device__ __forceinline__ Duo block_exclusive(Duo mine, Duo& total) {
    __shared__ Duo wsum[kThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Duo inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int32_t c = __shfl_up(inc.c, o), s = __shfl_up(inc.s, o);
        if (lane >= o) inc = inc + Duo{c, s};
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    Duo base{0, 0};
    total = Duo{0, 0};
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) base = base + wsum[w];
        total = total + wsum[w];
    }
    __syncthreads();   // (wsum is written again by the next call)
    return Duo{base.c + inc.c - mine.c, base.s + inc.s - mine.s};
}

__device__ __forceinline__ void load_items(const int32_t* __restrict__ val, int32_t n, int64_t k0,
                                           int32_t (&x)[kScanItems]) {
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) x[t] = k0 + t < n ? val[k0 + t] : 0;
}

// 1 of 3: every tile's sum
__global__ __launch_bounds__(kThreads) void tracks_scan_reduce_kernel(const int32_t* __restrict__ val, int32_t n,
                                                                      Duo* __restrict__ tile_sum) {
    int32_t x[kScanItems];
    load_items(val, n, (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems, x);
    Duo mine{0, 0};
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) mine = mine + Duo{x[t] > 0, x[t]};
    Duo total;
    block_exclusive(mine, total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// 2 of 3: the exclusive scan of the tile sums, in place, by one workgroup; total[0] = the grand total
__global__ __launch_bounds__(kThreads) void tracks_scan_tiles_kernel(Duo* tile_sum, int32_t n_tiles,
                                                                     Duo* __restrict__ total_out) {
    Duo carry{0, 0};
    for (int32_t base = 0; base < n_tiles; base += kThreads) {   // (uniform trip count)
        const int32_t k = base + threadIdx.x;
        const Duo mine = k < n_tiles ? tile_sum[k] : Duo{0, 0};
        Duo total;
        const Duo ex = block_exclusive(mine, total);
        if (k < n_tiles) tile_sum[k] = carry + ex;
        carry = carry + total;
    }
    if (threadIdx.x == 0) *total_out = carry;
}

// 3 of 3: emit(k, value, index among the positive values, sum of the values before) for every positive value
template <class Emit>
__global__ __launch_bounds__(kThreads) void tracks_scan_apply_kernel(const int32_t* __restrict__ val, int32_t n,
                                                                     const Duo* __restrict__ tile_sum, Emit emit) {
    const int64_t k0 = (int64_t)blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int32_t x[kScanItems];
    load_items(val, n, k0, x);
    Duo mine{0, 0};
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) mine = mine + Duo{x[t] > 0, x[t]};
    Duo total;
    Duo at = tile_sum[blockIdx.x] + block_exclusive(mine, total);
#pragma unroll
    for (int t = 0; t < kScanItems; ++t) {
        if (x[t] > 0) emit((int32_t)(k0 + t), x[t], at.c, at.s);
        at = at + Duo{x[t] > 0, x[t]};
    }
}

// the components: index of a root, and per component its slab offset and length
struct EmitComponents {
    int32_t* root_comp;   // [n_space], written at the roots
    int32_t* comp_off;    // [n_comp]
    int32_t* comp_len;    // [n_comp]
    __device__ void operator()(int32_t k, int32_t v, int32_t idx, int32_t off) const {
        root_comp[k] = idx;
        comp_off[idx] = off;
        comp_len[idx] = v;
    }
};
// the tracks: a kept component's first observation, and pt_offsets
struct EmitTracks {
    int32_t* comp_obs;   // [n_comp], written at the kept components
    int32_t* pt_off;     // [n_tracks]
    __device__ void operator()(int32_t k, int32_t, int32_t idx, int32_t off) const {
        comp_obs[k] = off;
        pt_off[idx] = off;
    }
};

// ---- gather -------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void tracks_gather_kernel(int32_t n, const int32_t* __restrict__ label,
                                                                 const int32_t* __restrict__ root_comp,
                                                                 const int32_t* __restrict__ comp_off,
                                                                 int32_t* cursor, int32_t* __restrict__ slab) {
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= n) return;
    const int32_t r = label[v];
    if (r < 0) return;
    const int32_t c = root_comp[r];
    slab[comp_off[c] + atomicAdd(cursor + c, 1)] = (int32_t)v;   // (slot < comp_len[c]: the label pass counted it)
}

// ---- the per-component pass -------------------------------------------------------
// the image I with feat_off[I] <= id < feat_off[I + 1] (images may be empty)
__device__ __forceinline__ int32_t image_of(const int32_t* __restrict__ feat_off, int32_t n_img, int32_t id) {
    int32_t lo = 0, hi = n_img - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (feat_off[mid + 1] > id) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// This lane's member (id, im) against the members (bid, bim) of lanes
// (g + r) % W of its W-lane group, r = r_begin .. W - 1: ids below it, and
// whether another member shares its image.  An id < 0 is no member.  Every
// lane of the wave calls it (shuffles).
template <int W>
__device__ __forceinline__ void member_rounds(int g, int32_t id, int32_t im, int32_t bid, int32_t bim, int r_begin,
                                              int32_t& rank, bool& conflict) {
#pragma unroll 4
    for (int r = r_begin; r < W; ++r) {
        const int src = (g + r) & (W - 1);
        const int32_t oid = __shfl(bid, src, W), oim = __shfl(bim, src, W);
        if (oid >= 0 && oid != id) {
            rank += oid < id;
            conflict |= oim == im;
        }
    }
}

enum { kCntConflict = 0, kCntShort, kCntTracks, kCntObs, kCntMax, kCounts };

struct ComponentArgs {
    int32_t n_comp, n_img, min_len;
    const int32_t* feat_off;   // [n_img + 1]
    const int32_t* comp_off;   // [n_comp]
    const int32_t* comp_len;   // [n_comp]
    const int32_t* slab;       // [n_nodes], members in arrival order
    int32_t* sorted;           // [n_nodes], members by id (kept components)
    int32_t* sorted_img;       // [n_nodes], their images
    int32_t* slab_comp;        // [n_nodes], the component of a slab position
    int32_t* kept_len;         // [n_comp], 0 for a removed component
    unsigned long long* counts;   // [kCounts]
};

__global__ __launch_bounds__(kThreads) void tracks_component_kernel(ComponentArgs a) {
    __shared__ unsigned cnt[kCounts];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < kCounts) cnt[tid] = 0;
    __syncthreads();
    const int64_t cw = ((int64_t)blockIdx.x * (kThreads / 64) + wave) * kCompPerWave;   // the wave's first component
    unsigned c[kCounts] = {};
    auto verdict = [&](int32_t comp, int32_t n, bool conflict) {   // one lane per component
        if (conflict) {
            ++c[kCntConflict];
        } else if (n < a.min_len) {
            ++c[kCntShort];
        } else {
            ++c[kCntTracks];
            c[kCntObs] += (unsigned)n;
            c[kCntMax] = max(c[kCntMax], (unsigned)n);
        }
        a.kept_len[comp] = !conflict && n >= a.min_len ? n : 0;
    };
    {
        const int grp = lane / kGroup, g = lane % kGroup;
        const int64_t k = cw + grp;
        const bool has = k < a.n_comp;
        const int32_t o0 = has ? a.comp_off[k] : 0;
        const int32_t n = has ? a.comp_len[k] : 0;
        if (!__any(n > kGroup)) {
            // ---- a lane group per component ----
            const bool mine = g < n;
            const bool big = n > a.n_img;   // more members than images: a conflict by pigeonhole
            const int32_t id = mine ? a.slab[o0 + g] : -1;
            const int32_t im = mine ? image_of(a.feat_off, a.n_img, id) : -1;
            int32_t rank = 0;
            bool conf = false;
            if (!__all(!has || big))   // (wave-uniform: the rounds shuffle)
                member_rounds<kGroup>(g, id, im, id, im, 1, rank, conf);
            const unsigned long long m = __ballot(mine && conf);
            const bool conflict = big || ((m >> (grp * kGroup)) & ((1ull << kGroup) - 1)) != 0;
            if (mine) {
                a.slab_comp[o0 + g] = (int32_t)k;
                if (!conflict) {
                    a.sorted[o0 + rank] = id;
                    a.sorted_img[o0 + rank] = im;
                }
            }
            if (has && g == 0) verdict((int32_t)k, n, conflict);
        } else {
            // ---- a wave per component, all pairs in rounds of 64 ----
            for (int q = 0; q < kCompPerWave; ++q) {
                const int64_t kq = cw + q;
                if (kq >= a.n_comp) break;   // (wave-uniform)
                const int32_t q0 = a.comp_off[kq];
                const int32_t nq = a.comp_len[kq];
                bool conflict = nq > a.n_img;
                if (!conflict) {
                    const int nt = (nq + 63) / 64;
                    for (int ti = 0; ti < nt; ++ti) {
                        const int i = ti * 64 + lane;
                        const int32_t id = i < nq ? a.slab[q0 + i] : -1;
                        const int32_t im = id >= 0 ? image_of(a.feat_off, a.n_img, id) : -1;
                        int32_t rank = 0;
                        bool conf = false;
                        for (int tj = 0; tj < nt; ++tj) {
                            const int jn = tj * 64 + lane;
                            const int32_t bid = jn < nq ? a.slab[q0 + jn] : -1;
                            const int32_t bim = bid >= 0 ? image_of(a.feat_off, a.n_img, bid) : -1;
                            member_rounds<64>(lane, id, im, bid, bim, 0, rank, conf);
                        }
                        if (id >= 0) {   // (a conflict component's order is never read)
                            a.sorted[q0 + rank] = id;
                            a.sorted_img[q0 + rank] = im;
                        }
                        conflict |= __any(id >= 0 && conf) != 0;
                    }
                }
                for (int i = lane; i < nq; i += 64) a.slab_comp[q0 + i] = (int32_t)kq;
                if (lane == 0) verdict((int32_t)kq, nq, conflict);
            }
        }
    }
    // integer sums (and one maximum) per workgroup, then integer atomics: the same numbers every run
#pragma unroll
    for (int t = 0; t < kCounts; ++t) {
        unsigned v = c[t];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned w = __shfl_xor(v, o);
            v = t == kCntMax ? max(v, w) : v + w;
        }
        if (lane == 0 && v) {
            if (t == kCntMax) atomicMax(&cnt[t], v);
            else atomicAdd(&cnt[t], v);
        }
    }
    __syncthreads();
    if (tid < kCounts && cnt[tid]) {
        if (tid == kCntMax) atomicMax(&a.counts[tid], (unsigned long long)cnt[tid]);
        else atomicAdd(&a.counts[tid], (unsigned long long)cnt[tid]);
    }
}

// ---- the output -----------------------------------------------------------------
struct WriteArgs {
    int32_t n_nodes;
    const int32_t* feat_off;
    const int32_t* comp_off;
    const int32_t* kept_len;
    const int32_t* comp_obs;
    const int32_t* slab_comp;
    const int32_t* sorted;
    const int32_t* sorted_img;
    const double* xy;   // or null
    int32_t* obs_img;
    uint32_t* obs_feat;
    double* obs_uv;
};

__global__ __launch_bounds__(kThreads) void tracks_write_kernel(WriteArgs a) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= a.n_nodes) return;
    const int32_t c = a.slab_comp[p];
    if (a.kept_len[c] == 0) return;
    const int64_t q = (int64_t)a.comp_obs[c] + (p - a.comp_off[c]);
    const int32_t id = a.sorted[p], im = a.sorted_img[p];
    a.obs_img[q] = im;
    a.obs_feat[q] = (uint32_t)(id - a.feat_off[im]);
    if (a.xy) {
        a.obs_uv[2 * q] = a.xy[2 * (int64_t)id];
        a.obs_uv[2 * q + 1] = a.xy[2 * (int64_t)id + 1];
    }
}

// the three launches of the scan up to the totals, which the host reads to size
// what the third launch fills
struct Scan {
    DBuf<Duo> tiles, total;
    int32_t n = 0;
    const int32_t* val = nullptr;
    Duo sums(const int32_t* v, int32_t count, hipStream_t s) {
        val = v;
        n = count;
        const int32_t n_tiles = (int32_t)grid_of(n, kScanTile);
        tiles.alloc((size_t)n_tiles);
        total.alloc(1);
        hipLaunchKernelGGL(tracks_scan_reduce_kernel, dim3(n_tiles), dim3(kThreads), 0, s, val, n, tiles.p);
        hipLaunchKernelGGL(tracks_scan_tiles_kernel, dim3(1), dim3(kThreads), 0, s, tiles.p, n_tiles, total.p);
        SFM_HIP(hipGetLastError());
        Duo t{0, 0};
        SFM_HIP(hipMemcpyAsync(&t, total.p, sizeof t, hipMemcpyDeviceToHost, s));
        SFM_HIP(hipStreamSynchronize(s));
        return t;
    }
    template <class Emit>
    void apply(const Emit& emit, hipStream_t s) {
        hipLaunchKernelGGL(tracks_scan_apply_kernel<Emit>, dim3(grid_of(n, kScanTile)), dim3(kThreads), 0, s, val, n,
                           tiles.p, emit);
        SFM_HIP(hipGetLastError());
    }
};

}  // namespace

void tracks_device_build(sfm_ctx* ctx, const TracksInput& in, sfm_tracks& out) {
    hipStream_t s = ctx->stream;
    PhaseTimer pt("sfm_tracks_build");
    auto phase = [&](const char* name) {   // SFM_TIMING: the split by kernel group
        if (!PhaseTimer::on()) return;
        SFM_HIP(hipStreamSynchronize(s));
        pt.mark(name);
    };
    const size_t N = (size_t)in.n_space, E = (size_t)in.n_edges;
    DBuf<int32_t> feat_off, eu, ev, parent, label, size, root_comp;
    DBuf<uint8_t> touched;
    DBuf<double> xy;
    feat_off.alloc((size_t)in.n_img + 1); feat_off.upload(in.feat_off, (size_t)in.n_img + 1, s);
    eu.alloc(E); eu.upload(in.eu, E, s);
    ev.alloc(E); ev.upload(in.ev, E, s);
    if (in.xy) {
        xy.alloc(2 * N); xy.upload(in.xy, 2 * N, s);
    }
    parent.alloc(N); label.alloc(N); size.alloc(N); root_comp.alloc(N); touched.alloc(N);
    DBuf<unsigned long long> counts;
    counts.alloc(kCounts);
    hipEvent_t* ev_t = nullptr;
    if (ctx->time_kernels) {   // the kernels alone: the uploads drained first
        ev_t = ctx_events(ctx);
        SFM_HIP(hipStreamSynchronize(s));
        SFM_HIP(hipEventRecord(ev_t[0], s));
    }
    phase("upload");
    size.zero(s); touched.zero(s); counts.zero(s);
    hipLaunchKernelGGL(tracks_init_kernel, dim3(grid_of(N)), dim3(kThreads), 0, s, in.n_space, parent.p);
    hipLaunchKernelGGL(tracks_union_kernel, dim3(grid_of(E)), dim3(kThreads), 0, s, in.n_edges, eu.p, ev.p, parent.p,
                       touched.p);
    SFM_HIP(hipGetLastError());
    phase("union");
    hipLaunchKernelGGL(tracks_label_kernel, dim3(grid_of(N)), dim3(kThreads), 0, s, in.n_space, parent.p, touched.p,
                       label.p, size.p);
    SFM_HIP(hipGetLastError());
    phase("label");
    // the components
    Scan nodes;
    const Duo comps = nodes.sums(size.p, in.n_space, s);   // (components, touched nodes)
    const size_t n_comp = (size_t)comps.c, n_nodes = (size_t)comps.s;
    DBuf<int32_t> comp_off, comp_len, cursor, slab, sorted, sorted_img, slab_comp, kept_len, comp_obs;
    comp_off.alloc(n_comp); comp_len.alloc(n_comp); cursor.alloc(n_comp); kept_len.alloc(n_comp);
    comp_obs.alloc(n_comp);
    slab.alloc(n_nodes); sorted.alloc(n_nodes); sorted_img.alloc(n_nodes); slab_comp.alloc(n_nodes);
    cursor.zero(s);
    nodes.apply(EmitComponents{root_comp.p, comp_off.p, comp_len.p}, s);
    phase("scan");
    hipLaunchKernelGGL(tracks_gather_kernel, dim3(grid_of(N)), dim3(kThreads), 0, s, in.n_space, label.p, root_comp.p,
                       comp_off.p, cursor.p, slab.p);
    SFM_HIP(hipGetLastError());
    phase("gather");
    ComponentArgs ca{(int32_t)n_comp, in.n_img, in.min_len, feat_off.p, comp_off.p, comp_len.p, slab.p,
                     sorted.p,        sorted_img.p, slab_comp.p, kept_len.p, counts.p};
    hipLaunchKernelGGL(tracks_component_kernel, dim3(grid_of((int64_t)n_comp, (kThreads / 64) * kCompPerWave)),
                       dim3(kThreads), 0, s, ca);
    SFM_HIP(hipGetLastError());
    phase("component");
    // the tracks
    Scan kept;
    const Duo trk = kept.sums(kept_len.p, (int32_t)n_comp, s);   // (tracks, observations)
    const size_t n_trk = (size_t)trk.c, n_obs = (size_t)trk.s;
    DBuf<int32_t> pt_off, obs_img;
    DBuf<uint32_t> obs_feat;
    DBuf<double> obs_uv;
    pt_off.alloc(n_trk); obs_img.alloc(n_obs); obs_feat.alloc(n_obs);
    if (in.xy) obs_uv.alloc(2 * n_obs);
    if (n_trk) {
        kept.apply(EmitTracks{comp_obs.p, pt_off.p}, s);
        WriteArgs wa{(int32_t)n_nodes, feat_off.p, comp_off.p, kept_len.p,  comp_obs.p, slab_comp.p,
                     sorted.p,         sorted_img.p, xy.p,     obs_img.p,   obs_feat.p, obs_uv.p};
        hipLaunchKernelGGL(tracks_write_kernel, dim3(grid_of((int64_t)n_nodes)), dim3(kThreads), 0, s, wa);
        SFM_HIP(hipGetLastError());
    }
    phase("tracks");
    if (ev_t) {
        SFM_HIP(hipEventRecord(ev_t[1], s));
        SFM_HIP(hipEventSynchronize(ev_t[1]));
        float t = 0.f;
        SFM_HIP(hipEventElapsedTime(&t, ev_t[0], ev_t[1]));
        ctx->last_kernel_ms = t;
    }
    // download
    unsigned long long cn[kCounts] = {};
    std::vector<int32_t> off32(n_trk);
    out.obs_img.resize(n_obs);
    out.obs_feat.resize(n_obs);
    out.has_uv = in.xy != nullptr;
    if (in.xy) out.obs_uv.resize(2 * n_obs);
    SFM_HIP(hipMemcpyAsync(cn, counts.p, sizeof cn, hipMemcpyDeviceToHost, s));
    if (n_trk) SFM_HIP(hipMemcpyAsync(off32.data(), pt_off.p, n_trk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (n_obs) {
        SFM_HIP(hipMemcpyAsync(out.obs_img.data(), obs_img.p, n_obs * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        SFM_HIP(hipMemcpyAsync(out.obs_feat.data(), obs_feat.p, n_obs * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        if (in.xy)
            SFM_HIP(hipMemcpyAsync(out.obs_uv.data(), obs_uv.p, 2 * n_obs * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    SFM_HIP(hipStreamSynchronize(s));
    phase("download");
    out.pt_offsets.resize(n_trk + 1);
    for (size_t t = 0; t < n_trk; ++t) out.pt_offsets[t] = off32[t];
    out.pt_offsets[n_trk] = (int64_t)n_obs;
    out.st.n_nodes = (int64_t)n_nodes;
    out.st.n_edges = in.n_edges;
    out.st.n_components = (int64_t)n_comp;
    out.st.n_conflict = (int64_t)cn[kCntConflict];
    out.st.n_short = (int64_t)cn[kCntShort];
    out.st.n_tracks = (int64_t)cn[kCntTracks];
    out.st.n_obs = (int64_t)cn[kCntObs];
    out.st.max_track_len = (int64_t)cn[kCntMax];
    SFM_REQUIRE(out.st.n_tracks == (int64_t)n_trk && out.st.n_obs == (int64_t)n_obs, SFM_ERR_DEVICE,
                "track counters (%lld, %lld) disagree with the scan (%zu, %zu)", (long long)out.st.n_tracks,
                (long long)out.st.n_obs, n_trk, n_obs);
}

}  // namespace sfm
