// BA static gather-reduce (ba_reduce): tiles + image blocks -> RCS targets,
// one wave per target block, then the general points' product terms -Z_a Z_b'.
#include "ba_device.h"
namespace sfm {
namespace {
__device__ __forceinline__ double term_value(const DevProblem& P, const FlatTerm& q, int r, int cc) {
    // all three index forms computed and selected without branches, so the
    // reduce loops keep a batch of term loads in flight
    const int t = q.rs;   // kFlatSym: the origin's offset within the tile
    const int R = t / kTileR + r, C = t % kTileR + cc;
    const int64_t i_rows = q.off + (int64_t)r * q.rs + cc;
    const int64_t i_trans = q.off + (int64_t)cc * kTileR + r;
    const int64_t i_sym = q.off - t + (R >= C ? R * kTileR + C : C * kTileR + R);
    const int64_t idx = q.mode == kFlatRows ? i_rows : q.mode == kFlatTrans ? i_trans : i_sym;
    return (double)q.sign * P.src[idx];
}

// s += term k, k + step, ... (k < end), in that order.  Batches of kRB: the
// descriptors first, then the data they address; the next batch's
// descriptors are issued behind this batch's data loads, and the tail batch
// is masked (clamped loads, masked adds) -- so a lane's chain is about one
// global round trip per batch instead of two, and a few terms past a whole
// batch no longer run one dependent round trip pair each.  The additions are
// those of the term-at-a-time loop, in its order (same bits).  kRB = 8
// (profiles/r05/r_red, same box): reduce 34.2 -> 34.9 us at C4, 20.5 ->
// 19.0 at rank 0 of N = 8 (2836-2846 -> 2854-2856 LM-iters/s); 16 took the
// kernel to 208 VGPRs, 2 waves per SIMD, and C4's reduce to 49.5 us.
#ifndef SFM_REDUCE_BATCH
#define SFM_REDUCE_BATCH 8
#endif
constexpr int kRB = SFM_REDUCE_BATCH;   // terms per batch (A/B builds only)
__device__ __forceinline__ double sum_terms(const DevProblem& P, int k, int step, int end, int r, int cc) {
    double s = 0.0;
    if (k >= end) return s;
    const int k_safe = k;
    FlatTerm d[kRB];
    auto ld_desc = [&](int k0) {
#pragma unroll
        for (int j = 0; j < kRB; ++j) {
            const int kj = k0 + j * step;
            d[j] = P.terms[kj < end ? kj : k_safe];
        }
    };
    ld_desc(k);
    for (; k < end; k += kRB * step) {
        double v[kRB];
#pragma unroll
        for (int j = 0; j < kRB; ++j) v[j] = term_value(P, d[j], r, cc);
        if (k + kRB * step < end) ld_desc(k + kRB * step);
#pragma unroll
        for (int j = 0; j < kRB; ++j)
            if (k + j * step < end) s += v[j];
    }
    return s;
}

__device__ __forceinline__ double* target_base(const DevProblem& P, int kind) {
    switch (kind) {
        case 0: return P.Sband;
        case 1: return P.Sarrow;
        case 2: return P.Scorner;
        case 3: return P.rhs;
        case 4: return P.bF;
        case 5: return P.cnF;
        default: return P.Sdense;
    }
}

// Longer term lists are summed by a whole workgroup (256 parallel chains);
// shorter ones by one lane per element.  A camera's band blocks collect
// ~2 * points-per-camera / chunk-points terms (about 80 at C4), the
// intrinsics corner one per chunk (thousands).
constexpr int kLongTerms = 256;

// vectors_only (iteration 0, before the Jacobi scales): bF and cnF only
__device__ __forceinline__ bool skip_kind(int kind, int vectors_only) {
    return vectors_only && kind != kDstBF && kind != kDstCnF;
}

// P.red_waves (1, 2 or 4) waves per target: wave w of a target sums its
// lane groups' terms w, w + W, ... (in units of G), and the partials are added
// in (wave, group) order -- fixed, so deterministic.  More waves per target
// shorten the chain of dependent term loads where targets collect many terms
// (a landmark shard at N = 8 has ~30-point chunks, so ~170 tile terms per
// band block against ~80 at N = 1).
template <bool FUSED>
__device__ void reduce_segment(const DevProblem& P, int vectors_only, int sg);

// n_short_blocks: the short targets' workgroups; FUSED: every workgroup past
// them is one segment of a long target (reduce_segment<true>), so the whole
// reduce is one launch instead of three
// zero_first: the first workgroup of the zero list (world > 1: the blocks
// other shards write, cleared before the all-reduce; 16 per workgroup, every
// kind, also in the vectors-only pass)
template <bool FUSED>
__global__ __launch_bounds__(256) void reduce_kernel(DevProblem P, int vectors_only, int n_short_blocks,
                                                     int zero_first) {
    if ((int)blockIdx.x >= zero_first) {
        const int wave = threadIdx.x >> 6, e = threadIdx.x & 63;
        for (int q = 0; q < 4; ++q) {
            const int z = ((int)blockIdx.x - zero_first) * 16 + wave * 4 + q;
            if (z >= P.n_zero) break;
            const ReduceTarget T = P.targets[P.n_targets + z];
            const int E = T.rows * T.cols;
            if (e < E) {
                const int r = e / T.cols, cc = e % T.cols;
                target_base(P, T.dst_kind)[T.dst + (T.cols == 1 ? r : r * T.ld + cc)] = 0.0;
            }
        }
        return;
    }
    if (FUSED && (int)blockIdx.x >= n_short_blocks) {
        reduce_segment<true>(P, vectors_only, blockIdx.x - n_short_blocks);
        return;
    }
    const int W = P.red_waves, wave = threadIdx.x >> 6, e = threadIdx.x & 63;
    const int t = blockIdx.x * (4 / W) + wave / W, ws = wave - (wave / W) * W;
    __shared__ double part[4][64];
    bool live = t < P.n_targets;
    ReduceTarget T{};
    if (live) {
        T = P.targets[t];
        live = !skip_kind(T.dst_kind, vectors_only) && T.c_end - T.c_begin <= kLongTerms;
    }
    // G = 64 / E lane groups of the target's E elements: group g sums terms
    // g, g + G, ... (a 6-vector target keeps 60 lanes busy instead of 6)
    const int E = live ? T.rows * T.cols : 64, G = 64 / E, g = e / E, el = e - g * E;
    const int r = live ? el / T.cols : 0, cc = live ? el % T.cols : 0;
    // a target is a chain of dependent global round trips (term descriptor,
    // then data): sum_terms keeps 16 terms and the next 16 descriptors in flight
    double s = 0.0;
    if (live && g < G) s = sum_terms(P, T.c_begin + ws * G + g, G * W, T.c_end, r, cc);
    if (W > 1) {   // (uniform over the launch: every wave reaches the barrier)
        part[wave][e] = s;
        __syncthreads();
        if (!live || ws != 0 || g != 0) return;
        s = 0.0;
        for (int w = 0; w < W; ++w)
            for (int q = 0; q < G; ++q) s += part[wave + w][q * E + el];
    } else if (G > 1) {
        part[wave][e] = s;
        wsync();
        if (!live || g != 0) return;
        s = 0.0;
        for (int q = 0; q < G; ++q) s += part[wave][q * E + el];
    } else if (!live || g != 0) {   // (G = 1: lanes past the E elements)
        return;
    }
    const bool vec = T.cols == 1;
    target_base(P, T.dst_kind)[T.dst + (vec ? r : r * T.ld + cc)] = s;
}

// Long targets, pass 1: one workgroup per kReduceSeg-term segment, one term
// per thread (every element of the block, <= 36, in registers); the 256
// partial blocks are combined by xor-butterflies and wave order (fixed).
// (one workgroup: segment sg of its long target, partial into lpart[sg];
// FUSED: stored write-through, and the target's last segment to finish adds
// the partials in segment order -- the same sum as reduce_long_kernel)
template <bool FUSED>
__device__ __forceinline__ void reduce_segment(const DevProblem& P, int vectors_only, int sg) {
    const int j = P.lsum.seg[2 * sg], k0 = P.lsum.seg[2 * sg + 1];
    const ReduceTarget T = P.targets[P.lsum.targets[j]];
    if (skip_kind(T.dst_kind, vectors_only)) return;   // (uniform over the workgroup)
    // each wave a quarter of the segment, in G = 64 / E lane groups of the
    // target's E elements (as reduce_kernel); partials added in (wave, group)
    // order, fixed
    const int E = T.rows * T.cols, G = 64 / E;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane / E, el = lane - g * E;
    constexpr int kQ = kReduceSeg / 4;
    const int q0 = k0 + wave * kQ, q1 = min(min(k0 + kReduceSeg, (int)T.c_end), q0 + kQ);
    double s = 0.0;
    if (g < G) s = sum_terms(P, q0 + g, G, q1, el / T.cols, el % T.cols);
    __shared__ double part[4][64];
    __shared__ int last;
    part[wave][lane] = s;
    __syncthreads();
    if ((int)threadIdx.x < E) {
        const int t = threadIdx.x;
        double tot = 0.0;
        for (int w = 0; w < 4; ++w)
            for (int q = 0; q < G; ++q) tot += part[w][q * E + t];
        if (FUSED) st_wt64(P.lsum.part + (size_t)sg * 36 + t, tot);
        else P.lsum.part[(size_t)sg * 36 + t] = tot;
    }
    if (!FUSED) return;
    // the partial is drained before the ticket; the last arriver reads every
    // partial of the target write-through (no fences: the counter form)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int s0 = P.lsum.seg_off[j], s1 = P.lsum.seg_off[j + 1];
    if (threadIdx.x == 0)
        last = __hip_atomic_fetch_add((gu32_t*)(P.lcount + j), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
               (unsigned)(s1 - s0 - 1);
    __syncthreads();
    if (!last) return;
    if ((int)threadIdx.x < E) {
        const int e = threadIdx.x;
        double t = 0.0;
#pragma unroll 8
        for (int q = s0; q < s1; ++q) t += ld_wt64(P.lsum.part + (size_t)q * 36 + e);
        const int r = e / T.cols, cc = e % T.cols;
        target_base(P, T.dst_kind)[T.dst + (T.cols == 1 ? r : r * T.ld + cc)] = t;
    }
    if (threadIdx.x == 0)   // ready for the next launch (stream order)
        __hip_atomic_store((gu32_t*)(P.lcount + j), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void reduce_seg_kernel(DevProblem P, int vectors_only) {
    reduce_segment<false>(P, vectors_only, blockIdx.x);
}

// pass 2 of a long list: segment partials added in segment order; the sum
// terms' total is the target's value, the product terms' (SUBTRACT, never in
// a vectors-only pass) is subtracted from it
template <bool SUBTRACT>
__global__ __launch_bounds__(64) void reduce_long_kernel(DevProblem P, int vectors_only) {
    const LongList& L = SUBTRACT ? P.lprod : P.lsum;
    const int j = blockIdx.x;
    const ReduceTarget T = P.targets[L.targets[j]];
    if (!SUBTRACT && skip_kind(T.dst_kind, vectors_only)) return;
    const int E = T.rows * T.cols, e = threadIdx.x;
    if (e >= E) return;
    double t = 0.0;
#pragma unroll 8
    for (int sg = L.seg_off[j]; sg < L.seg_off[j + 1]; ++sg) t += L.part[(size_t)sg * 36 + e];
    const int r = e / T.cols, cc = e % T.cols;
    double* dst = target_base(P, T.dst_kind) + T.dst + (T.cols == 1 ? r : (int64_t)r * T.ld + cc);
    if (SUBTRACT) *dst -= t;
    else *dst = t;
}

// Product terms of the general points: target element (r, c) -= sum over the
// target's terms (in order) of Z_a[r] . Z_b[c] (3-vectors).  One wave per
// target, one lane per element; runs after reduce_kernel has written the sum
// terms.
// Lists longer than this (the intrinsics arrow and corner collect one term
// per general point) go through preduce_seg_kernel + reduce_long_kernel<true>.
constexpr int kLongPTerms = 64;

// sum over the product terms q = qa + g, qa + g + G, ... < qb of
// Z_a[3r..3r+2] . Z_b[3cc..3cc+2] (ascending, one term after another, as a
// plain per-lane loop would).  The Z blocks are staged through LDS kPtB terms
// at a time: the wave loads each term's two blocks once, coalesced (the rows
// are contiguous 3-vectors), instead of every lane gathering its own six
// doubles per term (36 lanes x 6 scattered 8-byte loads per term made the
// reduce address-bound).  Round 6: in 16-byte pieces -- a term's two blocks
// are ceil(3 ra / 2) + ceil(3 rb / 2) pieces (18 for 6 x 6), the batch's 288
// pieces five wave loads instead of sixteen 8-byte ones -- each piece's two
// doubles put in their padded LDS places.  Rows are padded to 4 doubles in
// LDS (two 16-byte reads per 3-vector).  ra / rb: rows of the a / b block
// (b = w: 1 row).
constexpr int kPtB = 16;   // terms per staged batch of the product-term reduce
constexpr int kPtLds = kPtB * 12 * 4 + 2 * kPtB;   // doubles of LDS per wave (<= 6 + 6 rows per term, the terms)
constexpr int kPtRounds = (kPtB * 18 + 63) / 64;   // a lane's 16-byte pieces per batch
typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));   // (Z blocks are 8-byte aligned)
// ch > 0 (a block target with an even number of columns, round 6): the lane
// also sums element (r, cc + ch) into s1 -- one read of Z_a's row r for two
// elements, and half the lanes per element, so three lane groups share a
// 6 x 6 target's terms instead of one (36 of 64 lanes)
__device__ __forceinline__ double pterm_sum(const DevProblem& P, int qa, int qb, int G, int g, int r, int cc,
                                            int ra, int rb, double* lds, int ch, double& s1) {
    const double* Z = P.Z;
    const int lane = threadIdx.x & 63;
    const int la = 3 * ra, lb = 3 * rb;                          // doubles per a / b block
    const int na2 = (la + 1) >> 1, n2 = na2 + ((lb + 1) >> 1);   // 16-byte pieces per term
    double* La = lds;                          // [kPtB][ra][4]
    double* Lb = lds + kPtB * ra * 4;          // [kPtB][rb][4]
    PTerm* Lt = reinterpret_cast<PTerm*>(lds + kPtB * 12 * 4);   // [kPtB] the batch's terms
    // this lane's pieces (the same in every batch): piece f = lane + 64 q is
    // term f / n2's piece o = f % n2, doubles 2o, 2o + 1 of its a block (o <
    // na2) or of its b block; an odd block's last piece carries one double
    // (its second is read and dropped: Z is allocated two doubles longer)
    int pt[kPtRounds], pe[kPtRounds], d0[kPtRounds], d1[kPtRounds];
#pragma unroll
    for (int q = 0; q < kPtRounds; ++q) {
        const int f = lane + 64 * q, t = f / n2, o = f - t * n2;
        const bool sb = o >= na2;
        const int e = sb ? 2 * (o - na2) : 2 * o, len = sb ? lb : la;
        const int rows = sb ? rb : ra, base = (sb ? kPtB * ra * 4 : 0) + t * rows * 4;
        pt[q] = t < kPtB ? t : kPtB;
        pe[q] = e | (sb ? 256 : 0);
        d0[q] = base + (e / 3) * 4 + e % 3;
        d1[q] = e + 1 < len ? base + ((e + 1) / 3) * 4 + (e + 1) % 3 : -1;
    }
    double s = 0.0;
    s1 = 0.0;
    // software pipeline: batch b + 1's pieces are loaded into registers while
    // batch b is multiplied from LDS, and batch b + 2's term offsets with them
    // (two scalars, not a PTerm: the struct was promoted to LDS, and its
    // store there waited for the load it was meant to prefetch)
    const int2* pt2 = reinterpret_cast<const int2*>(P.pterms);
    int2 nxt = make_int2(0, 0);
    auto load_offs = [&](int q0) {   // batch q0's term offsets -> nxt
        if (lane < min(kPtB, qb - q0)) nxt = pt2[q0 + lane];
    };
    d2u v[kPtRounds];
    auto load_pieces = [&](int nb) {   // the staged batch's (Lt) pieces -> v
        // every piece's load in flight at once (unconditional: pieces past
        // the batch read term 0's first piece)
#pragma unroll
        for (int q = 0; q < kPtRounds; ++q) {
            const bool live = pt[q] < nb;
            const PTerm tm = Lt[live ? pt[q] : 0];
            const int32_t off = live ? ((pe[q] & 256) ? tm.zb : tm.za) + (pe[q] & 255) : tm.za;
            v[q] = *reinterpret_cast<const d2u*>(Z + off);
        }
    };
    if (qa >= qb) return s;
    load_offs(qa);
    int nb = min(kPtB, qb - qa);
    if (lane < nb) Lt[lane] = PTerm{nxt.x, nxt.y};
    load_offs(qa + kPtB);
    wsync();
    load_pieces(nb);
    for (int q0 = qa; q0 < qb; q0 += kPtB) {
        wsync();   // (the previous batch's reads of La / Lb and Lt are done)
#pragma unroll
        for (int q = 0; q < kPtRounds; ++q)
            if (pt[q] < nb) {
                lds[d0[q]] = v[q].x;
                if (d1[q] >= 0) lds[d1[q]] = v[q].y;
            }
        // the next batch: its offsets to Lt, its pieces in flight
        const int q1 = q0 + kPtB, nb1 = min(kPtB, qb - q1);
        if (nb1 > 0 && lane < nb1) Lt[lane] = PTerm{nxt.x, nxt.y};
        if (nb1 > 0) load_offs(q1 + kPtB);
        wsync();
        if (nb1 > 0) load_pieces(nb1);
        if (g >= 0) {
            // this group's terms in the batch: j = g - (q0 - qa) mod G, + G, ...
            int j = (g - (q0 - qa) % G + G) % G;
            for (; j < nb; j += G) {
                const double2 a01 = *reinterpret_cast<const double2*>(La + (j * ra + r) * 4);
                const double a2 = La[(j * ra + r) * 4 + 2];
                const double2 b01 = *reinterpret_cast<const double2*>(Lb + (j * rb + cc) * 4);
                const double b2 = Lb[(j * rb + cc) * 4 + 2];
                s += a01.x * b01.x + a01.y * b01.y + a2 * b2;
                if (ch) {
                    const double2 c01 = *reinterpret_cast<const double2*>(Lb + (j * rb + cc + ch) * 4);
                    const double c2 = Lb[(j * rb + cc + ch) * 4 + 2];
                    s1 += a01.x * c01.x + a01.y * c01.y + a2 * c2;
                }
            }
        }
        nb = nb1;
    }
    wsync();
    return s;
}

// A product-term target's lane layout: E2 lane slots of one element (r, cc)
// -- or two, (r, cc) and (r, cc + ch), when the target has an even number of
// columns -- in G = 64 / E2 lane groups; slot e2 = r * (ch ? ch : cols) + cc.
struct PLanes {
    int E2, G, g, r, cc, ch;
    __device__ __forceinline__ PLanes(const ReduceTarget& T, int lane) {
        const bool vec = T.cols == 1;
        ch = (!vec && (T.cols & 1) == 0) ? T.cols / 2 : 0;
        const int w = ch ? ch : T.cols;
        E2 = T.rows * w;
        G = 64 / E2;
        g = lane / E2;
        const int e2 = lane - g * E2;
        r = e2 / w;
        cc = e2 % w;
        if (g >= G) g = -1;
    }
    // element e (= r * cols + c) of the target: its slot and which sum
    __device__ __forceinline__ int slot(const ReduceTarget& T, int e, bool& second) const {
        const int rr = e / T.cols, c = e % T.cols;
        second = ch && c >= ch;
        return rr * (ch ? ch : T.cols) + (second ? c - ch : c);
    }
};

// One wave per target: its E = rows x cols elements are computed by
// G = 64 / E lane groups, group g summing terms g, g + G, ... (a 6-vector
// target keeps 60 lanes busy, a 6x6 block 36); the group partials are then
// added in group order (fixed, so deterministic).
__global__ __launch_bounds__(256) void preduce_kernel(DevProblem P) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + wave;
    __shared__ double part[4][64];
    ReduceTarget T{};
    bool act = t < P.n_targets;
    if (act) {
        T = P.targets[t];
        act = T.p_end > T.p_begin && T.p_end - T.p_begin <= kLongPTerms;
    }
    if (!act) return;   // whole waves only: the exchange below is wave-local
    __shared__ __attribute__((aligned(16))) double stage[4][kPtLds];
    __shared__ double part1[4][64];
    const PLanes pl(T, lane);
    const int E = T.rows * T.cols;
    const bool vec = T.cols == 1;
    double s1;
    const double s = pterm_sum(P, T.p_begin, T.p_end, pl.G, pl.g, pl.r, pl.cc, T.rows, vec ? 1 : T.cols, stage[wave],
                               pl.ch, s1);
    part[wave][lane] = s;
    part1[wave][lane] = s1;
    wsync();
    if (lane < E) {
        bool second;
        const int e2 = pl.slot(T, lane, second);
        const double* src = second ? part1[wave] : part[wave];
        double tot = 0.0;
        for (int k = 0; k < pl.G; ++k) tot += src[k * pl.E2 + e2];
        const int r = lane / T.cols, cc = lane % T.cols;
        target_base(P, T.dst_kind)[T.dst + (vec ? r : (int64_t)r * T.ld + cc)] -= tot;
    }
}

// Long product-term lists, pass 1: one workgroup per kReduceSeg-term segment,
// each wave a quarter of it, laid out as in preduce_kernel (G lane groups of
// E elements); the partials added in (wave, group) order, fixed.
__global__ __launch_bounds__(256) void preduce_seg_kernel(DevProblem P) {
    const int sg = blockIdx.x;
    const int j = P.lprod.seg[2 * sg], k0 = P.lprod.seg[2 * sg + 1];
    const ReduceTarget T = P.targets[P.lprod.targets[j]];
    const int E = T.rows * T.cols;
    const bool vec = T.cols == 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const PLanes pl(T, lane);
    constexpr int kQ = kReduceSeg / 4;
    const int q0 = k0 + wave * kQ, q1 = min(min(k0 + kReduceSeg, (int)T.p_end), q0 + kQ);
    __shared__ __attribute__((aligned(16))) double stage[4][kPtLds];
    double s1 = 0.0;
    const double s = q0 < q1 ? pterm_sum(P, q0, q1, pl.G, pl.g, pl.r, pl.cc, T.rows, vec ? 1 : T.cols, stage[wave],
                                         pl.ch, s1)
                             : 0.0;
    __shared__ double part[4][64], part1[4][64];
    part[wave][lane] = s;
    part1[wave][lane] = s1;
    __syncthreads();
    if ((int)threadIdx.x < E) {
        const int t = threadIdx.x;
        bool second;
        const int e2 = pl.slot(T, t, second);
        double tot = 0.0;
        for (int w = 0; w < 4; ++w)
            for (int k = 0; k < pl.G; ++k) tot += (second ? part1[w] : part[w])[k * pl.E2 + e2];
        P.lprod.part[(size_t)sg * 36 + t] = tot;
    }
}

// (pass 2: reduce_long_kernel<true>, segment partials added in segment order
// and subtracted from the target)

}  // namespace

void ba_reduce(const DevProblem& P, bool vectors_only, hipStream_t s) {
    if (P.n_targets <= 0 && P.n_zero <= 0) return;
    const int per_block = 4 / P.red_waves, nb = (P.n_targets + per_block - 1) / per_block;
    const bool split = P.red_split != 0;   // SFM_CTX_BA_SPLIT_REDUCE: three launches
    const int nz = (P.n_zero + 15) / 16;   // zero-list workgroups, last in the grid
    if (P.lsum.n > 0 && !split) {
        hipLaunchKernelGGL(reduce_kernel<true>, dim3(nb + P.lsum.n_seg + nz), dim3(256), 0, s, P, vectors_only ? 1 : 0,
                           nb, nb + P.lsum.n_seg);
        SFM_HIP(hipGetLastError());
    } else {
        hipLaunchKernelGGL(reduce_kernel<false>, dim3(nb + nz), dim3(256), 0, s, P, vectors_only ? 1 : 0, nb, nb);
        SFM_HIP(hipGetLastError());
    }
    if (P.lsum.n > 0 && split) {
        hipLaunchKernelGGL(reduce_seg_kernel, dim3(P.lsum.n_seg), dim3(256), 0, s, P, vectors_only ? 1 : 0);
        SFM_HIP(hipGetLastError());
        hipLaunchKernelGGL(reduce_long_kernel<false>, dim3(P.lsum.n), dim3(64), 0, s, P, vectors_only ? 1 : 0);
        SFM_HIP(hipGetLastError());
    }
    // product terms (general points) land on the matrix and rhs targets
    if (P.n_gpt > 0 && !vectors_only) {
        hipLaunchKernelGGL(preduce_kernel, dim3((P.n_targets + 3) / 4), dim3(256), 0, s, P);
        SFM_HIP(hipGetLastError());
        if (P.lprod.n > 0) {
            hipLaunchKernelGGL(preduce_seg_kernel, dim3(P.lprod.n_seg), dim3(256), 0, s, P);
            SFM_HIP(hipGetLastError());
            hipLaunchKernelGGL(reduce_long_kernel<true>, dim3(P.lprod.n), dim3(64), 0, s, P, 0);
            SFM_HIP(hipGetLastError());
        }
    }
}

int reduce_long_threshold() { return kLongTerms; }
int preduce_long_threshold() { return kLongPTerms; }

}  // namespace sfm
