// The match plan (sfm_match_plan_*, sfm_match_dense*): a descriptor collection
// resident in HBM and the pair lists run over it with the kernels of match.hip
// (exact RATIO / MUTUAL) and cascade.hip (CASCADE).
//   * layout: every image's rows are padded to a multiple of kRowPad and the
//     collection ends in kRowPad guard rows, so a kernel tile may read past an
//     image's last row.  uint8 rows become int8 a - 128 with |a'|^2 and the
//     packed key base per row (match_prep); float rows that are integers in
//     [0, 255] are converted and take that path, other float rows stay f32.
//   * a run writes (idx, d) per query into [n_pairs][stride] outputs that only
//     grow, in launch batches of the pair list (kMaxWorkgroups, kMaxGridPairs);
//     they leave as sorted (i, j, d) lists or as an order-independent digest.
#include <algorithm>
#include <array>
#include <cstring>
#include <type_traits>
#include <vector>

#include "cascade.h"
#include "common.h"
#include "match.h"

using namespace sfm;

struct sfm_match_plan {
    sfm_ctx* ctx = nullptr;
    int32_t n_img = 0;
    std::vector<int64_t> row0;   // padded row start per image
    std::vector<int32_t> nrows;
    int32_t max_n = 0;
    int64_t rows = 0;            // padded rows in total
    DBuf<uint8_t> desc;
    DBuf<float> descf;           // f32 collection that is not integer-valued (match_f32_kernel)
    bool f32 = false;
    DBuf<int32_t> nrm, ntr, img_n;
    DBuf<int64_t> img_row0;
    // last run
    int32_t mode = 0;
    int64_t n_pairs = 0, stride = 0;
    std::vector<int32_t> pairs_h;
    DBuf<int32_t> pairs_d, out_idx, out_d, tmp_idx, tmp_d;
    DBuf<unsigned long long> digest;
    // cascade hashing tables, built by the first CASCADE run and rebuilt when
    // the set of images in the pair list (the zero-mean input) changes
    std::vector<int32_t> casc_used;
    bool casc_ready = false;
    bool casc_pinned = false;    // set by sfm_match_plan_cascade_index
    DBuf<float> casc_proj, casc_zm;
    DBuf<int64_t> casc_colsum;
    DBuf<uint32_t> casc_code;
    DBuf<uint64_t> casc_bkt;
    DBuf<int32_t> casc_boff, casc_blist, casc_img;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int64_t launches = 0;
};

namespace {

int64_t padded(int64_t n) { return (n + kRowPad - 1) / kRowPad * kRowPad; }

// The row layout of a collection whose image i has off[i + 1] - off[i] rows.
void layout_rows(sfm_match_plan* p, const int64_t* off, int32_t n_img) {
    p->n_img = n_img;
    p->row0.resize(n_img);
    p->nrows.resize(n_img);
    int64_t rows = 0;
    for (int i = 0; i < n_img; ++i) {
        const int64_t n = off[i + 1] - off[i];
        SFM_REQUIRE(n >= 0 && n < (1 << 24), SFM_ERR_INVALID_ARG, "image %d has %lld rows", i,
                    (long long)n);
        p->row0[i] = rows;
        p->nrows[i] = (int32_t)n;
        p->max_n = std::max<int32_t>(p->max_n, (int32_t)n);
        rows += padded(n);
    }
    p->rows = rows + kRowPad;  // guard rows for tile over-reads
}

// ... and its device copy (queued after the descriptor rows)
void upload_layout(sfm_match_plan* p) {
    hipStream_t s = p->ctx->stream;
    p->img_n.alloc(p->n_img);
    p->img_n.upload(p->nrows.data(), p->n_img, s);
    p->img_row0.alloc(p->n_img);
    p->img_row0.upload(p->row0.data(), p->n_img, s);
}

// image i's rows (srcs, optional: they start at srcs[i] instead of desc + 128 off[i])
template <class T>
const T* image_rows(const T* desc, const int64_t* off, const T* const* srcs, int i) {
    return srcs ? srcs[i] : desc + off[i] * 128;
}

// the descriptor rows in the plan's layout, pad rows = fill, in page-locked
// staging from the context's host cache (a pageable source made each upload
// of a 300-image loop's collection cost milliseconds)
template <class T>
HostVec<T> stage_rows(const sfm_match_plan* p, const T* desc, const int64_t* off, const T* const* srcs,
                      T fill) {
    HostVec<T> staging((size_t)p->rows * 128, fill);
    for (int i = 0; i < p->n_img; ++i)
        if (p->nrows[i])
            std::memcpy(&staging[(size_t)p->row0[i] * 128], image_rows(desc, off, srcs, i),
                        (size_t)p->nrows[i] * 128 * sizeof(T));
    return staging;
}

void upload_collection(sfm_match_plan* p, const uint8_t* desc, const int64_t* off, int32_t n_img,
                       const uint8_t* const* srcs = nullptr) {
    hipStream_t s = p->ctx->stream;
    layout_rows(p, off, n_img);
    const int64_t rows = p->rows;
    PhaseTimer tm("upload_collection");
    if (PhaseTimer::on()) {   // diagnostic: is anything still queued before this call?
        SFM_HIP(hipStreamSynchronize(s));
        tm.mark("presync");
    }
    const HostVec<uint8_t> staging = stage_rows<uint8_t>(p, desc, off, srcs, 128);  // pad rows -> a' = 0
    HostVec<int64_t> rstart(rows, 0);
    HostVec<int32_t> rvalid(rows, 0);
    for (int i = 0; i < n_img; ++i)
        for (int64_t r = 0, n = padded(p->nrows[i]); r < n; ++r) {
            rstart[p->row0[i] + r] = p->row0[i];
            rvalid[p->row0[i] + r] = r < p->nrows[i];
        }
    tm.mark("stage");
    p->desc.alloc(staging.size());
    tm.mark("alloc");
    p->desc.upload(staging.data(), staging.size(), s);
    if (PhaseTimer::on()) SFM_HIP(hipStreamSynchronize(s));
    tm.mark("copy");
    DBuf<int64_t> rs;
    DBuf<int32_t> rv;
    rs.alloc(rows);
    rv.alloc(rows);
    rs.upload(rstart.data(), rows, s);
    rv.upload(rvalid.data(), rows, s);
    p->nrm.alloc(rows);
    p->ntr.alloc(rows);
    match_prep(p->desc.p, p->nrm.p, p->ntr.p, rs.p, rv.p, rows, s);
    upload_layout(p);
    tm.mark("rest");
    SFM_HIP(hipStreamSynchronize(s));  // staging buffers die here
    tm.mark("sync");
}

// float descriptors: integers in [0, 255] (what cv::SIFT stores) are
// converted exactly and take the u8 path; anything else is kept as f32
bool f32_is_u8(const float* d, int64_t n) {
    for (int64_t k = 0; k < n; ++k) {
        const float v = d[k];
        if (!(v >= 0.f && v <= 255.f) || v != (float)(int)v) return false;
    }
    return true;
}

void upload_collection(sfm_match_plan* p, const float* desc, const int64_t* off, int32_t n_img,
                       const float* const* srcs = nullptr) {
    bool u8 = true;
    for (int i = 0; i < n_img && u8; ++i)
        u8 = f32_is_u8(image_rows(desc, off, srcs, i), (off[i + 1] - off[i]) * 128);
    if (u8) {
        std::vector<uint8_t> b((size_t)std::max<int64_t>(off[n_img] - off[0], 0) * 128);
        for (int i = 0; i < n_img; ++i) {
            const float* src = image_rows(desc, off, srcs, i);
            uint8_t* dst = b.data() + (off[i] - off[0]) * 128;
            for (int64_t k = 0; k < (off[i + 1] - off[i]) * 128; ++k) dst[k] = (uint8_t)src[k];
        }
        std::vector<int64_t> o(off, off + n_img + 1);
        for (auto& v : o) v -= off[0];
        upload_collection(p, b.data(), o.data(), n_img);
        return;
    }
    p->f32 = true;
    layout_rows(p, off, n_img);
    const HostVec<float> staging = stage_rows<float>(p, desc, off, srcs, 0.f);
    p->descf.alloc(staging.size());
    p->descf.upload(staging.data(), staging.size(), p->ctx->stream);
    upload_layout(p);
    SFM_HIP(hipStreamSynchronize(p->ctx->stream));  // staging dies here
}

// (the kernel arguments below are brace-initialised: the values stand in the
// field order of the structs in cascade.h and match.h)
CascTables casc_tables(sfm_match_plan* p) {
    return {reinterpret_cast<const int8_t*>(p->desc.p), p->nrm.p, p->img_row0.p, p->img_n.p, p->rows,
            p->casc_code.p, p->casc_bkt.p, p->casc_boff.p, p->casc_blist.p};
}

void check_pairs(const sfm_match_plan* p, const int32_t* pairs, int64_t n_pairs, bool cascade) {
    for (int64_t q = 0; q < 2 * n_pairs; ++q)
        SFM_REQUIRE(pairs[q] >= 0 && pairs[q] < p->n_img, SFM_ERR_INVALID_ARG, "pair %lld out of range",
                    (long long)(q / 2));
    SFM_REQUIRE(!(p->f32 && cascade), SFM_ERR_UNSUPPORTED,
                "cascade hashing needs integer descriptors in [0, 255] (this f32 collection is not)");
}

// Hash tables for the images of this pair list (zero-mean over exactly those
// images, as Cascade_Hashing_Matcher_Regions' used_index).
void casc_prepare(sfm_match_plan* p, const int32_t* pairs, int64_t n_pairs, bool pin) {
    hipStream_t s = p->ctx->stream;
    std::vector<char> seen(p->n_img, 0);
    for (int64_t q = 0; q < 2 * n_pairs; ++q) seen[pairs[q]] = 1;
    std::vector<int32_t> used;
    for (int i = 0; i < p->n_img; ++i)
        if (seen[i]) used.push_back(i);
    if (p->casc_ready) {
        if (used == p->casc_used) {
            p->casc_pinned = p->casc_pinned || pin;
            return;
        }
        if (!pin && p->casc_pinned &&
            std::includes(p->casc_used.begin(), p->casc_used.end(), used.begin(), used.end()))
            return;   // a part of the indexed list
    }
    p->casc_pinned = pin;
    SFM_REQUIRE(p->max_n < (1 << 21), SFM_ERR_UNSUPPORTED,
                "cascade hashing: %d descriptors in one image (limit 2^21)", p->max_n);
    CascTables t = casc_tables(p);
    if (!p->casc_proj.p) {
        std::vector<float> proj;
        casc_projections(proj);
        p->casc_proj.alloc(proj.size());
        p->casc_proj.upload(proj.data(), proj.size(), s);
        p->casc_zm.alloc(kCascCode);
        p->casc_colsum.alloc((size_t)std::max(1, p->n_img) * kCascCode);
        p->casc_code.alloc((size_t)p->rows * 4);
        p->casc_bkt.alloc((size_t)p->rows);
        p->casc_boff.alloc((size_t)std::max(1, p->n_img) * kCascGroups * (kCascBuckets + 1));
        p->casc_blist.alloc((size_t)p->rows * kCascGroups);
        p->casc_img.alloc(std::max(1, p->n_img));
        t = casc_tables(p);
        casc_colsum(t, p->n_img, p->casc_colsum.p, s);
    }
    std::vector<int64_t> colsum((size_t)p->n_img * kCascCode);
    if (p->n_img)
        SFM_HIP(hipMemcpyAsync(colsum.data(), p->casc_colsum.p, colsum.size() * 8,
                               hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    float zm[kCascCode];
    casc_zero_mean(colsum.data(), p->nrows.data(), used, zm);
    p->casc_zm.upload(zm, kCascCode, s);
    if (!used.empty()) p->casc_img.upload(used.data(), used.size(), s);
    casc_hash(t, p->casc_proj.p, p->casc_zm.p, p->casc_img.p, (int)used.size(), p->max_n, s);
    SFM_HIP(hipStreamSynchronize(s));   // host zm / image list die here
    p->casc_used = std::move(used);
    p->casc_ready = true;
}

// fn(b0, nb) for every batch [b0, b0 + nb) of at most `batch` of n_pairs pairs
template <class F>
void for_batches(int64_t n_pairs, int64_t batch, F&& fn) {
    for (int64_t b0 = 0; b0 < n_pairs; b0 += batch) fn(b0, std::min(batch, n_pairs - b0));
}

// A launch batch of a nearest-neighbour kernel: its pairs, its part of the outputs.
struct NnBatch {
    const int32_t* pairs;
    int32_t n, qblocks;
    int32_t *out_idx, *out_d;
};

// A nearest-neighbour kernel with `qb` queries per workgroup over the last run's pair list.
template <class F>
void run_nn(sfm_match_plan* p, int qb, int32_t* out_idx, int32_t* out_d, F&& launch) {
    const int qblocks = std::max(1, (p->max_n + qb - 1) / qb);
    for_batches(p->n_pairs, std::max<int64_t>(1, kMaxWorkgroups / qblocks), [&](int64_t b0, int64_t nb) {
        const int64_t o = b0 * p->stride;
        launch(NnBatch{p->pairs_d.p + 2 * b0, (int32_t)nb, qblocks, out_idx + o, out_d + o});
        ++p->launches;
    });
}

// The exact top-2 (ratio_test) or nearest-only kernel; swap: queries = I, database = J.
void run_top2(sfm_match_plan* p, int swap, int ratio_test, float r2, int32_t* out_idx, int32_t* out_d) {
    hipStream_t s = p->ctx->stream;
    if (p->f32)
        run_nn(p, kF32QB, out_idx, out_d, [&](const NnBatch& b) {
            match_f32({p->descf.p, p->img_row0.p, p->img_n.p, b.pairs, b.n, b.qblocks, swap, r2, p->stride,
                       b.out_idx, b.out_d}, ratio_test, s);
        });
    else
        run_nn(p, kQB, out_idx, out_d, [&](const NnBatch& b) {
            match_top2({reinterpret_cast<const int8_t*>(p->desc.p), p->nrm.p, p->ntr.p, p->img_row0.p, p->img_n.p,
                        b.pairs, b.n, b.qblocks, swap, ratio_test, /*kmul*/ -512, r2, p->stride, b.out_idx, b.out_d},
                       ratio_test, s);
        });
}

void run_pairs(sfm_match_plan* p, const int32_t* pairs, int64_t n_pairs, const sfm_match_options* o,
               bool timed = true) {
    hipStream_t s = p->ctx->stream;
    SFM_REQUIRE(o && (o->mode == SFM_MATCH_RATIO || o->mode == SFM_MATCH_MUTUAL ||
                      o->mode == SFM_MATCH_CASCADE),
                SFM_ERR_INVALID_ARG, "bad match options");
    check_pairs(p, pairs, n_pairs, o->mode == SFM_MATCH_CASCADE);
    if (o->mode == SFM_MATCH_CASCADE) casc_prepare(p, pairs, n_pairs, false);
    p->mode = o->mode;
    p->n_pairs = n_pairs;
    p->stride = std::max<int64_t>(1, p->max_n);
    p->pairs_h.assign(pairs, pairs + 2 * n_pairs);
    if ((int64_t)p->pairs_d.n < 2 * n_pairs) p->pairs_d.alloc(std::max<int64_t>(2, 2 * n_pairs));
    p->pairs_d.upload(pairs, 2 * n_pairs, s);
    const size_t need = (size_t)std::max<int64_t>(1, n_pairs * p->stride);
    if (p->out_idx.n < need) { p->out_idx.alloc(need); p->out_d.alloc(need); }
    p->launches = 0;
    if (timed && !p->ev0) { SFM_HIP(hipEventCreate(&p->ev0)); SFM_HIP(hipEventCreate(&p->ev1)); }
    if (timed) SFM_HIP(hipEventRecord(p->ev0, s));
    const float r2 = o->ratio * o->ratio;
    if (o->mode == SFM_MATCH_CASCADE) {
        run_nn(p, kCascQB, p->out_idx.p, p->out_d.p, [&](const NnBatch& b) {
            casc_match({casc_tables(p), b.pairs, b.n, b.qblocks, r2, p->stride, b.out_idx, b.out_d}, p->max_n, s);
        });
    } else if (o->mode == SFM_MATCH_RATIO) {
        run_top2(p, 0, 1, r2, p->out_idx.p, p->out_d.p);
    } else if (n_pairs > 0) {
        if (p->tmp_idx.n < need) { p->tmp_idx.alloc(need); p->tmp_d.alloc(need); }
        // nn over J for every row of I, and nn over I for every row of J
        run_top2(p, 1, 0, 0.f, p->out_idx.p, p->out_d.p);
        run_top2(p, 0, 0, 0.f, p->tmp_idx.p, p->tmp_d.p);
        for_batches(p->n_pairs, kMaxGridPairs, [&](int64_t b0, int64_t nb) {
            match_mutual(p->out_idx.p + b0 * p->stride, p->out_d.p + b0 * p->stride,
                         p->tmp_idx.p + b0 * p->stride, p->pairs_d.p + 2 * b0, p->img_n.p, (int)nb,
                         p->max_n, p->stride, s);
            ++p->launches;
        });
    }
    if (timed) SFM_HIP(hipEventRecord(p->ev1, s));
}

// {digest, match count} of the last run
std::array<unsigned long long, 2> run_digest(sfm_match_plan* p) {
    hipStream_t s = p->ctx->stream;
    if (!p->digest.p) p->digest.alloc(2);
    p->digest.zero(s);
    for_batches(p->n_pairs, kMaxGridPairs, [&](int64_t b0, int64_t nb) {
        match_digest(p->out_idx.p + b0 * p->stride, p->out_d.p + b0 * p->stride, p->pairs_d.p + 2 * b0,
                     p->img_n.p, p->mode, b0, (int)nb, p->stride, p->digest.p, s);
    });
    std::array<unsigned long long, 2> h;
    SFM_HIP(hipMemcpyAsync(h.data(), p->digest.p, sizeof h, hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    return h;
}

// A stored distance as a float: the f32 kernel's float bits, or the exact integer.
float distance_f32(const sfm_match_plan* p, int32_t bits) {
    float f = (float)bits;
    if (p->f32) std::memcpy(&f, &bits, 4);
    return f;
}

// D = int32_t: exact integer squared distances (u8 collections); D = float:
// float squared distances (any collection; integers convert exactly)
template <class D>
void fetch_results(sfm_match_plan* p, int64_t* counts, uint32_t* i, uint32_t* j, D* d2) {
    const size_t n = (size_t)(p->n_pairs * p->stride);
    std::vector<int32_t> hi(n), hd(n);
    if (n) {
        SFM_HIP(hipMemcpyAsync(hi.data(), p->out_idx.p, n * 4, hipMemcpyDeviceToHost, p->ctx->stream));
        SFM_HIP(hipMemcpyAsync(hd.data(), p->out_d.p, n * 4, hipMemcpyDeviceToHost, p->ctx->stream));
    }
    SFM_HIP(hipStreamSynchronize(p->ctx->stream));
    int64_t off = 0;
    std::vector<std::pair<uint64_t, int32_t>> v;
    for (int64_t q = 0; q < p->n_pairs; ++q) {
        const int I = p->pairs_h[2 * q], J = p->pairs_h[2 * q + 1];
        const bool qJ = p->mode != SFM_MATCH_MUTUAL;
        const int n_out = qJ ? p->nrows[J] : p->nrows[I];
        v.clear();
        for (int t = 0; t < n_out; ++t) {
            const int m = hi[(size_t)q * p->stride + t];
            if (m < 0) continue;
            const uint32_t ii = qJ ? (uint32_t)m : (uint32_t)t;
            const uint32_t jj = qJ ? (uint32_t)t : (uint32_t)m;
            v.emplace_back(((uint64_t)ii << 32) | jj, hd[(size_t)q * p->stride + t]);
        }
        std::sort(v.begin(), v.end());  // IndMatch::getDeduplicated order
        counts[q] = (int64_t)v.size();
        if (i) {
            for (const auto& m : v) {
                i[off] = (uint32_t)(m.first >> 32);
                j[off] = (uint32_t)(m.first & 0xffffffffu);
                if constexpr (std::is_same<D, float>::value) d2[off] = distance_f32(p, m.second);
                else d2[off] = m.second;
                ++off;
            }
        }
    }
}

template <class D>
int plan_fetch(sfm_match_plan* p, int64_t* counts, uint32_t* i, uint32_t* j, D* d2) {
    return guarded([&] {
        SFM_REQUIRE(p && counts, SFM_ERR_INVALID_ARG, "null argument");
        SFM_REQUIRE((std::is_same<D, float>::value || !p->f32), SFM_ERR_INVALID_ARG,
                    "float distances: this collection is not integer-valued (sfm_match_plan_fetch_f32)");
        CtxScope scope_(p->ctx);
        fetch_results(p, counts, i, j, d2);
        return SFM_OK;
    });
}

template <class T>
int plan_create(sfm_ctx* ctx, const T* desc, const int64_t* offsets, int32_t n_img, sfm_match_plan** out) {
    return guarded([&] {
        SFM_REQUIRE(ctx && out && offsets && n_img >= 0, SFM_ERR_INVALID_ARG, "null argument");
        SFM_REQUIRE(desc || offsets[n_img] == (std::is_same<T, float>::value ? offsets[0] : 0),
                    SFM_ERR_INVALID_ARG, "null descriptors");
        CtxScope scope_(ctx);
        auto* p = new sfm_match_plan;
        p->ctx = ctx;
        try {
            upload_collection(p, desc, offsets, n_img);
        } catch (...) {
            delete p;
            throw;
        }
        *out = p;
        return SFM_OK;
    });
}

// One pair through a plan on the stack.  D = int32_t: the distances are
// downloaded as they are; D = float: decoded on the host.
template <class T, class D>
int match_dense(sfm_ctx* ctx, const T* a, int32_t n_a, const T* b, int32_t n_b, const sfm_match_options* o,
                int32_t* match_idx, D* match_d2) {
    return guarded([&] {
        SFM_REQUIRE(ctx && o && match_idx && match_d2 && n_a >= 0 && n_b >= 0 &&
                        (a || n_a == 0) && (b || n_b == 0),
                    SFM_ERR_INVALID_ARG, "bad arguments");
        CtxScope scope_(ctx);
        PhaseTimer tm("sfm_match_dense");
        const int64_t off[3] = {0, n_a, (int64_t)n_a + n_b};
        const T* srcs[2] = {a, b};
        sfm_match_plan plan;
        plan.ctx = ctx;
        tm.mark("stage");
        upload_collection(&plan, (const T*)nullptr, off, 2, srcs);
        tm.mark("upload");
        const int32_t pair[2] = {0, 1};
        run_pairs(&plan, pair, 1, o, false);
        tm.mark("launch");
        const int32_t n_out = o->mode != SFM_MATCH_MUTUAL ? n_b : n_a;
        constexpr bool decode = std::is_same<D, float>::value;
        std::vector<int32_t> bits(decode ? std::max(n_out, 1) : 0);
        void* d_dst = decode ? (void*)bits.data() : (void*)match_d2;
        if (n_out) {
            SFM_HIP(hipMemcpyAsync(match_idx, plan.out_idx.p, (size_t)n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
            SFM_HIP(hipMemcpyAsync(d_dst, plan.out_d.p, (size_t)n_out * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        SFM_HIP(hipStreamSynchronize(ctx->stream));
        tm.mark("sync+download");
        if constexpr (decode)
            for (int32_t q = 0; q < n_out; ++q)
                match_d2[q] = match_idx[q] < 0 ? -1.f : distance_f32(&plan, bits[q]);
        return SFM_OK;
    });
}

}  // namespace

extern "C" int sfm_match_plan_create(sfm_ctx* ctx, const uint8_t* desc, const int64_t* offsets,
                                     int32_t n_img, sfm_match_plan** out) {
    return plan_create(ctx, desc, offsets, n_img, out);
}

extern "C" int sfm_match_plan_create_f32(sfm_ctx* ctx, const float* desc, const int64_t* offsets,
                                         int32_t n_img, sfm_match_plan** out) {
    return plan_create(ctx, desc, offsets, n_img, out);
}

extern "C" int sfm_match_plan_run(sfm_match_plan* p, const int32_t* pairs, int64_t n_pairs,
                                  const sfm_match_options* o, int64_t* total) {
    return guarded([&] {
        SFM_REQUIRE(p && (pairs || n_pairs == 0) && n_pairs >= 0, SFM_ERR_INVALID_ARG,
                    "bad arguments");
        CtxScope scope_(p->ctx);
        run_pairs(p, pairs, n_pairs, o);
        if (total) *total = (int64_t)run_digest(p)[1];
        return SFM_OK;
    });
}

extern "C" int sfm_match_plan_cascade_index(sfm_match_plan* p, const int32_t* pairs, int64_t n_pairs) {
    return guarded([&] {
        SFM_REQUIRE(p && (pairs || n_pairs == 0) && n_pairs >= 0, SFM_ERR_INVALID_ARG,
                    "bad arguments");
        check_pairs(p, pairs, n_pairs, true);
        CtxScope scope_(p->ctx);
        casc_prepare(p, pairs, n_pairs, true);
        return SFM_OK;
    });
}

extern "C" int sfm_match_plan_digest(sfm_match_plan* p, uint64_t* digest) {
    return guarded([&] {
        SFM_REQUIRE(p && digest, SFM_ERR_INVALID_ARG, "null argument");
        CtxScope scope_(p->ctx);
        *digest = run_digest(p)[0];
        return SFM_OK;
    });
}

extern "C" int sfm_match_plan_fetch(sfm_match_plan* p, int64_t* counts, uint32_t* i, uint32_t* j,
                                    int32_t* d2) {
    return plan_fetch(p, counts, i, j, d2);
}

extern "C" int sfm_match_plan_fetch_f32(sfm_match_plan* p, int64_t* counts, uint32_t* i, uint32_t* j,
                                        float* d2) {
    return plan_fetch(p, counts, i, j, d2);
}

extern "C" int sfm_match_plan_get_last_ms(sfm_match_plan* p, double* ms, int64_t* launches) {
    return guarded([&] {
        SFM_REQUIRE(p && ms, SFM_ERR_INVALID_ARG, "null argument");
        float f = 0.f;
        if (p->ev0) {
            SFM_HIP(hipEventSynchronize(p->ev1));
            SFM_HIP(hipEventElapsedTime(&f, p->ev0, p->ev1));
        }
        *ms = f;
        if (launches) *launches = p->launches;
        return SFM_OK;
    });
}

extern "C" int sfm_match_plan_destroy(sfm_match_plan* p) {
    return guarded([&] {
        if (!p) return SFM_OK;
        CtxScope scope_(p->ctx);
        (void)hipStreamSynchronize(p->ctx->stream);
        if (p->ev0) { (void)hipEventDestroy(p->ev0); (void)hipEventDestroy(p->ev1); }
        delete p;
        return SFM_OK;
    });
}

extern "C" int sfm_match_dense(sfm_ctx* ctx, const uint8_t* a, int32_t n_a, const uint8_t* b,
                               int32_t n_b, const sfm_match_options* o, int32_t* match_idx,
                               int32_t* match_d2) {
    return match_dense(ctx, a, n_a, b, n_b, o, match_idx, match_d2);
}

extern "C" int sfm_match_dense_f32(sfm_ctx* ctx, const float* a, int32_t n_a, const float* b, int32_t n_b,
                                   const sfm_match_options* o, int32_t* match_idx, float* match_d2) {
    return match_dense(ctx, a, n_a, b, n_b, o, match_idx, match_d2);
}
