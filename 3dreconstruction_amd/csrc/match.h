// Exact descriptor matcher (SFM_MATCH_RATIO, SFM_MATCH_MUTUAL): what the
// kernels of match.hip and the plan in match_plan.cpp share -- the row layout
// constants, the kernel arguments and one launch wrapper per kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sfm {

constexpr int kQB = 512;           // queries per workgroup of match_top2_kernel (match.hip: waves x tiles)
constexpr int kRowPad = kQB > 256 ? kQB : 256;  // rows of every image padded to this multiple
constexpr int kF32QB = 256;        // queries per workgroup of match_f32_kernel (one per thread)

// Launch limits; a longer pair list runs in batches.
constexpr int64_t kMaxWorkgroups = 1 << 22;  // match_top2 / match_f32 / casc_match: n_pairs * qblocks
constexpr int64_t kMaxGridPairs = 65535;     // match_mutual (grid.y) and match_digest (grid.x): n_pairs

struct MatchArgs {
    const int8_t* desc;        // padded rows x 128 (int8, a - 128)
    const int32_t* nrm;        // |a'|^2 per padded row
    const int32_t* ntr;        // (|a'|^2 << 8) | (row & 255); INT_MAX for pad rows
    const int64_t* img_row0;   // first padded row of each image
    const int32_t* img_n;      // valid rows per image
    const int32_t* pairs;      // (I, J) per pair of this batch
    int32_t n_pairs;
    int32_t qblocks;           // query blocks per pair (max over the batch)
    int32_t swap;              // 0: queries = J, database = I; 1: queries = I, db = J
    int32_t ratio_test;        // apply d1 < r2*d2 (RATIO mode)
    int32_t kmul;              // -512 (runtime, keeps v_mad_i32_i24)
    float r2;
    int64_t out_stride;        // entries per pair in the outputs
    int32_t* out_idx;          // [n_pairs][out_stride]
    int32_t* out_d;            // [n_pairs][out_stride]
};

struct MatchF32Args {
    const float* desc;         // padded rows x 128 (f32)
    const int64_t* img_row0;
    const int32_t* img_n;
    const int32_t* pairs;
    int32_t n_pairs;
    int32_t qblocks;           // 256-query blocks per pair
    int32_t swap;
    float r2;
    int64_t out_stride;
    int32_t* out_idx;
    int32_t* out_d;            // float bits of the squared distance
};

// u8 -> int8 in place, |a'|^2 and the packed key base of every padded row
// (row_img_start: first padded row of the row's image; row_valid: 0 for pad rows)
void match_prep(uint8_t* desc, int32_t* nrm, int32_t* ntr, const int64_t* row_img_start,
                const int32_t* row_valid, int64_t n_rows, hipStream_t s);
// a.n_pairs * a.qblocks workgroups; ratio: nearest + ratio test, else nearest only
void match_top2(const MatchArgs& a, bool ratio, hipStream_t s);
void match_f32(const MatchF32Args& a, bool ratio, hipStream_t s);
// MUTUAL: keep (q, t) iff idx_q[q] = t and idx_t[t] = q; q over the rows of I (at most max_n)
void match_mutual(int32_t* idx_q, int32_t* d_q, const int32_t* idx_t, const int32_t* pairs,
                  const int32_t* img_n, int n_pairs, int max_n, int64_t stride, hipStream_t s);
// adds the digest of pairs [pair_base, pair_base + n_pairs) to out[0] and their match count to out[1]
void match_digest(const int32_t* idx, const int32_t* d, const int32_t* pairs, const int32_t* img_n,
                  int mode, int64_t pair_base, int n_pairs, int64_t stride, unsigned long long* out,
                  hipStream_t s);

}  // namespace sfm
