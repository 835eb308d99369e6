// The Schur kernel's batch rule (batch_fits / batch_count, csrc/ba_types.h) on
// the host: for every batch shape the kernels are built with, a walk over a
// chunk never takes a batch above the point or observation cap, takes the
// longest batch that fits, and always advances while every track is within
// the cap; a track one above the cap yields the empty batch the planner's
// max_obs <= schur4_obs test keeps off the 64-row kernel.  No GPU, no library.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../3dreconstruction_amd/csrc/ba_types.h"

using namespace sfm;

static int g_bad = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (++g_bad < 20) std::printf("FAIL line %d: %s\n", __LINE__, #c); \
        }                                                                 \
    } while (0)

// walks a chunk of the given tracks; returns its batches, -1 on a stall
template <class Off>
static long walk(const std::vector<int>& tracks, int sp, int so) {
    const int np = (int)tracks.size();
    std::vector<Off> off(np + 1);
    std::vector<int> ref(np + 1);
    ref[0] = 0;
    for (int p = 0; p < np; ++p) ref[p + 1] = ref[p] + tracks[p];
    for (int p = 0; p <= np; ++p) off[p] = (Off)ref[p];
    CHECK((int)off[np] == ref[np]);   // the offsets fit the type
    long batches = 0;
    for (int p0 = 0; p0 < np;) {
        const int n = batch_count(off.data(), p0, np, sp, so);
        if (n == 0) return -1;
        CHECK(n <= sp && p0 + n <= np);
        CHECK(ref[p0 + n] - ref[p0] <= so);
        // the longest that fits: the next point would break a cap (or there is none)
        CHECK(n == sp || p0 + n == np || ref[p0 + n + 1] - ref[p0] > so);
        for (int j = 0; j < n; ++j) CHECK(batch_fits(off.data(), p0, j, np, sp, so));
        CHECK(!batch_fits(off.data(), p0, n, np, sp, so));
        p0 += n;
        ++batches;
    }
    return batches;
}

int main() {
    struct Shape { int sp, so; };
    std::vector<Shape> shapes;
    for (int cm = 0; cm < 3; ++cm) shapes.push_back({schur4_pts(cm), schur4_obs(cm)});
    shapes.push_back({kSubPts, kSubObs});
    long total = 0;
    for (const Shape& s : shapes) {
        CHECK(s.so <= 64 && s.sp >= 1 && 9 * s.sp <= 64);   // one lane per observation / per-point sum entry
        CHECK(kChunkPts * s.so < 65536);                    // 16-bit chunk offsets
        // uniform tracks of 1 .. cap + 1, chunks of every length up to 2 sp + 1 and a full one
        for (int t = 1; t <= s.so + 1; ++t) {
            for (int np : {1, 2, s.sp - 1, s.sp, s.sp + 1, 2 * s.sp, 2 * s.sp + 1, kChunkPts}) {
                if (np < 1) continue;
                const std::vector<int> tracks(np, t);
                const long b16 = walk<uint16_t>(tracks, s.sp, s.so), b32 = walk<int32_t>(tracks, s.sp, s.so);
                CHECK(b16 == b32);
                if (t > s.so) {
                    CHECK(b32 == -1);   // above the cap: the empty batch
                    continue;
                }
                const int per = s.so / t < s.sp ? s.so / t : s.sp;
                CHECK(b32 == (np + per - 1) / per);
                total += b32;
            }
        }
        // mixed tracks within the cap
        uint64_t st = 0x9E3779B97F4A7C15ull + (uint64_t)s.sp * 64 + s.so;
        for (int rep = 0; rep < 2000; ++rep) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            const int np = 1 + (int)((st >> 33) % kChunkPts), hi = rep % 2 ? s.so : 12;
            std::vector<int> tracks(np);
            for (int& t : tracks) {
                st = st * 6364136223846793005ull + 1442695040888963407ull;
                t = 1 + (int)((st >> 33) % hi);
            }
            const long b16 = walk<uint16_t>(tracks, s.sp, s.so), b32 = walk<int32_t>(tracks, s.sp, s.so);
            CHECK(b32 > 0 && b16 == b32);
            total += b32;
            // one track above the cap somewhere: the walk stops there, not before
            tracks[np / 2] = s.so + 1;
            CHECK(walk<int32_t>(tracks, s.sp, s.so) == -1);
        }
    }
    // the shipped pinhole shape at the bench scene's tracks of 10: 6 points, 60 of 64 lanes
    {
        const std::vector<int> tracks(kChunkPts, 10);
        const int sp = schur4_pts(0), so = schur4_obs(0), per = so / 10 < sp ? so / 10 : sp;
        CHECK(walk<uint16_t>(tracks, sp, so) == (kChunkPts + per - 1) / per);
    }
    std::printf("%ld batches walked, %d bad\n", total, g_bad);
    return g_bad ? 1 : 0;
}
