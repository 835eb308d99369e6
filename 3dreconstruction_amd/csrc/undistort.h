// Dense hand-off, undistortion (include/sfmcore.h, "Dense hand-off"): what
// undistort.cpp (host: checks, the chunk plan, the host twin, the PNM writer)
// and undistort.hip (the kernel and the chunked upload / launch / download)
// share.
#pragma once
#include <cstdint>
#include <vector>

#include "common.h"

namespace sfm {

// The kernel's tile.  A lane produces kUndistortGroup consecutive pixels of
// one row and stores them as whole dwords (1 dword for 1 channel, 3 for 3); a
// wavefront covers kUndistortTileW = 64 * kUndistortGroup pixels of a row, and
// a workgroup is kUndistortTileH wavefronts, one row each.
constexpr int kUndistortGroup = 4;
constexpr int kUndistortTileW = 256;
constexpr int kUndistortTileH = 4;
// Device rows are padded: round_up(w, kUndistortGroup) * channels bytes, rounded
// up to kUndistortPitchAlign, so every lane's dwords are aligned and in the row.
constexpr int kUndistortPitchAlign = 64;
// every segment's rows start at a multiple of this in a chunk's device buffers
constexpr int kUndistortSegmentAlign = 256;
// sfm_undistort_opts.chunk_bytes == 0
constexpr int64_t kUndistortDefaultChunk = (int64_t)128 << 20;

inline int64_t undistort_pitch(int32_t w, int32_t ch) {
    const int64_t b = ((int64_t)w + kUndistortGroup - 1) / kUndistortGroup * kUndistortGroup * ch;
    return (b + kUndistortPitchAlign - 1) / kUndistortPitchAlign * kUndistortPitchAlign;
}
inline int64_t undistort_align_segment(int64_t bytes) {
    return (bytes + kUndistortSegmentAlign - 1) / kUndistortSegmentAlign * kUndistortSegmentAlign;
}

// One launch: the output rows [r0, r1) of an image, which sample the source
// rows [s0, s1) (a whole image: all of both).
struct UndistortSegment {
    int32_t img, r0, r1, s0, s1;
};
// what is resident together; its pitched rows fit the budget
typedef std::vector<UndistortSegment> UndistortChunk;

#ifndef SFM_UNDISTORT_HOST_ONLY
// undistort.hip.  Arguments already checked, SFM_CAM_RADIAL3, chunks not empty.
// Adds the pixels outside and of low weight to *n_outside / *n_low_weight;
// seconds[3]: upload, kernels, download, summed over the chunks.
void undistort_device(sfm_ctx* ctx, const std::vector<UndistortChunk>& chunks, const int32_t* img_intr,
                      const double* intr, const int32_t* wh, const int32_t* channels, const int64_t* img_off,
                      const uint8_t* pixels, const uint8_t* fill, uint8_t* out, int64_t* n_outside,
                      int64_t* n_low_weight, double* seconds);
#endif

}  // namespace sfm
