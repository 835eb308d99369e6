// Track colouring (include/sfmcore.h, "Track colouring"): what colorize.cpp
// (host: checks, the serial host twin, the sampling, the PLY writer) and
// colorize.hip (the assignment kernels) share.
#pragma once
#include <cstdint>

#include "common.h"
#include "recon.h"

namespace sfm {

// The device runs rounds in batches of kColorizeBatch (a pick and a colour
// launch each) and reads one word, the points left to colour, after each batch;
// a round after the last one does nothing, so a batch may overrun the end.
constexpr int kColorizeBatch = 32;
// the pick kernel: one workgroup of this many lanes reduces count[0 .. n_img)
constexpr int kColorizePickThreads = 256;
// the setup kernel (a lane per point) and the colour kernel (a lane per
// observation of the chosen image's list): lanes per workgroup
constexpr int kColorizeThreads = 256;

// The pixel under an observation: clamped in double, then truncated, as
// image(pt.y(), pt.x()) reads it.  One definition for the host twin and the kernel.
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int32_t colorize_pixel(double x, int32_t size) {
    const double hi = (double)(size - 1);
    return (int32_t)(x < 0.0 ? 0.0 : (x > hi ? hi : x));
}

#ifndef SFM_COLORIZE_HOST_ONLY
// colorize.hip.  Arguments already checked; n_obs > 0.  view / obs / px /
// order are the caller's host arrays; seconds[3]: index upload and setup,
// rounds, download.
void colorize_device_assign(sfm_ctx* ctx, int32_t n_img, int32_t n_pt, int32_t n_obs, const ReconIndex& ix,
                            const int32_t* obs_img, const double* obs_uv, const int32_t* wh, const uint8_t* pt_ok,
                            const uint8_t* keep_obs, int32_t* view, int64_t* obs, int32_t* px, int32_t* order,
                            int32_t* n_rounds, int64_t* n_to_colour, int64_t* n_coloured, double* seconds);
#endif

// The one PLY writer (cloud_and_poses.ply and colorized.ply): ASCII, double
// x y z + uchar red green blue, the points with pt_ok (NULL: all) ascending in
// rgb's colour (NULL: white), then the centres of the registered (NULL: all)
// cameras in green.  Throws SfmError.
void write_ply(const char* who, const char* path, int64_t n_pt, const double* X, const uint8_t* pt_ok,
               const uint8_t* rgb, int32_t n_img, const double* extr, const uint8_t* registered);

}  // namespace sfm
