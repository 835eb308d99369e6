// The images of a dense call as the C-ABI passes them (wh, channels, img_off,
// pixels, K, R, C), checked in one place for the depth maps, the fusion, the mesh
// and the texture (dense_views.cpp), and the thread pool of their host twins.
#pragma once
#include <cstdint>
#include <functional>
#include <vector>

#include "common.h"

namespace sfm {

struct DenseImage {
    int32_t w, h, loaded, channels;   // loaded: no pixels, or img_off >= 0; channels: 0 unless its pixels are used
    int64_t map_off, pix_off;         // pixels of the images before it; bytes into the colour pool from pool_lo
};
struct DenseImages {
    int32_t n_img = 0;
    std::vector<DenseImage> img;        // [n_img]
    int64_t n_map = 0;                  // pixels of all images
    int64_t pool_lo = 0, pool_hi = 0;   // the bytes of the colour pool that loaded images cover: uploaded from pool_lo on
};

// Per image, in index order: a positive size, fewer than 2^31 pixels (SFM_ERR_UNSUPPORTED; the others are
// SFM_ERR_INVALID_ARG), a finite K, R and C, 1 or 3 channels where its pixels are used, then also(i): a stage's
// further checks of image i, before image i + 1's.  pixels only with channels and img_off: the caller checks that.
void dense_images_prepare(const char* who, int32_t n_img, const int32_t* wh, const int32_t* channels,
                          const int64_t* img_off, const uint8_t* pixels, const double* K, const double* R, const double* C,
                          DenseImages& D, const std::function<void(int32_t)>& also = nullptr);
// M[9] = K R of image i, worked out in double and rounded once
void dense_KR(const double* K, const double* R, int32_t i, float* M);
// C of image i, rounded
void dense_C(const double* C, int32_t i, float* c);

// fn(item) for every item in [0, n), on up to 16 threads; returns when all are done
void dense_parallel_for(size_t n, const std::function<void(size_t)>& fn);

}  // namespace sfm
