// Mesh texturing (include/sfmcore.h, "Mesh texture"): what texture.cpp (host:
// checks, the atlas fit, the host twins, the textured PLY) and texture.hip (the
// kernels and the launches) share.
#pragma once
#include <cstdint>
#include <vector>

#include "dense_views.h"
#include "texture_point.h"

namespace sfm {

// sfm_mesh_texture_opts.device_bytes == 0
constexpr int64_t kTexDefaultDeviceBytes = (int64_t)4 << 30;

// What a call works on, checked and precomputed on the host (texture.cpp).
struct TexProblem {
    DenseImages images;                 // sizes, the colour pool's window
    std::vector<TexView> views;         // [n_img]
    int64_t max_pixels = 0;             // of the largest loaded image
    int64_t n_vertices = 0, n_triangles = 0;
    TexAtlas atlas{};
    uint8_t fill[3] = {0, 0, 0};
};

#ifndef SFM_DEPTHMAP_HOST_ONLY
// texture.hip.  Arguments already checked; seconds[3]: upload, kernels, download.
void tex_face_views_device(sfm_ctx* ctx, const TexProblem& P, const float* V, const int32_t* tri, int32_t* face_view,
                           int32_t* face_pixels, sfm_mesh_face_views_stats* st);
void tex_bake_device(sfm_ctx* ctx, const TexProblem& P, const uint8_t* pixels, const float* V, const uint8_t* vertex_rgb,
                     const int32_t* tri, const int32_t* face_view, uint8_t* texture, float* uv, sfm_mesh_bake_stats* st);
// both with face_view left on the device; face_view / face_pixels are downloaded when non-NULL
void tex_texture_device(sfm_ctx* ctx, const TexProblem& P, const uint8_t* pixels, const float* V, const uint8_t* vertex_rgb,
                        const int32_t* tri, int32_t* face_view, int32_t* face_pixels, uint8_t* texture, float* uv,
                        sfm_mesh_texture_stats* st);
#endif

}  // namespace sfm
