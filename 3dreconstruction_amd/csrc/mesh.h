// The mesh stage (include/sfmcore.h, "Mesh"): what mesh.cpp (host: checks, the
// grid fit, the host twins, the mesh's PLY) and mesh.hip (the kernels and the
// launches) share.
#pragma once
#include <cstdint>
#include <vector>

#include "dense_views.h"
#include "mesh_point.h"

namespace sfm {

// sfm_tsdf_opts.device_bytes == 0
constexpr int64_t kMeshDefaultDeviceBytes = (int64_t)4 << 30;
// the launch grid of the integration kernel: y and z of a HIP grid end at 65535
constexpr int32_t kMeshMaxNy = 65535 * kMeshTileY;
constexpr int32_t kMeshMaxNz = 65535;

static_assert(sizeof(MeshGrid) == sizeof(sfm_mesh_grid), "MeshGrid is sfm_mesh_grid");

// What an integration works on, checked and precomputed on the host (mesh.cpp).
struct MeshProblem {
    DenseImages images;               // sizes, maps, the colour pool's window
    std::vector<MeshView> views;      // [n_img]
    MeshGrid g{};
    int64_t n_vox = 0;
    float trunc = 0.0f;
};
// the mesh's arrays as the caller passes them (rgb may be NULL)
struct MeshOut {
    int64_t cap_vertices, cap_triangles;
    float* V;
    uint8_t* rgb;
    int32_t* tri;
};

inline int64_t mesh_blocks(int64_t n_vox) { return (n_vox + kMeshBlock - 1) / kMeshBlock; }
// mesh.cpp: "the mesh has .. vertices and .. triangles, the caps are ..": SFM_ERR_INVALID_ARG when a cap is too small
void mesh_require_caps(const char* who, const sfm_mesh_stats& st, const MeshOut& out);
// more than 2^31 - 1 vertices: SFM_ERR_UNSUPPORTED
void mesh_require_indexable(const char* who, int64_t n_vertices);

#ifndef SFM_DEPTHMAP_HOST_ONLY
// mesh.hip.  Arguments already checked; seconds[3]: upload, kernels, download.
void tsdf_device(sfm_ctx* ctx, const MeshProblem& P, const float* depth, const uint8_t* pixels, float* tsdf,
                 uint8_t* weight, uint8_t* rgb, uint8_t* has_rgb, int64_t* n_observed, double* seconds);
// When a cap is too small nothing is written, st holds both needs and the call throws.
void mesh_extract_device(sfm_ctx* ctx, const MeshGrid& g, int32_t min_weight, const float* tsdf, const uint8_t* weight,
                         const uint8_t* rgb, const uint8_t* has_rgb, const MeshOut& out, sfm_mesh_stats* st);
// both over one volume that stays on the device; tsdf / weight are downloaded when non-NULL
void mesh_reconstruct_device(sfm_ctx* ctx, const MeshProblem& P, const float* depth, const uint8_t* pixels,
                             int32_t min_weight, const MeshOut& out, float* tsdf, uint8_t* weight,
                             sfm_mesh_reconstruct_stats* st);
#endif

}  // namespace sfm
