// The binary little-endian PLY files of the dense stages (the cloud, the mesh,
// the textured mesh): one writer, and the check of a mesh's triangle indices.
#pragma once
#include <cstdint>
#include <cstdio>
#include <functional>
#include <string>

#include "common.h"

namespace sfm {

// Opens path and writes "ply", the format line, `elements` (element and property lines, each ended by a line
// break) and "end_header".  A file that cannot be opened or, in close(), written is SFM_ERR_INVALID_ARG.
struct PlyWriter {
    PlyWriter(const char* who, const char* path, const std::string& elements);
    ~PlyWriter();
    // n records of rec_bytes each; fill(k, p) writes record k at p.  Staged 4096 records at a time.
    void records(int64_t n, size_t rec_bytes, const std::function<void(int64_t, uint8_t*)>& fill);
    void close();
    const char *who_, *path_;
    std::FILE* f_;
};

// every index of tri[3 n_triangles] names one of n_vertices vertices, or SFM_ERR_INVALID_ARG
void require_triangles(const char* who, int64_t n_triangles, const int32_t* tri, int64_t n_vertices);

}  // namespace sfm
