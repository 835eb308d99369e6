// The PLY writer of the dense stages (dense_ply.h).
#include <algorithm>
#include <vector>

#include "dense_ply.h"

namespace sfm {

PlyWriter::PlyWriter(const char* who, const char* path, const std::string& elements)
    : who_(who), path_(path), f_(std::fopen(path, "wb")) {
    SFM_REQUIRE(f_, SFM_ERR_INVALID_ARG, "%s: cannot open %s for writing", who, path);
    std::fprintf(f_, "ply\nformat binary_little_endian 1.0\n%send_header\n", elements.c_str());
}

PlyWriter::~PlyWriter() {
    if (f_) std::fclose(f_);
}

void PlyWriter::records(int64_t n, size_t rec_bytes, const std::function<void(int64_t, uint8_t*)>& fill) {
    constexpr int64_t kChunk = 4096;
    std::vector<uint8_t> buf(rec_bytes * (size_t)std::min(kChunk, std::max<int64_t>(n, 1)));
    for (int64_t k0 = 0; k0 < n; k0 += kChunk) {
        const int64_t k1 = std::min(k0 + kChunk, n);
        uint8_t* p = buf.data();
        for (int64_t k = k0; k < k1; ++k, p += rec_bytes) fill(k, p);
        std::fwrite(buf.data(), 1, (size_t)(p - buf.data()), f_);
    }
}

void PlyWriter::close() {
    const bool bad = std::ferror(f_) != 0;
    const bool closed = std::fclose(f_) == 0;
    f_ = nullptr;
    SFM_REQUIRE(!bad && closed, SFM_ERR_INVALID_ARG, "%s: writing %s failed", who_, path_);
}

void require_triangles(const char* who, int64_t n_triangles, const int32_t* tri, int64_t n_vertices) {
    for (int64_t k = 0; k < 3 * n_triangles; ++k)
        SFM_REQUIRE(tri[k] >= 0 && tri[k] < n_vertices, SFM_ERR_INVALID_ARG, "%s: triangle %lld names vertex %d of %lld", who,
                    (long long)(k / 3), tri[k], (long long)n_vertices);
}

}  // namespace sfm
