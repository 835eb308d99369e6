// One lattice point of the mesh stage (include/sfmcore.h, "Mesh"): the
// arithmetic of the contract, once, for the kernels (mesh.hip) and the host
// twins (mesh.cpp).  Everything is float; every operation is a single IEEE
// operation in the stated order, and the two translation units that include
// this switch contraction off (#pragma clang fp contract(off) at their top), so
// the bytes agree.  The colours and the counts are integers.  The marching
// tetrahedra table is worked out from the orientation rule at compile time.
#pragma once
#include <cmath>
#include <cstdint>

#include "dense_common.h"

namespace sfm {

// a workgroup of the extraction kernels: this many consecutive raster indices
constexpr int kMeshBlock = 256;
// a workgroup of the integration kernel: kMeshTileX points along x by kMeshTileY along y
constexpr int kMeshTileX = 64;
constexpr int kMeshTileY = 4;

// An image of the call: M = K R and C, worked out in double and rounded once.
struct MeshView {
    float M[9], C[3];
    int32_t w, h, channels, loaded;   // channels 0: no colours; !loaded: no depth map
    int64_t map_off, pix_off;         // pixels into the maps; bytes into the colour pool
};
struct MeshGrid {
    float origin[3], voxel;
    int32_t nx, ny, nz, pad;
};

SFM_HD inline int64_t mesh_raster(const MeshGrid& g, int32_t i, int32_t j, int32_t k) {
    return ((int64_t)k * g.ny + j) * g.nx + i;
}
SFM_HD inline void mesh_position(const MeshGrid& g, int32_t i, int32_t j, int32_t k, float* X) {
    X[0] = g.origin[0] + (float)i * g.voxel;
    X[1] = g.origin[1] + (float)j * g.voxel;
    X[2] = g.origin[2] + (float)k * g.voxel;
}

// ---- integration ----------------------------------------------------------------------
// Lattice point (i, j, k) against the images in index order.  rgb / has_rgb are
// written only when pixels is given.  Returns the point's weight.
SFM_HD inline int32_t mesh_integrate_point(const MeshView* views, int32_t n_img, const MeshGrid& g, float trunc,
                                           const float* depth, const uint8_t* pixels, int32_t i, int32_t j,
                                           int32_t k, float* tsdf, uint8_t* rgb, uint8_t* has_rgb) {
    float X[3];
    mesh_position(g, i, j, k, X);
    float sum = 0.0f;
    int32_t count = 0;
    uint32_t col[3] = {0, 0, 0}, m = 0;
    for (int32_t v = 0; v < n_img; ++v) {
        const MeshView& V = views[v];
        if (!V.loaded) continue;
        float x, y, z;
        project_point(V.M, V.C, X, &x, &y, &z);
        if (!(z > 0.0f)) continue;
        const int64_t idx = nearest_pixel(x, y, V.w, V.h);
        if (idx < 0) continue;
        const float d = depth[V.map_off + idx];
        if (!(d > 0.0f)) continue;
        const float sd = d - z;
        if (sd < -trunc) continue;
        const float t = (sd < trunc ? sd : trunc) / trunc;
        sum = sum + t;
        ++count;
        if (pixels && V.channels && fabsf(sd) <= trunc) {
            add_color(pixels + V.pix_off + idx * V.channels, V.channels, col);
            ++m;
        }
    }
    *tsdf = count > 0 ? sum / (float)count : 0.0f;
    if (pixels) {
        for (int c = 0; c < 3; ++c) rgb[c] = m ? mean_u8(col[c], m) : (uint8_t)0;
        *has_rgb = m ? 1 : 0;
    }
    return count < 255 ? count : 255;
}

// ---- the marching tetrahedra table ----------------------------------------------------
// Corner c of a cell is the bits (x, y, z) of c.  Tetrahedron t follows the axis
// permutation kMeshPerm[t] = (p1, p2, p3): its corners are 0, e_p1, e_p1 + e_p2, 7.
constexpr int kMeshPerm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
// corners 1 and 2 of the six tetrahedra, three bits each (plain integers, so device code needs no table)
constexpr uint32_t mesh_pack_corners(int n) {
    uint32_t v = 0;
    for (int t = 0; t < 6; ++t)
        v |= (uint32_t)((1 << kMeshPerm[t][0]) | (n == 2 ? 1 << kMeshPerm[t][1] : 0)) << (3 * t);
    return v;
}
constexpr uint32_t kMeshCorner1 = mesh_pack_corners(1), kMeshCorner2 = mesh_pack_corners(2);
SFM_HD constexpr int mesh_tet_corner(int t, int n) {
    return n == 0 ? 0 : (n == 1 ? (int)((kMeshCorner1 >> (3 * t)) & 7u) : (n == 2 ? (int)((kMeshCorner2 >> (3 * t)) & 7u) : 7));
}
// An edge of a tetrahedron is (n << 2) | m over its corners n < m.  A case is the
// bits "corner n is inside"; it has n_tri triangles of three edges each.
struct MeshCase {
    uint8_t n_tri, edge[6];
};
struct MeshTable {
    MeshCase c[6][16];
};
constexpr int mesh_edge_code(int a, int b) { return a < b ? (a << 2) | b : (b << 2) | a; }
// twice the midpoint of an edge, component a
constexpr int mesh_mid2(int t, int e, int a) {
    return ((mesh_tet_corner(t, e >> 2) >> a) & 1) + ((mesh_tet_corner(t, e & 3) >> a) & 1);
}
constexpr MeshTable mesh_make_table() {
    MeshTable T{};
    for (int t = 0; t < 6; ++t)
        for (int cs = 0; cs < 16; ++cs) {
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, n_in = 0, n_out = 0;
            for (int n = 0; n < 4; ++n) {
                if ((cs >> n) & 1)
                    in[n_in++] = n;
                else
                    out[n_out++] = n;
            }
            MeshCase& M = T.c[t][cs];
            if (n_in == 1 || n_in == 3) {
                const int a = n_in == 1 ? in[0] : out[0];
                const int* o = n_in == 1 ? out : in;
                M.n_tri = 1;
                for (int v = 0; v < 3; ++v) M.edge[v] = (uint8_t)mesh_edge_code(a, o[v]);
            } else if (n_in == 2) {
                const int q[4] = {mesh_edge_code(in[0], out[0]), mesh_edge_code(in[0], out[1]),
                                  mesh_edge_code(in[1], out[1]), mesh_edge_code(in[1], out[0])};
                M.n_tri = 2;
                const int order[6] = {0, 1, 2, 0, 2, 3};
                for (int v = 0; v < 6; ++v) M.edge[v] = (uint8_t)q[order[v]];
            }
            // orientation: the normal of the triangle over the edges' midpoints
            // looks from the inside corners to the outside ones
            bool decided = true;
            for (int tr = 0; tr < M.n_tri; ++tr) {
                int A[3] = {0, 0, 0}, B[3] = {0, 0, 0}, C[3] = {0, 0, 0}, dir[3] = {0, 0, 0};
                for (int a = 0; a < 3; ++a) {
                    A[a] = mesh_mid2(t, M.edge[3 * tr], a);
                    B[a] = mesh_mid2(t, M.edge[3 * tr + 1], a) - A[a];
                    C[a] = mesh_mid2(t, M.edge[3 * tr + 2], a) - A[a];
                    for (int n = 0; n < n_out; ++n) dir[a] += n_in * ((mesh_tet_corner(t, out[n]) >> a) & 1);
                    for (int n = 0; n < n_in; ++n) dir[a] -= n_out * ((mesh_tet_corner(t, in[n]) >> a) & 1);
                }
                const int dot = (B[1] * C[2] - B[2] * C[1]) * dir[0] + (B[2] * C[0] - B[0] * C[2]) * dir[1] +
                                (B[0] * C[1] - B[1] * C[0]) * dir[2];
                if (dot == 0) decided = false;   // never: a multiple of the tetrahedron's volume (checked below)
                if (dot < 0) {
                    const uint8_t s = M.edge[3 * tr + 1];
                    M.edge[3 * tr + 1] = M.edge[3 * tr + 2];
                    M.edge[3 * tr + 2] = s;
                }
            }
            if (!decided) M.n_tri = 255;
        }
    return T;
}
constexpr bool mesh_table_sound(const MeshTable& T) {
    for (int t = 0; t < 6; ++t)
        for (int cs = 0; cs < 16; ++cs)
            if (T.c[t][cs].n_tri > 2) return false;
    return true;
}
static_assert(mesh_table_sound(mesh_make_table()), "the orientation rule decides every case");

// the slot of the owned edge along offset bits o (1 .. 7): x y z xy xz yz xyz
// and back: 1 2 4 3 5 6 7 and 0 1 3 2 4 5 6, three bits an entry (plain integers again)
SFM_HD constexpr int mesh_offset_of_slot(int s) { return (int)((0x1F5711u >> (3 * s)) & 7u); }
SFM_HD constexpr int mesh_slot_of_offset(int o) { return (int)((0x1AC4C8u >> (3 * (o - 1))) & 7u); }
constexpr bool mesh_slots_sound() {
    const int off[7] = {1, 2, 4, 3, 5, 6, 7};
    for (int s = 0; s < 7; ++s)
        if (mesh_offset_of_slot(s) != off[s] || mesh_slot_of_offset(off[s]) != s) return false;
    return true;
}
static_assert(mesh_slots_sound(), "slots 0 .. 6 are the offsets x y z xy xz yz xyz");

// ---- extraction -----------------------------------------------------------------------
SFM_HD inline bool mesh_observed(const uint8_t* weight, int32_t min_weight, int64_t at) {
    return (int32_t)weight[at] >= min_weight;
}

// The 7-bit mask of the owned edges of lattice point (i, j, k) that carry a
// vertex, the triangles of its own cell (0 when the cell is not live) and how
// many of them are degenerate.
SFM_HD inline uint32_t mesh_point_marks(const MeshGrid& g, const float* tsdf, const uint8_t* weight,
                                        int32_t min_weight, int32_t i, int32_t j, int32_t k, int32_t* n_tri,
                                        int32_t* n_degenerate) {
    static constexpr MeshTable T = mesh_make_table();
    // bit (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1): that neighbour exists and is observed
    uint32_t obs = 0;
    for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int32_t x = i + dx, y = j + dy, z = k + dz;
                if (x < 0 || y < 0 || z < 0 || x >= g.nx || y >= g.ny || z >= g.nz) continue;
                if (mesh_observed(weight, min_weight, mesh_raster(g, x, y, z)))
                    obs |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
            }
    // live[e]: the cell at (i, j, k) - e (e: bits x y z) is live
    uint32_t live = 0;
    for (int e = 0; e < 8; ++e) {
        bool all = true;
        for (int c = 0; c < 8; ++c) {
            const int dx = (c & 1) - (e & 1), dy = ((c >> 1) & 1) - ((e >> 1) & 1), dz = ((c >> 2) & 1) - ((e >> 2) & 1);
            all = all && ((obs >> ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1))) & 1u);
        }
        if (all) live |= 1u << e;
    }
    *n_tri = 0;
    *n_degenerate = 0;
    if (!((obs >> 13) & 1u)) return 0;   // the point itself is not observed
    // the point and its seven forward neighbours, the corners of its own cell: inside, and tsdf == 0
    uint32_t inside = 0, zero = 0;
    for (int c = 0; c < 8; ++c) {
        const int dx = c & 1, dy = (c >> 1) & 1, dz = (c >> 2) & 1;
        if ((obs >> ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1))) & 1u) {
            const float t = tsdf[mesh_raster(g, i + dx, j + dy, k + dz)];
            if (t < 0.0f) inside |= 1u << c;
            if (t == 0.0f) zero |= 1u << c;
        }
    }
    uint32_t mask = 0;
    for (int s = 0; s < 7; ++s) {
        const int o = mesh_offset_of_slot(s);
        const int dx = o & 1, dy = (o >> 1) & 1, dz = (o >> 2) & 1;
        if (!((obs >> ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1))) & 1u)) continue;
        if ((inside & 1u) == ((inside >> o) & 1u)) continue;
        // the cells that contain both ends: (i, j, k) - e with e zero where o is set
        bool used = false;
        for (int e = 0; e < 8; ++e) used = used || (!(e & o) && ((live >> e) & 1u));
        if (used) mask |= 1u << s;
    }
    if (live & 1u)
        for (int tt = 0; tt < 6; ++tt) {
            uint32_t cs = 0, zs = 0;
            for (int n = 0; n < 4; ++n) {
                const int c = mesh_tet_corner(tt, n);
                cs |= ((inside >> c) & 1u) << n;
                zs |= ((zero >> c) & 1u) << n;
            }
            const MeshCase& M = T.c[tt][cs];
            *n_tri += M.n_tri;
            for (int tr = 0; tr < M.n_tri; ++tr) {
                // per corner of the tetrahedron with tsdf == 0: how many of the triangle's edges end in it
                uint32_t once = 0, twice = 0;
                for (int v = 0; v < 3; ++v) {
                    const int e = M.edge[3 * tr + v];
                    const uint32_t ends = ((1u << (e >> 2)) | (1u << (e & 3))) & zs;
                    twice |= once & ends;
                    once |= ends;
                }
                if (twice) ++*n_degenerate;
            }
        }
    return mask;
}

// The vertex on the owned edge `slot` of lattice point (i, j, k).  rgb_in NULL: no colours.
SFM_HD inline void mesh_edge_vertex(const MeshGrid& g, const float* tsdf, const uint8_t* rgb_in,
                                    const uint8_t* has_rgb, int32_t i, int32_t j, int32_t k, int slot, float* X,
                                    uint8_t* rgb) {
    const int o = mesh_offset_of_slot(slot);
    const int32_t bi = i + (o & 1), bj = j + ((o >> 1) & 1), bk = k + ((o >> 2) & 1);
    const int64_t a = mesh_raster(g, i, j, k), b = mesh_raster(g, bi, bj, bk);
    float Xa[3], Xb[3];
    mesh_position(g, i, j, k, Xa);
    mesh_position(g, bi, bj, bk, Xb);
    const float ta = tsdf[a], tb = tsdf[b];
    const float u = ta / (ta - tb);
    for (int c = 0; c < 3; ++c) X[c] = Xa[c] + u * (Xb[c] - Xa[c]);
    if (rgb_in) {
        int64_t from = u < 0.5f ? a : b;
        if (!has_rgb[from]) from = u < 0.5f ? b : a;
        const bool any = has_rgb[from] != 0;
        for (int c = 0; c < 3; ++c) rgb[c] = any ? rgb_in[3 * from + c] : (uint8_t)0;
    }
}

// The triangles of the live cell (i, j, k), written to tri (three indices each,
// the cell's place in the output) in (tetrahedron, triangle) order; returns how many.
SFM_HD inline int32_t mesh_cell_triangles(const MeshGrid& g, const float* tsdf, const int32_t* vert_base,
                                          const uint8_t* mask, int32_t i, int32_t j, int32_t k, int32_t* tri) {
    static constexpr MeshTable T = mesh_make_table();
    uint32_t inside = 0;
    for (int c = 0; c < 8; ++c)
        if (tsdf[mesh_raster(g, i + (c & 1), j + ((c >> 1) & 1), k + ((c >> 2) & 1))] < 0.0f) inside |= 1u << c;
    int32_t n = 0;
    for (int tt = 0; tt < 6; ++tt) {
        uint32_t cs = 0;
        for (int c = 0; c < 4; ++c) cs |= ((inside >> mesh_tet_corner(tt, c)) & 1u) << c;
        const MeshCase& M = T.c[tt][cs];
        for (int v = 0; v < 3 * M.n_tri; ++v) {
            const int e = M.edge[v];
            const int ca = mesh_tet_corner(tt, e >> 2), cb = mesh_tet_corner(tt, e & 3);
            const int64_t owner = mesh_raster(g, i + (ca & 1), j + ((ca >> 1) & 1), k + ((ca >> 2) & 1));
            const int slot = mesh_slot_of_offset(cb ^ ca);
            tri[3 * n + v] = vert_base[owner] + __builtin_popcount((uint32_t)mask[owner] & ((1u << slot) - 1u));
        }
        n += M.n_tri;
    }
    return n;
}

}  // namespace sfm
