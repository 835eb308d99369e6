// Relative pose (include/sfmcore.h, "Relative pose"), the
// arithmetic written once for the device kernel (relpose.hip) and the serial
// host twin (relpose.cpp, sfm_relpose_host): the pieces of the five-point
// essential-matrix solver (Gauss-Jordan elimination, the ten cubic
// constraints, Nister's degree-10 polynomial, its Sturm sequence, the root
// search and the model of a root), the error of a correspondence under E, the
// a-contrario NFA term, Horn's closed-form motions of E, the cheirality test
// of a correspondence and its ray angle.
//
// The solver is cut into pieces so that the kernel can spread them over a
// workgroup (one matrix entry, one constraint row, one grid point or one root
// per lane) while the host runs the same pieces in a loop: every number is
// produced by the same operation sequence in both, so the search computes the
// same bits.  Only + - * / and sqrt (frexp / ldexp inside acransac.h's log10;
// atan2 for the one reported angle): the including file sets
// `#pragma clang fp contract(off)` first.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "acransac.h"
#include "track.h"
#include "tri_point.h"

namespace sfm {
namespace {

#if !defined(__HIPCC__)   // a plain host compiler
using std::atan2;
#endif

constexpr int kE5Sample = 5;            // MINIMUM_SAMPLES
constexpr int kE5MaxModels = 10;        // MAX_MODELS
constexpr double kE5NullPivot = 1e-12;  // smallest pivot of the 5x9 elimination (rows of unit bearings)
constexpr double kE5ElimPivot = 1e-13;  // smallest pivot of the 10x20 elimination (unit basis vectors)
constexpr int kE5Grid = 256;            // Sturm evaluations on [-B, B], one per lane
constexpr int kE5SturmBisect = 64;      // Sturm bisections to separate the roots of one grid cell
constexpr int kE5SignBisect = 200;      // sign bisections on an isolated root (acransac.h's bisect)
constexpr double kE5RootBound = 1e12;   // the Cauchy bound is clamped to this
constexpr int kE5Poly = kE5MaxModels + 1;   // coefficients of a degree-10 polynomial

__host__ __device__ inline double relpose_inf() { return __builtin_inf(); }

// ---- Gauss-Jordan, serially ---------------------------------------------------
// A (R x C, row-major) to reduced row echelon form on R pivot columns.  FULL
// (the 5x9 system): step c takes the largest |A[r][k]| over the rows r >= c and
// the columns k not yet taken (the lowest (r, k) on a tie) and records k as
// pc[c].  Otherwise (the 10x20 system) column c itself, the largest |A[r][c]|,
// r >= c (the lowest r on a tie).  The pivot row is swapped to row c and
// divided by the pivot, then f times it is subtracted from every other row, f
// that row's entry of the pivot column.  False: a pivot not above thr (or not
// a number).  The kernel runs the same steps with one entry per lane
// (relpose.hip, gj_lds).
template <int R, int C, bool FULL>
__host__ __device__ inline bool e5_pivot(const double* A, int c, uint32_t used, double thr, int& pr, int& pk) {
    double best = -1.0;
    pr = c;
    pk = c;
    for (int r = c; r < R; ++r) {
        if constexpr (FULL) {
            for (int k = 0; k < C; ++k) {
                const double v = fabs(A[r * C + k]);
                if (!((used >> k) & 1u) && v > best) { best = v; pr = r; pk = k; }
            }
        } else {
            const double v = fabs(A[r * C + c]);
            if (v > best) { best = v; pr = r; }
        }
    }
    return best > thr;
}
template <int R, int C, bool FULL>
__host__ __device__ inline bool e5_gauss_jordan(double* A, double thr, int* pc) {
    uint32_t used = 0;
    for (int c = 0; c < R; ++c) {
        int piv, pk;
        if (!e5_pivot<R, C, FULL>(A, c, used, thr, piv, pk)) return false;
        used |= 1u << pk;
        pc[c] = pk;
        if (piv != c)
            for (int k = 0; k < C; ++k) {
                const double t = A[c * C + k];
                A[c * C + k] = A[piv * C + k];
                A[piv * C + k] = t;
            }
        const double pv = A[c * C + pk];
        for (int k = 0; k < C; ++k) A[c * C + k] = A[c * C + k] / pv;
        for (int r = 0; r < R; ++r) {
            if (r == c) continue;
            const double f = A[r * C + pk];
            for (int k = 0; k < C; ++k) A[r * C + k] = A[r * C + k] - f * A[c * C + k];
        }
    }
    return true;
}

// entry (i, c) of the 5x9 epipolar system: b_J' E b_I = 0 in E's row-major entries
__host__ __device__ inline double e5_epipolar_entry(const double* bI, const double* bJ, int i, int c) {
    return bJ[3 * i + c / 3] * bI[3 * i + c % 3];
}

// Basis vector v (0..3: X, Y, Z, W) of the null space of the reduced 5x9
// system with pivot columns pc[5].  Null vector u belongs to the u-th free
// column f (ascending): 1 at f, -A5[r][f] at pc[r], 0 elsewhere.  The basis
// is the four of them mixed by the rows of the orthogonal matrix of the
// quaternion (1, 2, 3, 4), each scaled to unit length: with the raw vectors a
// solution whose entries at the free columns vanish (a forward motion) would
// lie at infinity of E = x X + y Y + z Z + W.
__host__ __device__ inline void e5_basis_vector(const double* A5, const int* pc, int v, double* b) {
    const double Q[4][4] = {{1, -2, -3, -4}, {2, 1, -4, 3}, {3, 4, 1, -2}, {4, -3, 2, 1}};
    int rowof[9], fc[4], nf = 0;
    for (int i = 0; i < 9; ++i) rowof[i] = -1;
    for (int r = 0; r < 5; ++r) rowof[pc[r]] = r;
    for (int i = 0; i < 9; ++i)
        if (rowof[i] < 0 && nf < 4) fc[nf++] = i;
    double n2 = 0.0;
    for (int i = 0; i < 9; ++i) {
        double e[4];
        for (int u = 0; u < 4; ++u) e[u] = rowof[i] >= 0 ? -A5[rowof[i] * 9 + fc[u]] : (i == fc[u] ? 1.0 : 0.0);
        b[i] = ((Q[v][0] * e[0] + Q[v][1] * e[1]) + Q[v][2] * e[2]) + Q[v][3] * e[3];
        n2 = n2 + b[i] * b[i];
    }
    const double s = sqrt(n2);
    for (int i = 0; i < 9; ++i) b[i] = b[i] / s;
}

// ---- polynomials in (x, y, z) of E = x X + y Y + z Z + W -----------------------
// degree 1: [x, y, z, 1]; degree 2: [x2, y2, z2, xy, xz, yz, x, y, z, 1];
// degree 3, Nister's column order: [x3, y3, x2y, xy2, x2z, x2, y2z, y2, xyz, xy,
// xz2, xz, x, yz2, yz, y, z3, z2, z, 1]
__host__ __device__ inline int e5_m11(int i, int j) {
    const int8_t T[16] = {0, 3, 4, 6, 3, 1, 5, 7, 4, 5, 2, 8, 6, 7, 8, 9};
    return T[4 * i + j];
}
__host__ __device__ inline int e5_m21(int i, int j) {
    const int8_t T[40] = {0,  2,  4,  5,  3,  1,  6,  7,  10, 13, 16, 17, 2,  3,  8,  9,  4,  8,  10, 11,
                          8,  6,  13, 14, 5,  9,  11, 12, 9,  7,  14, 15, 11, 14, 17, 18, 12, 15, 18, 19};
    return T[4 * i + j];
}
// c[10] += a[4] * b[4]
__host__ __device__ inline void e5_mul11(const double (&a)[4], const double (&b)[4], double (&c)[10]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) c[e5_m11(i, j)] = c[e5_m11(i, j)] + a[i] * b[j];
}
// c[20] += a[10] * b[4]
__host__ __device__ inline void e5_mul21(const double (&a)[10], const double (&b)[4], double (&c)[20]) {
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) c[e5_m21(i, j)] = c[e5_m21(i, j)] + a[i] * b[j];
}
// entry (r, c) of E as a degree-1 polynomial; basis[v][9]
__host__ __device__ inline void e5_entry(const double* basis, int r, int c, double (&p)[4]) {
#pragma unroll
    for (int v = 0; v < 4; ++v) p[v] = basis[9 * v + 3 * r + c];
}

// (E E')_ik, i <= k, as a degree-2 polynomial: the sum over l of E_il E_kl
__host__ __device__ inline void e5_eet(const double* basis, int i, int k, double* out) {
    double d[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int l = 0; l < 3; ++l) {
        double a[4], b[4];
        e5_entry(basis, i, l, a);
        e5_entry(basis, k, l, b);
        e5_mul11(a, b, d);
    }
    for (int e = 0; e < 10; ++e) out[e] = d[e];
}
// where (E E')_ik is among the six polynomials 00, 01, 02, 11, 12, 22
__host__ __device__ inline int e5_sym(int i, int k) {
    const int lo = i < k ? i : k, hi = i < k ? k : i;
    return lo == 0 ? hi : lo == 1 ? 2 + hi : 5;
}

// constraint row 0: det E
__host__ __device__ inline void e5_row_det(const double* basis, double* row) {
    double c[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = 0; j < 3; ++j) {   // E_0j times its cofactor E_1u E_2w - E_1w E_2u
        const int u = (j + 1) % 3, w = (j + 2) % 3;
        double a[4], b[4], p[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, m[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        e5_entry(basis, 1, u, a);
        e5_entry(basis, 2, w, b);
        e5_mul11(a, b, p);
        e5_entry(basis, 1, w, a);
        e5_entry(basis, 2, u, b);
        e5_mul11(a, b, m);
        for (int e = 0; e < 10; ++e) p[e] = p[e] - m[e];
        e5_entry(basis, 0, j, a);
        e5_mul21(p, a, c);
    }
    for (int e = 0; e < 20; ++e) row[e] = c[e];
}
// constraint row 1 + 3 i + j: entry (i, j) of 2 E E' E - tr(E E') E, from the
// six polynomials of E E' (eet[6][10])
__host__ __device__ inline void e5_row_trace(const double* eet, const double* basis, int i, int j, double* row) {
    double c[20] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) {
        double lam[10], a[4];
        const double* g = eet + 10 * e5_sym(i, k);
        for (int e = 0; e < 10; ++e) {
            lam[e] = 2.0 * g[e];
            if (k == i) lam[e] = lam[e] - ((eet[e] + eet[30 + e]) + eet[50 + e]);
        }
        e5_entry(basis, k, j, a);
        e5_mul21(lam, a, c);
    }
    for (int e = 0; e < 20; ++e) row[e] = c[e];
}

// ---- Nister's polynomial ------------------------------------------------------
// From the reduced 10x20 system A: rows 4..9 have their pivots at x2z, x2, y2z,
// y2, xyz, xy, so (row 4 + 2q) - z (row 5 + 2q), q < 3, are three equations
// [3] x + [3] y + [4] = 0 with polynomials in z: Bz[q][0..2][5], ascending.
__host__ __device__ inline void e5_bz(const double* A, double* Bz) {
    for (int q = 0; q < 3; ++q) {
        const double* e = A + 20 * (4 + 2 * q);
        const double* f = A + 20 * (5 + 2 * q);
        double* b = Bz + 15 * q;
        for (int v = 0; v < 2; ++v) {   // x: columns 10..12, y: 13..15
            const int o = 10 + 3 * v;
            b[5 * v] = e[o + 2];
            b[5 * v + 1] = e[o + 1] - f[o + 2];
            b[5 * v + 2] = e[o] - f[o + 1];
            b[5 * v + 3] = -f[o];
            b[5 * v + 4] = 0.0;
        }
        b[10] = e[19];
        b[11] = e[18] - f[19];
        b[12] = e[17] - f[18];
        b[13] = e[16] - f[17];
        b[14] = -f[16];
    }
}
// a[0..3] b[0..3] - c[0..3] d[0..3] into m[0..6]
__host__ __device__ inline void e5_minor(const double* a, const double* b, const double* c, const double* d,
                                         double* m) {
    double p[7] = {0, 0, 0, 0, 0, 0, 0}, q[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            p[i + j] = p[i + j] + a[i] * b[j];
            q[i + j] = q[i + j] + c[i] * d[j];
        }
    for (int i = 0; i < 7; ++i) m[i] = p[i] - q[i];
}
// det Bz, degree 10 in z, ascending into p[11]: the expansion along the column
// of the constant terms
__host__ __device__ inline void e5_poly10(const double* Bz, double* p) {
    const double *k = Bz, *l = Bz + 15, *m = Bz + 30;
    double m0[7], m1[7], m2[7];
    e5_minor(l, m + 5, l + 5, m, m0);       // lx my - ly mx
    e5_minor(k, m + 5, k + 5, m, m1);       // kx my - ky mx
    e5_minor(k, l + 5, k + 5, l, m2);       // kx ly - ky lx
    for (int i = 0; i < kE5Poly; ++i) p[i] = 0.0;
    for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 7; ++j) p[i + j] = p[i + j] + ((k[10 + i] * m0[j] - l[10 + i] * m1[j]) + m[10 + i] * m2[j]);
}

__host__ __device__ inline double e5_horner(const double* c, int deg, double x) {
    double v = c[deg];
    for (int i = deg - 1; i >= 0; --i) v = v * x + c[i];
    return v;
}

// The Sturm sequence of p (degree <= 10): sc[k][11] ascending, degrees sdeg[k].
// s0 = p / |lead|, s1 = s0' / deg, s(k+1) = -rem(s(k-1), s(k)) / |lead|; a
// remainder's leading terms below 1e-14 of its largest coefficient are
// dropped, and the sequence ends at a constant or a vanishing remainder.
// Returns the number of polynomials and the root bound B = min(1 + max
// |s0[i]|, kE5RootBound); 0: p has no degree >= 1 or is not finite.
__host__ __device__ inline int e5_sturm(const double* p, double* sc, int* sdeg, double* B) {
    int d = kE5MaxModels;
    for (int i = 0; i <= kE5MaxModels; ++i)
        if (!track_finite(p[i])) return 0;
    while (d >= 0 && p[d] == 0.0) --d;
    if (d < 1) return 0;
    const double a0 = fabs(p[d]);
    double big = 0.0;
    for (int i = 0; i <= d; ++i) {
        sc[i] = p[i] / a0;
        if (i < d && fabs(sc[i]) > big) big = fabs(sc[i]);
    }
    if (!track_finite(big)) return 0;
    *B = 1.0 + big <= kE5RootBound ? 1.0 + big : kE5RootBound;
    sdeg[0] = d;
    for (int i = 1; i <= d; ++i) sc[kE5Poly + i - 1] = (double)i * sc[i] / (double)d;
    sdeg[1] = d - 1;
    int n = 2;
    while (n < kE5Poly && sdeg[n - 1] >= 1) {
        const double* u = sc + kE5Poly * (n - 2);
        const double* v = sc + kE5Poly * (n - 1);
        const int du = sdeg[n - 2], dv = sdeg[n - 1];
        double r[kE5Poly];
        for (int i = 0; i <= du; ++i) r[i] = u[i];
        for (int k = du - dv; k >= 0; --k) {
            const double q = r[dv + k] / v[dv];
            for (int j = 0; j < dv; ++j) r[j + k] = r[j + k] - q * v[j];
        }
        double rmax = 0.0;
        for (int j = 0; j < dv; ++j)
            if (fabs(r[j]) > rmax) rmax = fabs(r[j]);
        if (!(rmax > 0.0) || !track_finite(rmax)) break;
        int dr = dv - 1;
        while (dr > 0 && !(fabs(r[dr]) > 1e-14 * rmax)) --dr;
        const double a = fabs(r[dr]);
        double* w = sc + kE5Poly * n;
        for (int i = 0; i <= dr; ++i) w[i] = -r[i] / a;
        sdeg[n] = dr;
        ++n;
    }
    return n;
}
// sign changes of the sequence at x (zeros skipped)
__host__ __device__ inline int e5_sturm_count(const double* sc, const int* sdeg, int n, double x) {
    int changes = 0, prev = 0;
    for (int k = 0; k < n; ++k) {
        const double v = e5_horner(sc + kE5Poly * k, sdeg[k], x);
        const int sg = v > 0.0 ? 1 : v < 0.0 ? -1 : 0;
        if (sg != 0) {
            changes += prev != 0 && sg != prev;
            prev = sg;
        }
    }
    return changes;
}
// grid point g of [-B, B]
__host__ __device__ inline double e5_grid(double B, int g) { return -B + (double)g * ((2.0 * B) / (double)(kE5Grid - 1)); }

// Real root number j (ascending, j < cnt[0] - cnt[kE5Grid - 1]) of s0 from the
// Sturm counts cnt[] at the grid points: the grid cell that holds it, Sturm
// bisection (at most kE5SturmBisect halvings) until the cell holds that root
// alone with a change of sign, then bisection on the sign of s0 as acransac.h's
// bisect does.
__host__ __device__ inline double e5_root(const double* sc, const int* sdeg, int n, const int* cnt, double B, int j) {
    int g = 0;
    while (g < kE5Grid - 2 && cnt[0] - cnt[g + 1] <= j) ++g;
    double lo = e5_grid(B, g), hi = e5_grid(B, g + 1);
    int clo = cnt[g], chi = cnt[g + 1], r = j - (cnt[0] - cnt[g]);
    bool bracket = false, up = false;
    for (int it = 0; it < kE5SturmBisect; ++it) {
        if (clo - chi == 1) {
            const double fl = e5_horner(sc, sdeg[0], lo), fh = e5_horner(sc, sdeg[0], hi);
            if ((fl < 0.0 && fh > 0.0) || (fl > 0.0 && fh < 0.0)) {
                bracket = true;
                up = fl < 0.0;
                break;
            }
        }
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        const int cm = e5_sturm_count(sc, sdeg, n, mid);
        const int k = clo - cm;
        if (r < k) { hi = mid; chi = cm; }
        else { r -= k; lo = mid; clo = cm; }
    }
    if (bracket)
        for (int it = 0; it < kE5SignBisect; ++it) {
            const double mid = 0.5 * (lo + hi);
            if (!(mid > lo && mid < hi)) break;
            const double gv = e5_horner(sc, sdeg[0], mid);
            if ((gv < 0.0) == up) lo = mid;
            else hi = mid;
        }
    return 0.5 * (lo + hi);
}

// The essential matrix of the root z: (x, y, 1) is the cross product of two
// rows of Bz(z), the pair with the largest third component (the first on a
// tie); E = x X + y Y + z Z + W scaled to Frobenius norm sqrt(2).  False when
// it is not finite.
__host__ __device__ inline bool e5_model(const double* Bz, const double* basis, double z, double* E) {
    double b[3][3];
    for (int q = 0; q < 3; ++q) {
        b[q][0] = e5_horner(Bz + 15 * q, 3, z);
        b[q][1] = e5_horner(Bz + 15 * q + 5, 3, z);
        b[q][2] = e5_horner(Bz + 15 * q + 10, 4, z);
    }
    double cx = 0.0, cy = 0.0, cz = 0.0;
    for (int s = 0; s < 3; ++s) {
        const int u = s == 2 ? 1 : 0, w = s == 0 ? 1 : 2;   // (0,1), (0,2), (1,2)
        const double c0 = b[u][1] * b[w][2] - b[u][2] * b[w][1];
        const double c1 = b[u][2] * b[w][0] - b[u][0] * b[w][2];
        const double c2 = b[u][0] * b[w][1] - b[u][1] * b[w][0];
        if (fabs(c2) > fabs(cz)) { cx = c0; cy = c1; cz = c2; }
    }
    const double x = cx / cz, y = cy / cz;
    double n2 = 0.0;
    for (int i = 0; i < 9; ++i) {
        E[i] = ((x * basis[i] + y * basis[9 + i]) + z * basis[18 + i]) + basis[27 + i];
        n2 = n2 + E[i] * E[i];
    }
    const double s = sqrt(n2 / 2.0);
    bool fin = s > 0.0;
    for (int i = 0; i < 9; ++i) {
        E[i] = E[i] / s;
        fin = fin && track_finite(E[i]);
    }
    return fin;
}

// workspace of one serial solve
struct E5Work {
    double A5[45], basis[36], eet[60], A[200], Bz[45], poly[kE5Poly], sc[kE5Poly * kE5Poly], B;
    int sdeg[kE5Poly], cnt[kE5Grid];
};

// The five-point solver, serially: unit bearings bI[3i..], bJ[3i..], i < 5, to
// at most ten E[9 m], roots ascending.  0 for a degenerate sample.
__host__ __device__ inline int e5_solve(const double* bI, const double* bJ, double* E, E5Work& w) {
    for (int i = 0; i < 5; ++i)
        for (int c = 0; c < 9; ++c) w.A5[9 * i + c] = e5_epipolar_entry(bI, bJ, i, c);
    int pc[10];
    if (!e5_gauss_jordan<5, 9, true>(w.A5, kE5NullPivot, pc)) return 0;
    for (int v = 0; v < 4; ++v) e5_basis_vector(w.A5, pc, v, w.basis + 9 * v);
    for (int i = 0, e = 0; i < 3; ++i)
        for (int k = i; k < 3; ++k, ++e) e5_eet(w.basis, i, k, w.eet + 10 * e);
    e5_row_det(w.basis, w.A);
    for (int r = 0; r < 9; ++r) e5_row_trace(w.eet, w.basis, r / 3, r % 3, w.A + 20 * (1 + r));
    if (!e5_gauss_jordan<10, 20, false>(w.A, kE5ElimPivot, pc)) return 0;
    e5_bz(w.A, w.Bz);
    e5_poly10(w.Bz, w.poly);
    const int ns = e5_sturm(w.poly, w.sc, w.sdeg, &w.B);
    if (ns == 0) return 0;
    for (int g = 0; g < kE5Grid; ++g) w.cnt[g] = e5_sturm_count(w.sc, w.sdeg, ns, e5_grid(w.B, g));
    int nr = w.cnt[0] - w.cnt[kE5Grid - 1];
    if (nr > kE5MaxModels) nr = kE5MaxModels;
    int nm = 0;
    for (int j = 0; j < nr; ++j) {
        const double z = e5_root(w.sc, w.sdeg, ns, w.cnt, w.B, j);
        if (e5_model(w.Bz, w.basis, z, E + 9 * nm)) ++nm;
    }
    return nm;
}

// ---- the error of a correspondence, the NFA term --------------------------------
// With a = E b_I, the epipolar line of the correspondence in image J's
// undistorted pixels is (a0 / f0, a1 / f1, .) and the pixel's homogeneous
// product with it (a . b_J) / b_J2: the squared distance is their quotient.
// inJ: image J's intrinsics block (its focal lengths are all that enters).
template <int CM>
__host__ __device__ inline double relpose_error(const double* E, const double* inJ, const double* bi, const double* bj) {
    const double a0 = E[0] * bi[0] + E[1] * bi[1] + E[2] * bi[2];
    const double a1 = E[3] * bi[0] + E[4] * bi[1] + E[5] * bi[2];
    const double a2 = E[6] * bi[0] + E[7] * bi[1] + E[8] * bi[2];
    const double f0 = inJ[0], f1 = CM == SFM_CAM_PINHOLE ? inJ[1] : inJ[0];
    const double d = (a0 * bj[0] + a1 * bj[1] + a2 * bj[2]) / bj[2];
    const double l0 = a0 / f0, l1 = a1 / f1;
    const double e = d * d / (l0 * l0 + l1 * l1);
    return track_finite(e) ? e : relpose_inf();
}

// NFA of the k smallest errors, the k-th being e (point-to-line: mult_error 0.5)
__host__ __device__ inline double relpose_nfa(double loge0, double logalpha0, double e, int64_t k, float logc_n,
                                              float logc_k) {
    const double logalpha = logalpha0 + 0.5 * det_log10(e + 1.1920928955078125e-07);
    return loge0 + logalpha * (double)(k - kE5Sample) + (double)logc_n + (double)logc_k;
}

// ---- the motions of E (Horn 1990) ----------------------------------------------
// t t' = tr(E E') / 2 I - E E': t is the row of its largest diagonal entry (the
// first on a tie) over the root of that entry.  With C the matrix of cofactors
// of E (rows e1 x e2, e2 x e0, e0 x e1 of E's rows): Ra = (C - [t]x E) / (t.t),
// Rb = (C + [t]x E) / (t.t).  Motion m of four: R = m < 2 ? Ra : Rb, and t
// negated for odd m.  False: E has no such diagonal entry above 0.
__host__ __device__ inline bool relpose_motions(const double* E, double* Ra, double* Rb, double* t) {
    double G[3][3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) G[r][c] = E[3 * r] * E[3 * c] + E[3 * r + 1] * E[3 * c + 1] + E[3 * r + 2] * E[3 * c + 2];
    const double h = 0.5 * ((G[0][0] + G[1][1]) + G[2][2]);
    int i = 0;
    double best = h - G[0][0];
    for (int r = 1; r < 3; ++r)
        if (h - G[r][r] > best) { best = h - G[r][r]; i = r; }
    if (!(best > 0.0) || !track_finite(best)) return false;
    const double s = sqrt(best);
    for (int c = 0; c < 3; ++c) t[c] = (c == i ? best : -G[i][c]) / s;
    const double tt = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2];
    double Cf[9], TE[9];
    for (int r = 0; r < 3; ++r) {
        const double* u = E + 3 * ((r + 1) % 3);
        const double* v = E + 3 * ((r + 2) % 3);
        Cf[3 * r] = u[1] * v[2] - u[2] * v[1];
        Cf[3 * r + 1] = u[2] * v[0] - u[0] * v[2];
        Cf[3 * r + 2] = u[0] * v[1] - u[1] * v[0];
    }
    for (int c = 0; c < 3; ++c) {   // t x (column c of E)
        TE[c] = t[1] * E[6 + c] - t[2] * E[3 + c];
        TE[3 + c] = t[2] * E[c] - t[0] * E[6 + c];
        TE[6 + c] = t[0] * E[3 + c] - t[1] * E[c];
    }
    bool fin = true;
    for (int a = 0; a < 9; ++a) {
        Ra[a] = (Cf[a] - TE[a]) / tt;
        Rb[a] = (Cf[a] + TE[a]) / tt;
        fin = fin && track_finite(Ra[a]) && track_finite(Rb[a]);
    }
    return fin;
}

template <int CM>
__host__ __device__ inline bool relpose_front(double z) {
    return CM == SFM_CAM_SNAVELY ? z < 0.0 : z > 0.0;
}

// Is the two-view triangulation (tri_point.h: the two Grams summed, tri_solve4)
// of the bearings bi (camera [I | 0]) and bj (camera [R | t]) in front of both?
template <int CM>
__host__ __device__ inline bool relpose_in_front(const double* R, const double* t, const double* bi, const double* bj) {
    CamPre ci{}, cj{};
    ci.R[0] = ci.R[4] = ci.R[8] = 1.0;
    for (int a = 0; a < 9; ++a) cj.R[a] = R[a];
    for (int a = 0; a < 3; ++a) cj.t[a] = t[a];
    const double vi[3] = {bi[0], bi[1], bi[2]}, vj[3] = {bj[0], bj[1], bj[2]};
    double Gi[10], Gj[10], X[3];
    tri_gram(ci, vi, Gi);
    tri_gram(cj, vj, Gj);
    for (int e = 0; e < 10; ++e) Gi[e] = Gi[e] + Gj[e];
    if (!tri_solve4(Gi, X)) return false;
    const double zj = ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + t[2];
    return relpose_front<CM>(X[2]) && relpose_front<CM>(zj);
}
// bit m of the result: the correspondence is in front under motion m
template <int CM>
__host__ __device__ inline uint32_t relpose_front_mask(const double* Ra, const double* Rb, const double* t,
                                                       const double* bi, const double* bj) {
    const double tn[3] = {-t[0], -t[1], -t[2]};
    uint32_t m = 0;
    m |= relpose_in_front<CM>(Ra, t, bi, bj) ? 1u : 0u;
    m |= relpose_in_front<CM>(Ra, tn, bi, bj) ? 2u : 0u;
    m |= relpose_in_front<CM>(Rb, t, bi, bj) ? 4u : 0u;
    m |= relpose_in_front<CM>(Rb, tn, bi, bj) ? 8u : 0u;
    return m;
}

// The winner of the cheirality vote over the four counts: the largest (the
// lowest motion on a tie) when the largest of the others over it is below
// front_ratio; -1 otherwise.
__host__ __device__ inline int relpose_vote(const int64_t* cnt, double front_ratio) {
    int b = 0;
    for (int m = 1; m < 4; ++m)
        if (cnt[m] > cnt[b]) b = m;
    int64_t second = 0;
    for (int m = 0; m < 4; ++m)
        if (m != b && cnt[m] > second) second = cnt[m];
    if (cnt[b] <= 0) return -1;
    return (double)second / (double)cnt[b] < front_ratio ? b : -1;
}

// The rays b_I and R' b_J: |b_I - R' b_J|^2, which grows with their angle and
// orders the median's sort, and the angle itself in degrees.
__host__ __device__ inline void relpose_rays(const double* R, const double* bi, const double* bj, double (&c)[3]) {
    for (int j = 0; j < 3; ++j) c[j] = (R[j] * bj[0] + R[3 + j] * bj[1]) + R[6 + j] * bj[2];
}
__host__ __device__ inline double relpose_angle_key(const double* R, const double* bi, const double* bj) {
    double c[3];
    relpose_rays(R, bi, bj, c);
    const double d0 = bi[0] - c[0], d1 = bi[1] - c[1], d2 = bi[2] - c[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}
__host__ __device__ inline double relpose_angle_deg(const double* R, const double* bi, const double* bj) {
    double c[3];
    relpose_rays(R, bi, bj, c);
    const double x0 = bi[1] * c[2] - bi[2] * c[1], x1 = bi[2] * c[0] - bi[0] * c[2], x2 = bi[0] * c[1] - bi[1] * c[0];
    const double sn = sqrt((x0 * x0 + x1 * x1) + x2 * x2);
    const double cs = (bi[0] * c[0] + bi[1] * c[1]) + bi[2] * c[2];
    return atan2(sn, cs) * (180.0 / 3.14159265358979323846);
}

}  // namespace
}  // namespace sfm
