// BA point elimination (ba_schur): chunk points into MFMA tiles
// (schur_kernel), general points into Z rows (zbatch_kernel, zpoint_kernel).
#include <type_traits>

#include "ba_device.h"
namespace sfm {
namespace {
// Schur chunk kernel: one workgroup per tile group, one wavefront per chunk
//
// A tile group's chunks (<= kGroupChunks) share one slot layout.  Each wave
// owns its chunk's whole 80x80 tile as 15 lower 16x16 fp64 MFMA accumulators
// and walks the chunk in batches of <= kSubPts points / <= kSubObs (= 64)
// observations:
//   A  lane = observation: linearise, Jacobi-scale, stage Jx | f | J_intr
//   B  lane = point: V + D^2, Cholesky, L^-1, w = L^-1 g  (panel row 79)
//   C  lane = observation: M = Jx L^-T, camera rows of Z = J_c' M
//   C2 lane = (point, column): intrinsics rows of Z, ordered sum
//   D  tile -= panel panel' : ceil(3 npts / 4) k-steps x 15 MFMAs
// Inside the batch loop each wave syncs only itself (its LDS is its own), so
// co-resident waves overlap each other's VALU and MFMA phases; at the end the
// group's waves add their tiles in LDS in wave order and wave 0 writes the
// group's one tile.  Every sum has a fixed order, so results are
// bit-reproducible.

// LDS copy of a CamPre padded to 240 B (60 dwords): lanes of a batch read up
// to 10 different cameras' fields at once, and a 60-dword stride puts their
// 16-byte reads on disjoint banks (224 B = 56 dwords collided: 56 * 8 = 0 mod 64)
struct alignas(16) CamPreL {
    CamPre cp;
    double pad[2];
};
// next wave batch from p0: <= kSubPts points and <= kSubObs observations
// (cpoff = chunk-relative point offsets in LDS); returns its point count
// (batch_fits, ba_types.h, is the rule: the first lane that does not fit ends the batch)
template <int SP = kSubPts, int SO = kSubObs, class Off>
__device__ __forceinline__ int batch_points(const Off* cpoff, int p0, int np) {
    const int lane = threadIdx.x & 63;
    return __builtin_ctzll(~__ballot(batch_fits(cpoff, p0, lane, np, SP, SO)));
}

// rows of an LDS array at a compile-time stride S (in doubles)
template <int S>
struct LdsRows {
    double* p;
    __device__ __forceinline__ double* operator[](int q) const { return p + q * S; }
};

// lower 16x16 tiles (ti >= tj) of the NT x NT tile grid, row-major
__device__ constexpr int kTi[15] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4};
__device__ constexpr int kTj[15] = {0, 0, 1, 0, 1, 2, 0, 1, 2, 3, 0, 1, 2, 3, 4};

// NT = 5: rows 0..75 F blocks, row 79 = w, so -Z w comes out of the MFMA.
// NT = 4: rows 0..63 F blocks; -Z w (64 values) is a VALU dot product per lane.
// SP / SO: points / observations per wave batch.  The panel holds 3 columns
// per point padded to the MFMA k of 4 and NT*16 rows (NT = 4 keeps w apart).
// The pinhole NT = 4 kernel (kSlim) keeps its per-wave LDS small (8 one-wave
// workgroups per CU need <= 20480 B each, staging included), which is what
// lets it batch 6 points: only the 3 SP used panel columns are
// stored (the padding of the last k-step is read as literal zeros), the
// per-observation V | g_E shares lie over the panel (dead before phase B
// fills it, so the panel is zeroed after the per-point sums), J_intr and M
// share one odd-stride row per observation, and the chunk offsets and
// intrinsics rows are 16- and 8-bit.  With 6 points, phase C's 12 sums per
// point pass 64 lanes: with one intrinsics block in the chunk a lane takes
// the two columns that share an M entry (36 lanes); a chunk with several
// blocks takes the lane-per-(point, axis) sums (18 lanes x 4 sums, where 5
// points ran 60 lanes x 1: 9 % slower per launch than 5 / 52 on two-block
// chunks).  The BAL
// and RADIAL3 NT = 4 kernels and every NT = 5 kernel keep the wide layout
// and their code.
// SE: the solve's first pass also forms the Jacobi point scales (what
// point_scale_kernel computes) from the unscaled Jx it linearises anyway,
// writes them to scaleE and uses them, instead of a separate pass.
template <int CM, int NT, int SP = kSubPts, int SO = kSubObs, bool SE = false>
__global__ __launch_bounds__(64 * schur_group(NT)) __attribute__((amdgpu_waves_per_eu(2, 2))) void schur_kernel(
    DevProblem P, const CamPre* __restrict__ cps, const double* __restrict__ intr,
    const double* __restrict__ X, double radius, unsigned long long* __restrict__ stamps) {
    constexpr int IW = kIW<CM>;   // tile rows (and F columns) of an intrinsics block
    // intrinsics parameters with a Jacobian column: SNAVELY's 4th double is not one
    constexpr int NK = CM == SFM_CAM_SNAVELY ? 3 : IW;
    unsigned long long tacc[6] = {0, 0, 0, 0, 0, 0}, tprev = 0;
    if (stamps) tprev = stamp();
#define SFM_STAMP(k)                                      \
    if (stamps) {                                         \
        const unsigned long long tn_ = stamp();           \
        tacc[k] += tn_ - tprev;                           \
        tprev = tn_;                                      \
    }
    // LDS strides padded against bank conflicts (MI355X_MICROARCH.md §LDS):
    // panel rows 4 doubles past the tile width put the 12 (point, axis) rows
    // that the intrinsics pass updates at one column on distinct banks, and
    // 14-double observation rows spread ds_write_b128 lane groups.
    constexpr int kPK = 4 * ((3 * SP + 3) / 4), kPR = 16 * NT, kPS = kPR + 4;
    // per-observation rows use odd strides (in doubles): a wave's ds_*_b64 at
    // lane-strided rows then hits 32 distinct bank pairs (even strides of 4,
    // 6, 10 doubles were 2- to 4-way bank conflicts, SQ_LDS_BANK_CONFLICT)
    // pinhole: the 4 nonzeros of J_intr; SNAVELY / RADIAL3: both rows of every
    // parameter column (2 NK values)
    constexpr int kOb = CM == SFM_CAM_PINHOLE ? 5 : 2 * NK + 1;
    constexpr int kNTiles = NT * (NT + 1) / 2;
    constexpr int kComb = 5;                    // tiles per round of the group's tile sum
    // each wave's own LDS; its space also carries the wave's tiles to wave 0
    // at the end (kComb 16x16 tiles per round)
    constexpr bool kSlim = NT == 4 && CM == SFM_CAM_PINHOLE;
    constexpr int kPKs = kSlim ? 3 * SP : kPK;  // panel columns stored
    constexpr int kObU = CM == SFM_CAM_PINHOLE ? 4 : 2 * NK;   // J_intr values per observation
    constexpr int kRow = (kObU + 6) | 1;        // slim: J_intr | M row, odd stride
    struct WaveLdsWide {
        double panel[kPK][kPS];                 // [k][row]
        double wcol[NT == 4 ? kPK : 1];         // NT = 4: w = L^-1 g_E per panel column
        double ob[SO][kOb];                     // J_intr nonzeros (scaled) | pad
        // per observation: Jx'Jx (6) | Jx'f (3) until the per-point sums, then
        // M = Jx L^-T (6) from phase B on (obm: the same rows)
        double vs[SO][9];
        double vsum[SP][10];                    // per point: V (6) | g_E (3)
        int orow[SO];                           // tile row of the obs' intrinsics block
        int cpoff[kChunkPts + 1];               // chunk point offsets, relative to obs_begin
    };
    struct WaveLdsSlim {
        union {
            double panel[kPKs][kPS];            // [k][row], from phase B on
            double vs[SO][9];                   // Jx'Jx (6) | Jx'f (3) until the per-point sums
        };
        double wcol[kPKs];                      // w = L^-1 g_E per panel column
        double row[SO][kRow];                   // J_intr nonzeros (scaled) | M = Jx L^-T (6) | pad
        double vsum[SP][10];                    // per point: V (6) | g_E (3)
        unsigned short cpoff[kChunkPts + 1];    // chunk point offsets, relative to obs_begin
        unsigned char orow[SO];                 // tile row of the obs' intrinsics block
    };
    static_assert(!kSlim || (sizeof(double) * SO * 9 <= sizeof(double) * kPKs * kPS && kChunkPts * SO < 65536),
                  "slim layout: the shares fit the panel, the offsets 16 bits");
    using WaveLds = std::conditional_t<kSlim, WaveLdsSlim, WaveLdsWide>;
    union WaveU {
        WaveLds w;
        double comb[kComb * 256 + 64];          // kComb tiles + the NT = 4 -Zw column
    };
    static_assert(sizeof(WaveLds) >= sizeof(double) * (kComb * 256 + 64), "tile hand-over space");
    constexpr int GW = schur_group(NT);         // waves (chunks) per group
    __shared__ WaveU wl[GW];
    // group-level staging: every camera / intrinsics block the group touches
    __shared__ CamPreL scp[kCamSlots];
    __shared__ double csc[kCamSlots][6];        // camera column scales (0: constant image)
    __shared__ double isc[kIntrSlots][2 * IW];  // intrinsics | their column scales
    __shared__ int crow[kCamSlots], irow[kIntrSlots];
    // wave-uniform (scalar): the LDS bases and chunk fields below stay in SGPRs
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, grp = blockIdx.x;
    const int c0 = P.group_off[grp], n_sub = P.group_off[grp + 1] - c0;
    const int c = c0 + (wave < n_sub ? wave : 0);   // this wave's chunk (a wave past the group's chunks idles)
    const ChunkDesc& cd = P.chunks[c];
    WaveLds& W = wl[wave].w;
    double (&panel)[kPKs][kPS] = W.panel;
    auto& wcol = W.wcol;
    const LdsRows<9> vs{&W.vs[0][0]};
    LdsRows<kSlim ? kRow : kOb> ob;
    LdsRows<kSlim ? kRow : 9> obm;
    if constexpr (kSlim) {
        ob.p = &W.row[0][0];
        obm.p = &W.row[0][kObU];
    } else {
        ob.p = &W.ob[0][0];
        obm.p = &W.vs[0][0];
    }
    double (&vsum)[SP][10] = W.vsum;
    auto& orow = W.orow;
    auto& cpoff = W.cpoff;
    const int pb = cd.pt_begin, np = wave < n_sub ? cd.pt_end - pb : 0, ob0 = cd.obs_begin;
    // read once: a ChunkDesc load inside the batch loop would be waited on
    // with the in-order counter, i.e. together with the next batch's prefetch
    const bool one_intr = cd.n_intr == 1;
    const double inv_radius = 1.0 / radius;   // LM diagonal D^2 = clamp(diag) / radius (as step_kernel)

    for (int e = lane; e <= np; e += 64) cpoff[e] = P.pt_off[pb + e] - ob0;
    {   // the group's staging, by all its waves
        constexpr int kCpW = sizeof(CamPre) / 8;
        for (int e = threadIdx.x; e < cd.n_cams * kCpW; e += 64 * GW) {
            const int t = e / kCpW;
            reinterpret_cast<double*>(&scp[t].cp)[e - t * kCpW] =
                reinterpret_cast<const double*>(&cps[cd.cam_img[t]])[e - t * kCpW];
        }
        for (int e = threadIdx.x; e < cd.n_cams * 6; e += 64 * GW) {
            const int t = e / 6, col = cd.cam_col[t];
            csc[t][e - 6 * t] = col >= 0 ? P.scaleF[col + e - 6 * t] : 0.0;
        }
        if (threadIdx.x < cd.n_cams) crow[threadIdx.x] = cd.cam_row[threadIdx.x];
        if (threadIdx.x < IW * cd.n_intr) {
            const int t = threadIdx.x / IW, k = threadIdx.x - IW * t;
            isc[t][k] = intr[IW * cd.intr_id[t] + k];
            isc[t][IW + k] = P.scaleF[cd.intr_col[t] + k];
        }
        if (threadIdx.x < cd.n_intr) irow[threadIdx.x] = cd.intr_row[threadIdx.x];
    }

    v4d acc[kNTiles];
#pragma unroll
    for (int q = 0; q < kNTiles; ++q) acc[q] = v4d{0.0, 0.0, 0.0, 0.0};
    double wacc = 0.0;   // NT = 4: -(Z w)[lane]

    double xn2 = 0.0, gmx = 0.0;
    __syncthreads();
    // A batch's observation stream (uv, slot) and point data (X, column scale)
    // are fetched one batch ahead, so their HBM latency overlaps the current
    // batch's compute instead of opening every batch.
    struct BatchIn {
        int npts, slot, pl;
        double u0, u1, Xp[3], sE[3];
    };
    auto fetch = [&](int q0, BatchIn& in) {
        in.npts = q0 < np ? batch_points<SP, SO>(cpoff, q0, np) : 0;
        in.slot = 0; in.pl = 0; in.u0 = 0.0; in.u1 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { in.Xp[k] = 0.0; in.sE[k] = 1.0; }
        const int qo = cpoff[q0 < np ? q0 : np];
        if (lane < cpoff[q0 + in.npts] - qo) {
            const int o = ob0 + qo + lane;
            in.slot = P.obs_slot[o];
            const double2 uv = reinterpret_cast<const double2*>(P.obs_uv)[o];
            in.u0 = uv.x; in.u1 = uv.y;
#pragma unroll
            for (int j = 1; j < SP; ++j) in.pl += (j < in.npts && cpoff[q0 + j] - qo <= lane) ? 1 : 0;
            const size_t g = 3 * (size_t)(pb + q0 + in.pl);   // same address for the point's lanes
#pragma unroll
            for (int k = 0; k < 3; ++k) { in.Xp[k] = X[g + k]; in.sE[k] = P.scaleE[g + k]; }
        }
    };
    BatchIn nx;
    fetch(0, nx);
    // The first batch's loads complete before the loop.  Without this the
    // waitcnt pass merges the loop entry (loads pending in the registers the
    // loop body reads) with the back edge and waits on the counter inside
    // phase A of EVERY batch -- which, the counter being in order, also waits
    // for the next batch's prefetch, so its HBM latency was never hidden.
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    for (int p0 = 0; p0 < np;) {
        const int npts = nx.npts;   // batch [p0, p1)
        if (npts == 0) break;   // a point above SO observations: excluded by the planner
        const int p1 = p0 + npts;
        const int o0 = cpoff[p0], nobs = cpoff[p1] - o0;
        const int slot = nx.slot, pl = nx.pl;
        const double u0 = nx.u0, u1 = nx.u1;
        const double Xp[3] = {nx.Xp[0], nx.Xp[1], nx.Xp[2]};
        double sE[3] = {nx.sE[0], nx.sE[1], nx.sE[2]};
        fetch(p1, nx);
        auto zero_panel = [&]() {
#pragma unroll
            for (int e = lane; e < kPKs * kPS / 2; e += 64)
                reinterpret_cast<double2*>(&panel[0][0])[e] = double2{0.0, 0.0};
            if constexpr (NT == 4)
                if (lane < kPKs) wcol[lane] = 0.0;   // columns past 3 * npts stay zero
        };
        if constexpr (!kSlim) zero_panel();
        SFM_STAMP(0)
        // ---- A: observations -> scaled, corrected Jacobians -----------------
        LinT<CM> L;
        const int cs = slot & 255, is = (slot >> 8) & 255;
        if (lane < nobs) linearize<CM, true, true, true>(scp[cs].cp, &isc[is][0], Xp, u0, u1, P.huber_a, L);
        if constexpr (SE) {
            // column norms of the point's unscaled Jx, in observation and row
            // order (as point_scale_kernel): raw Jx staged in obm (free until B)
            if (lane < nobs) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int a = 0; a < 3; ++a) obm[lane][3 * r + a] = L.Jx[r][a];
            }
            wsync();
            if (lane < 3 * npts) {
                const int pt = lane / 3, a = lane - 3 * pt;
                const int q0 = cpoff[p0 + pt] - o0, q1 = cpoff[p0 + pt + 1] - o0;
                double cn = 0.0;
                for (int q = q0; q < q1; ++q) {
                    cn = fma(obm[q][a], obm[q][a], cn);
                    cn = fma(obm[q][3 + a], obm[q][3 + a], cn);
                }
                const double se = 1.0 / (1.0 + sqrt(cn));
                vsum[pt][a] = se;   // vsum is rewritten after phase A
                P.scaleE[3 * (size_t)(pb + p0 + pt) + a] = se;
            }
            wsync();
            if (lane < nobs) {
#pragma unroll
                for (int a = 0; a < 3; ++a) sE[a] = vsum[pl][a];
            }
            wsync();   // vsum is reused by the per-point sums below
        }
        if (lane < nobs) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
#pragma unroll
                for (int a = 0; a < 6; ++a) L.Jc[r][a] *= csc[cs][a];
#pragma unroll
                for (int a = 0; a < 3; ++a) L.Jx[r][a] *= sE[a];
            }
            // this observation's share of its point's V = Jx'Jx and g_E = Jx'f
            double cv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // V00 V10 V11 V20 V21 V22 | b0 b1 b2
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const double j0 = L.Jx[r][0], j1 = L.Jx[r][1], j2 = L.Jx[r][2], fr = L.f[r];
                cv[0] += j0 * j0; cv[1] += j1 * j0; cv[2] += j1 * j1;
                cv[3] += j2 * j0; cv[4] += j2 * j1; cv[5] += j2 * j2;
                cv[6] += j0 * fr; cv[7] += j1 * fr; cv[8] += j2 * fr;
            }
#pragma unroll
            for (int e = 0; e < 9; ++e) vs[lane][e] = cv[e];
            // J_intr rows are [x s, 0, s, 0] and [0, y s, 0, s]: keep the 4 nonzeros
            if constexpr (CM != SFM_CAM_PINHOLE) {
                // both rows of the parameter columns (SNAVELY f, l1, l2: column 3
                // is not a parameter; RADIAL3 f, ppx, ppy, k1, k2, k3)
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    ob[lane][2 * k] = L.Ji[0][k] * isc[is][IW + k];
                    ob[lane][2 * k + 1] = L.Ji[1][k] * isc[is][IW + k];
                }
            } else {
                ob[lane][0] = L.Ji[0][0] * isc[is][4];
                ob[lane][1] = L.Ji[1][1] * isc[is][5];
                ob[lane][2] = L.Ji[0][2] * isc[is][6];
                ob[lane][3] = L.Ji[1][3] * isc[is][7];
            }
            orow[lane] = irow[is];
        }
        wsync();
        // per-point sums in observation order, one lane per (point, entry)
        if (lane < 9 * npts) {
            const int pt = lane / 9, e = lane - 9 * pt;
            const int q0 = cpoff[p0 + pt] - o0, q1 = cpoff[p0 + pt + 1] - o0;
            double acc = 0.0;
            int q = q0;
            for (; q + 4 <= q1; q += 4) {   // loads in flight together, adds in order
                const double v0 = vs[q][e], v1 = vs[q + 1][e], v2 = vs[q + 2][e], v3 = vs[q + 3][e];
                acc += v0; acc += v1; acc += v2; acc += v3;
            }
            for (; q < q1; ++q) acc += vs[q][e];
            vsum[pt][e] = acc;
        }
        wsync();
        if constexpr (kSlim) {   // the shares are summed: their space becomes the panel
            zero_panel();
            wsync();
        }
        SFM_STAMP(1)
        // ---- B: every observation lane takes its point's V + D^2 and g_E (the
        // per-point sums above: identical on all lanes of the point), factors
        // it, and goes on to M = Jx L^-T and the camera rows of Z ----
        if (lane < nobs) {
            const int q0 = cpoff[p0 + pl] - o0;
            double V[6], b[3];   // V00 V10 V11 V20 V21 V22
#pragma unroll
            for (int e = 0; e < 6; ++e) V[e] = vsum[pl][e];
#pragma unroll
            for (int e = 0; e < 3; ++e) b[e] = vsum[pl][6 + e];
            const bool first = lane == q0;
            // gradient / norm bookkeeping at x (used after a relinearisation);
            // point_norms written out: the call changes this kernel's schedule
            if (first) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const double g = b[a] * rcp_nr(sE[a]);
                    xn2 += Xp[a] * Xp[a];
                    gmx = fmax(gmx, fabs(Xp[a] - (Xp[a] - g)));
                }
            }
            const auto [i00, i10, i11, i20, i21, i22] = point_factor(P, V, inv_radius);
            if (first) {
                const double w3[3] = {i00 * b[0], i10 * b[0] + i11 * b[1], i20 * b[0] + i21 * b[1] + i22 * b[2]};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if constexpr (NT == 5) panel[3 * pl + a][kTileWRow % kPR] = w3[a];
                    else wcol[3 * pl + a] = w3[a];
                }
            }
            double M[2][3];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                M[r][0] = L.Jx[r][0] * i00;
                M[r][1] = L.Jx[r][0] * i10 + L.Jx[r][1] * i11;
                M[r][2] = L.Jx[r][0] * i20 + L.Jx[r][1] * i21 + L.Jx[r][2] * i22;
            }
            const int row = crow[cs];
            if (row >= 0) {
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int k = 0; k < 6; ++k)
                        panel[3 * pl + a][row + k] = L.Jc[0][k] * M[0][a] + L.Jc[1][k] * M[1][a];
            }
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int a = 0; a < 3; ++a) obm[lane][3 * r + a] = M[r][a];
        }
        wsync();
        SFM_STAMP(2)
        // ---- C2: intrinsics rows, ordered per point ---------------------------
        // (register sums per run of observations sharing an intrinsics block)
        // One intrinsics block in the chunk (shared intrinsics, as C4 and the
        // SequentialActuator's single camera): every observation has the same
        // row, so the sums run without the run-boundary test (same fma order,
        // same bits as the general loops below).
        if (kSlim && one_intr && 12 * SP > 64) {
            // 12 sums per point pass 64 lanes: one lane per (point, axis, M
            // row r) takes columns r and r + 2, which share M[r][a] (each
            // sum's fma order as below)
            const int row = irow[0];
            if (lane < 6 * npts) {
                const int pt = lane / 6, rem = lane - 6 * pt, a = rem >> 1, r = rem & 1;
                const int mo = 3 * r + a;
                const int q0 = cpoff[p0 + pt] - o0, q1 = cpoff[p0 + pt + 1] - o0;
                double z0 = 0.0, z2 = 0.0;
                int q = q0;
                for (; q + 4 <= q1; q += 4) {
                    double j0[4], j2[4], mv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { j0[j] = ob[q + j][r]; j2[j] = ob[q + j][r + 2]; mv[j] = obm[q + j][mo]; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) { z0 = fma(j0[j], mv[j], z0); z2 = fma(j2[j], mv[j], z2); }
                }
                for (; q < q1; ++q) { z0 = fma(ob[q][r], obm[q][mo], z0); z2 = fma(ob[q][r + 2], obm[q][mo], z2); }
                panel[3 * pt + a][row + r] += z0;
                panel[3 * pt + a][row + r + 2] += z2;
            }
        } else if (one_intr) {
            constexpr int NZ = 3 * NK;   // (axis, column) sums per point
            const int row = irow[0];
            for (int e = lane; e < NZ * npts; e += 64) {
                const int pt = e / NZ, rem = e - NZ * pt, a = rem / NK, k = rem - NK * a;
                const int q0 = cpoff[p0 + pt] - o0, q1 = cpoff[p0 + pt + 1] - o0;
                double z = 0.0;
                int q = q0;
                if constexpr (CM == SFM_CAM_PINHOLE) {
                    // z_k = sum_q Ji[q][k] M[q][k & 1][a]
                    const int mo = 3 * (k & 1) + a;
                    for (; q + 4 <= q1; q += 4) {
                        double jv[4], mv[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) { jv[j] = ob[q + j][k]; mv[j] = obm[q + j][mo]; }
#pragma unroll
                        for (int j = 0; j < 4; ++j) z = fma(jv[j], mv[j], z);
                    }
                    for (; q < q1; ++q) z = fma(ob[q][k], obm[q][mo], z);
                } else {
                    for (; q + 2 <= q1; q += 2) {
                        double jv[4], mv[4];
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            jv[2 * j] = ob[q + j][2 * k]; jv[2 * j + 1] = ob[q + j][2 * k + 1];
                            mv[2 * j] = obm[q + j][a]; mv[2 * j + 1] = obm[q + j][3 + a];
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) z = fma(jv[j], mv[j], z);
                    }
                    for (; q < q1; ++q) {
                        z = fma(ob[q][2 * k], obm[q][a], z);
                        z = fma(ob[q][2 * k + 1], obm[q][3 + a], z);
                    }
                }
                panel[3 * pt + a][row + k] += z;
            }
        } else if constexpr (CM != SFM_CAM_PINHOLE) {
            // one lane per (point, axis, intrinsics column k < NK):
            // z_k = sum_q Ji[q][0][k] M[q][0][a] + Ji[q][1][k] M[q][1][a]
            for (int e = lane; e < 3 * NK * npts; e += 64) {
                const int pt = e / (3 * NK), rem = e - 3 * NK * pt, a = rem / NK, k = rem - NK * a;
                const int q0 = cpoff[p0 + pt] - o0, q1 = cpoff[p0 + pt + 1] - o0;
                int row = orow[q0];
                double z = 0.0;
                for (int q = q0; q < q1; ++q) {
                    const int rq = orow[q];
                    if (rq != row) {
                        panel[3 * pt + a][row + k] += z;
                        z = 0.0;
                        row = rq;
                    }
                    z = fma(ob[q][2 * k], obm[q][a], z);
                    z = fma(ob[q][2 * k + 1], obm[q][3 + a], z);
                }
                panel[3 * pt + a][row + k] += z;
            }
        } else if constexpr (12 * SP <= 64) {
            // one lane per (point, axis, intrinsics column): z_k = sum_q Ji[q][k] M[q][k & 1][a]
            if (lane < 12 * npts) {
                const int pt = lane / 12, rem = lane - 12 * pt, a = rem >> 2, k = rem & 3;
                const int mo = 3 * (k & 1) + a;
                const int q0 = cpoff[p0 + pt] - o0, q1 = cpoff[p0 + pt + 1] - o0;
                int row = orow[q0];
                double z = 0.0;
                auto step = [&](int rq, double jv, double mv) {
                    if (rq != row) {
                        panel[3 * pt + a][row + k] += z;
                        z = 0.0;
                        row = rq;
                    }
                    z = fma(jv, mv, z);
                };
                int q = q0;
                for (; q + 4 <= q1; q += 4) {   // operands of 4 observations loaded together
                    int rq[4];
                    double jv[4], mv[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { rq[j] = orow[q + j]; jv[j] = ob[q + j][k]; mv[j] = obm[q + j][mo]; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) step(rq[j], jv[j], mv[j]);
                }
                for (; q < q1; ++q) step(orow[q], ob[q][k], obm[q][mo]);
                panel[3 * pt + a][row + k] += z;
            }
        } else if (lane < 3 * npts) {
            const int pt = lane / 3, a = lane - 3 * pt;
            const int q0 = cpoff[p0 + pt] - o0, q1 = cpoff[p0 + pt + 1] - o0;
            int row = orow[q0];
            double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0;
            for (int q = q0; q < q1; ++q) {
                const int rq = orow[q];
                if (rq != row) {
                    panel[3 * pt + a][row + 0] += z0; panel[3 * pt + a][row + 1] += z1;
                    panel[3 * pt + a][row + 2] += z2; panel[3 * pt + a][row + 3] += z3;
                    z0 = z1 = z2 = z3 = 0.0;
                    row = rq;
                }
                const double m0 = obm[q][a], m1 = obm[q][3 + a];
                z0 += ob[q][0] * m0;
                z1 += ob[q][1] * m1;
                z2 += ob[q][2] * m0;
                z3 += ob[q][3] * m1;
            }
            panel[3 * pt + a][row + 0] += z0; panel[3 * pt + a][row + 1] += z1;
            panel[3 * pt + a][row + 2] += z2; panel[3 * pt + a][row + 3] += z3;
        }
        wsync();
        SFM_STAMP(3)
        // ---- D: tile += panel panel' on the fp64 MFMA -------------------------
        // all operands first (padding columns are zero: stored, or literal
        // where the panel ends at 3 SP columns), then the MFMAs
        const int kk = lane >> 4, ii = lane & 15;
        constexpr int kKs = kPK / 4;
        double op[kKs][NT];
#pragma unroll
        for (int ks = 0; ks < kKs; ++ks)
#pragma unroll
            for (int t = 0; t < NT; ++t)
                op[ks][t] = (4 * ks + 3 < kPKs || 4 * ks + kk < kPKs) ? panel[4 * ks + kk][16 * t + ii] : 0.0;
#pragma unroll
        for (int ks = 0; ks < kKs; ++ks)
#pragma unroll
            for (int q = 0; q < kNTiles; ++q)
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(op[ks][kTi[q]], op[ks][kTj[q]], acc[q], 0, 0, 0);
        if constexpr (NT == 4) {
#pragma unroll
            for (int k = 0; k < kPKs; ++k) wacc += panel[k][lane] * wcol[k];
        }
        wsync();
        SFM_STAMP(4)
        p0 = p1;
    }
    // ---- the group's tile: waves 1.. hand their accumulators to wave 0
    // through their own LDS, kComb 16x16 tiles per round, added in wave order;
    // wave 0 writes the negated tile, its lower 16x16 tiles only (the gather
    // reads upper blocks at their symmetric partner, FlatTerm modes)
    __syncthreads();   // every wave is past its batch loop: its LDS is free
    double* out = P.tiles + (size_t)grp * kTileR * kTileR;
#pragma unroll
    for (int q0 = 0; q0 < kNTiles; q0 += kComb) {
        if (wave > 0 && wave < n_sub) {
            double* cb = wl[wave].comb;
#pragma unroll
            for (int q = q0; q < q0 + kComb && q < kNTiles; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) cb[(q - q0) * 256 + r * 64 + lane] = acc[q][r];
            if (NT == 4 && q0 == 0) cb[kComb * 256 + lane] = wacc;
        }
        __syncthreads();
        if (wave == 0) {
            for (int w2 = 1; w2 < n_sub; ++w2) {
                const double* cb = wl[w2].comb;
#pragma unroll
                for (int q = q0; q < q0 + kComb && q < kNTiles; ++q)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[q][r] += cb[(q - q0) * 256 + r * 64 + lane];
                if (NT == 4 && q0 == 0) wacc += cb[kComb * 256 + lane];
            }
#pragma unroll
            for (int q = q0; q < q0 + kComb && q < kNTiles; ++q) {
                const int ti = kTi[q], tj = kTj[q];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * ti + (lane >> 4) + 4 * r, col = 16 * tj + (lane & 15);
                    out[row * kTileR + col] = -acc[q][r];
                }
            }
            if (NT == 4 && q0 == 0) out[kTileWRow * kTileR + lane] = -wacc;
        }
        if (q0 + kComb < kNTiles) __syncthreads();   // wave 0 has read this round
    }
    // ---- point partials of this wave's chunk (fixed-order wave reduction) ----
    double s1[1] = {xn2};
    wave_sum(s1);
    const double m1 = wave_max(gmx);
    if (lane == 0 && wave < n_sub) {
        P.part_s[2 * (size_t)c] = s1[0];
        P.part_s[2 * (size_t)c + 1] = m1;
    }
    SFM_STAMP(5)
    if (stamps && lane == 0 && wave < n_sub)
        for (int k = 0; k < 6; ++k) stamps[6 * (size_t)c + k] = tacc[k];
#undef SFM_STAMP
}

// General points (ba_plan.h): one wavefront per point -- any number of
// observations (rounds of 64), repeated views of one image, any number of
// intrinsics blocks.  The point is eliminated as in schur_kernel (V + D^2, its
// Cholesky L, w = L^-1 g_E, M = Jx L^-T per observation) and its eliminated
// rows Z_b = sum over the observations of block b of J_b' M (camera 6 x 3,
// intrinsics 4 x 3) plus w go to the Z buffer; preduce_kernel forms the RCS
// contributions -Z_a Z_b' and -Z_a w.  The point's Z is accumulated in LDS
// (dynamic: 64 x 19 staging doubles + the largest point's Z) in a fixed order:
// a camera block sums its adjacent run of observations (the planner sorts a
// general point's observations by image), an intrinsics block one masked
// wave sum per 64-observation round, rounds in order.

constexpr int kZStage = 19;   // doubles per staged observation row (18 used, odd stride)

template <int CM, bool SE>
__global__ __launch_bounds__(64) void zpoint_kernel(DevProblem P, const CamPre* __restrict__ cps,
                                                    const double* __restrict__ intr, const double* __restrict__ X,
                                                    double radius) {
    extern __shared__ __attribute__((aligned(16))) double zlds[];
    double* zc = zlds;                       // [64][kZStage] camera rows J_c' M of this round
    double* Zl = zlds + 64 * kZStage;        // the point's Z (blocks), accumulated
    __shared__ int cbl[64];
    const int lane = threadIdx.x, g = P.zlong[blockIdx.x];
    const int k = P.n_cpt + g;
    const int o0 = P.pt_off[k], o1 = P.pt_off[k + 1];
    const int b0 = P.gblk_off[g];
    const int zn = (int)(P.gz_off[g + 1] - P.gz_off[g]) - 3;
    const double Xp[3] = {X[3 * (size_t)k], X[3 * (size_t)k + 1], X[3 * (size_t)k + 2]};
    double sE[3];
    // observation o at x: loss-corrected Jacobians, unscaled
    constexpr int IW = kIW<CM>;
    auto lin = [&](int o, LinT<CM>& L) {
        const int img = P.obs_img[o];
        const double2 uv = reinterpret_cast<const double2*>(P.obs_uv)[o];
        linearize<CM, true, true, true>(cps[img], intr + IW * (size_t)P.img_intr[img], Xp, uv.x, uv.y, P.huber_a, L);
    };
    if constexpr (SE) {
        // the solve's first pass: Ceres' Jacobi point scales from the column
        // norms of the unscaled point Jacobian
        double cn[3] = {0.0, 0.0, 0.0};
        for (int o = o0 + lane; o < o1; o += 64) {
            LinT<CM> L;
            lin(o, L);
#pragma unroll
            for (int a = 0; a < 3; ++a) cn[a] += L.Jx[0][a] * L.Jx[0][a] + L.Jx[1][a] * L.Jx[1][a];
        }
        wave_sum(cn);
#pragma unroll
        for (int a = 0; a < 3; ++a) sE[a] = 1.0 / (1.0 + sqrt(cn[a]));
        if (lane < 3) P.scaleE[3 * (size_t)k + lane] = sE[lane];
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) sE[a] = P.scaleE[3 * (size_t)k + a];
    }
    // V = Jx' Jx, g_E = Jx' f over the point (scaled), summed by the wave
    double v9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // V00 V10 V11 V20 V21 V22 | b0 b1 b2
    for (int o = o0 + lane; o < o1; o += 64) {
        LinT<CM> L;
        lin(o, L);
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const double j0 = L.Jx[r][0] * sE[0], j1 = L.Jx[r][1] * sE[1], j2 = L.Jx[r][2] * sE[2], fr = L.f[r];
            v9[0] += j0 * j0; v9[1] += j1 * j0; v9[2] += j1 * j1;
            v9[3] += j2 * j0; v9[4] += j2 * j1; v9[5] += j2 * j2;
            v9[6] += j0 * fr; v9[7] += j1 * fr; v9[8] += j2 * fr;
        }
    }
    wave_sum(v9);
    double V[6] = {v9[0], v9[1], v9[2], v9[3], v9[4], v9[5]};
    const double b[3] = {v9[6], v9[7], v9[8]};
    if (lane == 0) {   // gradient / norm bookkeeping at x
        double xn2 = 0.0, gmx = 0.0;
        point_norms(b, sE, Xp, xn2, gmx);
        P.part_s[2 * (size_t)(P.n_chunk + g)] = xn2;
        P.part_s[2 * (size_t)(P.n_chunk + g) + 1] = gmx;
    }
    const auto [i00, i10, i11, i20, i21, i22] = point_factor(P, V, 1.0 / radius);
    for (int e = lane; e < zn; e += 64) Zl[e] = 0.0;
    int prev_cb = -1;   // camera block of the previous round's last observation
    for (int base = o0; base < o1; base += 64) {
        const int o = base + lane;
        const bool act = o < o1;
        int cb = 0xffff, ib = -1;
        double zi[3 * IW];
#pragma unroll
        for (int e = 0; e < 3 * IW; ++e) zi[e] = 0.0;
        if (act) {
            LinT<CM> L;
            lin(o, L);
            const int img = P.obs_img[o];
            const int slot = P.obs_slot[o];
            cb = slot & 0xffff;
            ib = slot >> 16;
            double M[2][3];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const double j0 = L.Jx[r][0] * sE[0], j1 = L.Jx[r][1] * sE[1], j2 = L.Jx[r][2] * sE[2];
                M[r][0] = j0 * i00;
                M[r][1] = j0 * i10 + j1 * i11;
                M[r][2] = j0 * i20 + j1 * i21 + j2 * i22;
            }
            const int colc = P.img_colc[img], coli = P.img_coli[img];
            if (cb != 0xffff) {
#pragma unroll
                for (int r = 0; r < 6; ++r) {
                    const double s = P.scaleF[colc + r];
#pragma unroll
                    for (int a = 0; a < 3; ++a)
                        zc[lane * kZStage + 3 * r + a] = (L.Jc[0][r] * s) * M[0][a] + (L.Jc[1][r] * s) * M[1][a];
                }
            }
            const int ni = CM == SFM_CAM_SNAVELY ? 3 : IW;
#pragma unroll
            for (int r = 0; r < IW; ++r) {
                if (r >= ni) continue;
                const double s = P.scaleF[coli + r];
#pragma unroll
                for (int a = 0; a < 3; ++a) zi[3 * r + a] = (L.Ji[0][r] * s) * M[0][a] + (L.Ji[1][r] * s) * M[1][a];
            }
        }
        cbl[lane] = act ? cb : -2;
        wsync();
        // camera blocks: the first observation of each run sums the run in order
        const bool head = act && cb != 0xffff && (lane == 0 || cbl[lane - 1] != cb);
        if (head) {
            double acc[18];
#pragma unroll
            for (int e = 0; e < 18; ++e) acc[e] = zc[lane * kZStage + e];
            for (int q = lane + 1; q < 64 && cbl[q] == cb; ++q)
#pragma unroll
                for (int e = 0; e < 18; ++e) acc[e] += zc[q * kZStage + e];
            double* dst = Zl + P.gblk_z[b0 + cb];
            const bool cont = lane == 0 && cb == prev_cb;   // run continued from the previous round
#pragma unroll
            for (int e = 0; e < 18; ++e) dst[e] = cont ? dst[e] + acc[e] : acc[e];
        }
        prev_cb = cbl[63] >= 0 ? cbl[63] : -1;
        // intrinsics blocks: one masked wave sum per distinct block of the round
        unsigned long long pend = __ballot(act);
        while (pend) {
            const int src = __builtin_ctzll(pend);
            const int j = __shfl(ib, src);
            const bool mine = act && ib == j;
            double v[3 * IW];
#pragma unroll
            for (int e = 0; e < 3 * IW; ++e) v[e] = mine ? zi[e] : 0.0;
            wave_sum(v);
            const int nz = 3 * (CM == SFM_CAM_SNAVELY ? 3 : IW);
            double mine_v = 0.0;   // v[lane] without a dynamically indexed register array
#pragma unroll
            for (int e = 0; e < 3 * IW; ++e) mine_v = lane == e ? v[e] : mine_v;
            if (lane < nz) Zl[P.gblk_z[b0 + j] + lane] += mine_v;
            pend &= ~__ballot(mine);
        }
        wsync();
    }
    double* Zg = P.Z + P.gz_off[g];
    for (int e = lane; e < zn; e += 64) Zg[e] = Zl[e];
    if (lane < 3) {
        const double w3[3] = {i00 * b[0], i10 * b[0] + i11 * b[1], i20 * b[0] + i21 * b[1] + i22 * b[2]};
        Zg[zn + lane] = lane == 0 ? w3[0] : lane == 1 ? w3[1] : w3[2];
    }
}

// Short general points (<= kZShortObs observations), a batch of consecutive
// points per wave, one lane per observation (zpoint_kernel spent a wave on
// each point, 10 of 64 lanes busy at random-k visibility, and linearised every
// observation twice).  Each observation is linearised once; every per-point
// sum (column norms, V | g_E, a camera block's run, an intrinsics block) is
// taken by the first lane of its group over the group's LDS rows in
// observation order, so the result is fixed.
constexpr int kZRow = 19;   // LDS row stride (doubles) of a lane's staged values
template <int CM, bool SE>
__global__ __launch_bounds__(64) void zbatch_kernel(DevProblem P, const CamPre* __restrict__ cps,
                                                    const double* __restrict__ intr, const double* __restrict__ X,
                                                    double radius) {
    constexpr int IW = kIW<CM>;
    constexpr int NI = CM == SFM_CAM_SNAVELY ? 3 : IW;   // intrinsics parameters with a column
    // camera rows J_c' M (18), then (round 6: one array, not two -- 2 -> 3
    // workgroups per SIMD) the intrinsics rows J_i' M (3 NI); before them
    // V | g_E (9), column norms (3)
    __shared__ double rc[64][kZRow];
    __shared__ double pv[kZBatchPts][12]; // per point: V (6) | g_E (3) | sE (3)
    __shared__ int poff[kZBatchPts + 1], okey[64], oib[64];
    const int lane = threadIdx.x;
    const int g0 = P.zbatch[2 * blockIdx.x], g1 = P.zbatch[2 * blockIdx.x + 1], np = g1 - g0;
    const int oA = P.pt_off[P.n_cpt + g0];
    if (lane <= np) poff[lane] = P.pt_off[P.n_cpt + g0 + lane] - oA;
    wsync();
    const int nobs = poff[np];
    const bool act = lane < nobs;
    int pl = 0;   // this lane's point within the batch
    for (int j = 1; j < np; ++j) pl += poff[j] <= lane ? 1 : 0;
    const int g = g0 + pl, k = P.n_cpt + g, o = oA + lane;
    const bool head = act && lane == poff[pl];   // the point's first observation
    double Xp[3] = {0.0, 0.0, 0.0};
    LinT<CM> L{};
    int img = 0, cb = 0xffff, ib = 0;
    if (act) {
#pragma unroll
        for (int a = 0; a < 3; ++a) Xp[a] = X[3 * (size_t)k + a];
        img = P.obs_img[o];
        const int slot = P.obs_slot[o];
        cb = slot & 0xffff;
        ib = slot >> 16;
        const double2 uv = reinterpret_cast<const double2*>(P.obs_uv)[o];
        linearize<CM, true, true, true>(cps[img], intr + IW * (size_t)P.img_intr[img], Xp, uv.x, uv.y, P.huber_a, L);
    }
    // per-point sums of n values staged in rc by every lane: the head lane adds
    // its point's rows in order into pv[pl][at..at+n)
    auto point_sum = [&](int n, int at) {
        wsync();
        if (head) {
            for (int e = 0; e < n; ++e) {
                double acc = rc[lane][e];
                for (int q = lane + 1; q < poff[pl + 1]; ++q) acc += rc[q][e];
                pv[pl][at + e] = acc;
            }
        }
        wsync();
    };
    double sE[3];
    if constexpr (SE) {
        // the solve's first pass: Ceres' Jacobi point scales from the column
        // norms of the unscaled point Jacobian
        if (act)
#pragma unroll
            for (int a = 0; a < 3; ++a) rc[lane][a] = L.Jx[0][a] * L.Jx[0][a] + L.Jx[1][a] * L.Jx[1][a];
        point_sum(3, 9);
        if (head)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double se = 1.0 / (1.0 + sqrt(pv[pl][9 + a]));
                pv[pl][9 + a] = se;
                P.scaleE[3 * (size_t)k + a] = se;
            }
        wsync();
#pragma unroll
        for (int a = 0; a < 3; ++a) sE[a] = pv[pl][9 + a];
    } else {
#pragma unroll
        for (int a = 0; a < 3; ++a) sE[a] = act ? P.scaleE[3 * (size_t)k + a] : 1.0;
    }
    // V = Jx' Jx, g_E = Jx' f per point (scaled)
    double j[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int a = 0; a < 3; ++a) j[r][a] = L.Jx[r][a] * sE[a];
    if (act) {
        double v9[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const double fr = L.f[r];
            v9[0] += j[r][0] * j[r][0]; v9[1] += j[r][1] * j[r][0]; v9[2] += j[r][1] * j[r][1];
            v9[3] += j[r][2] * j[r][0]; v9[4] += j[r][2] * j[r][1]; v9[5] += j[r][2] * j[r][2];
            v9[6] += j[r][0] * fr; v9[7] += j[r][1] * fr; v9[8] += j[r][2] * fr;
        }
#pragma unroll
        for (int e = 0; e < 9; ++e) rc[lane][e] = v9[e];
    }
    point_sum(9, 0);
    double V[6], b[3];
#pragma unroll
    for (int e = 0; e < 6; ++e) V[e] = pv[pl][e];
#pragma unroll
    for (int e = 0; e < 3; ++e) b[e] = pv[pl][6 + e];
    if (head) {   // gradient / norm bookkeeping at x
        double xn2 = 0.0, gmx = 0.0;
        point_norms(b, sE, Xp, xn2, gmx);
        P.part_s[2 * (size_t)(P.n_chunk + g)] = xn2;
        P.part_s[2 * (size_t)(P.n_chunk + g) + 1] = gmx;
    }
    const auto [i00, i10, i11, i20, i21, i22] = point_factor(P, V, 1.0 / radius);
    double M[2][3];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        M[r][0] = j[r][0] * i00;
        M[r][1] = j[r][0] * i10 + j[r][1] * i11;
        M[r][2] = j[r][0] * i20 + j[r][1] * i21 + j[r][2] * i22;
    }
    if (act) {
        if (cb != 0xffff) {
            const int colc = P.img_colc[img];
#pragma unroll
            for (int r = 0; r < 6; ++r) {
                const double sc = P.scaleF[colc + r];
#pragma unroll
                for (int a = 0; a < 3; ++a) rc[lane][3 * r + a] = (L.Jc[0][r] * sc) * M[0][a] + (L.Jc[1][r] * sc) * M[1][a];
            }
        }
    }
    okey[lane] = act ? (pl << 17 | cb) : -1;
    oib[lane] = ib;
    wsync();
    double* Zp = P.Z + P.gz_off[g];
    const int b0 = P.gblk_off[g], pend = poff[pl + 1];
    if (act) {
        // camera block: the first lane of a run of one (point, camera block)
        // adds the run in order (the planner sorts a point's views by image)
        if (cb != 0xffff && (lane == poff[pl] || okey[lane - 1] != okey[lane])) {
            double acc[18];
#pragma unroll
            for (int e = 0; e < 18; ++e) acc[e] = rc[lane][e];
            for (int q = lane + 1; q < pend && okey[q] == okey[lane]; ++q)
#pragma unroll
                for (int e = 0; e < 18; ++e) acc[e] += rc[q][e];
            double* dst = Zp + P.gblk_z[b0 + cb];
#pragma unroll
            for (int e = 0; e < 18; ++e) dst[e] = acc[e];
        }
    }
    wsync();   // (the camera rows are read; the intrinsics rows take their place)
    if (act) {
        const int coli = P.img_coli[img];
#pragma unroll
        for (int r = 0; r < NI; ++r) {
            const double sc = P.scaleF[coli + r];
#pragma unroll
            for (int a = 0; a < 3; ++a) rc[lane][3 * r + a] = (L.Ji[0][r] * sc) * M[0][a] + (L.Ji[1][r] * sc) * M[1][a];
        }
    }
    wsync();
    if (act) {
        // intrinsics block: the point's first lane with that block adds all of
        // the point's lanes with it, in order
        bool first = true;
        for (int q = poff[pl]; q < lane; ++q) first = first && oib[q] != ib;
        if (first) {
            double acc[3 * NI];
#pragma unroll
            for (int e = 0; e < 3 * NI; ++e) acc[e] = rc[lane][e];
            for (int q = lane + 1; q < pend; ++q)
                if (oib[q] == ib)
#pragma unroll
                    for (int e = 0; e < 3 * NI; ++e) acc[e] += rc[q][e];
            double* dst = Zp + P.gblk_z[b0 + ib];
#pragma unroll
            for (int e = 0; e < 3 * IW; ++e) dst[e] = e < 3 * NI ? acc[e < 3 * NI ? e : 0] : 0.0;   // SNAVELY: row 3 is 0
        }
        if (head) {   // w = L^-1 g_E after the point's blocks
            const int zn = (int)(P.gz_off[g + 1] - P.gz_off[g]) - 3;
            Zp[zn] = i00 * b[0];
            Zp[zn + 1] = i10 * b[0] + i11 * b[1];
            Zp[zn + 2] = i20 * b[0] + i21 * b[1] + i22 * b[2];
        }
    }
}

}  // namespace

void ba_schur(const DevProblem& P, const CamPre* cp, const double* intr, const double* X, double radius,
              hipStream_t s, unsigned long long* stamps, bool scale_e) {
    by_flag(scale_e, [&](auto tag) {
        constexpr bool SE = decltype(tag)::value;
        if (P.n_zbatch > 0) {
            SFM_BY_MODEL_ALL(P, hipLaunchKernelGGL((zbatch_kernel<CM, SE>), dim3(P.n_zbatch), dim3(64), 0, s, P, cp,
                                                   intr, X, radius));
            SFM_HIP(hipGetLastError());
        }
        if (P.n_zlong > 0) {
            const size_t lds = (64 * kZStage + (size_t)P.gz_max) * sizeof(double);
            SFM_BY_MODEL_ALL(P, {
                if (lds > 64 * 1024) set_dyn_lds((const void*)zpoint_kernel<CM, SE>, lds);
                hipLaunchKernelGGL((zpoint_kernel<CM, SE>), dim3(P.n_zlong), dim3(64), lds, s, P, cp, intr, X, radius);
            });
            SFM_HIP(hipGetLastError());
        }
        if (P.n_group <= 0) return;
        // 64-row tiles: batches of schur4_pts(CM) points (ba_types.h) at 8 waves
        // per CU.  Pinhole runs 6 points / 60 observations: with the wide
        // per-wave layout that shape's LDS allowed fewer waves and measured 9%
        // slower than 5 / 52; with the slim layout it is 20384 B per one-wave
        // workgroup (8 fit 160 KB) and C4 measured 358.7 -> 339.9 us per
        // launch, 1159 -> 1192 LM-iters/s (profiles/r07/a_batch6)
        const dim3 grid(P.n_group), block(64 * schur_group(P.tile_nt));
        if (P.tile_nt == 4)
            SFM_BY_MODEL_ALL(P, hipLaunchKernelGGL((schur_kernel<CM, 4, schur4_pts(CM), schur4_obs(CM), SE>), grid, block,
                                                   0, s, P, cp, intr, X, radius, stamps));
        else
            SFM_BY_MODEL_ALL(P, hipLaunchKernelGGL((schur_kernel<CM, 5, kSubPts, kSubObs, SE>), grid, block, 0, s, P, cp,
                                                   intr, X, radius, stamps));
        SFM_HIP(hipGetLastError());
    });
}

}  // namespace sfm
