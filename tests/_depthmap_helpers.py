"""Reference for the depth-map tests (test_depthmap.py, test_depthmap_gpu.py):
a numpy float32 restatement of the contract in include/sfmcore.h ("Dense depth
maps"): the per-pair matrices, the random numbers, the plane cost, the
red/black passes, the filter and the view selection, written from that comment
(numpy does these IEEE operations one by one, without fusing, so the comparison
is for equality).  The fixtures are rendered here too: a textured plane (a
seeded 8-bit noise image bilinearly enlarged, plus two sinusoids) seen by
pinhole cameras through ray-plane intersection, so depth and normal are
analytic.  Each reference is computed once and shared."""
import functools
import math

import numpy as np

import _helpers as H
import _wash_helpers as W

abi, api = H.abi, W.api
F = np.float32
M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-5, 0), (5, 0), (0, -5), (0, 5))


# ---- random numbers -------------------------------------------------------------------
def mix64(z):
    with np.errstate(over="ignore"):
        z = np.asarray(z, np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def pixel_seed(seed, img, idx):
    with np.errstate(over="ignore"):
        s = mix64(np.array([(seed ^ ((img * 0xD1B54A32D192ED03) & M64)) & M64], np.uint64))[0]
        return mix64(s + np.asarray(idx, np.uint64) * np.uint64(GOLD))


def uniform(base, k):
    with np.errstate(over="ignore"):
        return (mix64(base + np.uint64((k * GOLD) & M64)) >> np.uint64(40)).astype(F) * F(2.0 ** -24)


# ---- the host's double precision part -------------------------------------------------
def mul33(a, b):
    return [a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + a[3 * r + 2] * b[6 + c] for r in range(3) for c in range(3)]


def inv33(m):
    c0, c1, c2 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
    det = m[0] * c0 + m[1] * c1 + m[2] * c2
    return [c0 / det, (m[2] * m[7] - m[1] * m[8]) / det, (m[1] * m[5] - m[2] * m[4]) / det,
            c1 / det, (m[0] * m[8] - m[2] * m[6]) / det, (m[2] * m[3] - m[0] * m[5]) / det,
            c2 / det, (m[1] * m[6] - m[0] * m[7]) / det, (m[0] * m[4] - m[1] * m[3]) / det]


def gray_of(im):
    im = np.asarray(im, np.uint8)
    if im.ndim == 2:
        return im
    v = im.astype(np.uint32)
    return ((77 * v[..., 0] + 150 * v[..., 1] + 29 * v[..., 2] + 128) >> 8).astype(np.uint8)


class Views:
    """what the host precomputes: per image Ki, the range and its inverses, the gray image; per pair A, b"""

    def __init__(self, wh, K, R, C, nb_off, nb_view, drange=None, images=None):
        self.n = len(wh) // 2
        self.wh = [(int(wh[2 * i]), int(wh[2 * i + 1])) for i in range(self.n)]
        K = [[float(v) for v in np.asarray(K[i]).reshape(-1)] for i in range(self.n)]
        R = [[float(v) for v in np.asarray(R[i]).reshape(-1)] for i in range(self.n)]
        C = [[float(v) for v in np.asarray(C[i]).reshape(-1)] for i in range(self.n)]
        Kinv = [inv33(k) for k in K]
        self.Ki = [np.array(k, np.float64).astype(F) for k in Kinv]
        self.nbs = []
        for i in range(self.n):
            pairs = []
            for q in range(int(nb_off[i]), int(nb_off[i + 1])):
                j = int(nb_view[q])
                Rt = [R[i][3 * c + r] for r in range(3) for c in range(3)]
                KR = mul33(K[j], R[j])
                A = mul33(mul33(KR, Rt), Kinv[i])
                dc = [C[i][a] - C[j][a] for a in range(3)]
                b = [KR[3 * r] * dc[0] + KR[3 * r + 1] * dc[1] + KR[3 * r + 2] * dc[2] for r in range(3)]
                pairs.append((j, np.array(A, np.float64).astype(F), np.array(b, np.float64).astype(F)))
            self.nbs.append(pairs)
        self.gray = [None if images is None or images[i] is None else gray_of(images[i]) for i in range(self.n)]
        self.loaded = [images is None or images[i] is not None for i in range(self.n)]
        self.active = [self.loaded[i] and len(self.nbs[i]) > 0 for i in range(self.n)]
        if drange is not None:
            d = np.asarray(drange, F).reshape(-1, 2)
            self.dmin, self.dmax = d[:, 0], d[:, 1]
            with np.errstate(all="ignore"):
                self.imin, self.imax = F(1.0) / self.dmax, F(1.0) / self.dmin
        sizes = [w * h for w, h in self.wh]
        self.map_off = [sum(sizes[:i]) for i in range(self.n)]
        self.n_map = sum(sizes)


# ---- the per-pixel arithmetic, vectorised over pixels ---------------------------------
def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def mul_pixel(M, x, y):
    return [(M[3 * k] * x + M[3 * k + 1] * y) + M[3 * k + 2] for k in range(3)]


def plane_offset(n, d, ray):
    return dot3(n, [d * ray[0], d * ray[1], d * ray[2]])


def face_camera(n, ray):
    flip = dot3(n, ray) > 0
    return [np.where(flip, -c, c) for c in n]


def normalize(v):
    ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return [v[0] / ln, v[1] / ln, v[2] / ln]


def ref_sums(g, px, py, r):
    sa, saa = np.zeros(len(px), F), np.zeros(len(px), F)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            a = g[py + dy, px + dx].astype(F)
            sa, saa = sa + a, saa + a * a
    return sa, saa


def pair_cost(V, i, pair, px, py, r, t, n, sa, saa):
    j, A, b = pair
    N = F((2 * r + 1) ** 2)
    if not V.loaded[j]:
        return np.full(len(px), 2.0, F)
    g, gj = V.gray[i], V.gray[j]
    wj, hj = V.wh[j]
    Ki = V.Ki[i]
    ok = np.ones(len(px), bool)
    sb, sbb, sab = (np.zeros(len(px), F) for _ in range(3))
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            qx, qy = (px + dx).astype(F), (py + dy).astype(F)
            z = t / dot3(n, mul_pixel(Ki, qx, qy))
            a3 = mul_pixel(A, qx, qy)
            h0, h1, h2 = z * a3[0] + b[0], z * a3[1] + b[1], z * a3[2] + b[2]
            x, y = h0 / h2, h1 / h2
            ok &= (z > 0) & (h2 > 0) & (x >= 0) & (x <= F(wj - 1)) & (y >= 0) & (y <= F(hj - 1))
            x = np.where(ok, x, F(0))
            y = np.where(ok, y, F(0))
            x0f, y0f = np.floor(x), np.floor(y)
            fx, fy = x - x0f, y - y0f
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, wj - 1), np.minimum(y0 + 1, hj - 1)
            g00, g10, g01, g11 = (gj[yy, xx].astype(F) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
            top, bot = g00 + fx * (g10 - g00), g01 + fx * (g11 - g01)
            s = top + fy * (bot - top)
            a = g[py + dy, px + dx].astype(F)
            sb, sbb, sab = sb + s, sbb + s * s, sab + a * s
    va, vb, cov = saa - (sa * sa) / N, sbb - (sb * sb) / N, sab - (sa * sb) / N
    good = ok & (va >= N) & (vb >= N)
    c = np.clip(cov / np.sqrt(np.where(good, va * vb, F(1))), F(-1), F(1))
    return np.where(good, F(1) - c, F(2)).astype(F)


def plane_cost(V, i, px, py, r, n_best, rp, d, n, sa, saa):
    with np.errstate(all="ignore"):
        t = plane_offset(n, d, rp)
        costs = np.sort(np.stack([pair_cost(V, i, p, px, py, r, t, n, sa, saa) for p in V.nbs[i]]), axis=0)
        m = min(n_best, len(V.nbs[i]))
        total = np.zeros(len(px), F)
        for k in range(m):
            total = total + costs[k]
        return total / F(m)


def random_plane(V, i, rp, u0, u1, u2):
    inv = V.imin[i] + u0 * (V.imax[i] - V.imin[i])
    d = F(1) / inv
    n = normalize([F(2) * u1 - F(1), F(2) * u2 - F(1), np.full(len(u0), -1.0, F)])
    return d, face_camera(n, rp)


def estimated_grid(V, i, r):
    w, h = V.wh[i]
    ys, xs = np.mgrid[r:max(h - r, r), r:max(w - r, r)]
    return xs.reshape(-1).astype(np.int64), ys.reshape(-1).astype(np.int64)


def depthmap_ref(V, r=3, iterations=3, n_best=2, seed=0, init_depth=None, init_normal=None):
    """the maps of the whole call, flat: depth, normal, cost, and the counts"""
    depth, normal, cost = np.zeros(V.n_map, F), np.zeros((V.n_map, 3), F), np.zeros(V.n_map, F)
    n_est = n_inv = 0
    with np.errstate(all="ignore"):
        for i in range(V.n):
            if not V.active[i]:
                continue
            w, h = V.wh[i]
            D, Nn, Cc = np.zeros((h, w), F), np.zeros((h, w, 3), F), np.full((h, w), 2.0, F)
            px, py = estimated_grid(V, i, r)
            if len(px):
                idx = py * w + px
                base = pixel_seed(seed, i, idx)
                rp = mul_pixel(V.Ki[i], px.astype(F), py.astype(F))
                sa, saa = ref_sums(V.gray[i], px, py, r)
                if init_depth is not None:
                    d = np.asarray(init_depth, F)[V.map_off[i] + idx]
                    n3 = np.asarray(init_normal, F).reshape(-1, 3)[V.map_off[i] + idx]
                    n = [n3[:, 0], n3[:, 1], n3[:, 2]]
                else:
                    d, n = random_plane(V, i, rp, uniform(base, 0), uniform(base, 1), uniform(base, 2))
                D[py, px] = d
                Nn[py, px] = np.stack(n, -1)
                Cc[py, px] = plane_cost(V, i, px, py, r, n_best, rp, d, n, sa, saa)
            for it in range(iterations):
                for colour in (0, 1):
                    sel = ((px + py) & 1) == colour
                    if not sel.any():
                        continue
                    ax, ay = px[sel], py[sel]
                    base = pixel_seed(seed, i, ay * w + ax)
                    rp = mul_pixel(V.Ki[i], ax.astype(F), ay.astype(F))
                    sa, saa = ref_sums(V.gray[i], ax, ay, r)
                    d, c = D[ay, ax], Cc[ay, ax]
                    n = [Nn[ay, ax, k] for k in range(3)]
                    for ox, oy in OFFSETS:
                        sx, sy = ax + ox, ay + oy
                        est = (sx >= r) & (sx < w - r) & (sy >= r) & (sy < h - r)
                        sx, sy = np.where(est, sx, ax), np.where(est, sy, ay)
                        ns = [Nn[sy, sx, k] for k in range(3)]
                        rs = mul_pixel(V.Ki[i], sx.astype(F), sy.astype(F))
                        dp = plane_offset(ns, D[sy, sx], rs) / dot3(ns, rp)
                        est &= (dp >= V.dmin[i]) & (dp <= V.dmax[i])
                        cc = plane_cost(V, i, ax, ay, r, n_best, rp, dp, ns, sa, saa)
                        take = est & (cc < c)
                        c, d = np.where(take, cc, c), np.where(take, dp, d)
                        n = [np.where(take, ns[k], n[k]) for k in range(3)]
                    u = [uniform(base, 3 + 7 * it + k) for k in range(7)]
                    delta = F(0.1) / F(1 << it)
                    inv = F(1) / d + (delta * (F(2) * u[0] - F(1))) * (V.imax[i] - V.imin[i])
                    inv = np.where(inv < V.imin[i], V.imin[i], inv)
                    inv = np.where(inv > V.imax[i], V.imax[i], inv)
                    d2 = F(1) / inv
                    n2 = face_camera(normalize([n[k] + delta * (F(2) * u[1 + k] - F(1)) for k in range(3)]), rp)
                    for d2, n2 in ((d2, n2), random_plane(V, i, rp, u[4], u[5], u[6])):
                        cc = plane_cost(V, i, ax, ay, r, n_best, rp, d2, n2, sa, saa)
                        take = cc < c
                        c, d = np.where(take, cc, c), np.where(take, d2, d)
                        n = [np.where(take, n2[k], n[k]) for k in range(3)]
                    D[ay, ax], Cc[ay, ax] = d, c
                    Nn[ay, ax] = np.stack(n, -1)
            o = V.map_off[i]
            depth[o:o + w * h], normal[o:o + w * h], cost[o:o + w * h] = D.reshape(-1), Nn.reshape(-1, 3), Cc.reshape(-1)
            n_est += len(px)
            n_inv += int((Cc[py, px] >= 2).sum())
    return dict(depth=depth, normal=normal.reshape(-1), cost=cost, n_estimated=n_est, n_invalid=n_inv)


def filter_ref(V, depth, cost, max_cost=0.5, rel_tol=0.01, min_consistent=2):
    depth, cost = np.asarray(depth, F), np.asarray(cost, F)
    out, agree_out, counts = np.zeros(V.n_map, F), np.zeros(V.n_map, np.uint8), np.zeros((V.n, 2), np.int64)
    with np.errstate(all="ignore"):
        for i in range(V.n):
            w, h = V.wh[i]
            o = V.map_off[i]
            ys, xs = np.mgrid[0:h, 0:w]
            px, py = xs.reshape(-1), ys.reshape(-1)
            d = depth[o:o + w * h]
            cand = (d > 0) & (cost[o:o + w * h] <= F(max_cost))
            agree = np.zeros(w * h, np.int64)
            for j, A, b in V.nbs[i]:
                wj, hj = V.wh[j]
                ap = mul_pixel(A, px.astype(F), py.astype(F))
                h0, h1, z = d * ap[0] + b[0], d * ap[1] + b[1], d * ap[2] + b[2]
                x, y = np.floor(h0 / z + F(0.5)), np.floor(h1 / z + F(0.5))
                ok = (z > 0) & (x >= 0) & (x <= F(wj - 1)) & (y >= 0) & (y <= F(hj - 1))
                xi, yi = np.where(ok, x, 0).astype(np.int64), np.where(ok, y, 0).astype(np.int64)
                dj = depth[V.map_off[j] + yi * wj + xi]
                agree += ok & (dj > 0) & (np.abs(z - dj) <= F(rel_tol) * z)
            keep = cand & (agree >= min(min_consistent, len(V.nbs[i])))
            out[o:o + w * h] = np.where(keep, d, F(0))
            agree_out[o:o + w * h] = np.where(cand, agree, 0)
            counts[i] = int(cand.sum()), int(keep.sum())
    return dict(depth=out, n_agree=agree_out, counts=counts)


# ---- view selection -------------------------------------------------------------------
def views_select_ref(scene, opt_angle=10.0, min_angle=3.0, max_scale=1.6, range_margin=0.25, min_shared=10,
                     max_neighbors=4):
    K, plat = np.asarray(scene["K"], np.float64).reshape(-1, 9), scene["image_platform"]
    R, C = np.asarray(scene["R"], np.float64).reshape(-1, 9), np.asarray(scene["C"], np.float64).reshape(-1, 3)
    X, off, view = np.asarray(scene["vert_X"], np.float32).reshape(-1, 3), scene["vert_off"], scene["vert_view"]
    n = len(plat)
    score, angle, shared = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n), np.int64)
    zs = [[] for _ in range(n)]
    for v in range(len(off) - 1):
        x = [float(c) for c in X[v]]
        seen = [int(k) for k in view[off[v]:off[v + 1]]]
        z = {i: sum(R[i][6 + a] * (x[a] - C[i][a]) for a in range(3)) for i in seen}
        for i in seen:
            if z[i] > 0:
                zs[i].append(z[i])
        for i in seen:
            for j in seen:
                if i == j:
                    continue
                u, w = [C[i][a] - x[a] for a in range(3)], [C[j][a] - x[a] for a in range(3)]
                c = sum(u[a] * w[a] for a in range(3)) / (math.sqrt(sum(a * a for a in u)) * math.sqrt(sum(a * a for a in w)))
                theta = math.degrees(math.acos(max(-1.0, min(1.0, c))))
                s = (K[plat[i]][0] / z[i]) / (K[plat[j]][0] / z[j])
                w_scale = s * s if s < 1 else ((max_scale / s) ** 2 if s > max_scale else 1.0)
                score[i, j] += min(theta / opt_angle, 1.0) ** 1.5 * w_scale
                angle[i, j] += theta
                shared[i, j] += 1
    lists, scores, drange = [], [], np.zeros((n, 2), np.float32)
    for i in range(n):
        cand = [j for j in range(n) if j != i and shared[i, j] >= max(min_shared, 1)
                and angle[i, j] / shared[i, j] >= min_angle]
        cand = sorted(cand, key=lambda j: (-score[i, j], j))[:max_neighbors]
        lists.append(cand)
        scores.append([score[i, j] for j in cand])
        if cand and zs[i]:
            drange[i] = min(zs[i]) / (1 + range_margin), max(zs[i]) * (1 + range_margin)
    return lists, scores, drange


# ---- fixtures -------------------------------------------------------------------------
def texture(seed, contrast=1.0, cell=0.25):
    """tex(u, v) on the plane's own coordinates (one noise cell per `cell` units), 8-bit range"""
    noise = np.random.default_rng(seed).integers(0, 256, (64, 64)).astype(np.float64)

    def tex(u, v):
        a, b = u / cell + 32.0, v / cell + 32.0
        a0, b0 = np.floor(a), np.floor(b)
        fa, fb = a - a0, b - b0
        ia, ib = a0.astype(np.int64) % 64, b0.astype(np.int64) % 64
        ia1, ib1 = (ia + 1) % 64, (ib + 1) % 64
        t = ((1 - fa) * (1 - fb) * noise[ib, ia] + fa * (1 - fb) * noise[ib, ia1] + (1 - fa) * fb * noise[ib1, ia]
             + fa * fb * noise[ib1, ia1])
        t = 128.0 + contrast * (0.7 * (t - 128.0) + 25.0 * np.sin(9.0 * u + 2.0 * v) + 25.0 * np.sin(7.0 * v - 3.0 * u))
        return np.clip(np.rint(t), 0, 255).astype(np.uint8)
    return tex


def look_rotation(yaw):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, 0.0, -s], [0.0, 1.0, 0.0], [s, 0.0, c]])


class Fixture:
    """cameras on a baseline along x looking down +z at fronto-parallel planes
    z = near where x < 0 (a half plane in front, only when near is set) and z =
    far elsewhere; every image with every other as neighbours (at most n_nb)."""

    def __init__(self, w, h, centres, far=4.0, near=None, f=None, seed=1, yaws=None, channels=None, neighbours=None,
                 margin=0.25, cell=0.25, contrast=1.0):
        n = len(centres)
        self.n, self.w, self.h, self.near, self.far = n, w, h, near, far
        f = f if f is not None else 1.2 * w
        self.K = np.array([[f, 0, 0.5 * w - 0.5, 0, f, 0.5 * h - 0.5, 0, 0, 1.0]] * n).reshape(n, 3, 3)
        self.R = np.stack([look_rotation((yaws or [0.0] * n)[i]) for i in range(n)])
        self.C = np.array(centres, np.float64).reshape(n, 3)
        self.wh = np.array([w, h] * n, np.int32)
        tex = texture(seed, contrast, cell)
        self.images, self.gt_depth, self.gt_normal = [], [], []
        ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
        for i in range(n):
            ray_c = np.stack([(xs - self.K[i, 0, 2]) / f, (ys - self.K[i, 1, 2]) / f, np.ones_like(xs)], -1)
            ray_w = ray_c @ self.R[i]                 # R' applied to every ray
            lam_far = (far - self.C[i, 2]) / ray_w[..., 2]
            lam = lam_far
            if near is not None:
                lam_near = (near - self.C[i, 2]) / ray_w[..., 2]
                front = (self.C[i, 0] + lam_near * ray_w[..., 0]) < 0.0
                lam = np.where(front, lam_near, lam_far)
            Xw = self.C[i] + lam[..., None] * ray_w
            g = tex(Xw[..., 0] + 0.37 * Xw[..., 2], Xw[..., 1])
            ch = (channels or [1] * n)[i]
            self.images.append(g if ch == 1 else np.stack([g, g // 2 + 64, (3 * g.astype(np.int32) // 4).astype(np.uint8)], -1))
            self.gt_depth.append(lam.astype(F))
            nc = self.R[i] @ np.array([0.0, 0.0, -1.0])
            self.gt_normal.append(np.broadcast_to(nc.astype(F), (h, w, 3)).copy())
        nbs = neighbours if neighbours is not None else [[j for j in range(n) if j != i] for i in range(n)]
        self.nb_off = np.concatenate([[0], np.cumsum([len(a) for a in nbs])]).astype(np.int64)
        self.nb_view = np.array([j for a in nbs for j in a], np.int32)
        zs = [far] if near is None else [near, far]
        self.drange = np.array([[min(zs) / (1 + margin), max(zs) * (1 + margin)]] * n, F)

    def views(self):
        return Views(self.wh, self.K, self.R, self.C, self.nb_off, self.nb_view, self.drange, self.images)

    def run(self, ctx, opts=None, init=False):
        init_d = np.concatenate([d.reshape(-1) for d in self.gt_depth]) if init else None
        init_n = np.concatenate([m.reshape(-1) for m in self.gt_normal]) if init else None
        return api.depthmap(ctx, self.wh, self.K, self.R, self.C, self.nb_off, self.nb_view, self.drange, self.images,
                            opts, init_depth=init_d, init_normal=init_n)

    def filter(self, ctx, res, opts=None):
        return api.depthmap_filter(ctx, self.wh, self.K, self.R, self.C, self.nb_off, self.nb_view, res["depth"],
                                   res["cost"], opts)

    def reprojection_shift(self, i, depth):
        """per pixel: how far the estimate's projection into the widest-baseline
        neighbour lies from the ground truth's, in pixels"""
        nb = self.nb_view[self.nb_off[i]:self.nb_off[i + 1]]
        j = max(nb, key=lambda k: np.linalg.norm(self.C[k] - self.C[i]))
        ys, xs = np.mgrid[0:self.h, 0:self.w].astype(np.float64)
        ray = np.stack([xs, ys, np.ones_like(xs)], -1) @ np.linalg.inv(self.K[i]).T

        def project(d):
            Xw = (ray * d[..., None]) @ self.R[i] + self.C[i]
            p = (Xw - self.C[j]) @ self.R[j].T @ self.K[j].T
            return p[..., :2] / p[..., 2:3]
        return np.linalg.norm(project(depth.astype(np.float64)) - project(self.gt_depth[i].astype(np.float64)), axis=-1)


def step_band(fx, i, r):
    """the columns of image i within r of the step's edge (at most 2 r + 1 of them)"""
    edge = fx.K[i, 0, 2] + fx.K[i, 0, 0] * (0.0 - fx.C[i, 0]) / fx.near
    m = np.zeros((fx.h, fx.w), bool)
    m[:, np.abs(np.arange(fx.w) - edge) <= r] = True
    return m


def shares(fx, filtered, r, band=False):
    """(the share of the estimated pixels that the filter kept, the share of
    those that are correct: the depth error moves the projection in the
    widest-baseline neighbour by less than half a pixel)"""
    est = kept = good = 0
    for i in range(fx.n):
        d = filtered["depth_maps"][i]
        k = d > 0
        m = np.zeros_like(k)
        m[r:fx.h - r, r:fx.w - r] = True
        if band:
            b = step_band(fx, i, r)
            assert b.any(axis=0).sum() <= 2 * r + 1
            m &= ~b
        shift = fx.reprojection_shift(i, np.where(k, d, 1))
        est, kept, good = est + m.sum(), kept + (k & m).sum(), good + (k & m & (shift < 0.5)).sum()
    return kept / est, good / max(kept, 1)


def opts(r=3, iterations=3, n_best=2, seed=0, device_bytes=0):
    o = api.depthmap_default_options()
    o.half_window, o.iterations, o.n_best, o.seed, o.device_bytes = r, iterations, n_best, seed, device_bytes
    return o


def same_maps(a, b):
    for k in ("depth", "normal", "cost"):
        assert np.asarray(a[k], F).tobytes() == np.asarray(b[k], F).tobytes(), k


def check_against_ref(res, ref):
    same_maps(res, ref)
    assert res["stats"]["n_estimated"] == ref["n_estimated"] and res["stats"]["n_invalid"] == ref["n_invalid"]


def check_filter(res, ref):
    assert res["depth"].tobytes() == ref["depth"].tobytes() and res["n_agree"].tobytes() == ref["n_agree"].tobytes()
    assert np.array_equal(res["counts"], ref["counts"])
    assert res["stats"]["n_candidates"] == ref["counts"][:, 0].sum() and res["stats"]["n_kept"] == ref["counts"][:, 1].sum()


@functools.lru_cache(maxsize=None)
def small_fixture():
    """24 x 20, three views (two neighbours each), r = 2"""
    return Fixture(24, 20, [(-0.25, 0, 0), (0, 0, 0), (0.3, 0.02, 0)], far=4.0, seed=11)


@functools.lru_cache(maxsize=None)
def plane_fixture():
    """the accuracy fixture: 48 x 40, three views, the defaults"""
    return Fixture(48, 40, [(-0.35, 0, 0), (0, 0, 0), (0.35, 0.03, 0)], far=4.0, seed=5, cell=0.4)


@functools.lru_cache(maxsize=None)
def step_fixture():
    """two planes at different depths meeting in a vertical step at world x = 0"""
    return Fixture(48, 40, [(-0.3, 0, 0), (0, 0, 0), (0.3, 0.03, 0)], far=4.3, near=3.7, seed=6, cell=0.5)


@functools.lru_cache(maxsize=None)
def reference(name, r, iterations, seed, init):
    fx = dict(small=small_fixture, plane=plane_fixture, step=step_fixture)[name]()
    init_d = np.concatenate([d.reshape(-1) for d in fx.gt_depth]) if init else None
    init_n = np.concatenate([m.reshape(-1) for m in fx.gt_normal]) if init else None
    return depthmap_ref(fx.views(), r, iterations, 2, seed, init_d, init_n)


class Merged:
    """several fixtures in one call (their neighbour indices shifted), optionally
    with images taken out (not loaded) or left without neighbours"""

    def __init__(self, fixtures, unloaded=(), alone=()):
        self.images, nbs, at = [], [], 0
        for fx in fixtures:
            for i in range(fx.n):
                self.images.append(fx.images[i])
                nbs.append([at + int(j) for j in fx.nb_view[fx.nb_off[i]:fx.nb_off[i + 1]]])
            at += fx.n
        for i in unloaded:
            self.images[i] = None
        for i in alone:
            nbs[i] = []
        self.n = at
        self.wh = np.concatenate([fx.wh for fx in fixtures])
        self.K, self.R = np.concatenate([fx.K for fx in fixtures]), np.concatenate([fx.R for fx in fixtures])
        self.C = np.concatenate([fx.C for fx in fixtures])
        self.drange = np.concatenate([fx.drange for fx in fixtures])
        self.nb_off = np.concatenate([[0], np.cumsum([len(a) for a in nbs])]).astype(np.int64)
        self.nb_view = np.array([j for a in nbs for j in a], np.int32)

    def views(self):
        return Views(self.wh, self.K, self.R, self.C, self.nb_off, self.nb_view, self.drange, self.images)

    def run(self, ctx, opts=None):
        return api.depthmap(ctx, self.wh, self.K, self.R, self.C, self.nb_off, self.nb_view, self.drange, self.images, opts)

    def filter(self, ctx, res, opts=None):
        return api.depthmap_filter(ctx, self.wh, self.K, self.R, self.C, self.nb_off, self.nb_view, res["depth"],
                                   res["cost"], opts)
