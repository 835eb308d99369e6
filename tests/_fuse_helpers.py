"""Reference for the fusion tests (test_depthfuse.py, test_depthfuse_gpu.py): a
numpy float32 restatement of the contract in include/sfmcore.h ("Dense
fusion"), written from that comment: the fusion pair lists, the fate rule, the
fused values, the CSR expansion of the view lists, and a PLY reader.  numpy
does these IEEE operations one by one, without fusing, so every comparison is
for equality.  The fixtures are _depthmap_helpers' rendered planes, whose
depths and normals are analytic, so agreement is controlled by hand."""
import functools

import numpy as np

import _depthmap_helpers as DH

abi, api = DH.abi, DH.api
F = np.float32
MAX_PAIRS = 32
NONE, EMITTED, SUPPRESSED = 0, 1, 2


# ---- the contract ---------------------------------------------------------------------
def pair_lists(n_img, nb_off, nb_view):
    """per image its fusion pair list, and how many entries were dropped"""
    own = [[int(j) for j in nb_view[int(nb_off[i]):int(nb_off[i + 1])]] for i in range(n_img)]
    lists, dropped = [], 0
    for i in range(n_img):
        full = own[i] + [j for j in range(n_img) if i in own[j] and j not in own[i]]
        dropped += max(len(full) - MAX_PAIRS, 0)
        lists.append(full[:MAX_PAIRS])
    return lists, dropped


def rot_t(Rf, v):
    """R' v, R row-major float32"""
    return [(Rf[c] * v[0] + Rf[3 + c] * v[1]) + Rf[6 + c] * v[2] for c in range(3)]


class Problem:
    def __init__(self, wh, K, R, C, nb_off, nb_view, depth, normal, images=None):
        wh = np.asarray(wh, np.int32).reshape(-1)
        self.n = len(wh) // 2
        self.lists, self.dropped = pair_lists(self.n, nb_off, nb_view)
        off = np.concatenate([[0], np.cumsum([len(a) for a in self.lists])]).astype(np.int64)
        flat = np.array([j for a in self.lists for j in a], np.int32)
        # the double-precision part (Ki, A, b) is the depth maps': the same formulas over the fusion lists
        self.V = DH.Views(wh, K, R, C, off, flat)
        self.Rf = [np.asarray(R[i], np.float64).reshape(-1).astype(F) for i in range(self.n)]
        self.Cf = [np.asarray(C[i], np.float64).reshape(-1).astype(F) for i in range(self.n)]
        self.colours = images is not None
        self.loaded = [images is None or images[i] is not None for i in range(self.n)]
        self.images = images
        depth, normal = np.asarray(depth, F).reshape(-1), np.asarray(normal, F).reshape(-1, 3)
        self.d, self.nrm = [], []
        for i, (w, h) in enumerate(self.V.wh):
            o = self.V.map_off[i]
            self.d.append(depth[o:o + w * h] if self.loaded[i] else np.zeros(w * h, F))
            self.nrm.append(normal[o:o + w * h])

    def world_normal(self, i, idx):
        n = self.nrm[i][idx]
        return rot_t(self.Rf[i], [n[:, 0], n[:, 1], n[:, 2]])

    def world_point(self, i, idx, d):
        w = self.V.wh[i][0]
        ray = DH.mul_pixel(self.V.Ki[i], (idx % w).astype(F), (idx // w).astype(F))
        v = rot_t(self.Rf[i], [d * ray[0], d * ray[1], d * ray[2]])
        return [v[c] + self.Cf[i][c] for c in range(3)]

    def rgb(self, i, idx):
        if self.images[i] is None:
            return np.zeros((len(idx), 3), np.int64)
        im = np.asarray(self.images[i], np.uint8)
        im = im.reshape(-1, 1) if im.ndim == 2 or im.shape[-1] == 1 else im.reshape(-1, 3)
        return np.broadcast_to(im[idx], (len(idx), 3)).astype(np.int64)


def fuse_ref(wh, K, R, C, nb_off, nb_view, depth, normal, images=None, rel_tol=0.01, min_normal_cos=-1.0):
    """the cloud and the counts; also per image the fates and, for the chain
    check, the lowest agreeing image and the pixel it was hit at"""
    P = Problem(wh, K, R, C, nb_off, nb_view, depth, normal, images)
    out = dict(X=[], N=[], rgb=[], n_views=[], view_mask=[], src_image=[], src_pixel=[])
    fates, low_j, low_q = [], [], []
    with np.errstate(all="ignore"):
        for i in range(P.n):
            w, h = P.V.wh[i]
            idx = np.arange(w * h, dtype=np.int64)
            px, py = (idx % w).astype(F), (idx // w).astype(F)
            d = P.d[i]
            valid = d > 0
            Ni = P.world_normal(i, idx)
            agree, hit = [], []
            lj, lq = np.full(w * h, P.n, np.int64), np.full(w * h, -1, np.int64)
            for j, A, b in P.V.nbs[i]:
                wj, hj = P.V.wh[j]
                ap = DH.mul_pixel(A, px, py)
                h0, h1, z = d * ap[0] + b[0], d * ap[1] + b[1], d * ap[2] + b[2]
                x, y = np.floor(h0 / z + F(0.5)), np.floor(h1 / z + F(0.5))
                ok = valid & (z > 0) & (x >= 0) & (x <= F(wj - 1)) & (y >= 0) & (y <= F(hj - 1))
                q = np.where(ok, y, 0).astype(np.int64) * wj + np.where(ok, x, 0).astype(np.int64)
                dj = P.d[j][q]
                ok &= (dj > 0) & (np.abs(z - dj) <= F(rel_tol) * z)
                if min_normal_cos > -1:
                    ok &= DH.dot3(Ni, P.world_normal(j, q)) >= F(min_normal_cos)
                agree.append(ok)
                hit.append(q)
                better = ok & (j < lj)
                lj, lq = np.where(better, j, lj), np.where(better, q, lq)
            fate = np.where(valid, np.where(lj < i, SUPPRESSED, EMITTED), NONE)
            fates.append(fate)
            low_j.append(lj)
            low_q.append(lq)
            e = np.nonzero(fate == EMITTED)[0]
            sx, sn = P.world_point(i, e, d[e]), [c[e] for c in Ni]
            own = [c.copy() for c in sn]
            col = P.rgb(i, e) if P.colours else None
            m, mask = np.ones(len(e), np.int64), np.zeros(len(e), np.uint32)
            for k, (j, A, b) in enumerate(P.V.nbs[i]):
                a, q = agree[k][e], hit[k][e]
                xj, nj = P.world_point(j, q, P.d[j][q]), P.world_normal(j, q)
                sx = [np.where(a, sx[c] + xj[c], sx[c]) for c in range(3)]
                sn = [np.where(a, sn[c] + nj[c], sn[c]) for c in range(3)]
                if P.colours and a.any():
                    qq = np.where(a, q, 0)
                    col = col + np.where(a[:, None], P.rgb(j, qq), 0)
                m += a
                mask |= (a.astype(np.uint32) << np.uint32(k))
            fm = m.astype(F)
            ln = np.sqrt((sn[0] * sn[0] + sn[1] * sn[1]) + sn[2] * sn[2])
            out["X"].append(np.stack([sx[c] / fm for c in range(3)], -1).astype(F))
            out["N"].append(np.stack([np.where(ln > 0, sn[c] / ln, own[c]) for c in range(3)], -1).astype(F))
            if P.colours:
                out["rgb"].append(((2 * col + m[:, None]) // (2 * m[:, None])).astype(np.uint8))
            out["n_views"].append(m.astype(np.uint8))
            out["view_mask"].append(mask)
            out["src_image"].append(np.full(len(e), i, np.int32))
            out["src_pixel"].append(e.astype(np.int32))
    res = {k: (np.concatenate(v) if v else None) for k, v in out.items()}
    res.update(fates=fates, low_j=low_j, low_q=low_q, lists=P.lists,
               n_points=len(res["src_image"]), n_suppressed=int(sum((f == SUPPRESSED).sum() for f in fates)),
               n_pairs_dropped=P.dropped)
    return res


def views_ref(lists, src_image, view_mask):
    off, idx = [0], []
    for i, m in zip(src_image, view_mask):
        idx.append(int(i))
        idx += [lists[int(i)][k] for k in range(32) if (int(m) >> k) & 1]
        off.append(len(idx))
    return np.array(off, np.int64), np.array(idx, np.int32)


def read_ply(path):
    """(header lines, dict of columns) of a binary little-endian vertex-only PLY"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")[:-1]
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int(lines[2].split()[2])
    types = dict(float="<f4", uchar="u1")
    dt = np.dtype([(ln.split()[2], types[ln.split()[1]]) for ln in lines if ln.startswith("property")])
    body = np.frombuffer(raw[end:], dt)
    assert len(body) == n and len(raw) == end + n * dt.itemsize
    return lines, body


# ---- comparing ------------------------------------------------------------------------
KEYS = ("X", "N", "rgb", "n_views", "view_mask", "src_image", "src_pixel")


def same_cloud(a, b, keys=KEYS):
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k


def check_against_ref(res, ref):
    same_cloud(res, ref)
    st = res["stats"]
    assert (st["n_points"], st["n_suppressed"], st["n_pairs_dropped"]) == (
        ref["n_points"], ref["n_suppressed"], ref["n_pairs_dropped"])


# ---- fixtures -------------------------------------------------------------------------
class Scene:
    """several fixtures in one call, with the maps given by hand: the exact
    depths and normals of the rendered planes unless replaced"""

    def __init__(self, fixtures, unloaded=(), alone=(), colours=True):
        m = DH.Merged(fixtures, unloaded, alone)
        self.m, self.n = m, m.n
        self.wh, self.K, self.R, self.C, self.nb_off, self.nb_view = m.wh, m.K, m.R, m.C, m.nb_off, m.nb_view
        self.images = m.images if colours else None
        self.depth_maps = [d.copy() for fx in fixtures for d in fx.gt_depth]
        self.normal_maps = [g.copy() for fx in fixtures for g in fx.gt_normal]

    @property
    def depth(self):
        return np.concatenate([d.reshape(-1) for d in self.depth_maps]).astype(F)

    @property
    def normal(self):
        return np.concatenate([g.reshape(-1) for g in self.normal_maps]).astype(F)

    def keep_only(self, i, idx):
        """image i keeps its depth at the raster indices idx only"""
        d = self.depth_maps[i].reshape(-1)
        keep = np.zeros(len(d), bool)
        keep[np.asarray(idx, np.int64)] = True
        d[~keep] = 0

    def args(self):
        return (self.wh, self.K, self.R, self.C, self.nb_off, self.nb_view, self.depth, self.normal)

    def run(self, ctx, opts=None):
        return api.depthmap_fuse(ctx, *self.args(), images=self.images, opts=opts)

    def ref(self, rel_tol=0.01, min_normal_cos=-1.0):
        return fuse_ref(*self.args(), images=self.images, rel_tol=rel_tol, min_normal_cos=min_normal_cos)


def fuse_opts(rel_tol=0.01, min_normal_cos=-1.0, device_bytes=0):
    o = api.depthmap_fuse_default_options()
    o.rel_tol, o.min_normal_cos, o.device_bytes = rel_tol, min_normal_cos, device_bytes
    return o


def group(w, h, n=3, channels=None, seed=2, f=None):
    """n views of w x h on a baseline looking at the plane z = 4, every view with every other"""
    step = 0.12
    return DH.Fixture(w, h, [(step * k, 0.01 * k, 0) for k in range(n)], far=4.0, seed=seed, channels=channels,
                      f=f if f is not None else 1.2 * max(w, 8))


def star_fixture():
    """34 images of 8 x 6 that all list image 0 (which lists nobody): image 0 has 33 reverse pairs"""
    n = 34
    return DH.Fixture(8, 6, [(0.01 * k, 0, 0) for k in range(n)], far=4.0, seed=4,
                      neighbours=[[]] + [[0] for _ in range(n - 1)])


@functools.lru_cache(maxsize=None)
def estimated(name, r, iterations, seed):
    """fixture (a): a §5k fixture estimated and filtered by the host twins
    (whose bytes test_depthmap.py pins), once"""
    fx = dict(plane=DH.plane_fixture, small=DH.small_fixture)[name]()
    est = fx.run(None, DH.opts(r=r, iterations=iterations, seed=seed))
    flt = fx.filter(None, est)
    return fx, est, flt
