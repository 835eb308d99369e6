"""Reference for the mesh tests (test_mesh.py, test_mesh_gpu.py): a numpy
float32 restatement of the contract in include/sfmcore.h ("Mesh"), written from
that comment: the integration of depth maps into a TSDF, the marching
tetrahedra table derived from the orientation rule in integer arithmetic, the
extraction with its vertex and triangle order, a topology check and a PLY
reader.  numpy does these IEEE operations one by one, without fusing, so every
comparison is for equality.  Each reference is computed once and shared."""
import functools
import itertools

import numpy as np

import _depthmap_helpers as DH
import _fuse_helpers as FH

abi, api = DH.abi, DH.api
F = np.float32
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))      # xyz xzy yxz yzx zxy zyx
SLOT_OFFSETS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))


class Grid:
    def __init__(self, origin, voxel, dims):
        self.origin = np.asarray(origin, F)
        self.voxel = F(voxel)
        self.dims = tuple(int(d) for d in dims)
        self.n = self.dims[0] * self.dims[1] * self.dims[2]

    def c(self):
        return api.mesh_grid(self.origin, self.voxel, self.dims)

    def positions(self):
        """[nz, ny, nx] float32 arrays of x, y, z: origin_c + (float)i_c * voxel"""
        nx, ny, nz = self.dims
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        return [self.origin[c] + a.astype(F) * self.voxel for c, a in enumerate((i, j, k))]


# ---- integration ----------------------------------------------------------------------
def integrate_ref(wh, K, R, C, depth, grid, images=None, trunc=0.0):
    wh = np.asarray(wh, np.int32).reshape(-1)
    n_img = len(wh) // 2
    depth = np.asarray(depth, F).reshape(-1)
    trunc = F(trunc) if trunc > 0 else F(3.0) * grid.voxel
    X = [a.reshape(-1) for a in grid.positions()]
    total, count = np.zeros(grid.n, F), np.zeros(grid.n, np.int64)
    col, m = np.zeros((grid.n, 3), np.int64), np.zeros(grid.n, np.int64)
    at = 0
    with np.errstate(all="ignore"):
        for v in range(n_img):
            w, h = int(wh[2 * v]), int(wh[2 * v + 1])
            d_img, at = depth[at:at + w * h], at + w * h
            if images is not None and images[v] is None:
                continue
            k = [float(a) for a in np.asarray(K[v], np.float64).reshape(-1)]
            r = [float(a) for a in np.asarray(R[v], np.float64).reshape(-1)]
            M = np.array([k[3 * a] * r[b] + k[3 * a + 1] * r[3 + b] + k[3 * a + 2] * r[6 + b]
                          for a in range(3) for b in range(3)], np.float64).astype(F)
            Cf = np.asarray(C[v], np.float64).reshape(-1).astype(F)
            q = [X[c] - Cf[c] for c in range(3)]
            h0, h1, z = DH.dot3(M[0:3], q), DH.dot3(M[3:6], q), DH.dot3(M[6:9], q)
            x, y = np.floor(h0 / z + F(0.5)), np.floor(h1 / z + F(0.5))
            ok = (z > 0) & (x >= 0) & (x <= F(w - 1)) & (y >= 0) & (y <= F(h - 1))
            idx = np.where(ok, y, 0).astype(np.int64) * w + np.where(ok, x, 0).astype(np.int64)
            d = d_img[idx]
            sd = d - z
            ok &= (d > 0) & ~(sd < -trunc)
            t = np.where(sd < trunc, sd, trunc) / trunc
            total = np.where(ok, total + t, total)
            count += ok
            if images is not None:
                im = np.asarray(images[v], np.uint8)
                im = im.reshape(-1, 1) if im.ndim == 2 or im.shape[-1] == 1 else im.reshape(-1, 3)
                near = ok & (np.abs(sd) <= trunc)
                col += np.where(near[:, None], np.broadcast_to(im[idx], (grid.n, 3)).astype(np.int64), 0)
                m += near
        tsdf = np.where(count > 0, total / np.maximum(count, 1).astype(F), F(0)).astype(F)
    out = dict(tsdf=tsdf, weight=np.minimum(count, 255).astype(np.uint8), rgb=None, has_rgb=None,
               n_observed=int((count > 0).sum()))
    if images is not None:
        mm = np.maximum(m, 1)[:, None]
        out["rgb"] = np.where(m[:, None] > 0, (2 * col + mm) // (2 * mm), 0).astype(np.uint8)
        out["has_rgb"] = (m > 0).astype(np.uint8)
    return out


# ---- the case table from the orientation rule -----------------------------------------
def tet_corners(t):
    """the four corners of tetrahedron t as integer points of the unit cell"""
    p = PERMS[t]
    c = [np.zeros(3, np.int64)]
    for axis in p:
        nxt = c[-1].copy()
        nxt[axis] += 1
        c.append(nxt)
    return c


@functools.lru_cache(maxsize=None)
def case_table():
    """table[t][case] = list of triangles, each three edges (n, m), n < m, over the
    tetrahedron's corners; case bit n: corner n is inside"""
    table = []
    for t in range(6):
        P = tet_corners(t)
        row = []
        for cs in range(16):
            ins = [n for n in range(4) if (cs >> n) & 1]
            outs = [n for n in range(4) if not (cs >> n) & 1]
            e = lambda a, b: (min(a, b), max(a, b))
            if len(ins) in (1, 3):
                a = ins[0] if len(ins) == 1 else outs[0]
                b, c, d = outs if len(ins) == 1 else ins
                tris = [[e(a, b), e(a, c), e(a, d)]]
            elif len(ins) == 2:
                (a1, a2), (b1, b2) = ins, outs
                q = [e(a1, b1), e(a1, b2), e(a2, b2), e(a2, b1)]
                tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
            else:
                tris = []
            fixed = []
            for tri in tris:
                # twice the midpoints; len(ins) len(outs) times the direction: all integers
                A, B, Cc = (P[n] + P[m] for n, m in tri)
                direction = len(ins) * sum(P[n] for n in outs) - len(outs) * sum(P[n] for n in ins)
                dot = int(np.dot(np.cross(B - A, Cc - A), direction))
                assert dot != 0
                fixed.append(tri if dot > 0 else [tri[0], tri[2], tri[1]])
            row.append(fixed)
        table.append(row)
    return table


# ---- extraction -----------------------------------------------------------------------
def _shift(a, dx, dy, dz, fill=False):
    """b[k, j, i] = a[k + dz, j + dy, i + dx], `fill` outside"""
    out = np.full_like(a, fill)
    nz, ny, nx = a.shape

    def rng(n, d):
        return (slice(max(-d, 0), n - max(d, 0)), slice(max(d, 0), n - max(-d, 0)))
    (zt, zs), (yt, ys), (xt, xs) = rng(nz, dz), rng(ny, dy), rng(nx, dx)
    out[zt, yt, xt] = a[zs, ys, xs]
    return out


def extract_ref(grid, tsdf, weight, rgb=None, has_rgb=None, min_weight=1):
    nx, ny, nz = grid.dims
    T = np.asarray(tsdf, F).reshape(nz, ny, nx)
    obs = np.asarray(weight, np.uint8).reshape(nz, ny, nx) >= min_weight
    inside = obs & (T < 0)
    live = np.ones_like(obs)
    for dx, dy, dz in itertools.product((0, 1), repeat=3):
        live &= _shift(obs, dx, dy, dz)
    carries = np.zeros((nz, ny, nx, 7), bool)
    for s, (dx, dy, dz) in enumerate(SLOT_OFFSETS):
        used = np.zeros_like(obs)
        for ex, ey, ez in itertools.product((0, 1), repeat=3):
            if ex * dx + ey * dy + ez * dz == 0:
                used |= _shift(live, -ex, -ey, -ez)
        carries[..., s] = obs & _shift(obs, dx, dy, dz) & (inside != _shift(inside, dx, dy, dz)) & used
    flat = carries.reshape(-1, 7)
    vid = (np.cumsum(flat.reshape(-1)) - 1).reshape(-1, 7)
    owner, slot = np.nonzero(flat)
    # the vertices
    pos = [a.reshape(-1) for a in grid.positions()]
    off = np.array([dx + nx * (dy + ny * dz) for dx, dy, dz in SLOT_OFFSETS], np.int64)
    a, b = owner, owner + off[slot]
    tf = T.reshape(-1)
    with np.errstate(all="ignore"):
        u = tf[a] / (tf[a] - tf[b])
        V = np.stack([pos[c][a] + u * (pos[c][b] - pos[c][a]) for c in range(3)], -1).astype(F)
    vrgb = None
    if rgb is not None:
        rgb, has = np.asarray(rgb, np.uint8).reshape(-1, 3), np.asarray(has_rgb, np.uint8).reshape(-1) != 0
        first, second = np.where(u < F(0.5), a, b), np.where(u < F(0.5), b, a)
        src = np.where(has[first], first, second)
        vrgb = np.where(has[src][:, None], rgb[src], 0).astype(np.uint8)
    # the triangles
    cells = np.nonzero(live.reshape(-1))[0]
    table = case_table()
    corner_off = lambda p: int(p[0]) + nx * (int(p[1]) + ny * int(p[2]))
    slot_of = {o: s for s, o in enumerate(SLOT_OFFSETS)}
    tri = np.zeros((len(cells), 6, 2, 3), np.int64)
    valid = np.zeros((len(cells), 6, 2), bool)
    degenerate = 0
    ins_f, zero_f = inside.reshape(-1), (tf == 0)
    for t in range(6):
        P = tet_corners(t)
        cs = sum(ins_f[cells + corner_off(P[n])].astype(np.int64) << n for n in range(4))
        for case in range(1, 15):
            sel = np.nonzero(cs == case)[0]
            if not len(sel):
                continue
            for k, edges in enumerate(table[t][case]):
                ends = np.zeros((len(sel), 4), np.int64)
                for v, (n, m) in enumerate(edges):
                    own = cells[sel] + corner_off(P[n])
                    tri[sel, t, k, v] = vid[own, slot_of[tuple(int(x) for x in P[m] - P[n])]]
                    for q in (n, m):
                        ends[:, q] += zero_f[cells[sel] + corner_off(P[q])]
                valid[sel, t, k] = True
                degenerate += int((ends >= 2).any(axis=1).sum())
    return dict(V=V, rgb=vrgb, tri=tri[valid].astype(np.int32), n_vertices=len(V), n_triangles=int(valid.sum()),
                n_degenerate=degenerate, owner=owner, slot=slot, cells=cells)


def mesh_topology(tri):
    """the undirected edges used once, twice and more often, whether a directed
    edge repeats, and V - E + F over the vertices that the triangles name"""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    d = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    _, dc = np.unique(d, axis=0, return_counts=True)
    und, uc = np.unique(np.sort(d, axis=1), axis=0, return_counts=True)
    return dict(once=und[uc == 1], twice=und[uc == 2], more=und[uc > 2], directed_repeats=bool((dc > 1).any()),
                euler=len(np.unique(tri)) - len(und) + len(tri))


def signed_volume(V, tri):
    P = np.asarray(V, np.float64)[np.asarray(tri, np.int64)]
    return float(np.einsum("ij,ij->i", P[:, 0], np.cross(P[:, 1], P[:, 2])).sum() / 6.0)


def rule_direction_dots(grid, tsdf, res):
    """per triangle: the dot product of its float64 normal with (mean of the
    outside corners - mean of the inside corners) of its tetrahedron; the
    triangles of `res` must be those of extract_ref on a fully live volume, whose
    order (cell, tetrahedron, triangle) is walked again here"""
    nx, ny, nz = grid.dims
    T = np.asarray(tsdf, F).reshape(-1)
    pos = np.stack([a.reshape(-1) for a in grid.positions()], -1).astype(np.float64)
    V, out, at = np.asarray(res["V"], np.float64), [], 0
    for cell in res["cells"]:
        for t in range(6):
            P = tet_corners(t)
            idx = [cell + int(p[0]) + nx * (int(p[1]) + ny * int(p[2])) for p in P]
            ins = [n for n in range(4) if T[idx[n]] < 0]
            outs = [n for n in range(4) if not T[idx[n]] < 0]
            for _ in range({0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[len(ins)]):
                A, B, Cc = V[res["tri"][at]]
                direction = pos[[idx[n] for n in outs]].mean(0) - pos[[idx[n] for n in ins]].mean(0)
                out.append(float(np.dot(np.cross(B - A, Cc - A), direction)))
                at += 1
    assert at == len(res["tri"])
    return np.array(out)


def read_mesh_ply(path):
    """(header lines, vertex records, faces [m, 3]) of a binary little-endian PLY with triangular faces"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")[:-1]
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    face_at = next(k for k, ln in enumerate(lines) if ln.startswith("element face"))
    n, m = int(lines[2].split()[2]), int(lines[face_at].split()[2])
    types = dict(float="<f4", uchar="u1")
    dt = np.dtype([(ln.split()[2], types[ln.split()[1]]) for ln in lines[3:face_at]])
    assert lines[face_at + 1] == "property list uchar int vertex_indices"
    verts = np.frombuffer(raw[end:end + n * dt.itemsize], dt)
    ft = np.dtype([("n", "u1"), ("v", "<i4", 3)])
    faces = np.frombuffer(raw[end + n * dt.itemsize:], ft)
    assert len(faces) == m and len(raw) == end + n * dt.itemsize + m * ft.itemsize and (faces["n"] == 3).all()
    return lines, verts, faces["v"]


# ---- comparing ------------------------------------------------------------------------
def same_volume(a, b):
    for k in ("tsdf", "weight", "rgb", "has_rgb"):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k


def same_mesh(a, b):
    for k in ("V", "rgb", "tri"):
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
            continue
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), k


def check_mesh(res, ref):
    same_mesh(res, ref)
    st = res["stats"]
    assert (st["n_vertices"], st["n_triangles"], st["n_degenerate"]) == (
        ref["n_vertices"], ref["n_triangles"], ref["n_degenerate"])


def check_volume(res, ref):
    same_volume(res, ref)
    assert res["stats"]["n_observed"] == ref["n_observed"]


def referenced(res):
    return len(np.unique(res["tri"])) == len(res["V"])


# ---- fixtures -------------------------------------------------------------------------
class Volume:
    """a hand-made volume: tsdf, weight and optionally colours over a grid"""

    def __init__(self, grid, tsdf, weight=None, rgb=None, has_rgb=None):
        self.grid = grid
        self.tsdf = np.ascontiguousarray(np.asarray(tsdf, F).reshape(-1))
        self.weight = np.ones(grid.n, np.uint8) if weight is None else np.asarray(weight, np.uint8).reshape(-1)
        self.rgb, self.has_rgb = rgb, has_rgb

    def run(self, ctx, opts=None):
        return api.mesh_extract(ctx, self.grid.c(), self.tsdf, self.weight, self.rgb, self.has_rgb, opts)

    @functools.lru_cache(maxsize=None)
    def ref(self, min_weight=1):
        return extract_ref(self.grid, self.tsdf, self.weight, self.rgb, self.has_rgb, min_weight)


def mesh_opts(min_weight=1):
    o = api.mesh_default_options()
    o.min_weight = min_weight
    return o


def tsdf_opts(trunc=0.0, device_bytes=0):
    o = api.tsdf_default_options()
    o.trunc, o.device_bytes = trunc, device_bytes
    return o


@functools.lru_cache(maxsize=None)
def config_volume():
    """(768, 2, 2): cell c at x = 3 c, 3 c + 1 has corner configuration c, with
    non-zero values of varied size; the plane x = 3 c + 2 is unobserved"""
    g = Grid((0.0, 0.0, 0.0), 0.5, (768, 2, 2))
    t, w = np.zeros((2, 2, 768), F), np.ones((2, 2, 768), np.uint8)
    w[:, :, 2::3] = 0
    for c in range(256):
        for corner in range(8):
            dx, dy, dz = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
            mag = F(0.125) + F(0.0625) * F((c * 7 + corner * 3) % 11)
            t[dz, dy, 3 * c + dx] = -mag if (c >> corner) & 1 else mag
    col = np.random.default_rng(3).integers(0, 256, (g.n, 3)).astype(np.uint8)
    has = (np.arange(g.n) % 5 != 0).astype(np.uint8)
    return Volume(g, t, w, col, has)


def _distance_grid():
    return Grid((-1.0, -0.875, -0.75), 0.125, (17, 15, 13))


@functools.lru_cache(maxsize=None)
def sphere_volume(slab=False):
    g = _distance_grid()
    x, y, z = (a.astype(np.float64) for a in g.positions())
    t = (np.sqrt((x - 0.03) ** 2 + (y - 0.02) ** 2 + (z + 0.01) ** 2) - 0.61).astype(F)
    w = np.full(g.n, 2, np.uint8).reshape(13, 15, 17)
    if slab:
        w[:, :, 8] = 0     # the plane i = 8 is unobserved: the sphere is cut open
    return Volume(g, t, w)


@functools.lru_cache(maxsize=None)
def torus_volume():
    g = _distance_grid()
    x, y, z = (a.astype(np.float64) for a in g.positions())
    ring = np.sqrt((x - 0.03) ** 2 + (y - 0.02) ** 2) - 0.55
    return Volume(g, (np.sqrt(ring ** 2 + (z + 0.01) ** 2) - 0.21).astype(F))


def tilted_plane_volume(dims):
    """a plane through the middle of the lattice, tilted so that it crosses every row of cells"""
    g = Grid((-0.3, 0.2, 1.0), 0.25, dims)
    x, y, z = (a.astype(np.float64) for a in g.positions())
    mid = [float(g.origin[c]) + 0.5 * float(g.voxel) * (dims[c] - 1) for c in range(3)]
    t = 0.05 * (x - mid[0]) + 0.21 * (y - mid[1]) + (z - mid[2]) + 0.013
    return Volume(g, t.astype(F))


def emit_volume(pattern):
    """513 x 2 x 2, outside everywhere except one inside corner in chosen cells:
    'lane0': the cell at lane 0 of every block of 256, 'lane63': at lane 63 of
    every wavefront, 'last': the last cell, 'none': no crossing"""
    g = Grid((0.0, 0.0, 0.0), 1.0, (513, 2, 2))
    t = np.full((2, 2, 513), 0.5, F)
    cells = dict(lane0=[0, 256], lane63=list(range(63, 512, 64)), last=[511], none=[])[pattern]
    for i in cells:
        t[0, 0, i] = F(-0.25)
    return Volume(g, t)


class PlaneScene:
    """views of the plane z = 4 with exact depths, R = I, translated in x and y
    only, and a lattice around the plane whose z planes miss z = 4 by half a voxel"""

    def __init__(self, fixtures, unloaded=(), colours=True, dims=(33, 25, 16), voxel=0.0625):
        self.sc = FH.Scene(fixtures, unloaded=unloaded, colours=colours)
        self.grid = Grid((-1.0, -0.75, 4.0 - (dims[2] / 2 - 0.5) * voxel), voxel, dims)
        self.far = 4.0

    def args(self):
        s = self.sc
        return (s.wh, s.K, s.R, s.C, s.depth, self.grid.c())

    def run(self, ctx, opts=None):
        return api.tsdf_integrate(ctx, *self.args(), images=self.sc.images, opts=opts)

    def ref(self, trunc=0.0):
        s = self.sc
        return integrate_ref(s.wh, s.K, s.R, s.C, s.depth, self.grid, s.images, trunc)


@functools.lru_cache(maxsize=None)
def plane_scene(colours=True, unloaded=()):
    return PlaneScene([DH.plane_fixture()], unloaded=unloaded, colours=colours)


@functools.lru_cache(maxsize=None)
def nine_scene():
    """9 images of three sizes (one and three channels), image 4 unloaded"""
    groups = [FH.group(24, 20, channels=[1, 3, 1]), FH.group(17, 13, seed=3), FH.group(31, 9, channels=[3, 3, 1], seed=4)]
    return PlaneScene(groups, unloaded=(4,), dims=(21, 13, 10), voxel=0.125)


@functools.lru_cache(maxsize=None)
def integration_ref(name, trunc=0.0):
    return integration_scene(name).ref(trunc)


def integration_scene(name):
    return dict(colour=lambda: plane_scene(True), plain=lambda: plane_scene(False),
                unloaded=lambda: plane_scene(True, (1,)), nine=nine_scene)[name]()
