"""Reference for the texturing tests (test_texture.py, test_texture_gpu.py): a
numpy restatement of the contract in include/sfmcore.h ("Mesh texture"),
written from that comment: integers are Python ints or int64, floats are
np.float32 with every operation separate, so every comparison is for equality.
Also the scene builders: cameras whose pixels are world units, strips of small
faces, quads, fans, an occluder in front of a wall.  Each reference is computed
once per scene and shared."""
import functools

import numpy as np

import _depthmap_helpers as DH

abi, api = DH.abi, DH.api
F = np.float32
LIMIT = F(1048576.0)


# ---- the restatement ------------------------------------------------------------------
def view_constants(K, R, C):
    k = [float(a) for a in np.asarray(K, np.float64).reshape(-1)]
    r = [float(a) for a in np.asarray(R, np.float64).reshape(-1)]
    M = np.array([k[3 * a] * r[b] + k[3 * a + 1] * r[3 + b] + k[3 * a + 2] * r[6 + b] for a in range(3) for b in range(3)],
                 np.float64).astype(F)
    return M, np.asarray(C, np.float64).reshape(-1).astype(F)


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def project(M, Cf, X):
    """X: three float32 arrays -> h0 / z, h1 / z, z"""
    q = [X[c] - Cf[c] for c in range(3)]
    with np.errstate(all="ignore"):
        h0, h1, z = dot3(M[0:3], q), dot3(M[3:6], q), dot3(M[6:9], q)
        return h0 / z, h1 / z, z


def edge_inclusive(dx, dy):
    return dy > 0 or (dy == 0 and dx > 0)


def face_in_view(M, Cf, w, h, P):
    """P [3, 3] float32: None when not drawable, else dict(X, Y (Python ints, exchanged), wz, A2, box, inside, front)"""
    x, y, z = project(M, Cf, [P[:, c] for c in range(3)])
    with np.errstate(all="ignore"):
        if not ((z > 0).all() and (np.abs(x) <= LIMIT).all() and (np.abs(y) <= LIMIT).all()):
            return None
    X = [int(np.floor(v * F(16.0) + F(0.5))) for v in x]
    Y = [int(np.floor(v * F(16.0) + F(0.5))) for v in y]
    wz = [F(1.0) / v for v in z]
    inside = bool(((x >= 0) & (x <= F(w - 1)) & (y >= 0) & (y <= F(h - 1))).all())
    e1, e2 = P[1] - P[0], P[2] - P[0]
    n = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
    front = bool(dot3(n, Cf - P[0]) > 0)
    A2 = (X[1] - X[0]) * (Y[2] - Y[0]) - (X[2] - X[0]) * (Y[1] - Y[0])
    if A2 < 0:
        X[1], X[2], Y[1], Y[2], wz[1], wz[2], A2 = X[2], X[1], Y[2], Y[1], wz[2], wz[1], -A2
    box = (max(-(-min(X) // 16), 0), min(max(X) // 16, w - 1), max(-(-min(Y) // 16), 0), min(max(Y) // 16, h - 1))
    return dict(X=X, Y=Y, wz=wz, A2=A2, box=box, inside=inside, front=front)


def face_pixels_in_view(fc, face):
    """the covered pixels of a drawable face: (py, px) int arrays and their keys (uint64)"""
    px0, px1, py0, py1 = fc["box"]
    if fc["A2"] == 0 or px0 > px1 or py0 > py1:
        return None
    py, px = np.mgrid[py0:py1 + 1, px0:px1 + 1].astype(np.int64)
    X, Y = fc["X"], fc["Y"]
    cover, E = np.ones(px.shape, bool), []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        dx, dy = X[b] - X[a], Y[b] - Y[a]
        e = np.int64(dx) * (16 * py - Y[a]) - np.int64(dy) * (16 * px - X[a])
        cover &= (e > 0) | ((e == 0) & edge_inclusive(dx, dy))
        E.append(e)
    py, px, E = py[cover], px[cover], [e[cover] for e in E]
    with np.errstate(all="ignore"):
        num = (E[0].astype(F) * fc["wz"][0] + E[1].astype(F) * fc["wz"][1]) + E[2].astype(F) * fc["wz"][2]
        d = np.array([fc["A2"]], np.int64).astype(F) / num
    key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(face)
    return py, px, key


def face_views_ref(wh, K, R, C, V, tri, loaded=None):
    """dict(face_view, face_pixels, n_not_drawable, covered [n_img, n], won [n_img, n], eligible [n_img, n])"""
    wh = np.asarray(wh, np.int32).reshape(-1, 2)
    V, tri = np.asarray(V, F).reshape(-1, 3), np.asarray(tri, np.int32).reshape(-1, 3)
    n_img, n = len(wh), len(tri)
    covered, won = np.zeros((n_img, n), np.int64), np.zeros((n_img, n), np.int64)
    eligible = np.zeros((n_img, n), bool)
    refused = 0
    for v in range(n_img):
        if loaded is not None and not loaded[v]:
            continue
        w, h = int(wh[v, 0]), int(wh[v, 1])
        M, Cf = view_constants(K[v], R[v], C[v])
        ident = np.full((h, w), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
        faces = []
        for f in range(n):
            fc = face_in_view(M, Cf, w, h, V[tri[f]])
            refused += fc is None
            pix = face_pixels_in_view(fc, f) if fc is not None else None
            faces.append((fc, pix))
            if pix is not None and len(pix[0]):
                ident[pix[0], pix[1]] = np.minimum(ident[pix[0], pix[1]], pix[2])
        for f, (fc, pix) in enumerate(faces):
            if pix is None:
                continue
            covered[v, f] = len(pix[0])
            won[v, f] = int(((ident[pix[0], pix[1]] & np.uint64(0xFFFFFFFF)) == np.uint64(f)).sum())
            eligible[v, f] = fc["front"] and fc["inside"] and covered[v, f] >= 1 and won[v, f] == covered[v, f]
    face_view, face_pixels = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for v in range(n_img):
        better = eligible[v] & (covered[v] > face_pixels)
        face_view[better], face_pixels[better] = v, covered[v][better]
    return dict(face_view=face_view, face_pixels=face_pixels, n_not_drawable=refused, covered=covered, won=won,
                eligible=eligible, n_textured=int((face_view >= 0).sum()), sum_pixels=int(face_pixels.sum()))


def atlas_ref(n_triangles, s):
    n_sq = (n_triangles + 1) // 2
    cols = 0
    while cols * cols < n_sq:
        cols += 1
    rows = -(-n_sq // cols) if cols else 0
    return cols * s, rows * s, cols


def texel_faces(n_triangles, s):
    """per texel of the atlas: face (or -1), half, a, b, l1, l2"""
    W, H, cols = atlas_ref(n_triangles, s)
    ty, tx = np.mgrid[0:H, 0:W].astype(np.int64)
    a, b = tx % s, ty % s
    half = (a + b > s - 2).astype(np.int64)
    f = 2 * ((ty // s) * cols + tx // s) + half
    f[f >= n_triangles] = -1
    den = F(s - 3)
    l1 = np.where(half == 1, s - 1 - a, a).astype(F) / den
    l2 = np.where(half == 1, s - 1 - b, b).astype(F) / den
    return f, half, a, b, l1, l2


def corners_ref(n_triangles, s):
    """[n, 3, 2] float32: the corners in texel units from the atlas's origin"""
    W, H, cols = atlas_ref(n_triangles, s)
    out = np.zeros((n_triangles, 3, 2), F)
    for f in range(n_triangles):
        ox, oy = F(((f // 2) % cols) * s), F(((f // 2) // cols) * s)
        c = ((F(0.5), F(0.5)), (F(s) - F(2.5), F(0.5)), (F(0.5), F(s) - F(2.5))) if f % 2 == 0 else (
            (F(s) - F(0.5), F(s) - F(0.5)), (F(2.5), F(s) - F(0.5)), (F(s) - F(0.5), F(2.5)))
        for k in range(3):
            out[f, k] = (ox + c[k][0], oy + c[k][1])
    return out


def uv_ref(n_triangles, s):
    W, H, _ = atlas_ref(n_triangles, s)
    c = corners_ref(n_triangles, s)
    uv = np.zeros((n_triangles, 3, 2), F)
    if n_triangles:
        uv[:, :, 0] = c[:, :, 0] / F(W)
        uv[:, :, 1] = F(1.0) - c[:, :, 1] / F(H)
    return uv


def round_byte(val):
    return np.floor(val + F(0.5)).astype(np.uint8)


def bake_ref(wh, K, R, C, V, tri, face_view, images, vertex_rgb=None, s=8, fill=(0, 0, 0)):
    """dict(texture [H, W, 3], uv [n, 3, 2])"""
    wh = np.asarray(wh, np.int32).reshape(-1, 2)
    V, tri = np.asarray(V, F).reshape(-1, 3), np.asarray(tri, np.int32).reshape(-1, 3)
    n = len(tri)
    W, H, _ = atlas_ref(n, s)
    f, half, a, b, l1, l2 = texel_faces(n, s)
    tex = np.empty((H, W, 3), np.uint8)
    tex[:] = np.asarray(fill, np.uint8)
    fv = np.asarray(face_view, np.int32)
    view = np.where(f >= 0, fv[np.maximum(f, 0)] if n else 0, -2)
    for v in sorted(set(view[view >= 0].tolist())):
        m = view == v
        ff, a1, a2 = f[m], l1[m], l2[m]
        P0, P1, P2 = (V[tri[ff, k]] for k in range(3))
        P = [(P0[:, c] + a1 * (P1[:, c] - P0[:, c])) + a2 * (P2[:, c] - P0[:, c]) for c in range(3)]
        M, Cf = view_constants(K[v], R[v], C[v])
        w, h = int(wh[v, 0]), int(wh[v, 1])
        xr, yr, z = project(M, Cf, P)
        ok = z > 0
        with np.errstate(all="ignore"):
            x = np.minimum(np.maximum(xr, F(0.0)), F(w - 1))
            y = np.minimum(np.maximum(yr, F(0.0)), F(h - 1))
        x, y = np.where(ok, x, F(0.0)), np.where(ok, y, F(0.0))
        gx, gy = np.floor(x), np.floor(y)
        dx, dy = x - gx, y - gy
        gx, gy = gx.astype(np.int64), gy.astype(np.int64)
        gx1, gy1 = np.minimum(gx + 1, w - 1), np.minimum(gy + 1, h - 1)
        im = np.asarray(images[v], np.uint8)
        im = (im.reshape(h, w, -1) if im.ndim == 3 else im.reshape(h, w, 1)).astype(F)
        if im.shape[2] == 1:
            im = np.repeat(im, 3, axis=2)
        p00, p10, p01, p11 = im[gy, gx], im[gy, gx1], im[gy1, gx], im[gy1, gx1]
        top = p00 + dx[:, None] * (p10 - p00)
        bot = p01 + dx[:, None] * (p11 - p01)
        val = round_byte(top + dy[:, None] * (bot - top))
        val[~ok] = np.asarray(fill, np.uint8)
        tex[m] = val
    if vertex_rgb is not None:
        m = view == -1
        ff, a1, a2 = f[m], l1[m], l2[m]
        c0, c1, c2 = (np.asarray(vertex_rgb, np.uint8).reshape(-1, 3)[tri[ff, k]].astype(F) for k in range(3))
        val = (c0 + a1[:, None] * (c1 - c0)) + a2[:, None] * (c2 - c0)
        tex[m] = round_byte(np.minimum(np.maximum(val, F(0.0)), F(255.0)))
    return dict(texture=tex, uv=uv_ref(n, s))


# ---- integer geometry for the tests ---------------------------------------------------
def polygon_centres(poly, w, h):
    """Pixel centres of a w x h image inside the convex polygon poly (integer pixel
    corners, in the order that makes every face's A2 positive), by the tie rule
    applied to the polygon's own edges."""
    n = 0
    for py in range(h):
        for px in range(w):
            ok = True
            for (xa, ya), (xb, yb) in zip(poly, poly[1:] + poly[:1]):
                dx, dy = xb - xa, yb - ya
                e = dx * (py - ya) - dy * (px - xa)
                ok = ok and (e > 0 or (e == 0 and edge_inclusive(dx, dy)))
            n += ok
    return n


def footprint_touched(s, a, b):
    """Does a bilinear fetch somewhere in half 0's closed UV triangle x >= 0.5, y >= 0.5,
    x + y <= s - 2 read texel (a, b) with a weight above 0?  The fetch at x reads texel a
    when a - 0.5 < x < a + 1.5.  In half texels, integers only: the least x is max(2a - 1,
    1), attained only where the triangle's own closed bound gives it."""
    if a < 0 or b < 0:                      # x < a + 1.5 <= 0.5: outside the triangle
        return False
    xl, yl = max(2 * a - 1, 1), max(2 * b - 1, 1)
    attained = 2 * a - 1 < 1 and 2 * b - 1 < 1
    return xl + yl < 2 * s - 4 or (xl + yl == 2 * s - 4 and attained)


def footprint_clean(s):
    """Every texel that a fetch inside a face's UV triangle reads belongs to that face's
    half of the square.  Half 1 is half 0 under (a, b) -> (s - 1 - a, s - 1 - b)."""
    for a in range(-2, s + 2):
        for b in range(-2, s + 2):
            if footprint_touched(s, a, b) and not (0 <= a < s and 0 <= b < s and a + b <= s - 2):
                return False             # half 0 reads a texel that is not its own
            a1, b1 = s - 1 - a, s - 1 - b
            if footprint_touched(s, a, b) and not (0 <= a1 < s and 0 <= b1 < s and a1 + b1 > s - 2):
                return False             # half 1, mirrored
    return True


# ---- scenes ---------------------------------------------------------------------------
class Scene:
    """Cameras with K = [f 0 0; 0 f 0; 0 0 1] and R = I: a point (X, Y, f) is seen at
    pixel (X - Cx, Y - Cy)."""

    def __init__(self, sizes, centres, V, tri, f=4.0, images=None, vertex_rgb=None, seed=0):
        self.wh = np.array(sizes, np.int32).reshape(-1, 2)
        n = len(self.wh)
        self.K = np.tile(np.array([f, 0, 0, 0, f, 0, 0, 0, 1], np.float64), (n, 1))
        self.R = np.tile(np.eye(3).reshape(-1), (n, 1))
        self.C = np.array(centres, np.float64).reshape(n, 3)
        self.V = np.asarray(V, F).reshape(-1, 3)
        self.tri = np.asarray(tri, np.int32).reshape(-1, 3)
        rng = np.random.default_rng(seed)
        if images is None:
            images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for w, h in self.wh]
        self.images = images
        self.vertex_rgb = vertex_rgb
        self.loaded = [im is not None for im in images]

    def cam(self):
        return (self.wh, self.K, self.R, self.C, self.V, self.tri)

    def views(self, ctx, opts=None):
        return api.mesh_face_views(ctx, *self.cam(), images=self.images, opts=opts)

    def bake(self, ctx, face_view, opts=None):
        return api.mesh_texture_bake(ctx, *self.cam(), face_view, images=self.images, vertex_rgb=self.vertex_rgb, opts=opts)

    def texture(self, ctx, opts=None, views=True):
        return api.mesh_texture(ctx, *self.cam(), images=self.images, vertex_rgb=self.vertex_rgb, opts=opts, views=views)

    def views_ref(self):
        return face_views_ref(self.wh, self.K, self.R, self.C, self.V, self.tri, self.loaded)

    def bake_ref(self, face_view, s=8, fill=(0, 0, 0)):
        return bake_ref(self.wh, self.K, self.R, self.C, self.V, self.tri, face_view, self.images, self.vertex_rgb, s, fill)


def opts(cell=8, fill=(0, 0, 0), device_bytes=0):
    o = api.mesh_texture_default_options()
    o.cell = cell
    o.fill[:] = list(fill)
    o.device_bytes = device_bytes
    return o


def quad(x0, y0, x1, y1, z=4.0, flip=False, diagonal=0):
    """two faces over the rectangle; the winding looks at a camera at z = 0 unless flip"""
    V = [(x0, y0, z), (x1, y0, z), (x1, y1, z), (x0, y1, z)]
    tri = [(0, 2, 1), (0, 3, 2)] if diagonal == 0 else [(0, 3, 1), (1, 3, 2)]
    if flip:
        tri = [(a, c, b) for a, b, c in tri]
    return V, tri


def merge(*meshes):
    V, tri = [], []
    for v, t in meshes:
        tri += [tuple(i + len(V) for i in f) for f in t]
        V += list(v)
    return V, tri


def strip_mesh(n_faces, pitch=2.5, per_row=24, x0=1.25, y0=0.75, size=2.25, z=4.0):
    """n_faces small faces, two a quad (the last quad keeps one when n_faces is odd), each quad with its own vertices"""
    V, tri = [], []
    for q in range((n_faces + 1) // 2):
        x, y = x0 + pitch * (q % per_row), y0 + pitch * (q // per_row)
        v, t = quad(x, y, x + size, y + size, z + 0.125 * (q % 3))
        tri += [tuple(i + len(V) for i in f) for f in t]
        V += v
    return V, tri[:n_faces]


@functools.lru_cache(maxsize=None)
def strip_scene(n_faces, size=(64, 48), two_views=True):
    V, tri = strip_mesh(n_faces)
    sizes = [size, size] if two_views else [size]
    centres = [(0, 0, 0), (0.375, 0.25, 0)] if two_views else [(0, 0, 0)]
    return Scene(sizes, centres, V, tri, seed=n_faces)


@functools.lru_cache(maxsize=None)
def named_scene(name):
    if name == "occlusion":      # a near quad in front of a wall of 4 x 3 quads, two views with parallax
        wall = merge(*[quad(4 + 12 * i, 4 + 12 * j, 16 + 12 * i, 16 + 12 * j, 8.0) for j in range(3) for i in range(4)])
        V, tri = merge(wall, quad(10, 6, 18, 14, 4.0))
        return Scene([(32, 24), (32, 24)], [(0, 0, 0), (-8, 0, 0)], V, tri, seed=1)
    if name == "backfacing":     # the near quad looks away: never eligible, but it hides the wall behind it
        V, tri = merge(quad(8, 8, 48, 40, 8.0), quad(6, 6, 12, 12, 4.0, flip=True))
        return Scene([(32, 24)], [(0, 0, 0)], V, tri, seed=2)
    if name == "not_drawable":   # a vertex behind the camera; a projection beyond 2^20 pixels
        V, tri = merge(quad(2, 2, 8, 8), ([(3, 3, 4), (9, 3, 4), (3, 9, -1)], [(0, 2, 1)]),
                       ([(3, 3, 4), (3.0e6, 3, 4), (3, 9, 4)], [(0, 2, 1)]))
        return Scene([(16, 12), (16, 12)], [(0, 0, 0), (1, 0, 0)], V, tri, seed=3)
    if name == "tie":            # two identical cameras
        V, tri = quad(2.5, 1.5, 12.25, 9.75)
        return Scene([(16, 12), (16, 12)], [(0, 0, 0), (0, 0, 0)], V, tri, seed=4)
    if name == "skipped":
        V, tri = quad(2.5, 1.5, 12.25, 9.75)
        sc = Scene([(16, 12), (16, 12), (16, 12)], [(0, 0, 0), (0, 0, 0), (0.5, 0, 0)], V, tri, seed=5)
        sc.images[0] = None
        sc.loaded[0] = False
        return sc
    if name == "mixed":          # a 1-channel image beside a 3-channel image; each quad is inside one view only
        V, tri = merge(quad(2, 2, 9, 9), quad(22, 2, 29, 9))
        sc = Scene([(16, 12), (17, 12)], [(0, 0, 0), (15, 0, 0)], V, tri, seed=6)
        sc.images[0] = sc.images[0][:, :, 0].copy()
        return sc
    if name == "large":          # one face pair over a whole 64 x 48 image, and a small quad in front of it
        V, tri = merge(quad(0, 0, 63, 47, 4.0), quad(40, 30, 90, 70, 8.0))
        return Scene([(64, 48)], [(0, 0, 0)], V, tri, seed=7)
    if name == "subpixel":       # faces smaller than a pixel, between the pixel centres
        V, tri = merge(*[quad(2.25 + i, 3.25, 2.75 + i, 3.75) for i in range(5)])
        return Scene([(16, 12)], [(0, 0, 0)], V, tri, seed=8)
    if name == "threshold":      # clipped boxes of 256 and of 272 pixels: either side of the wavefront path
        V, tri = merge(quad(1, 1, 16, 16), quad(20, 1, 36, 16))
        return Scene([(64, 48)], [(0, 0, 0)], V, tri, seed=9)
    raise KeyError(name)


def check_views(res, ref):
    assert np.array_equal(res["face_view"], ref["face_view"])
    assert np.array_equal(res["face_pixels"], ref["face_pixels"])
    st = res["stats"]
    assert st["n_textured"] == ref["n_textured"] and st["n_untextured"] == len(ref["face_view"]) - ref["n_textured"]
    assert st["n_not_drawable"] == ref["n_not_drawable"] and st["sum_pixels"] == ref["sum_pixels"]


def check_bake(res, ref):
    assert res["texture"].shape == ref["texture"].shape
    assert res["texture"].tobytes() == ref["texture"].tobytes()
    assert res["uv"].tobytes() == ref["uv"].tobytes()


def same_texture(a, b):
    assert a["texture"].tobytes() == b["texture"].tobytes() and a["uv"].tobytes() == b["uv"].tobytes()
    if "face_view" in a and "face_view" in b:
        assert a["face_view"].tobytes() == b["face_view"].tobytes() and a["face_pixels"].tobytes() == b["face_pixels"].tobytes()


def read_textured_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode().split("\n")
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[-1])
    V = np.frombuffer(body[:12 * nv], "<f4").reshape(-1, 3)
    rec = np.frombuffer(body[12 * nv:], np.dtype([("n", "u1"), ("tri", "<i4", 3), ("m", "u1"), ("uv", "<f4", 6)]))
    return lines, V, rec, nf, len(head) + len(b"end_header\n")
