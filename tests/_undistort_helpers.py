"""Reference for the undistortion tests (test_undistort.py,
test_undistort_gpu.py): a numpy restatement of the per-pixel contract in
include/sfmcore.h ("Dense hand-off"), float64 and float32 operations in the
stated order (numpy does these IEEE operations one by one, without fusing, so
the comparison is for equality), a random-image generator, a byte pool with odd
offsets and sentinel bytes between the images, and the named cases the CPU and
the GPU tests share (each reference is computed once)."""
import functools

import numpy as np

import _helpers as H
import _wash_helpers as W

abi, api = H.abi, W.api
RADIAL3, PINHOLE, SNAVELY = abi.SFM_CAM_RADIAL3, abi.SFM_CAM_PINHOLE, abi.SFM_CAM_SNAVELY
GAP, UNTOUCHED = 0xA5, 0x5A     # sentinels: between the images of `pixels`, and all of `out` before a call


def random_image(rng, w, h, ch):
    return rng.integers(0, 256, (h, w) if ch == 1 else (h, w, 3), dtype=np.uint8)


def source_xy(w, h, k):
    """(x, y, inside) of every output pixel, [h, w]"""
    f, ppx, ppy, k1, k2, k3 = (np.float64(v) for v in k)
    i = np.broadcast_to(np.arange(w, dtype=np.float64)[None, :], (h, w))
    j = np.broadcast_to(np.arange(h, dtype=np.float64)[:, None], (h, w))
    with np.errstate(all="ignore"):
        px, py = (i - ppx) / f, (j - ppy) / f
        r2 = px * px + py * py
        r4 = r2 * r2
        r6 = r4 * r2
        c = 1.0 + k1 * r2 + k2 * r4 + k3 * r6
        x, y = f * (px * c) + ppx, f * (py * c) + ppy
        inside = (x > -1.0) & (x < w) & (y > -1.0) & (y < h)
    return x, y, inside


def undistort_ref(img, k, fill=(0, 0, 0)):
    """the undistorted image and dict(n_outside, n_low_weight, x, y, inside, low)"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    ch = 1 if img.ndim == 2 else img.shape[2]
    src = img.reshape(h, w, ch).astype(np.float64)
    x, y, inside = source_xy(w, h, k)
    xf = np.where(inside, x, 0.0).astype(np.float32)
    yf = np.where(inside, y, 0.0).astype(np.float32)
    gxf, gyf = np.floor(xf), np.floor(yf)
    dx, dy = xf.astype(np.float64) - gxf.astype(np.float64), yf.astype(np.float64) - gyf.astype(np.float64)
    gx, gy = gxf.astype(np.int64), gyf.astype(np.int64)
    wx, wy = (1.0 - dx, dx), (1.0 - dy, dy)
    res, total = np.zeros((h, w, ch)), np.zeros((h, w))
    for a in (0, 1):                                  # rows outer, columns inner
        yy = gy + a
        for b in (0, 1):
            xx = gx + b
            ok = inside & (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
            wgt = wx[b] * wy[a]
            pix = src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]
            res = res + np.where(ok[..., None], pix * wgt[..., None], 0.0)     # (adding 0.0 changes nothing)
            total = total + np.where(ok, wgt, 0.0)
    low = inside & (total <= 0.2)
    with np.errstate(all="ignore"):
        res = np.where((total != 1.0)[..., None], res / total[..., None], res)
    byte = np.where((inside & ~low)[..., None], res + 0.5, 0.0).astype(np.uint8)
    out = np.where(inside[..., None], byte, np.asarray(fill, np.uint8)[None, None, :ch])
    return out.reshape(img.shape), dict(n_outside=int((~inside).sum()), n_low_weight=int(low.sum()), x=x, y=y,
                                        inside=inside, low=low)


def make_pool(images, gaps=None):
    """(channels, img_off, pixels): images[i] None is not loaded; gaps[i] sentinel
    bytes before image i (odd numbers give odd offsets) and gaps[-1] after the last"""
    n = len(images)
    gaps = [0] * (n + 1) if gaps is None else gaps
    channels, img_off, parts, at = np.ones(max(n, 1), np.int32), np.full(max(n, 1), -1, np.int64), [], 0
    for i, im in enumerate(images):
        parts.append(np.full(gaps[i], GAP, np.uint8))
        at += gaps[i]
        if im is None:
            continue
        im = np.ascontiguousarray(im, np.uint8)
        channels[i] = 1 if im.ndim == 2 else im.shape[2]
        img_off[i] = at
        parts.append(im.reshape(-1))
        at += im.size
    parts.append(np.full(gaps[n], GAP, np.uint8))
    pixels = np.concatenate(parts) if at + gaps[n] else np.zeros(1, np.uint8)
    return channels, img_off, pixels


class Batch:
    """images (None: not loaded; a placeholder size then), their cameras, and
    the reference of the whole call: the expected `out` pool and counts"""

    def __init__(self, images, sizes, img_intr, intr, fill=(0, 0, 0), gaps=None, model=RADIAL3):
        self.images, self.model, self.fill = images, model, fill
        self.wh = np.array(sizes, np.int32).reshape(-1)
        self.img_intr = np.array(img_intr, np.int32)
        self.intr = np.array(intr, np.float64).reshape(-1)
        self.pool = make_pool(images, gaps)
        self.want = np.full(len(self.pool[2]), UNTOUCHED, np.uint8)
        self.refs = []
        self.counts = dict(n_images=0, n_copied=0, n_pixels=0, n_outside=0, n_low_weight=0)
        for i, im in enumerate(images):
            if im is None:
                self.refs.append(None)
                continue
            self.counts["n_images"] += 1
            if model == PINHOLE:
                ref, info = im, None
                self.counts["n_copied"] += 1
            else:
                ref, info = undistort_ref(im, self.intr.reshape(-1, 6)[self.img_intr[i]], fill)
                self.counts["n_pixels"] += im.shape[0] * im.shape[1]
                self.counts["n_outside"] += info["n_outside"]
                self.counts["n_low_weight"] += info["n_low_weight"]
            self.refs.append(info)
            off = self.pool[1][i]
            self.want[off:off + im.size] = np.asarray(ref).reshape(-1)

    def opts(self, chunk_bytes=0):
        o = api.undistort_default_options()
        o.chunk_bytes = chunk_bytes
        o.fill[0], o.fill[1], o.fill[2] = self.fill
        return o

    def run(self, ctx, chunk_bytes=0):
        out = np.full(len(self.pool[2]), UNTOUCHED, np.uint8)
        return api.undistort(ctx, self.model, self.img_intr, self.intr, self.wh, opts=self.opts(chunk_bytes),
                             pool=self.pool, out=out)

    def check(self, res):
        """the bytes of the whole pool (sentinels outside the images included) and the counts"""
        assert res["out"].tobytes() == self.want.tobytes()
        for f, v in self.counts.items():
            assert res["stats"][f] == v, (f, res["stats"][f], v)


def same_result(a, b):
    assert a["out"].tobytes() == b["out"].tobytes()
    for f in ("n_images", "n_copied", "n_pixels", "n_outside", "n_low_weight", "n_chunks"):
        assert a["stats"][f] == b["stats"][f], f


def one_image(seed, w, h, ch, k, fill=(0, 0, 0)):
    return Batch([random_image(np.random.default_rng(seed), w, h, ch)], [w, h], [0], k, fill)


K_STRONG = (60.0, 33.5, 20.5, 0.8, 0.0, 0.0)
K_BARREL = (60.0, 33.5, 20.5, -0.25, 0.0, 0.0)
K_MIXED = (60.0, 33.5, 20.5, 0.3, -0.2, 0.1)


@functools.lru_cache(maxsize=None)
def case(name, ch):
    """the cases of the issue, by name and channel count"""
    if name == "strong":
        return one_image(1, 67, 41, ch, K_STRONG)
    if name == "barrel":
        return one_image(2, 67, 41, ch, K_BARREL)
    if name == "mixed_k":
        return one_image(3, 67, 41, ch, K_MIXED)
    if name == "tiny":
        return one_image(4, 5, 3, ch, (4.0, 2.5, 1.5, 0.5, 0.0, 0.0))
    if name == "one_pixel":
        return one_image(5, 1, 1, ch, (1.0, 0.5, 0.5, 0.1, 0.0, 0.0))
    if name == "identity":
        return one_image(6, 61, 47, ch, (61.37, 30.123, 22.987, 0.0, 0.0, 0.0))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mixed_batch(fill=(0, 0, 0)):
    """several sizes, both channel counts, odd offsets, two intrinsics blocks, an unloaded image in the middle"""
    rng = np.random.default_rng(7)
    shapes = [(67, 41, 3), (30, 50, 1), (40, 40, 3), (67, 41, 1), (9, 7, 3)]
    images = [random_image(rng, *s) for s in shapes]
    images[2] = None
    intr = [60.0, 33.5, 20.5, 0.8, 0.0, 0.0, 35.0, 14.2, 26.9, 0.3, -0.2, 0.1]
    return Batch(images, [s[:2] for s in shapes], [0, 1, 1, 0, 1], intr, fill, gaps=[3, 5, 0, 7, 1, 9])
