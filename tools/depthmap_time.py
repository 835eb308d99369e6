"""Times sfm_depthmap on one GPU: 8 synthetic views of 1024 x 768 on a circle
segment looking at a textured plane, 4 neighbours each, default options.
Prints the kernel time (stats seconds[1], HIP events) and the wall time of
calls 2-4, the host twin's wall time once (--host), and the kernel's rate in
patch samples per second (patch samples x hypotheses x neighbours x pixels).
Then sfm_depthmap_fuse over the filtered maps (four calls; the host twin once
with --host, bytes compared), its kernel time against the byte bound of one
read of depth, normal and mask plus one write of the cloud, and sfm_densify
against the three separate calls, alternating, --rounds each.

    python tools/depthmap_time.py [--host] [--views 8] [--size 1024 768]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
api = importlib.import_module("3dreconstruction_amd.api")


def scene(n, w, h, seed=1):
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (h // 4 + 64, w // 4 + 64)).astype(np.float32)
    f, far = 1.2 * w, 4.0
    K = np.array([[f, 0, 0.5 * w - 0.5, 0, f, 0.5 * h - 0.5, 0, 0, 1.0]] * n).reshape(n, 3, 3)
    R = np.stack([np.eye(3)] * n)
    C = np.array([[0.12 * (i - 0.5 * (n - 1)), 0.01 * (i % 2), 0.0] for i in range(n)])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    images = []
    for i in range(n):
        # the plane z = far: plane coordinates of every pixel, in quarter-pixel noise cells
        u = (C[i, 0] * f / far + xs) / 4.0 + 32.0
        v = (C[i, 1] * f / far + ys) / 4.0 + 32.0
        u0, v0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
        fu, fv = u - u0, v - v0
        u0, v0 = np.clip(u0, 0, noise.shape[1] - 2), np.clip(v0, 0, noise.shape[0] - 2)
        t = ((1 - fu) * (1 - fv) * noise[v0, u0] + fu * (1 - fv) * noise[v0, u0 + 1] + (1 - fu) * fv * noise[v0 + 1, u0]
             + fu * fv * noise[v0 + 1, u0 + 1])
        images.append(np.clip(np.rint(t), 0, 255).astype(np.uint8))
    nbs = [sorted(range(n), key=lambda j: (abs(j - i), j))[1:5] for i in range(n)]
    nb_off = np.concatenate([[0], np.cumsum([len(a) for a in nbs])]).astype(np.int64)
    nb_view = np.array([j for a in nbs for j in a], np.int32)
    drange = np.array([[far / 1.25, far * 1.25]] * n, np.float32)
    return np.array([w, h] * n, np.int32), K, R, C, nb_off, nb_view, drange, images


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="also time sfm_depthmap_host once")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=[1024, 768])
    ap.add_argument("--rounds", type=int, default=3, help="rounds of densify against the three calls")
    a = ap.parse_args()
    w, h = a.size
    args = scene(a.views, w, h)
    o = api.depthmap_default_options()
    r, its = o.half_window, o.iterations
    hyps = 1 + 10 * its        # the initial plane, then up to 8 propagated + 2 random planes per iteration
    samples = (2 * r + 1) ** 2 * hyps * 4 * (w - 2 * r) * (h - 2 * r) * a.views
    out = dict(views=a.views, size=[w, h], samples_upper=samples, calls=[])
    ctx = api.Context(0)
    pool = api._pixel_pool(args[7])
    dev = None
    for call in range(4):
        t0 = time.perf_counter()
        dev = api.depthmap(ctx, *args[:7], opts=o, pool=pool)
        wall = time.perf_counter() - t0
        s = dev["stats"]["seconds"]
        out["calls"].append(dict(wall_s=wall, upload_s=s[0], kernels_s=s[1], download_s=s[2],
                                 samples_per_s=samples / s[1] if s[1] > 0 else None))
    out["n_estimated"], out["n_invalid"] = dev["stats"]["n_estimated"], dev["stats"]["n_invalid"]
    t0 = time.perf_counter()
    f = api.depthmap_filter(ctx, *args[:6], dev["depth"], dev["cost"])
    out["filter"] = dict(wall_s=time.perf_counter() - t0, kernels_s=f["stats"]["seconds"][1], n_kept=f["stats"]["n_kept"],
                         n_candidates=f["stats"]["n_candidates"])
    KEYS = ("X", "N", "rgb", "n_views", "view_mask", "src_image", "src_pixel")
    out["fuse"] = []
    fu = None
    for call in range(4):
        t0 = time.perf_counter()
        fu = api.depthmap_fuse(ctx, *args[:6], f["depth"], dev["normal"], pool=pool)
        wall = time.perf_counter() - t0
        s = fu["stats"]["seconds"]
        n_pt, n_map = fu["stats"]["n_points"], len(f["depth"])
        # one read of depth (4), normal (12), mask and fate (5), one write of them, one write of the cloud (40 B a point)
        bound = n_map * (4 + 12) + 2 * n_map * 5 + n_pt * 40
        out["fuse"].append(dict(wall_s=wall, upload_s=s[0], kernels_s=s[1], download_s=s[2], bound_bytes=bound,
                                bytes_per_s=bound / s[1] if s[1] > 0 else None))
    out["fuse_points"], out["fuse_suppressed"] = fu["stats"]["n_points"], fu["stats"]["n_suppressed"]
    out["densify"], out["separate"] = [], []
    same = True
    for rnd in range(a.rounds):
        t0 = time.perf_counter()
        one = api.densify(ctx, *args[:7], opts=o, pool=pool, maps=False)
        out["densify"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        d3 = api.depthmap(ctx, *args[:7], opts=o, pool=pool)
        f3 = api.depthmap_filter(ctx, *args[:6], d3["depth"], d3["cost"])
        c3 = api.depthmap_fuse(ctx, *args[:6], f3["depth"], d3["normal"], pool=pool)
        out["separate"].append(time.perf_counter() - t0)
        same = same and all(one[k].tobytes() == c3[k].tobytes() for k in KEYS)
    out["densify_equals_separate"] = same
    ctx.close()
    if a.host:
        t0 = time.perf_counter()
        fh = api.depthmap_fuse(None, *args[:6], f["depth"], dev["normal"], pool=pool)
        out["fuse_host_wall_s"] = time.perf_counter() - t0
        out["fuse_host_equals_device"] = all(fh[k].tobytes() == fu[k].tobytes() for k in KEYS)
    if a.host:
        t0 = time.perf_counter()
        host = api.depthmap(None, *args[:7], opts=o, pool=pool)
        out["host_wall_s"] = time.perf_counter() - t0
        out["host_equals_device"] = all(host[k].tobytes() == dev[k].tobytes() for k in ("depth", "normal", "cost"))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
