"""Times the mesh stage on one GPU: tools/depthmap_time.py's case (8 synthetic
views of 1024 x 768 looking at a textured plane) densified, a grid fitted
around the cloud at --resolution, then sfm_tsdf_integrate and sfm_mesh_extract
(four calls each: kernel time from HIP events against the byte bound, wall
time from Python), sfm_mesh_reconstruct against the two calls chained,
alternating, --rounds each, and with --host each host twin once (bytes
compared).  Byte bounds: integration reads every depth pixel once and writes
the volume (9 B a lattice point with colours, 5 B without); extraction reads
the volume twice (mark, then vertices and triangles) and writes the mesh once.

--plane needs no GPU: the rendered plane fixture of the tests (48 x 40, three
views, defaults, seed 3) estimated, filtered, fused and meshed by the host
twins; prints the mean distance to the true plane of the fused cloud's points
and of the mesh's vertices.

    python tools/mesh_time.py [--host] [--resolution 256] [--views 8] [--size 1024 768]
    python tools/mesh_time.py --plane
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
api = importlib.import_module("3dreconstruction_amd.api")
from depthmap_time import scene  # noqa: E402

MESH = ("V", "rgb", "tri")


def plane():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _fuse_helpers as FH
    fx, est, flt = FH.estimated("plane", 3, 3, 3)
    cam = (fx.wh, fx.K, fx.R, fx.C)
    cloud = api.depthmap_fuse(None, *cam, fx.nb_off, fx.nb_view, flt["depth"], est["normal"], images=fx.images)
    out = dict(cloud_points=len(cloud["X"]), cloud_mean_distance=float(np.abs(cloud["X"][:, 2] - fx.far).mean()), meshes=[])
    for res in (32, 64, 128):
        grid = api.mesh_grid_fit(cloud["X"], res, 2)
        m = api.mesh_reconstruct(None, *cam, flt["depth"], grid, images=fx.images)
        out["meshes"].append(dict(resolution=res, dims=list(grid.dims), voxel=grid.voxel, vertices=len(m["V"]),
                                  triangles=len(m["tri"]), degenerate=m["stats"]["mesh"]["n_degenerate"],
                                  mean_distance=float(np.abs(m["V"][:, 2] - fx.far).mean()) if len(m["V"]) else None))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true", help="also time the host twins once")
    ap.add_argument("--plane", action="store_true", help="the accuracy on the rendered plane fixture (host twins only)")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=[1024, 768])
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3, help="rounds of reconstruct against the two calls")
    a = ap.parse_args()
    if a.plane:
        return plane()
    w, h = a.size
    wh, K, R, C, nb_off, nb_view, drange, images = scene(a.views, w, h)
    pool = api._pixel_pool(images)
    ctx = api.Context(0)
    dense = api.densify(ctx, wh, K, R, C, nb_off, nb_view, drange, pool=pool)
    depth = dense["depth_filtered"]
    grid = api.mesh_grid_fit(dense["X"], a.resolution, 2)
    n_vox, n_map = int(np.prod(list(grid.dims))), len(depth)
    out = dict(views=a.views, size=[w, h], cloud_points=len(dense["X"]), dims=list(grid.dims), voxel=grid.voxel,
               lattice_points=n_vox, integrate=[], extract=[])
    cam = (wh, K, R, C, depth, grid)
    vol = mesh = None
    for call in range(4):
        t0 = time.perf_counter()
        vol = api.tsdf_integrate(ctx, *cam, pool=pool)
        wall = time.perf_counter() - t0
        s = vol["stats"]["seconds"]
        bound = 4 * n_map + 9 * n_vox
        out["integrate"].append(dict(wall_s=wall, upload_s=s[0], kernels_s=s[1], download_s=s[2], bound_bytes=bound,
                                     bytes_per_s=bound / s[1] if s[1] > 0 else None,
                                     point_images_per_s=n_vox * a.views / s[1] if s[1] > 0 else None))
    out["n_observed"] = vol["stats"]["n_observed"]
    caps = None
    for call in range(4):
        t0 = time.perf_counter()
        mesh = api.mesh_extract(ctx, grid, vol["tsdf"], vol["weight"], vol["rgb"], vol["has_rgb"],
                                cap_vertices=caps and caps[0], cap_triangles=caps and caps[1])
        wall = time.perf_counter() - t0
        st = mesh["stats"]
        caps = (st["n_vertices"], st["n_triangles"])
        s = st["seconds"]
        bound = 2 * 9 * n_vox + 2 * 6 * n_vox + 15 * st["n_vertices"] + 12 * st["n_triangles"]
        out["extract"].append(dict(wall_s=wall, two_calls=call == 0, upload_s=s[0], kernels_s=s[1], download_s=s[2],
                                   bound_bytes=bound, bytes_per_s=bound / s[1] if s[1] > 0 else None))
    out["vertices"], out["triangles"], out["degenerate"] = caps[0], caps[1], mesh["stats"]["n_degenerate"]
    out["reconstruct"], out["separate"] = [], []
    same = True
    for rnd in range(a.rounds):
        t0 = time.perf_counter()
        one = api.mesh_reconstruct(ctx, *cam, pool=pool, cap_vertices=caps[0], cap_triangles=caps[1])
        out["reconstruct"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        v2 = api.tsdf_integrate(ctx, *cam, pool=pool)
        m2 = api.mesh_extract(ctx, grid, v2["tsdf"], v2["weight"], v2["rgb"], v2["has_rgb"], cap_vertices=caps[0],
                              cap_triangles=caps[1])
        out["separate"].append(time.perf_counter() - t0)
        same = same and all(one[k].tobytes() == m2[k].tobytes() for k in MESH)
    out["reconstruct_equals_separate"] = same
    ctx.close()
    if a.host:
        t0 = time.perf_counter()
        vh = api.tsdf_integrate(None, *cam, pool=pool)
        out["integrate_host_wall_s"] = time.perf_counter() - t0
        out["integrate_host_equals_device"] = all(vh[k].tobytes() == vol[k].tobytes() for k in ("tsdf", "weight", "rgb", "has_rgb"))
        t0 = time.perf_counter()
        mh = api.mesh_extract(None, grid, vol["tsdf"], vol["weight"], vol["rgb"], vol["has_rgb"], cap_vertices=caps[0],
                              cap_triangles=caps[1])
        out["extract_host_wall_s"] = time.perf_counter() - t0
        out["extract_host_equals_device"] = all(mh[k].tobytes() == mesh[k].tobytes() for k in MESH)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
