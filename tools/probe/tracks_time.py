#!/usr/bin/env python3
"""Track building at the C3 scale: device time of sfm_tracks_build
(sfm_ctx_last_kernel_ms, the kernels alone) against the wall time of the serial
host twin sfm_tracks_build_host on the same input.  Not a test.

The input comes from tests/_tracks_helpers.generate: 500 images x 4096
features, exhaustive pairs, about 100 matches per pair (landmarks of 2 .. 23
views filling the feature slots), 1 % false matches.

  python tools/probe/tracks_time.py [--images 500] [--features 4096] [--reps 7]

SFM_TIMING=1 in the environment adds the host-timed split by kernel group of
every device build to stderr (each group then ends in a synchronise)."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _tracks_helpers as T  # noqa: E402

abi = importlib.import_module("3dreconstruction_amd._abi")
api = importlib.import_module("3dreconstruction_amd.api")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--features", type=int, default=4096)
    ap.add_argument("--views", type=int, default=23, help="largest number of views of a landmark")
    ap.add_argument("--false-frac", type=float, default=0.01)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()

    t0 = time.perf_counter()
    # landmarks enough to fill every image's feature slots at the mean track length
    n_land = int(a.images * a.features / ((2 + a.views) / 2))
    case = T.generate(a.images, a.features, n_land, false_frac=a.false_frac, seed=0xC3, views=(2, a.views))
    pairs, counts, i, j = case["matches"]
    xy = np.random.default_rng(1).uniform(0, 4000, (int(case["feat_off"][-1]), 2))
    print(f"input: {a.images} images x {a.features} features, {len(counts)} pairs, {int(counts.sum())} matches "
          f"({counts.mean():.1f} per pair), {n_land} landmarks, {case['n_false']} false matches; generated in "
          f"{time.perf_counter() - t0:.1f} s", flush=True)

    def build(ctx):
        t = api.Tracks(ctx, case["n_img"], case["feat_off"], case["matches"], xy=xy)
        st = t.stats()
        return t, st

    host_s = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        th, st_h = build(None)
        host_s.append(time.perf_counter() - t0)
        if _ + 1 < a.host_reps:
            th.close()
    print(f"host twin: {json.dumps(st_h)}", flush=True)

    ctx = api.Context(0, flags=abi.SFM_CTX_TIME_KERNELS)
    ms = importlib.import_module("ctypes").c_double()
    dev_ms, wall_s = [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        td, st_d = build(ctx)
        w = time.perf_counter() - t0
        assert ctx.lib.sfm_ctx_last_kernel_ms(ctx.h, ms) == 0
        if r >= a.warmup:
            dev_ms.append(ms.value)
            wall_s.append(w)
        if r + 1 < a.warmup + a.reps:
            td.close()
    assert st_d == st_h, (st_d, st_h)
    fh, fd = th.fetch(), td.fetch()
    same = all(np.array_equal(fh[k], fd[k]) for k in ("pt_offsets", "obs_img", "obs_feat")) and \
        fh["obs_uv"].tobytes() == fd["obs_uv"].tobytes()
    assert same, "device and host tracks differ"
    out = {"images": a.images, "features": a.features, "matches": int(counts.sum()), "stats": st_d,
           "device_kernel_ms": {"min": min(dev_ms), "median": float(np.median(dev_ms)), "max": max(dev_ms)},
           "device_call_wall_ms": {"min": 1e3 * min(wall_s), "median": 1e3 * float(np.median(wall_s)),
                                   "max": 1e3 * max(wall_s)},
           "host_twin_wall_ms": {"min": 1e3 * min(host_s), "median": 1e3 * float(np.median(host_s)),
                                 "max": 1e3 * max(host_s)},
           "reps": a.reps, "host_reps": a.host_reps, "identical": same}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
