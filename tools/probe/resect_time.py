#!/usr/bin/env python3
"""Camera resection at the engine's shape: device time of sfm_resect
(sfm_ctx_last_kernel_ms, the kernel alone) and the whole call from Python,
against the wall time of the serial host twin sfm_resect_host.  Not a test.

The input comes from tests/_resect_helpers.make_problem: 256 images x 2000
correspondences, 30 % outliers, 4096 iterations, no bound, for the pinhole and
the RADIAL3 model.  The host twin runs one thread; it is timed on the first
--host-images images (the same problems) and reported per image.

  python tools/probe/resect_time.py [--images 256] [--n 2000] [--reps 7] [--host-images 4]"""
import argparse
import ctypes
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

import _resect_helpers as R  # noqa: E402

abi = importlib.import_module("3dreconstruction_amd._abi")
api = importlib.import_module("3dreconstruction_amd.api")


def stats(v, scale=1.0):
    return {"min": scale * min(v), "median": scale * float(np.median(v)), "max": scale * max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--iterations", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-images", type=int, default=4)
    a = ap.parse_args()
    ctx = api.Context(0, flags=abi.SFM_CTX_TIME_KERNELS)
    ms = ctypes.c_double()
    o = R.opts(max_iterations=a.iterations)
    for model in (abi.SFM_CAM_PINHOLE, abi.SFM_CAM_RADIAL3):
        probs = [R.make_problem(model, a.n, a.outliers, 1000 + q) for q in range(a.images)]
        t0 = time.perf_counter()
        host = R.run(None, probs[:a.host_images], o)
        host_ms = 1e3 * (time.perf_counter() - t0) / max(a.host_images, 1)
        dev_ms, wall_s = [], []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            dev = R.run(ctx, probs, o)
            w = time.perf_counter() - t0
            assert ctx.lib.sfm_ctx_last_kernel_ms(ctx.h, ms) == 0
            if r >= a.warmup:
                dev_ms.append(ms.value)
                wall_s.append(w)
        R.compare_results(dev[:a.host_images], host)
        print(json.dumps({"model": model, "images": a.images, "n": a.n, "iterations": a.iterations,
                          "kept": sum(r["status"] == R.OK for r in dev),
                          "mean_inliers": float(np.mean([r["n_inliers"] for r in dev])),
                          "mean_iterations_run": float(np.mean([r["iterations"] for r in dev])),
                          "device_kernel_ms": stats(dev_ms), "device_call_wall_ms": stats(wall_s, 1e3),
                          "host_twin_ms_per_image": host_ms, "host_images": a.host_images, "reps": a.reps}),
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
