#!/usr/bin/env python3
"""SIFT extraction at a batch shape: device time of sfm_sift's kernels
(SFM_CTX_TIME_KERNELS: the summary's kernel_ms, the event pairs around each
stretch of launches) and the whole call from Python, against the wall time of
the serial host twin sfm_sift_host on the same box.  Not a test.

The input is sfm_synth_image: --images blob-field images of --w x --h with
distinct seeds.  The host twin runs one thread; it is timed on the first
--host-images images and reported per image, and its output is compared bit
for bit with the device's for those images.

  python tools/probe/sift_time.py [--images 64] [--w 640] [--h 480] [--reps 7] [--host-images 4]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

abi = importlib.import_module("3dreconstruction_amd._abi")
api = importlib.import_module("3dreconstruction_amd.api")


def stats(v, scale=1.0):
    return {"min": scale * min(v), "median": scale * float(np.median(v)), "max": scale * max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-images", type=int, default=4)
    a = ap.parse_args()
    batch = np.stack([api.synth_image(a.w, a.h, 100 + i) for i in range(a.images)])
    ctx = api.Context(0, flags=abi.SFM_CTX_TIME_KERNELS)
    t0 = time.perf_counter()
    host = api.sift(None, batch[:a.host_images])
    host_ms = 1e3 * (time.perf_counter() - t0) / max(a.host_images, 1)
    dev_ms, wall_s = [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        dev = api.sift(ctx, batch)
        w = time.perf_counter() - t0
        if r >= a.warmup:
            dev_ms.append(dev[2]["kernel_ms"])
            wall_s.append(w)
    for i in range(a.host_images):
        assert dev[1][i] == host[1][i] and dev[0][i][0].tobytes() == host[0][i][0].tobytes()
        assert np.array_equal(dev[0][i][1], host[0][i][1])
    print(json.dumps({"images": a.images, "w": a.w, "h": a.h, "features": int(dev[1].sum()),
                      "keypoints": int(dev[2]["n_keypoints"]), "device_kernel_ms": stats(dev_ms),
                      "device_kernel_ms_per_image": stats(dev_ms, 1.0 / a.images),
                      "device_call_wall_ms": stats(wall_s, 1e3), "host_twin_ms_per_image": host_ms,
                      "host_images": a.host_images, "reps": a.reps}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
