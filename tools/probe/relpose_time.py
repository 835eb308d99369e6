#!/usr/bin/env python3
"""Relative pose at the engine's shape: device time of sfm_relpose
(sfm_ctx_last_kernel_ms, the kernel alone) and the whole call from Python,
against the wall time of the serial host twin sfm_relpose_host and the device
time of the F-matrix filter sfm_fmatrix_ac on the same matches at the same
iteration count.  Not a test.

The input comes from tests/_relpose_helpers.make_pair: 512 pairs x 500
matches, 30 % outliers, 4096 iterations, pinhole.  The host twin runs one
thread; it is timed on the first --host-pairs pairs (the same problems) and
reported per pair.

  python tools/probe/relpose_time.py [--pairs 512] [--n 500] [--reps 7] [--host-pairs 4]"""
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

import _relpose_helpers as P  # noqa: E402

abi = importlib.import_module("3dreconstruction_amd._abi")
api = importlib.import_module("3dreconstruction_amd.api")


def stats(v, scale=1.0):
    return {"min": scale * min(v), "median": scale * float(np.median(v)), "max": scale * max(v)}


def fmatrix(ctx, pairs, iterations):
    """sfm_fmatrix_ac over the same matches"""
    off = np.zeros(len(pairs) + 1, np.int64)
    off[1:] = np.cumsum([p["n"] for p in pairs])
    xy = np.ascontiguousarray(np.concatenate([p["xy"] for p in pairs]))
    wh = np.ascontiguousarray(np.tile(np.array(P.WH4, np.int32), len(pairs)))
    o = abi.FMatrixOpts()
    o.precision, o.max_iterations = 4.0, iterations
    res = (abi.FMatrixResult * len(pairs))()
    inl = np.zeros(int(off[-1]), np.int32)
    rc = ctx.lib.sfm_fmatrix_ac(ctx.h, len(pairs), abi.ptr(off, abi.i64p), abi.ptr(xy, abi.f64p),
                                abi.ptr(wh, abi.i32p), ctypes.byref(o), res, abi.ptr(inl, abi.i32p))
    assert rc == 0, rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=512)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--outliers", type=float, default=0.3)
    ap.add_argument("--iterations", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-pairs", type=int, default=4)
    a = ap.parse_args()
    ctx = api.Context(0, flags=abi.SFM_CTX_TIME_KERNELS)
    ms = ctypes.c_double()
    o = P.opts(max_iterations=a.iterations)
    model = abi.SFM_CAM_PINHOLE
    pairs = [P.make_pair(model, a.n, a.outliers, 2000 + q) for q in range(a.pairs)]
    t0 = time.perf_counter()
    host = P.run(None, pairs[:a.host_pairs], o)
    host_ms = 1e3 * (time.perf_counter() - t0) / max(a.host_pairs, 1)
    dev_ms, wall_s, f_ms = [], [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        dev = P.run(ctx, pairs, o)
        w = time.perf_counter() - t0
        assert ctx.lib.sfm_ctx_last_kernel_ms(ctx.h, ms) == 0
        if r >= a.warmup:
            dev_ms.append(ms.value)
            wall_s.append(w)
        fmatrix(ctx, pairs, a.iterations)
        assert ctx.lib.sfm_ctx_last_kernel_ms(ctx.h, ms) == 0
        if r >= a.warmup:
            f_ms.append(ms.value)
    P.compare_results(dev[:a.host_pairs], host)
    print(json.dumps({"model": model, "pairs": a.pairs, "n": a.n, "iterations": a.iterations,
                      "ok": sum(r["status"] == P.OK for r in dev),
                      "mean_inliers": float(np.mean([r["n_inliers"] for r in dev])),
                      "mean_iterations_run": float(np.mean([r["iterations"] for r in dev])),
                      "device_kernel_ms": stats(dev_ms), "device_kernel_ms_per_pair": stats(dev_ms, 1.0 / a.pairs),
                      "device_call_wall_ms": stats(wall_s, 1e3), "fmatrix_kernel_ms": stats(f_ms),
                      "fmatrix_kernel_ms_per_pair": stats(f_ms, 1.0 / a.pairs),
                      "host_twin_ms_per_pair": host_ms, "host_pairs": a.host_pairs, "reps": a.reps}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
