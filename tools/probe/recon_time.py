#!/usr/bin/env python3
"""Incremental reconstruction: the wall time of the three round queries on a
device handle (sfm_recon_visibility / sfm_recon_gather / sfm_recon_select: the
state's upload, the kernels, the compacted download) against the same queries
on the host twin's handle (a serial walk), per call, and the wall time of the
whole driver split by stage (sfm_recon_stats.seconds).  Not a test.

Queries: the tracks of a synthetic scene (sfm_synth_ba: --cams cameras, --points
points, --views views each), half of the images registered, half of the points
reconstructed; the gather lists --gather unregistered images.
Driver: tests/_recon_helpers.ArcScene with --arc-images images and --arc-points
points, 0.5 px noise, adjust = 1, RADIAL3 with one intrinsics block.

  python tools/probe/recon_time.py [--cams 200] [--points 200000] [--views 6] [--reps 7]"""
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

import _helpers as H  # noqa: E402
import _recon_helpers as RH  # noqa: E402

abi = importlib.import_module("3dreconstruction_amd._abi")
api = importlib.import_module("3dreconstruction_amd.api")
STAGES = ("pair_search", "visibility", "gather", "select", "resect", "triangulate", "solve", "wash")


def timed(fn, reps, warmup=2):
    out = []
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        fn()
        if r >= warmup:
            out.append(1e3 * (time.perf_counter() - t0))
    return {"min": min(out), "median": float(np.median(out)), "max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cams", type=int, default=200)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--gather", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--arc-images", type=int, default=24)
    ap.add_argument("--arc-points", type=int, default=6000)
    a = ap.parse_args()
    ctx = api.Context(0)
    sc = H.Scene(a.cams, a.points, a.views, vis_mode=1, lib=abi.load())
    prob = sc.problem()
    rng = np.random.default_rng(1)
    reg = rng.random(sc.n_cam) < 0.5
    ok = rng.random(sc.n_pt) < 0.5
    X = sc.gt_X
    images = np.flatnonzero(~reg)[:a.gather]
    import platform
    import torch
    arch = getattr(torch.cuda.get_device_properties(0), "gcnArchName", "")
    out = {"measured_on": {"gpu": f"{torch.cuda.get_device_name(0)} {arch}".strip(),
                           "host": platform.machine() + " " + platform.system(),
                           "host_cpus": os.cpu_count()},
           "cams": sc.n_cam, "points": sc.n_pt, "observations": sc.n_obs, "gather_images": len(images), "reps": a.reps}
    handles = {"device": api.ReconTracks(ctx, prob), "host": api.ReconTracks(None, prob)}
    for name, h in handles.items():
        out[name + "_ms"] = {
            "visibility": timed(lambda: h.visibility(ok), a.reps),
            "gather": timed(lambda: h.gather(X, ok, images), a.reps),
            "select_new": timed(lambda: h.select(reg, ok, RH.NEW), a.reps),
            "select_solved": timed(lambda: h.select(reg, ok, RH.SOLVED, 2), a.reps)}
    d, h = handles["device"], handles["host"]
    assert d.visibility(ok).tobytes() == h.visibility(ok).tobytes()
    RH.same_select(d.select(reg, ok, RH.SOLVED, 2), h.select(reg, ok, RH.SOLVED, 2))
    for x in handles.values():
        x.close()
    arc = RH.ArcScene(abi.SFM_CAM_RADIAL3, n_img=a.arc_images, n_pt=a.arc_points, noise=0.5, n_bad=40)
    t0 = time.perf_counter()
    res = arc.run(ctx, RH.recon_opts(1), cap_cands=4096)
    wall = time.perf_counter() - t0
    st = res["stats"]
    out["driver"] = {"images": arc.n_img, "points": arc.tracks.n_pt, "observations": arc.tracks.n_obs,
                     "registered": st["n_registered"], "reconstructed": st["n_points"], "rounds": st["n_rounds"],
                     "final_rmse": st["final_adjust"]["ba"]["rmse_final"], "wall_s": wall,
                     "stage_s": dict(zip(STAGES, st["seconds"]))}
    print(json.dumps(out), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
