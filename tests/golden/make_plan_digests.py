#!/usr/bin/env python3
"""Record tests/golden/plan_digests.json: the planner's digest (every array the
device reads, sfm_ba_grown_digest) of a fixed set of synthetic problems.

    python tests/golden/make_plan_digests.py --commit <the commit of the build>

The file pins the planner across refactors, so it is recorded from a build of
the commit a refactor starts from, never from the refactored tree: check that
commit out, build it, and run this script (copied there if it is older than
the script) against its library.  tests/test_plan_golden.py reads the cases
and the growth pairs from here.  CPU only.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)
import _helpers as H  # noqa: E402
from plan_digest import CASES as TOOL_CASES  # noqa: E402

abi = H.abi

# (n_cam, n_pt, k, vis_mode, n_intr, model): the tool's cases but the
# 1000-camera one (it stays in the tool: seconds, not milliseconds), world 1
CASES = [c[:6] for c in TOOL_CASES if c[0] < 1000]
# one growth pair per camera model that has a case: the first case of each, in
# visibility mode 0 (the other modes' scenes get a reordered camera order or a
# wide band, and such a plan seeds no grown one: build_plan_grown declines)
PAIRS = [next(c[:3] + (0,) + c[4:] for c in CASES if c[5] == m) for m in sorted({c[5] for c in CASES})]


def name(case):
    n_cam, n_pt, k, vis, n_intr, model = case
    return f"scene {n_cam}/{n_pt}/{k}/v{vis}/i{n_intr}/m{model}"


def scene(case):
    n_cam, n_pt, k, vis, n_intr, model = case
    return H.Scene(n_cam, n_pt, k, vis_mode=vis, n_intr=n_intr, model=model, seed=n_cam * 7 + vis)


def without_last_image(sc):
    """The problem of `sc` before its last image arrived: that image and its
    observations removed (every point keeps its other observations, in order:
    a point's observations ascend by image, so the full scene appends to it)."""
    last = sc.n_cam - 1
    keep = sc.obs_img != last
    arrays = {
        "pt_offsets": np.concatenate([[0], np.cumsum(np.add.reduceat(keep.astype(np.int64), sc.pt_offsets[:-1]))])
                        .astype(np.int64),
        "obs_img": np.ascontiguousarray(sc.obs_img[keep]),
        "obs_uv": np.ascontiguousarray(sc.obs_uv.reshape(-1, 2)[keep].reshape(-1)),
        "img_intr": np.ascontiguousarray(sc.img_intr[:last]),
    }
    pr = abi.BAProblem()
    pr.n_img, pr.n_intr, pr.n_pt, pr.n_obs = last, sc.n_intr, sc.n_pt, int(keep.sum())
    pr.pt_offsets = abi.ptr(arrays["pt_offsets"], abi.i64p)
    pr.obs_img = abi.ptr(arrays["obs_img"], abi.i32p)
    pr.obs_uv = abi.ptr(arrays["obs_uv"], abi.f64p)
    pr.img_intr = abi.ptr(arrays["img_intr"], abi.i32p)
    pr.const_img, pr.camera_model, pr.huber_a = sc.const_img, sc.model, sc.huber
    pr._keep = arrays
    return pr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    ap.add_argument("--out", default=os.path.join(HERE, "plan_digests.json"))
    a = ap.parse_args()
    api = importlib.import_module("3dreconstruction_amd.api")
    out = {"commit": a.commit, "cases": {}, "pairs": {}}
    for case in CASES:
        sc = scene(case)   # (owns the problem's arrays)
        p = sc.problem()
        out["cases"][name(case)] = f"{api.ba_grown_digest(p, p)[0]:016x}"   # (the fresh plan's)
    for case in PAIRS:
        sc = scene(case)
        fresh, grown, reused = api.ba_grown_digest(without_last_image(sc), sc.problem())
        assert reused >= 0 and grown == fresh, name(case)
        out["pairs"][name(case)] = f"{fresh:016x}"
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("plan digests written:", len(out["cases"]), "cases,", len(out["pairs"]), "pairs")


if __name__ == "__main__":
    main()
