"""Shared by the SIFT tests (test_sift.py, test_sift_gpu.py): the golden
fixtures the reference's own extractor wrote (tests/golden/vlfeat_view{0,1,2}
at 640 x 480, vlfeat_sift_<w>x<h> at the small sizes; make_golden.py and
make_sift_golden.py), their input images rebuilt by sfm_synth_image, and the
comparison against them.

Bounds.  The reference against itself rebuilt with free
reassociation differs by at most 0.0077 in a feature (x, y, sigma, wrapped
angle) and by 1 grey level in a descriptor component.  The host twin measured
against the goldens differs by 0 in both, at every size below.  The bounds are
the larger of the reference's own figures and twice the measured ones: 0.0077
and 1 level.  At most 1 % of the features of an image may miss them."""
import functools
import importlib
import os

import numpy as np

import _helpers as H

abi = H.abi
api = importlib.import_module("3dreconstruction_amd.api")
GOLDEN = os.path.join(H.ROOT, "tests", "golden")

FEAT_BOUND = 0.0077
DESC_BOUND = 1
EXEMPT = 0.01

# name -> (w, h, (seed, angle, tx, ty, scale), features in the golden file)
CASES = {
    "vlfeat_view0": (640, 480, (7, 0.0, 0.0, 0.0, 1.0), 325),
    "vlfeat_view1": (640, 480, (7, 0.2, 12.0, -7.0, 1.1), 267),
    "vlfeat_view2": (640, 480, (7, -0.35, -20.0, 15.0, 0.9), 369),
    "vlfeat_sift_160x120": (160, 120, (7, 0.0, 0.0, 0.0, 1.0), 40),
    "vlfeat_sift_96x64": (96, 64, (7, 0.0, 0.0, 0.0, 1.0), 14),
    "vlfeat_sift_161x97": (161, 97, (7, 0.0, 0.0, 0.0, 1.0), 39),
}
VIEWS = ["vlfeat_view0", "vlfeat_view1", "vlfeat_view2"]
SMALL = ["vlfeat_sift_160x120", "vlfeat_sift_96x64", "vlfeat_sift_161x97"]


@functools.lru_cache(maxsize=None)
def image(name):
    w, h, view, _ = CASES[name]
    g = api.synth_image(w, h, *view)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def seed_image(w, h, seed):
    g = api.synth_image(w, h, seed)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def golden(name):
    n = CASES[name][3]
    kp = np.fromfile(os.path.join(GOLDEN, name + ".kp"), np.float32).reshape(-1, 4)
    u8 = np.fromfile(os.path.join(GOLDEN, name + ".u8"), np.uint8).reshape(-1, 128)
    assert len(kp) == len(u8) == n
    return kp, u8


@functools.lru_cache(maxsize=None)
def host(name):
    """the host twin's features of a golden case (computed once)"""
    out, n, _ = api.sift(None, image(name))
    return out[0], int(n[0])


def against_golden(name, xyso, desc, n):
    """counts equal, order the same: feature i pairs with golden feature i;
    prints the largest differences and how many features miss the bounds"""
    kp, u8 = golden(name)
    assert n == len(kp) == len(xyso) == len(desc), (name, n, len(kp))
    df = np.abs(xyso[:, :3].astype(np.float64) - kp[:, :3]).max(1)
    da = np.abs(xyso[:, 3].astype(np.float64) - kp[:, 3])
    da = np.minimum(da, np.abs(2 * np.pi - da))
    f = np.maximum(df, da)
    d = np.abs(desc.astype(np.int32) - u8.astype(np.int32)).max(1)
    miss = int(((f > FEAT_BOUND) | (d > DESC_BOUND)).sum())
    print(f"{name}: {n} features, largest feature difference {f.max():.3g} (bound {FEAT_BOUND}), largest "
          f"descriptor difference {d.max()} levels (bound {DESC_BOUND}), {int((d > 0).sum())} descriptors differ, "
          f"{miss} features exempted of at most {int(EXEMPT * n)}")
    assert miss <= EXEMPT * n, (name, miss, float(f.max()), int(d.max()))
    return miss


def same(a, b):
    """two results of api.sift, bit for bit"""
    (fa, na, _), (fb, nb, _) = a, b
    np.testing.assert_array_equal(na, nb)
    for (xa, da), (xb, db) in zip(fa, fb):
        assert xa.tobytes() == xb.tobytes()
        np.testing.assert_array_equal(da, db)
