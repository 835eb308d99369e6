"""Depth-map fusion on the device: sfm_depthmap_fuse against its host twin and
against the numpy restatement (_fuse_helpers.py), bytes and counts, on the
smallest shapes that reach each device-only branch: raster lengths around the
wavefront and the workgroup, emit patterns per block, block bases that cross
images; and sfm_densify against the three device calls chained.  The maps are
built by hand (exact plane depths), so PatchMatch runs only end to end."""
import os
import re

import numpy as np
import pytest

import _depthmap_helpers as DH
import _fuse_helpers as FH

abi, api = DH.abi, DH.api
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BLOCK = 256   # csrc/fuse_point.h kFuseBlock: pixels of a raster per workgroup
# rasters of 1, 63, 64, 65, 255, 256, 257 and 513 pixels
SHAPES = [(1, 1), (9, 7), (8, 8), (13, 5), (17, 15), (16, 16), (257, 1), (27, 19)]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def test_constants_mirror_the_header():
    src = open(os.path.join(ROOT, "3dreconstruction_amd", "csrc", "fuse_point.h")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kFuse\w+) = (\d+);", src)}
    assert got == {"kFuseMaxPairs": FH.MAX_PAIRS, "kFuseBlock": BLOCK}
    assert (abi.FUSE_MAX_PAIRS, abi.FUSE_BLOCK) == (FH.MAX_PAIRS, BLOCK)


def three_way(ctx, sc, opts=None, **ref_kw):
    ref = sc.ref(**ref_kw)
    dev, host = sc.run(ctx, opts), sc.run(None, opts)
    FH.check_against_ref(host, ref)
    FH.check_against_ref(dev, ref)
    return ref


def test_raster_lengths_in_one_call(ctx):
    assert [w * h for w, h in SHAPES] == [1, 63, 64, 65, 255, 256, 257, 513]
    sc = FH.Scene([FH.group(w, h, seed=3 + k) for k, (w, h) in enumerate(SHAPES)])
    ref = three_way(ctx, sc)
    assert ref["n_suppressed"] > 0 and len(set(ref["src_image"])) > len(SHAPES)


def test_emit_patterns(ctx):
    w, h = 27, 19           # 513 pixels: blocks of 256, 256 and 1
    n = w * h
    lone = lambda seed: DH.Fixture(w, h, [(0, 0, 0)], far=4.0, seed=seed, neighbours=[[]])
    # images 0..5 agree with nobody: every pixel with a depth is emitted
    patterns = [np.arange(n),                  # all
                np.zeros(0, np.int64),         # none
                np.arange(0, n, 2),            # alternating
                np.arange(0, n, BLOCK),        # only lane 0 of each block
                np.arange(63, n, 64),          # only lane 63 of each wavefront
                np.array([n - 1])]             # only the last pixel of the image
    # images 6 7 8: 7 has 6's camera and depths, so all of it is suppressed, between two that emit
    trio = DH.Fixture(w, h, [(0, 0, 0), (0, 0, 0), (0.3, 0, 0)], far=4.0, seed=9)
    sc = FH.Scene([lone(20 + k) for k in range(len(patterns))] + [trio])
    for i, idx in enumerate(patterns):
        sc.keep_only(i, idx)
    ref = three_way(ctx, sc)
    for i, idx in enumerate(patterns):
        assert np.array_equal(ref["src_pixel"][ref["src_image"] == i], idx)
    assert (ref["fates"][7] == FH.SUPPRESSED).all()
    assert (ref["src_image"] == 6).sum() == n and (ref["src_image"] == 8).any()


def test_pair_lists_colours_and_unloaded(ctx):
    three_way(ctx, FH.Scene([FH.star_fixture()]))
    fx = DH.Fixture(24, 20, [(-0.25, 0, 0), (0, 0, 0), (0.3, 0.02, 0)], far=4.0, seed=11, neighbours=[[], [0, 2], [0]])
    three_way(ctx, FH.Scene([fx]))
    fxs = [FH.group(13, 5, channels=[3, 1, 3]), FH.group(9, 7, channels=[1, 3, 1], seed=7)]
    ref = three_way(ctx, FH.Scene(fxs, unloaded=(1,)))
    assert (ref["fates"][1] == FH.NONE).all()
    plain = FH.Scene(fxs, colours=False)
    three_way(ctx, plain)
    rc, arrays, st = api.depthmap_fuse_raw(ctx, *plain.args(), fill=7)
    assert rc == 0 and (arrays["rgb"] == 7).all() and st["n_points"] > 0


def test_cap_points_too_small(ctx):
    sc = FH.Scene([FH.group(27, 19)])
    need = sc.ref()["n_points"]
    rc, arrays, st = api.depthmap_fuse_raw(ctx, *sc.args(), images=sc.images, cap_points=need - 1, fill=9)
    assert rc == abi.SFM_ERR_INVALID_ARG and st["n_points"] == need
    assert b"cap_points" in abi.load().sfm_last_error()
    assert all((a == 9).all() for a in arrays.values())
    # the context is still good
    FH.check_against_ref(sc.run(ctx), sc.ref())


def test_normal_test_on(ctx):
    fx = FH.group(17, 15)
    sc = FH.Scene([fx])
    for cos, cols in ((0.95, slice(0, 8)), (0.85, slice(8, 17))):
        sc.normal_maps[1][:, cols] = np.array([np.sqrt(1 - cos * cos), 0, -cos], F)
    on = three_way(ctx, sc, FH.fuse_opts(min_normal_cos=0.9), min_normal_cos=0.9)
    assert on["n_points"] > sc.ref()["n_points"]


def test_densify_end_to_end(ctx):
    fx = DH.small_fixture()
    o = DH.opts(r=2, iterations=1, seed=3)
    est = fx.run(ctx, o)
    flt = fx.filter(ctx, est)
    cloud = api.depthmap_fuse(ctx, fx.wh, fx.K, fx.R, fx.C, fx.nb_off, fx.nb_view, flt["depth"], est["normal"],
                              images=fx.images)
    assert cloud["stats"]["n_points"] > 0 and cloud["stats"]["n_suppressed"] > 0
    args = (fx.wh, fx.K, fx.R, fx.C, fx.nb_off, fx.nb_view, fx.drange, fx.images, o)
    host = api.densify_host(*args)
    for res in (api.densify(ctx, *args), host):
        FH.same_cloud(res, cloud)
        DH.same_maps(res, est)
        assert res["depth_filtered"].tobytes() == flt["depth"].tobytes()
        assert res["n_agree"].tobytes() == flt["n_agree"].tobytes() and np.array_equal(res["counts"], flt["counts"])
        st = res["stats"]
        assert st["fuse"]["n_points"] == cloud["stats"]["n_points"]
        assert st["fuse"]["n_suppressed"] == cloud["stats"]["n_suppressed"]
        assert st["filter"]["n_kept"] == flt["stats"]["n_kept"]
        assert st["filter"]["n_candidates"] == flt["stats"]["n_candidates"]
        assert st["depthmap"]["n_estimated"] == est["stats"]["n_estimated"]
        assert st["depthmap"]["n_invalid"] == est["stats"]["n_invalid"]
    FH.same_cloud(api.densify(ctx, *args, maps=False), cloud)
