"""GPU: relative pose (sfm_relpose) against its host twin and the numpy
reference of _relpose_helpers.py: host against device, run against run, the
shapes at the workgroup-stride and sort-buffer boundaries, and the chain
relpose -> triangulate -> resect that starts a scene from nothing."""
import numpy as np
import pytest

import _relpose_helpers as P

abi, api = P.abi, P.api
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("model", P.MODELS)
def test_shapes_host_device_and_rerun(ctx, model):
    """one call with every SHAPES size side by side: the device result passes
    the reference's checks, equals the host twin's (integers and inliers
    exactly, doubles to 1e-9) and a second device run bit for bit"""
    pairs = P.shape_pairs(model)
    o = P.opts(max_iterations=256)
    dev = P.run(ctx, pairs, o)
    P.check_shapes(pairs, dev)
    P.compare_results(dev, P.run(None, pairs, o))
    P.identical(dev, P.run(ctx, pairs, o))


def test_sort_switch_sizes(ctx):
    """8192 correspondences sort in LDS, 8193 in global memory"""
    pairs = [P.make_pair(abi.SFM_CAM_PINHOLE, n, 0.3, 131) for n in (8192, 8193)]
    o = P.opts(precision=0.0, max_iterations=32)
    dev = P.run(ctx, pairs, o)
    for p, r in zip(pairs, dev):
        P.check_model(p, r, precision=0.0)
        assert not p["outlier"][r["inliers"]].any()
    P.compare_results(dev, P.run(None, pairs, o))
    P.identical(dev, P.run(ctx, pairs, o))


@pytest.mark.parametrize("model", P.MODELS)
def test_device_five_point(ctx, model):
    for iters in (1, 8):
        p = P.make_pair(model, 60, 0.0, 121 + model, sigma=0.0)
        r = P.run(ctx, [p], P.opts(max_iterations=iters))[0]
        rot, dirn = P.pose_errors(p, r)
        print(f"model {model}, {iters} iterations: error_max {r['error_max']:.3e} px, rotation {rot:.3e}, t {dirn:.3e}")
        assert r["status"] == P.OK and r["n_inliers"] == 60
        assert r["error_max"] <= 1e-6
        assert max(rot, dirn) <= P.MARGIN * P.NOISE_FREE_POSE


def test_mixed_batch(ctx):
    """an all-outlier pair, a pair with a non-finite pixel and points behind a
    camera, and two pairs sharing one intrinsics block"""
    model = abi.SFM_CAM_RADIAL3
    none = P.make_pair(model, 100, 1.0, 182)
    b = P.make_pair(model, 120, 0.2, 183)
    b["xy"][5, 2] = np.nan
    behind = [3, 40, 77]          # image J sees the mirror image of these, far from their epipolar lines
    lo, hi = P.R.image_box(model)
    b["xy"][behind, 2:] = lo + hi - b["xy"][behind, 2:]
    Et = P.essential(b["R"], b["t"])
    assert (P.errors(model, Et, b["intr"], b["intr"], b["xy"][behind]) >= 50.0 ** 2).all()
    b["outlier"][[5] + behind] = True
    a = P.make_pair(model, 200, 0.3, 181)
    o = P.opts(max_iterations=128)
    alone = P.run(ctx, [a], o)
    pi, intr = [0, 0, 1, 1, 0, 0], np.concatenate([a["intr"], b["intr"]])
    dev = P.run(ctx, [none, b, a], o, pair_intr=pi, intr=intr)
    assert dev[0]["status"] == P.NO_MODEL and dev[0]["n_inliers"] == 0 and not dev[0]["pose"].any()
    assert not dev[0]["E"].any() and dev[0]["error_max"] == 0.0
    P.check_model(b, dev[1])
    P.check_motion(b, dev[1])
    assert not np.isin([5] + behind, dev[1]["inliers"]).any()
    P.identical(dev[2:], alone)
    P.compare_results(dev, P.run(None, [none, b, a], o, pair_intr=pi, intr=intr))


def test_argument_errors_come_before_the_device(ctx):
    p = P.make_pair(abi.SFM_CAM_PINHOLE, 20, 0.0, 171)
    with pytest.raises(api.SfmError) as ei:
        api.relpose(ctx, abi.SFM_CAM_PINHOLE, [p["xy"]], [0, 3], p["intr"], [P.WH4])
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG
    with pytest.raises(api.SfmError) as ei:
        api.relpose(ctx, abi.SFM_CAM_PINHOLE, [p["xy"]], [0, 0], p["intr"], [P.WH4], P.opts(max_iterations=-2))
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG


def test_chain_relpose_triangulate_resect(ctx):
    assert P.chain(ctx) <= P.MARGIN * P.CHAIN
