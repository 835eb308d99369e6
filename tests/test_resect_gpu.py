"""GPU: camera resection (sfm_resect) against its host twin and the numpy
reference of _resect_helpers.py: host against device, run against run, the
shapes at the workgroup-stride and sort-buffer boundaries, and the chain
gather -> resect -> triangulate on a synthetic scene."""
import numpy as np
import pytest

import _helpers as H
import _resect_helpers as R
import _tri_helpers as T

abi, api = R.abi, R.api
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("model", R.MODELS)
def test_shapes_host_device_and_rerun(ctx, model):
    """one call with every SHAPES size side by side: the device result passes
    the reference's checks, equals the host twin's (integers and inliers
    exactly, doubles to 1e-9) and a second device run bit for bit"""
    probs = R.shape_problems(model)
    o = R.opts(max_iterations=256)
    dev = R.run(ctx, probs, o)
    R.check_shapes(probs, dev)
    R.compare_results(dev, R.run(None, probs, o))
    R.identical(dev, R.run(ctx, probs, o))


@pytest.mark.parametrize("model", R.MODELS)
def test_recovery_and_noise_free(ctx, model):
    p = R.make_problem(model, 300, 0.3, 11 + model)
    r = R.run(ctx, [p], R.opts(max_iterations=256))[0]
    R.check_model(p, r)
    R.check_refit(p, r)
    inl = r["inliers"]
    assert r["min_nfa"] < 0 and not p["outlier"][inl].any()
    assert (~p["outlier"][inl]).sum() >= 0.9 * (~p["outlier"]).sum()
    for iters in (1, 8):      # the device's P3P on its own
        q = R.make_problem(model, 60, 0.0, 21 + model, sigma=0.0)
        s = R.run(ctx, [q], R.opts(max_iterations=iters))[0]
        print(f"model {model}, {iters} iterations: error_max {s['error_max']:.3e} px, pose error "
              f"{R.pose_error(q, s['pose']):.3e}")
        assert s["status"] == R.OK and s["error_max"] <= 1e-6 and R.pose_error(q, s["pose"]) <= 1e-8


def test_sort_switch_sizes(ctx):
    """8192 correspondences sort in LDS, 8193 in global memory"""
    probs = [R.make_problem(abi.SFM_CAM_PINHOLE, n, 0.3, 31) for n in (8192, 8193)]
    o = R.opts(precision=float("inf"), max_iterations=32)
    dev = R.run(ctx, probs, o)
    for p, r in zip(probs, dev):
        R.check_model(p, r)
        assert not p["outlier"][r["inliers"]].any()
    R.compare_results(dev, R.run(None, probs, o))
    R.identical(dev, R.run(ctx, probs, o))


def test_bound_outliers_bad_pixels_and_intrinsics(ctx):
    model = abi.SFM_CAM_RADIAL3
    a = R.make_problem(model, 200, 0.3, 81)
    free = R.run(ctx, [a], R.opts(max_iterations=128))[0]
    prec = 0.6 * free["error_max"]
    cut = R.run(ctx, [a], R.opts(precision=prec, max_iterations=128))[0]
    R.check_model(a, cut, precision=prec)
    assert cut["error_max"] <= prec and cut["n_inliers"] < free["n_inliers"]
    # all outliers; a non-finite pixel and points behind the camera; shared and own intrinsics
    none = R.make_problem(model, 100, 1.0, 82)
    b = R.make_problem(model, 120, 0.2, 83)
    b["uv"][5] = np.nan
    behind = [3, 40, 77]
    P = b["X"][behind] @ b["R"].T + b["t"]
    P[:, 2] *= -1.0
    b["X"][behind] = (P - b["t"]) @ b["R"]
    o = R.opts(max_iterations=128)
    dev = R.run(ctx, [none, b, a], o, img_intr=[0, 1, 0], intr=np.concatenate([a["intr"], b["intr"]]))
    assert dev[0]["status"] == R.NO_MODEL and dev[0]["n_inliers"] == 0 and not dev[0]["pose"].any()
    R.check_model(b, dev[1])
    R.check_refit(b, dev[1])
    assert not np.isin([5] + behind, dev[1]["inliers"]).any()
    R.identical(dev[2:], [free])
    R.compare_results(dev, R.run(None, [none, b, a], o, img_intr=[0, 1, 0],
                                 intr=np.concatenate([a["intr"], b["intr"]])))


def test_argument_errors_come_before_the_device(ctx):
    p = R.make_problem(abi.SFM_CAM_PINHOLE, 20, 0.0, 71)
    with pytest.raises(api.SfmError) as ei:
        api.resect(ctx, abi.SFM_CAM_PINHOLE, [p["X"]], [p["uv"]], [3], p["intr"], [R.WH])
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG
    with pytest.raises(api.SfmError) as ei:
        api.resect(ctx, abi.SFM_CAM_PINHOLE, [p["X"]], [p["uv"]], [0], p["intr"], [R.WH], R.opts(max_iterations=-2))
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG


def test_chain_gather_resect_triangulate(ctx):
    """three held-out images of a noise-free scene, resected from the
    ground-truth points, land on the poses the generator observed from; the
    triangulation with those poses substituted keeps its points"""
    sc = H.Scene(12, 600, 4, seed=4321, noise=0.0, outliers=0.0)
    held = [2, 5, 9]
    off, X3, uv = api.resect_gather(sc.problem(), sc.gt_X, np.ones(sc.n_pt, bool), held)
    assert (np.diff(off) >= 50).all()
    res = api.resect(ctx, sc.model, [X3[off[q]:off[q + 1]] for q in range(3)],
                     [uv[off[q]:off[q + 1]] for q in range(3)], sc.img_intr[held], sc.gt_intr, [R.WH] * 3,
                     R.opts(max_iterations=64))
    extr = sc.gt_extr.copy().reshape(-1, 6)
    for q, im in enumerate(held):
        assert res[q]["status"] == R.OK
        d = np.abs(res[q]["pose"] - extr[im]).max()
        print(f"image {im}: {res[q]['n_inliers']} inliers of {off[q + 1] - off[q]}, |pose - truth| {d:.3e}")
        assert d <= 1e-9
        extr[im] = res[q]["pose"]
    tri = api.triangulate(ctx, sc.problem(), extr.reshape(-1), sc.gt_intr)
    assert (tri["status"] == T.OK).sum() >= sc.n_pt // 2
