"""CPU: camera resection (sfm_resect_host, sfm_resect_p3p, sfm_resect_gather)
against the numpy reference of _resect_helpers.py.  Every check takes what the
library reports and recomputes what must follow from it; none depends on how
the search is implemented."""
import ctypes as C

import numpy as np
import pytest

import _helpers as H
import _resect_helpers as R

abi, api = R.abi, R.api
SEEDS = {abi.SFM_CAM_PINHOLE: 11, abi.SFM_CAM_SNAVELY: 12, abi.SFM_CAM_RADIAL3: 13}
_cache = {}


def solved(model):
    """300 correspondences, 30 % outliers, 256 iterations: computed once"""
    if model not in _cache:
        p = R.make_problem(model, 300, 0.3, SEEDS[model])
        _cache[model] = (p, R.run(None, [p], R.opts(max_iterations=256))[0])
    return _cache[model]


@pytest.mark.parametrize("model", R.MODELS)
def test_p3p_property(model):
    worst_o = worst_c = worst_p = 0.0
    for b, X, Rt, t in R.p3p_triplets(model):
        models = api.resect_p3p(b, X)
        assert 1 <= len(models) <= 4
        best = np.inf
        for Rm, tm in models:
            worst_o = max(worst_o, np.abs(Rm.T @ Rm - np.eye(3)).max(), abs(np.linalg.det(Rm) - 1.0))
            P = X @ Rm.T + tm
            u = P / np.linalg.norm(P, axis=1)[:, None]
            worst_c = max(worst_c, np.linalg.norm(np.cross(u, b), axis=1).max())
            assert (np.einsum("ij,ij->i", P, b) > 0).all()        # all three distances positive
            best = min(best, max(np.abs(Rm - Rt).max(), np.abs(tm - t).max()))
        worst_p = max(worst_p, best)
    print(f"P3P model {model}: orthonormality {worst_o:.3e}, cross product {worst_c:.3e}, true pose {worst_p:.3e}")
    assert worst_o <= 1e-12
    assert worst_c <= 1e-9
    assert worst_p <= 1e-7


def test_p3p_degenerate_samples():
    b, X, _, _ = R.p3p_triplets(abi.SFM_CAM_PINHOLE, 1)[0]
    line = np.stack([X[0], X[1], X[0] + 2.5 * (X[1] - X[0])])
    assert api.resect_p3p(b, line) == []
    assert api.resect_p3p(b, np.stack([X[0], X[1], X[1]])) == []
    assert api.resect_p3p(b, np.stack([X[0], X[0], X[0]])) == []


@pytest.mark.parametrize("model", R.MODELS)
def test_nfa_self_consistency(model):
    p, r = solved(model)
    R.check_model(p, r)


@pytest.mark.parametrize("model", R.MODELS)
def test_refit(model):
    p, r = solved(model)
    R.check_refit(p, r)


@pytest.mark.parametrize("model", R.MODELS)
def test_recovery(model):
    """30 % outliers, 256 iterations: no generated outlier among the inliers, at
    least 90 % of the true inliers found, min_nfa < 0.  Observed on the host
    twin with these seeds: 99.0 % (pinhole), 99.5 % (SNAVELY), 98.1 % (RADIAL3)
    of the true inliers."""
    p, r = solved(model)
    inl = r["inliers"]
    share = (~p["outlier"][inl]).sum() / (~p["outlier"]).sum()
    print(f"model {model}: {len(inl)} inliers, {share:.1%} of the true inliers, min_nfa {r['min_nfa']:.2f}, "
          f"error_max {r['error_max']:.3f} px, pose error {R.pose_error(p, r['pose']):.3e}")
    assert r["status"] == R.OK and r["min_nfa"] < 0
    assert not p["outlier"][inl].any()
    assert share >= 0.9


@pytest.mark.parametrize("model", R.MODELS)
@pytest.mark.parametrize("iters", [1, 8])
def test_noise_free(model, iters):
    p = R.make_problem(model, 60, 0.0, 21 + model, sigma=0.0)
    r = R.run(None, [p], R.opts(max_iterations=iters))[0]
    print(f"model {model}, {iters} iterations: error_max {r['error_max']:.3e} px, pose error "
          f"{R.pose_error(p, r['pose']):.3e}")
    assert r["status"] == R.OK and r["n_inliers"] == 60
    assert r["error_max"] <= 1e-6
    assert R.pose_error(p, r["pose"]) <= 1e-8


@pytest.mark.parametrize("model", R.MODELS)
def test_shapes_in_one_call(model):
    probs = R.shape_problems(model)
    R.check_shapes(probs, R.run(None, probs, R.opts(max_iterations=256)))


@pytest.mark.parametrize("n", [8192, 8193])
def test_sort_switch_sizes(n):
    p = R.make_problem(abi.SFM_CAM_PINHOLE, n, 0.3, 31)
    r = R.run(None, [p], R.opts(precision=float("inf"), max_iterations=32))[0]
    R.check_model(p, r)
    assert not p["outlier"][r["inliers"]].any()


def test_finite_precision_cuts_the_sort_short():
    p, free = solved(abi.SFM_CAM_PINHOLE)
    prec = 0.6 * free["error_max"]
    r = R.run(None, [p], R.opts(precision=prec, max_iterations=256))[0]
    R.check_model(p, r, precision=prec)
    assert r["error_max"] <= prec and r["n_inliers"] < free["n_inliers"]


def test_all_outliers_give_no_model():
    p = R.make_problem(abi.SFM_CAM_PINHOLE, 100, 1.0, 41)
    r = R.run(None, [p], R.opts(max_iterations=64))[0]
    assert r["status"] == R.NO_MODEL and r["n_inliers"] == 0 and r["iterations"] > 0
    assert not r["pose"].any() and not r["pose_model"].any() and len(r["inliers"]) == 0


@pytest.mark.parametrize("model", R.MODELS)
def test_non_finite_pixel_and_points_behind(model):
    p = R.make_problem(model, 120, 0.2, 43 + model)
    p["uv"][5] = np.nan
    p["uv"][17, 0] = np.inf
    behind = [3, 40, 77]
    P = p["X"][behind] @ p["R"].T + p["t"]
    P[:, 2] *= -1.0
    p["X"][behind] = (P - p["t"]) @ p["R"]
    p["outlier"][[5, 17] + behind] = True
    r = R.run(None, [p], R.opts(max_iterations=128))[0]
    R.check_model(p, r)
    R.check_refit(p, r)
    assert not np.isin([5, 17] + behind, r["inliers"]).any()
    # three finite bearings in all: FEW
    q = R.make_problem(model, 10, 0.0, 47)
    q["uv"][3:] = np.nan
    assert R.run(None, [q])[0]["status"] == R.FEW


def test_shared_and_own_intrinsics():
    a = R.make_problem(abi.SFM_CAM_PINHOLE, 80, 0.2, 61)
    b = R.make_problem(abi.SFM_CAM_PINHOLE, 90, 0.2, 62)
    o = R.opts(max_iterations=64)
    own = R.run(None, [a, b], o)
    shared = R.run(None, [a, b], o, img_intr=[0, 0], intr=a["intr"])
    swapped = R.run(None, [a, b], o, img_intr=[1, 0], intr=np.concatenate([b["intr"], a["intr"]]))
    R.identical(own, shared)
    R.identical(own, swapped)
    # a second block that differs is the one image 1 reads
    other = a["intr"] * np.array([1.05, 1.05, 1.0, 1.0])
    moved = R.run(None, [a, b], o, img_intr=[0, 1], intr=np.concatenate([a["intr"], other]))
    R.identical(own[:1], moved[:1])
    assert not np.array_equal(own[1]["pose"], moved[1]["pose"])


def test_argument_errors():
    lib = abi.load()
    p = R.make_problem(abi.SFM_CAM_PINHOLE, 20, 0.0, 71)
    off = np.array([0, 20], np.int64)
    X, uv = np.ascontiguousarray(p["X"]), np.ascontiguousarray(p["uv"])
    ii, wh = np.zeros(1, np.int32), np.array(R.WH, np.int32)
    res, inl = (abi.ResectResult * 1)(), np.zeros(20, np.int32)
    P = abi.ptr

    def call(cm=0, n_img=1, off=off, X=X, uv=uv, ii=ii, intr=p["intr"], n_intr=1, wh=wh, o=None, res=res, inl=inl):
        return lib.sfm_resect_host(cm, n_img, P(off, abi.i64p), P(X, abi.f64p), P(uv, abi.f64p), P(ii, abi.i32p),
                                   P(intr, abi.f64p), n_intr, P(wh, abi.i32p), C.byref(o) if o else None, res,
                                   P(inl, abi.i32p))

    assert call() == abi.SFM_OK
    bad = abi.SFM_ERR_INVALID_ARG
    assert call(n_img=-1) == bad and call(n_intr=-1) == bad and call(cm=9) == bad
    assert call(off=np.array([0, -1], np.int64)) == bad and call(off=np.array([1, 20], np.int64)) == bad
    for k in ("off", "X", "uv", "ii", "intr", "wh", "res", "inl"):
        assert call(**{k: None}) == bad, k
    assert call(ii=np.ones(1, np.int32)) == bad and call(wh=np.array([0, 5], np.int32)) == bad
    assert call(o=R.opts(max_iterations=0)) == bad and call(o=R.opts(refine_iterations=-1)) == bad
    assert call(o=R.opts(precision=float("nan"))) == bad
    assert call(n_img=0, off=None, X=None, uv=None, ii=None, wh=None, res=None, inl=None) == abi.SFM_OK
    # the device entry point checks before any device call: no context, no device
    assert lib.sfm_resect(None, 0, 1, P(off, abi.i64p), P(X, abi.f64p), P(uv, abi.f64p), P(ii, abi.i32p),
                          P(p["intr"], abi.f64p), 1, P(wh, abi.i32p), None, res, P(inl, abi.i32p)) == bad
    d = api.resect_default_options()
    assert (d.precision, d.max_iterations, d.refine_iterations) == (0.0, 4096, 10)


def test_gather():
    sc = H.Scene(8, 120, 3, seed=77)
    ok = np.ones(sc.n_pt, bool)
    ok[::5] = False
    images = [6, 2]
    off, X3, uv = api.resect_gather(sc.problem(), sc.gt_X, ok, images)
    pt_of = np.repeat(np.arange(sc.n_pt), np.diff(sc.pt_offsets))
    for q, im in enumerate(images):
        sel = np.flatnonzero((sc.obs_img == im) & ok[pt_of])
        assert off[q + 1] - off[q] == len(sel) > 0
        np.testing.assert_array_equal(X3[off[q]:off[q + 1]], sc.gt_X.reshape(-1, 3)[pt_of[sel]])
        np.testing.assert_array_equal(uv[off[q]:off[q + 1]], sc.obs_uv.reshape(-1, 2)[sel])
    counts = np.diff(api.resect_gather(sc.problem(), sc.gt_X, ok, np.arange(sc.n_cam), counts_only=True))
    np.testing.assert_array_equal(counts, np.bincount(sc.obs_img[ok[pt_of]], minlength=sc.n_cam))
    with pytest.raises(api.SfmError):
        api.resect_gather(sc.problem(), sc.gt_X, ok, [1, 1])
    with pytest.raises(api.SfmError):
        api.resect_gather(sc.problem(), sc.gt_X, ok, [sc.n_cam])


def test_cpp_resect_facade():
    import os
    import subprocess
    exe = os.path.join(H.ROOT, "tests", "cpp", "resect_test")
    assert os.path.exists(exe), "run make (builds tests/cpp/resect_test)"
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
