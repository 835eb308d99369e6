"""CPU: relative pose (sfm_relpose_host, sfm_relpose_5pt) against the numpy
reference of _relpose_helpers.py.  Every check takes what the library reports
and recomputes what must follow from it; none depends on how the search is
implemented."""
import ctypes as C

import numpy as np
import pytest

import _helpers as H
import _relpose_helpers as P

abi, api = P.abi, P.api
SEEDS = {abi.SFM_CAM_PINHOLE: 111, abi.SFM_CAM_SNAVELY: 112, abi.SFM_CAM_RADIAL3: 113}
_cache = {}


def solved(model):
    """300 correspondences, 30 % outliers, 256 iterations: computed once"""
    if model not in _cache:
        p = P.make_pair(model, 300, 0.3, SEEDS[model])
        _cache[model] = (p, P.run(None, [p], P.opts(max_iterations=256))[0])
    return _cache[model]


@pytest.mark.parametrize("model", P.MODELS)
def test_fivept_property(model):
    worst_c = worst_e = worst_t = 0.0
    for bI, bJ, Et in P.fivept_samples(model):
        Es = api.relpose_5pt(bI, bJ)
        assert 1 <= len(Es) <= 10
        best = np.inf
        for E in Es:
            assert abs(np.linalg.norm(E) - np.sqrt(2.0)) <= 1e-12
            worst_c = max(worst_c, P.constraint_residual(E))
            worst_e = max(worst_e, np.abs(np.einsum("ij,jk,ik->i", bJ, E, bI)).max())
            best = min(best, np.abs(E - Et).max(), np.abs(E + Et).max())
        worst_t = max(worst_t, best)
    print(f"five-point model {model}: constraints {worst_c:.3e}, epipolar {worst_e:.3e}, true E {worst_t:.3e}")
    assert worst_c <= P.MARGIN * P.FIVEPT_CONSTRAINT
    assert worst_e <= P.MARGIN * P.FIVEPT_EPIPOLAR
    assert worst_t <= P.MARGIN * P.FIVEPT_TRUE_E


def test_fivept_degenerate_samples():
    bI, bJ, _ = P.fivept_samples(abi.SFM_CAM_PINHOLE, 1)[0]
    rep = [0, 1, 2, 3, 1]
    assert api.relpose_5pt(bI[rep], bJ[rep]) == []
    assert api.relpose_5pt(bI[[2] * 5], bJ[[2] * 5]) == []


@pytest.mark.parametrize("model", P.MODELS)
def test_nfa_self_consistency(model):
    p, r = solved(model)
    P.check_model(p, r)


@pytest.mark.parametrize("model", P.MODELS)
def test_motion_self_consistency(model):
    p, r = solved(model)
    P.check_motion(p, r)


@pytest.mark.parametrize("model", P.MODELS)
def test_recovery(model):
    """30 % outliers, 256 iterations: no generated outlier among the inliers, at
    least 90 % of the true inliers found, min_nfa < 0, the motion near truth.
    Observed on the host twin with these seeds: 97.1 % (pinhole), 95.7 %
    (SNAVELY), 100.0 % (RADIAL3) of the true inliers."""
    p, r = solved(model)
    inl = r["inliers"]
    share = (~p["outlier"][inl]).sum() / (~p["outlier"]).sum()
    rot, dirn = P.pose_errors(p, r)
    print(f"model {model}: {len(inl)} inliers, {share:.1%} of the true inliers, min_nfa {r['min_nfa']:.2f}, "
          f"error_max {r['error_max']:.3f} px, rotation {rot:.3e} rad, direction of t {dirn:.3e} rad")
    assert r["status"] == P.OK and r["min_nfa"] < 0
    assert not p["outlier"][inl].any()
    assert share >= 0.9
    assert rot <= P.MARGIN * P.RECOVERY_ROT and dirn <= P.MARGIN * P.RECOVERY_DIR


@pytest.mark.parametrize("model", P.MODELS)
@pytest.mark.parametrize("iters", [1, 8])
def test_noise_free(model, iters):
    p = P.make_pair(model, 60, 0.0, 121 + model, sigma=0.0)
    r = P.run(None, [p], P.opts(max_iterations=iters))[0]
    rot, dirn = P.pose_errors(p, r)
    print(f"model {model}, {iters} iterations: error_max {r['error_max']:.3e} px, rotation {rot:.3e}, t {dirn:.3e}")
    assert r["status"] == P.OK and r["n_inliers"] == 60 and r["n_front"] == 60
    assert r["error_max"] <= 1e-6
    assert max(rot, dirn) <= P.MARGIN * P.NOISE_FREE_POSE


@pytest.mark.parametrize("model", P.MODELS)
def test_shapes_in_one_call(model):
    pairs = P.shape_pairs(model)
    P.check_shapes(pairs, P.run(None, pairs, P.opts(max_iterations=256)))


@pytest.mark.parametrize("n", [8192, 8193])
def test_sort_switch_sizes(n):
    p = P.make_pair(abi.SFM_CAM_PINHOLE, n, 0.3, 131)
    r = P.run(None, [p], P.opts(precision=0.0, max_iterations=32))[0]
    P.check_model(p, r, precision=0.0)
    assert not p["outlier"][r["inliers"]].any()


def test_pure_rotation_has_no_parallax():
    p = P.make_pair(abi.SFM_CAM_PINHOLE, 300, 0.1, 141, t=np.zeros(3))
    r = P.run(None, [p], P.opts(max_iterations=256))[0]
    print(f"status {r['status']}, {r['n_inliers']} inliers, {r['n_front']} in front, angle {r['angle_median']:.4f} deg")
    assert r["status"] in (P.OK, P.AMBIGUOUS) and r["angle_median"] < 3.0
    P.check_model(p, r)
    P.check_motion(p, r)


@pytest.mark.parametrize("model", P.MODELS)
def test_forward_motion(model):
    fwd = np.array([0.0, 0.0, -1.0 if model == abi.SFM_CAM_SNAVELY else 1.0])
    p = P.make_pair(model, 300, 0.2, 145 + model, w=[0.02, -0.03, 0.01], t=fwd)
    r = P.run(None, [p], P.opts(max_iterations=256))[0]
    rot, dirn = P.pose_errors(p, r)
    print(f"model {model}: {r['n_inliers']} inliers, {r['n_front']} in front, rotation {rot:.3e}, t {dirn:.3e}")
    assert r["status"] == P.OK and r["n_front"] == r["n_inliers"]
    P.check_motion(p, r)
    assert not p["outlier"][r["inliers"]].any()
    assert rot <= P.MARGIN * P.RECOVERY_ROT and dirn <= P.MARGIN * P.RECOVERY_DIR


def test_ambiguous_vote_keeps_E_and_inliers():
    p, ok = solved(abi.SFM_CAM_PINHOLE)
    r = P.run(None, [p], P.opts(max_iterations=256, front_ratio=0.0))[0]
    assert r["status"] == P.AMBIGUOUS and not r["pose"].any() and r["n_front"] == 0 and r["angle_median"] == 0.0
    np.testing.assert_array_equal(r["E"], ok["E"])
    np.testing.assert_array_equal(r["inliers"], ok["inliers"])
    assert r["min_nfa"] == ok["min_nfa"] and r["error_max"] == ok["error_max"]
    P.check_motion(p, r, front_ratio=0.0)


def test_all_outliers_give_no_model():
    p = P.make_pair(abi.SFM_CAM_PINHOLE, 100, 1.0, 151)
    r = P.run(None, [p], P.opts(max_iterations=64))[0]
    assert r["status"] == P.NO_MODEL and r["n_inliers"] == 0 and r["iterations"] > 0
    assert not r["pose"].any() and not r["E"].any() and len(r["inliers"]) == 0


def test_non_finite_pixels_and_few():
    p = P.make_pair(abi.SFM_CAM_RADIAL3, 120, 0.2, 153)
    p["xy"][5, 0] = np.nan
    p["xy"][17, 3] = np.inf
    p["outlier"][[5, 17]] = True
    r = P.run(None, [p], P.opts(max_iterations=128))[0]
    P.check_model(p, r)
    P.check_motion(p, r)
    assert not np.isin([5, 17], r["inliers"]).any()
    q = P.make_pair(abi.SFM_CAM_RADIAL3, 10, 0.0, 157)
    q["xy"][5:, 1] = np.nan          # five pairs of finite bearings in all
    assert P.run(None, [q])[0]["status"] == P.FEW


def test_shared_and_own_intrinsics():
    a = P.make_pair(abi.SFM_CAM_PINHOLE, 80, 0.2, 161)
    b = P.make_pair(abi.SFM_CAM_PINHOLE, 90, 0.2, 162)
    o = P.opts(max_iterations=64)
    own = P.run(None, [a, b], o)
    shared = P.run(None, [a, b], o, pair_intr=[0, 0, 0, 0], intr=a["intr"])
    P.identical(own, shared)
    # image J of the second pair reads a block of its own
    other = a["intr"] * np.array([1.05, 1.05, 1.0, 1.0])
    moved = P.run(None, [a, b], o, pair_intr=[0, 0, 0, 1], intr=np.concatenate([a["intr"], other]))
    P.identical(own[:1], moved[:1])
    assert not np.array_equal(own[1]["E"], moved[1]["E"])
    b2 = dict(b, intrJ=other)
    P.check_model(b2, moved[1])
    P.check_motion(b2, moved[1])


def test_argument_errors():
    lib = abi.load()
    p = P.make_pair(abi.SFM_CAM_PINHOLE, 20, 0.0, 171)
    off = np.array([0, 20], np.int64)
    xy = np.ascontiguousarray(p["xy"])
    ii, wh = np.zeros(2, np.int32), np.array(P.WH4, np.int32)
    res, inl = (abi.RelposeResult * 1)(), np.zeros(20, np.int32)
    Q = abi.ptr

    def call(cm=0, n_pairs=1, off=off, xy=xy, ii=ii, intr=p["intr"], n_intr=1, wh=wh, o=None, res=res, inl=inl):
        return lib.sfm_relpose_host(cm, n_pairs, Q(off, abi.i64p), Q(xy, abi.f64p), Q(ii, abi.i32p), Q(intr, abi.f64p),
                                    n_intr, Q(wh, abi.i32p), C.byref(o) if o else None, res, Q(inl, abi.i32p))

    assert call() == abi.SFM_OK
    bad = abi.SFM_ERR_INVALID_ARG
    assert call(n_pairs=-1) == bad and call(n_intr=-1) == bad and call(cm=9) == bad
    assert call(off=np.array([0, -1], np.int64)) == bad and call(off=np.array([1, 20], np.int64)) == bad
    for k in ("off", "xy", "ii", "intr", "wh", "res", "inl"):
        assert call(**{k: None}) == bad, k
    assert call(ii=np.array([0, 1], np.int32)) == bad and call(wh=np.array([5, 5, 0, 5], np.int32)) == bad
    assert call(o=P.opts(max_iterations=0)) == bad and call(o=P.opts(front_ratio=float("nan"))) == bad
    assert call(o=P.opts(precision=float("nan"))) == bad
    assert call(n_pairs=0, off=None, xy=None, ii=None, wh=None, res=None, inl=None) == abi.SFM_OK
    # the device entry point checks before any device call: no context, no device
    assert lib.sfm_relpose(None, 0, 1, Q(off, abi.i64p), Q(xy, abi.f64p), Q(ii, abi.i32p), Q(p["intr"], abi.f64p), 1,
                           Q(wh, abi.i32p), None, res, Q(inl, abi.i32p)) == bad
    d = api.relpose_default_options()
    assert (d.precision, d.max_iterations, d.front_ratio) == (4.0, 4096, 0.7)


def test_chain_on_the_host():
    assert P.chain(None) <= P.MARGIN * P.CHAIN


def test_cpp_relpose_facade():
    import os
    import subprocess
    exe = os.path.join(H.ROOT, "tests", "cpp", "relpose_test")
    assert os.path.exists(exe), "run make (builds tests/cpp/relpose_test)"
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
