"""GPU: post-BA outlier rejection (sfm_ba_wash, sfm_ba_plan_wash; kernels in
csrc/ba_wash.hip) against the numpy fp64 reference of _wash_helpers.

Tolerances: residual 1e-9 px and max angle 1e-9 deg absolute (fp64 eps 2.2e-16
x pixel magnitudes <= 4e3 x tens of operations ~ 1e-11, two decades of
margin); masks and every count exact.  Every threshold sits in the middle of
a gap (> 1e-6) of the reference's own values, so no comparison is on a
borderline and nothing is excluded from it."""
import ctypes as C

import numpy as np
import pytest

import _helpers as H
import _wash_helpers as W

pytestmark = pytest.mark.gpu
abi, api = H.abi, W.api


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _flip_z(sc):
    """the same scene seen by cameras looking down -z: X -> -X, t -> -t negates
    every P = R X + t, which SFM_CAM_SNAVELY's p = -P / P2 does not see"""
    for a in (sc.X, sc.gt_X):
        a *= -1.0
    for a in (sc.extr, sc.gt_extr):
        a.reshape(-1, 6)[:, 3:] *= -1.0
    return sc


def _shuffled(sc, seed=3):
    """every point's observations in a random order"""
    rng = np.random.default_rng(seed)
    perm = np.concatenate([sc.pt_offsets[p] + rng.permutation(sc.pt_offsets[p + 1] - sc.pt_offsets[p])
                           for p in range(sc.n_pt)])
    sc.obs_img = np.ascontiguousarray(sc.obs_img[perm])
    sc.obs_uv = np.ascontiguousarray(sc.obs_uv.reshape(-1, 2)[perm].reshape(-1))
    return sc


# name -> (scene, blend of ground truth and the perturbed start the wash is evaluated at)
SCENES = {
    "band": (lambda: H.Scene(12, 600, 4, outliers=0.05), 0.1),                 # chunk points
    "long_tracks": (lambda: H.Scene(40, 120, 16, outliers=0.05), 0.2),         # general points (gobs_perm)
    "random_shuffled": (lambda: _shuffled(H.Scene(30, 400, 6, vis_mode=1, outliers=0.05, seed=11)), 0.1),
    "radial3": (lambda: H.Scene(12, 400, 4, n_intr=12, model=abi.SFM_CAM_RADIAL3, outliers=0.05), 0.1),
    "snavely": (lambda: _flip_z(H.Scene(12, 400, 4, model=abi.SFM_CAM_SNAVELY, outliers=0.05)), 0.3),
}
_cache = {}


def _case(name):
    """(scene, parameters, placed options, reference), computed once"""
    if name not in _cache:
        mk, alpha = SCENES[name]
        sc = mk()
        e, i, x = W.blend(sc, alpha)
        o, ref = W.placed_opts(sc, e, i, x)
        _cache[name] = (sc, (e, i, x), o, ref)
    return _cache[name]


@pytest.mark.parametrize("name", list(SCENES))
def test_parity_one_shot(ctx, name):
    sc, (e, i, x), o, ref = _case(name)
    W.assert_not_vacuous(ref)           # the reference alone: some of every rule
    if name == "snavely":               # cameras look down -z: cheirality keeps the inliers
        assert (ref["depth"] < 0).all() and ref["stats"]["n_obs_depth"] == 0
    if name == "long_tracks":
        assert api.ba_describe(sc.problem()).n_general_pts == sc.n_pt
    if name == "band":
        assert api.ba_describe(sc.problem()).n_chunk_pts == sc.n_pt
    got = api.ba_wash(ctx, sc.problem(), e, i, x, W.abi_opts(o))
    W.compare(got, ref)


class _Arrays:
    """a problem assembled from per-point observation lists"""

    def __init__(self, sc, tracks, X):
        self.n_cam, self.n_intr, self.model = sc.n_cam, sc.n_intr, sc.model
        self.img_intr, self.const_img, self.huber = sc.img_intr, sc.const_img, sc.huber
        self.n_pt = len(tracks)
        self.pt_offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
        self.n_obs = int(self.pt_offsets[-1])
        flat = [ob for t in tracks for ob in t]
        self.obs_img = np.array([ob[0] for ob in flat], np.int32)
        self.obs_uv = np.array([ob[1] for ob in flat], np.float64).reshape(-1)
        self.X = np.ascontiguousarray(X, np.float64).reshape(-1)

    problem = H.Scene.problem


def _tracks(sc):
    uv = sc.obs_uv.reshape(-1, 2)
    return [[(int(sc.obs_img[o]), uv[o].copy()) for o in range(sc.pt_offsets[p], sc.pt_offsets[p + 1])]
            for p in range(sc.n_pt)]


def test_hand_built_shapes(ctx):
    sc = H.Scene(6, 60, 3, outliers=0.05)
    e, i, x = W.blend(sc, 0.05)
    X = x.reshape(-1, 3).copy()
    tr = [[ob for ob in t if ob[0] != 5] for t in _tracks(sc)]     # image 5 unobserved
    assert all(len(t) >= 2 for t in tr[:5])
    tr[0] = tr[0][:1]                                               # one observation
    tr[1] = tr[1] + [tr[1][0]]                                      # twice by the same image
    tr[2] = [tr[2][0], (tr[2][0][0], tr[2][0][1] + 0.3)]            # only twice by the same image
    # point 3 reflected through the centre of its first camera: P -> -P there
    # (behind it, same projection); point 4 has a NaN coordinate
    R = W.rotations(e)[tr[3][0][0]]
    cen = -R.T @ e.reshape(-1, 6)[tr[3][0][0], 3:]
    X[3] = 2 * cen - X[3]
    X[4, 1] = np.nan
    pr = _Arrays(sc, tr, X)
    o, ref = W.placed_opts(pr, e, i, pr.X)
    o3 = pr.pt_offsets[3]
    assert ref["norm"][o3] < o["max_residual_px"] and ref["depth"][o3] < 0      # an inlier but for its depth
    assert ref["code"][o3] == W.DEPTH
    got = api.ba_wash(ctx, pr.problem(), e, i, pr.X, W.abi_opts(o))
    W.compare(got, ref)
    assert not got["keep_pt"][0] and not got["keep_obs"][0]                     # short
    assert got["max_angle"][2] == 0.0 and ref["max_angle"][2] == 0.0            # one image: angle exactly 0
    assert not got["keep_obs"][o3]
    a4, b4 = pr.pt_offsets[4], pr.pt_offsets[5]
    assert (ref["code"][a4:b4] == W.DEPTH).all() and ref["removed"][4] == W.SHORT
    assert not got["keep_pt"][4] and not got["keep_obs"][a4:b4].any() and np.isnan(got["residual"][a4:b4]).all()
    # without the cheirality rule the reflected observation is judged by its residual alone
    o0 = dict(o, cheirality=0)
    ref0 = W.ref_wash(pr, e, i, pr.X, o0)
    assert ref0["code"][o3] == 0
    got0 = api.ba_wash(ctx, pr.problem(), e, i, pr.X, W.abi_opts(o0))
    W.compare(got0, ref0)
    assert got0["stats"]["n_obs_depth"] == b4 - a4                              # the NaN point's only


def test_wave_boundaries_of_the_point_pass(ctx):
    """points of exactly 64, 65 and 130 observations (one, two and three rounds
    of a wave), next to short ones and one without observations"""
    sc = H.Scene(130, 24, 130, outliers=0.05)
    assert (np.diff(sc.pt_offsets) == 130).all()
    e, i, x = W.blend(sc, 0.1)
    tr = _tracks(sc)
    for p, n in {0: 64, 1: 65, 3: 3, 4: 16, 5: 17, 6: 1, 7: 0, 9: 63, 10: 128, 11: 129}.items():
        tr[p] = tr[p][:n]
    pr = _Arrays(sc, tr, x)
    assert [len(t) for t in tr[:3]] == [64, 65, 130]
    o, ref = W.placed_opts(pr, e, i, pr.X)
    assert ref["stats"]["n_obs_residual"] >= 1 and ref["stats"]["n_pt_angle"] >= 1 and ref["stats"]["n_pt_kept"] >= 1
    got = api.ba_wash(ctx, pr.problem(), e, i, pr.X, W.abi_opts(o))
    W.compare(got, ref)


def test_long_run_of_points_without_observations(ctx):
    """more empty points in a row than an observation workgroup's offset window"""
    sc = H.Scene(6, 60, 3, outliers=0.05)
    e, i, x = W.blend(sc, 0.05)
    tr = _tracks(sc)
    tr = tr[:20] + [[] for _ in range(300)] + tr[20:]
    X = np.concatenate([x.reshape(-1, 3)[:20], np.zeros((300, 3)), x.reshape(-1, 3)[20:]])
    pr = _Arrays(sc, tr, X)
    o, ref = W.placed_opts(pr, e, i, pr.X)
    assert ref["stats"]["n_pt_short"] >= 300
    W.compare(api.ba_wash(ctx, pr.problem(), e, i, pr.X, W.abi_opts(o)), ref)


def _huber_cost(r, a=4.0):
    s = (r ** 2).sum(1)
    return 0.5 * np.where(s <= a * a, s, 2 * a * np.sqrt(s) - a * a).sum()


@pytest.fixture(scope="module", params=["band", "long_tracks"])
def solved(ctx, request):
    sc = SCENES[request.param][0]()
    plan = api.BAPlan(ctx, sc.problem(), *sc.params())
    rc, s = plan.run()
    assert rc == 0 and s.usable
    yield sc, plan, s
    plan.close()


def test_resident_equals_one_shot(ctx, solved):
    sc, plan, _ = solved
    e, i, x = plan.download()
    o, ref = W.placed_opts(sc, e, i, x)
    res = plan.wash(W.abi_opts(o))
    one = api.ba_wash(ctx, sc.problem(), e, i, x, W.abi_opts(o))
    for k in ("residual", "max_angle", "keep_obs", "keep_pt"):
        np.testing.assert_array_equal(res[k], one[k], err_msg=k)      # bit for bit
    assert res["stats"] == one["stats"]
    W.compare(res, ref)
    again = plan.wash(W.abi_opts(o))                                   # the kept maps and scratch
    for k in ("residual", "max_angle", "keep_obs", "keep_pt"):
        np.testing.assert_array_equal(again[k], res[k], err_msg=k)
    assert again["stats"] == res["stats"]


def test_residual_is_the_solvers(ctx, solved):
    sc, plan, s = solved
    r = plan.wash()["residual"]
    cost = _huber_cost(r, sc.huber)
    e, i, x = plan.download()
    orc = H.oracle_cost(sc, e, i, x)
    print(f"cost from wash residuals {cost!r}, final_cost {s.final_cost!r}, oracle {orc!r}")
    assert abs(cost - s.final_cost) <= 1e-9 * s.final_cost
    assert abs(cost - orc) <= 1e-9 * orc


def test_round_trip_solve_wash_apply_solve(ctx):
    sc = H.Scene(12, 600, 4, outliers=0.05)
    pr = sc.problem()
    e, i, x = sc.params()
    rc, s1 = api.ba_solve(ctx, pr, e, i, x)
    assert rc == 0 and s1.usable
    w1 = api.ba_wash(ctx, pr, e, i, x)
    rejected1 = w1["stats"]["n_obs_depth"] + w1["stats"]["n_obs_residual"]
    assert rejected1 > 0 and w1["stats"]["n_pt_kept"] > 0
    pr2, x2, pt_map = api.ba_wash_apply(pr, x, w1["keep_obs"], w1["keep_pt"])
    assert (pr2.n_pt, pr2.n_obs) == (w1["stats"]["n_pt_kept"], w1["stats"]["n_obs_kept"])
    x2 = x2.copy()
    rc, s2 = api.ba_solve(ctx, pr2, e, i, x2)
    assert rc == 0 and s2.usable
    w2 = api.ba_wash(ctx, pr2, e, i, x2)
    rejected2 = w2["stats"]["n_obs_depth"] + w2["stats"]["n_obs_residual"]
    print(f"rmse {s1.rmse_final} -> {s2.rmse_final}, rejected observations {rejected1} -> {rejected2}")
    assert s2.rmse_final < s1.rmse_final
    assert rejected2 < rejected1


def test_errors_and_null_outputs(ctx):
    sc, (e, i, x), o, ref = _case("band")
    pr = sc.problem()
    p = abi.ptr
    args = (ctx.h, C.byref(pr), p(e, abi.f64p), p(i, abi.f64p), p(x, abi.f64p), C.byref(W.abi_opts(o)))
    st = abi.BAWashStats()
    assert ctx.lib.sfm_ba_wash(*args, None, None, None, None, C.byref(st)) == 0
    assert {f: getattr(st, f) for f, _ in abi.BAWashStats._fields_} == ref["stats"]
    assert ctx.lib.sfm_ba_wash(*args, None, None, None, None, None) == 0
    ko = np.zeros(sc.n_obs, np.uint8)
    assert ctx.lib.sfm_ba_wash(*args, None, None, p(ko, abi.u8p), None, None) == 0
    np.testing.assert_array_equal(ko.astype(bool), ref["keep_obs"])
    bad = W.abi_opts(dict(o, min_track_len=0))
    with pytest.raises(api.SfmError) as ei:
        api.ba_wash(ctx, pr, e, i, x, bad)
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG
    plan = api.BAPlan(ctx, pr, e, i, x)
    try:
        # before any run: the parameters the plan was created with
        W.compare(plan.wash(W.abi_opts(o)), ref)
        assert ctx.lib.sfm_ba_plan_wash(plan.h, None, None, None, None, None, None) == 0
        with pytest.raises(api.SfmError) as ei:
            plan.wash(bad)
        assert ei.value.code == abi.SFM_ERR_INVALID_ARG
    finally:
        plan.close()


def test_sharded_plan_is_unsupported_one_shot_is_not():
    sc, (e, i, x), o, ref = _case("band")
    c2 = api.Context(0, rank=0, world_size=2, flags=abi.SFM_CTX_DIAG_NO_EXCHANGE)
    try:
        plan = api.BAPlan(c2, sc.problem(), e, i, x)
        with pytest.raises(api.SfmError) as ei:
            plan.wash()
        assert ei.value.code == abi.SFM_ERR_UNSUPPORTED
        plan.close()
        W.compare(api.ba_wash(c2, sc.problem(), e, i, x, W.abi_opts(o)), ref)   # the whole problem on any rank
    finally:
        c2.close()
