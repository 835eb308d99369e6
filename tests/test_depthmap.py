"""CPU: the depth maps' host twins (sfm_depthmap_host, sfm_depthmap_filter_host)
against the numpy restatement of the contract (_depthmap_helpers.py), byte for
byte and count for count; view selection against its restatement; that no
pixel's cost rises with another iteration; accuracy on rendered planes; the
argument checks; the stand-alone host program."""
import os
import subprocess

import numpy as np
import pytest

import _depthmap_helpers as DH

abi, api = DH.abi, DH.api
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 7


def test_cost_of_given_planes_equals_the_restatement():
    """iterations = 0 with the ground-truth planes: the cost evaluation alone"""
    fx = DH.small_fixture()
    res = fx.run(None, DH.opts(2, 0, 2, SEED), init=True)
    DH.check_against_ref(res, DH.reference("small", 2, 0, SEED, True))
    est = res["cost_maps"][1][2:-2, 2:-2]
    assert (est < 2).any() and res["stats"]["n_estimated"] == 3 * 20 * 16
    assert (res["cost_maps"][0][:2] == 2).all() and (res["depth_maps"][0][:2] == 0).all()


def test_random_planes_one_iteration_equals_the_restatement():
    """random init, propagation, refinement and the numbering of the draws"""
    fx = DH.small_fixture()
    res = fx.run(None, DH.opts(2, 1, 2, SEED))
    DH.check_against_ref(res, DH.reference("small", 2, 1, SEED, False))
    other = fx.run(None, DH.opts(2, 1, 2, SEED + 1))
    assert other["depth"].tobytes() != res["depth"].tobytes()
    n = res["normal"].reshape(-1, 3)[res["depth"] > 0]
    assert np.allclose(np.linalg.norm(n, axis=1), 1, atol=1e-6) and (n[:, 2] < 0).all()


def test_filter_equals_the_restatement():
    fx = DH.small_fixture()
    for it, init in ((0, True), (1, False)):
        res = fx.run(None, DH.opts(2, it, 2, SEED), init=init)
        f = fx.filter(None, res)
        DH.check_filter(f, DH.filter_ref(fx.views(), res["depth"], res["cost"]))
        assert 0 < f["stats"]["n_kept"] < f["stats"]["n_candidates"] or init
    o = api.depthmap_filter_default_options()
    assert (round(o.max_cost, 6), round(o.rel_tol, 6), o.min_consistent) == (0.5, 0.01, 2)
    o.min_consistent, o.max_cost = 1, 0.3
    f = fx.filter(None, res, o)
    DH.check_filter(f, DH.filter_ref(fx.views(), res["depth"], res["cost"], 0.3, 0.01, 1))


def test_cost_never_rises_with_another_iteration():
    """acceptance is strict, so with one seed iterations = k + 1 is no worse than k anywhere"""
    fx = DH.small_fixture()
    costs = [fx.run(None, DH.opts(2, k, 2, SEED))["cost"] for k in range(4)]
    for k in range(3):
        assert (costs[k + 1] <= costs[k]).all(), k
    assert (costs[3] < costs[0]).any()


def _selection_scene():
    rng = np.random.default_rng(3)
    n_v = 40
    X = np.zeros((n_v, 3), np.float32)
    X[:, 1], X[:, 2] = rng.uniform(-1, 1, n_v), rng.uniform(3.5, 4.5, n_v)    # on the plane x = 0
    C = np.array([(0, 0, 0), (0.5, 0, 0), (-0.5, 0, 0), (0.05, 0, 0), (0, 0.8, -3.0)], np.float64)
    views = [[0, 1, 2, 3, 4] if v < 12 else [0, 1, 2, 3] for v in range(n_v)]
    return dict(K=np.array([[60.0, 0, 31.5, 0, 60.0, 23.5, 0, 0, 1]]).reshape(1, 3, 3),
                image_platform=np.zeros(5, np.int32), R=np.stack([np.eye(3)] * 5), C=C, vert_X=X,
                vert_off=np.concatenate([[0], np.cumsum([len(a) for a in views])]).astype(np.int64),
                vert_view=np.array([i for a in views for i in a], np.uint32))


def _lists(sel):
    return [sel["nb_view"][sel["nb_off"][i]:sel["nb_off"][i + 1]].tolist() for i in range(len(sel["nb_off"]) - 1)]


def test_view_selection_equals_the_restatement():
    scene = _selection_scene()
    sel = api.depth_views_select(scene)
    lists, scores, drange = DH.views_select_ref(scene)
    assert _lists(sel) == lists
    got = np.split(sel["nb_score"], sel["nb_off"][1:-1])
    for a, b in zip(got, scores):
        assert np.allclose(a, b, rtol=1e-12, atol=0)
    flat = np.sort(np.concatenate([np.unique(s) for s in scores if len(s)]))
    assert sel["drange"].tobytes() == drange.tobytes() and (drange[:, 0] > 0).all()
    # the tie rule: cameras 1 and 2 mirror each other in the plane of the points
    assert lists[0][:2] == [1, 2] and got[0][0] == got[0][1] and lists[4][:2] == [1, 2]
    # min_angle: cameras 0 and 3 are 0.05 apart at depth 4 (0.7 degrees)
    assert 3 not in lists[0] and 0 not in lists[3] and 3 in lists[1]
    # scores that differ at all differ by far more than the tolerance
    per_image = [np.diff(np.sort(np.unique(s))) for s in scores if len(s) > 1]
    assert min(d.min() for d in per_image if len(d)) > 1e-6 * flat.max()
    # min_shared: camera 4 shares 12 vertices with the others
    assert lists[4] and all(4 in a for a in lists[:3])
    o = api.depth_views_default_options()
    assert (o.opt_angle, o.min_angle, o.max_scale, o.range_margin, o.min_shared, o.max_neighbors) == (10, 3, 1.6, 0.25, 10, 4)
    o.min_shared = 13
    strict = api.depth_views_select(scene, o)
    assert _lists(strict) == DH.views_select_ref(scene, min_shared=13)[0]
    assert _lists(strict)[4] == [] and not any(4 in a for a in _lists(strict)) and (strict["drange"][4] == 0).all()
    o.min_shared, o.max_neighbors = 10, 2
    assert _lists(api.depth_views_select(scene, o)) == [a[:2] for a in lists]
    o.max_neighbors = 9
    with pytest.raises(api.SfmError) as ei:
        api.depth_views_select(scene, o)
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG and str(ei.value)


# Measured with the numpy restatement (whose bytes the library's equal), seed 3,
# the defaults: the plane fixture keeps 0.651 of its estimated pixels and all of
# them are correct; the step fixture outside the excluded band keeps 0.538,
# 0.996 of them correct.
@pytest.mark.parametrize("name", ["plane", "step"])
def test_accuracy_on_rendered_planes(name):
    """three views of 48 x 40, the defaults.  At least half of the estimated
    pixels survive the filter and at least 0.9 of the survivors are correct (the
    depth error moves the projection in the widest-baseline neighbour by less
    than half a pixel).  The step fixture leaves out the columns within r of the
    step's edge in each image (at most 2 r + 1): a patch there straddles two
    planes."""
    fx = DH.plane_fixture() if name == "plane" else DH.step_fixture()
    res = fx.run(None, DH.opts(seed=3))
    ref = DH.reference(name, 3, 3, 3, False)
    DH.check_against_ref(res, ref)                     # both could still be wrong together: hence the ground truth
    f = fx.filter(None, res)
    survive, correct = DH.shares(fx, f, 3, band=name == "step")
    print(f"{name}: {survive:.3f} of the estimated pixels survive, {correct:.3f} of those are correct")
    assert survive >= 0.5 and correct >= 0.9


def _raises(code, fn, *a, **k):
    with pytest.raises(api.SfmError) as ei:
        fn(*a, **k)
    assert ei.value.code == code and len(str(ei.value)) > 0, (ei.value.code, str(ei.value))


def _call(fx, ctx=None, o=None, **over):
    a = dict(wh=fx.wh, K=fx.K, R=fx.R, Cc=fx.C, nb_off=fx.nb_off, nb_view=fx.nb_view, drange=fx.drange, images=fx.images)
    a.update(over)
    return api.depthmap(ctx, a["wh"], a["K"], a["R"], a["Cc"], a["nb_off"], a["nb_view"], a["drange"], a["images"], o,
                        pool=a.get("pool"))


def depthmap_checks(ctx):
    """every refusal of sfm_depthmap(_host), then a valid call (shared with the GPU tests)"""
    fx = DH.small_fixture()
    bad = abi.SFM_ERR_INVALID_ARG
    wh = fx.wh.copy()
    wh[2] = 0
    _raises(bad, _call, fx, ctx, wh=wh)
    channels, img_off, pixels = api._pixel_pool(fx.images)
    ch2 = channels.copy()
    ch2[1] = 2
    _raises(bad, _call, fx, ctx, pool=(ch2, img_off, pixels))
    for j in (3, -1, 0):                               # out of range twice, then image 0 naming itself
        nb = fx.nb_view.copy()
        nb[0] = j
        _raises(bad, _call, fx, ctx, nb_view=nb)
    for lo, hi in ((0.0, 5.0), (5.0, 5.0), (-1.0, 2.0), (3.0, np.inf), (np.nan, 4.0)):
        dr = fx.drange.copy()
        dr[1] = lo, hi
        _raises(bad, _call, fx, ctx, drange=dr)
    for name in ("K", "R", "Cc"):
        for v in (np.nan, np.inf):
            arr = np.array(dict(K=fx.K, R=fx.R, Cc=fx.C)[name], np.float64)
            arr[2].flat[0] = v
            _raises(bad, _call, fx, ctx, **{name: arr})
    for r in (0, 6, -1):
        _raises(bad, _call, fx, ctx, DH.opts(r, 0))
    _raises(bad, _call, fx, ctx, DH.opts(2, -1))
    _raises(bad, _call, fx, ctx, DH.opts(2, 0, 0))
    nine = np.array([0, 9, 9, 9], np.int64)            # image 0 with nine neighbours
    _raises(bad, _call, fx, ctx, nb_off=nine, nb_view=np.array([1, 2] * 4 + [1], np.int32))
    _raises(abi.SFM_ERR_UNSUPPORTED, _call, fx, ctx, DH.opts(2, 0, device_bytes=1000))
    res = _call(fx, ctx, DH.opts(2, 0, 2, SEED))
    assert res["stats"]["n_images"] == 3 and res["stats"]["resident_bytes"] > 3 * 24 * 20 * 21
    return res


def filter_checks(ctx):
    fx = DH.small_fixture()
    res = fx.run(None, DH.opts(2, 0, 2, SEED), init=True)
    bad = abi.SFM_ERR_INVALID_ARG

    def call(**over):
        a = dict(wh=fx.wh, K=fx.K, R=fx.R, Cc=fx.C, nb_off=fx.nb_off, nb_view=fx.nb_view)
        a.update(over)
        return api.depthmap_filter(ctx, a["wh"], a["K"], a["R"], a["Cc"], a["nb_off"], a["nb_view"],
                                   res["depth"], res["cost"], a.get("o"))
    wh = fx.wh.copy()
    wh[5] = -3
    _raises(bad, call, wh=wh)
    for j in (3, 0):
        nb = fx.nb_view.copy()
        nb[0] = j
        _raises(bad, call, nb_view=nb)
    K = fx.K.copy()
    K[0, 0, 0] = np.nan
    _raises(bad, call, K=K)
    _raises(bad, call, nb_off=np.array([0, 9, 9, 9], np.int64), nb_view=np.array([1, 2] * 4 + [1], np.int32))
    o = api.depthmap_filter_default_options()
    o.rel_tol = -1.0
    _raises(bad, call, o=o)
    DH.check_filter(call(), DH.filter_ref(fx.views(), res["depth"], res["cost"]))


def test_depthmap_argument_checks():
    res = depthmap_checks(None)
    DH.same_maps(res, DH.small_fixture().run(None, DH.opts(2, 0, 2, SEED)))


def test_filter_argument_checks():
    filter_checks(None)


def test_images_without_maps_succeed():
    """an image with no neighbours and an unloaded one: all-zero maps; a call of nothing"""
    fx = DH.small_fixture()
    images = [fx.images[0], None, fx.images[2], fx.images[1]]
    wh = np.array([24, 20] * 4, np.int32)
    K, R = np.concatenate([fx.K, fx.K[:1]]), np.concatenate([fx.R, fx.R[:1]])
    C = np.array([fx.C[0], fx.C[1], fx.C[2], fx.C[1]])
    nb_off, nb_view = np.array([0, 2, 3, 3, 5], np.int64), np.array([3, 1, 0, 0, 2], np.int32)
    drange = np.array([[3.2, 5], [3.2, 5], [0, 0], [3.2, 5]], np.float32)
    res = api.depthmap(None, wh, K, R, C, nb_off, nb_view, drange, images, DH.opts(2, 1, 2, SEED))
    V = DH.Views(wh, K, R, C, nb_off, nb_view, drange, images)
    DH.check_against_ref(res, DH.depthmap_ref(V, 2, 1, 2, SEED))
    assert res["stats"]["n_images"] == 2
    for i in (1, 2):
        assert not res["depth_maps"][i].any() and not res["cost_maps"][i].any() and not res["normal_maps"][i].any()
    assert (res["depth_maps"][0] > 0).any() and (res["cost_maps"][3][2:-2, 2:-2] < 2).any()
    empty = api.depthmap(None, [], np.zeros((0, 9)), np.zeros((0, 9)), np.zeros((0, 3)), [0], [], [], [])
    assert empty["stats"]["n_images"] == 0 and len(empty["depth"]) == 0


def test_cpp_depthmap_program(tmp_path):
    """the stand-alone host program (host twins, view selection and façade compiled in): the one a sanitizer build runs"""
    exe = os.path.join(ROOT, "tests", "cpp", "depthmap_test")
    assert os.path.exists(exe), "run make (builds tests/cpp/depthmap_test)"
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and "depthmap ok" in r.stdout, r.stdout + r.stderr
