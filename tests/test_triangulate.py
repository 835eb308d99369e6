"""CPU: sfm_triangulate_host (the serial loop over csrc/tri_point.h, the code
the device kernels run) against the numpy fp64 reference of _tri_helpers, on
the generator's scenes at ground-truth cameras and on hand-built tracks.
Tolerances and the threshold placement: _tri_helpers."""
import ctypes as C

import numpy as np
import pytest

import _helpers as H
import _tri_helpers as T
import _wash_helpers as W

abi, api = H.abi, W.api
MODELS = {"pinhole": abi.SFM_CAM_PINHOLE, "snavely": abi.SFM_CAM_SNAVELY, "radial3": abi.SFM_CAM_RADIAL3}
METHODS = {"linear": abi.SFM_TRI_LINEAR, "robust": abi.SFM_TRI_ROBUST}
SHAPES = {"band": (12, 200, 4), "long": (40, 60, 16)}
_scenes = {}


def scene(shape, model, **kw):
    key = (shape, model, tuple(sorted(kw.items())))
    if key not in _scenes:
        n_cam, n_pt, k = SHAPES[shape]
        kw.setdefault("outliers", 0.05)
        sc = H.Scene(n_cam, n_pt, k, model=model, lib=abi.load(),
                     n_intr=n_cam if model == abi.SFM_CAM_RADIAL3 else 1, **kw)
        _scenes[key] = T.flip_z(sc) if model == abi.SFM_CAM_SNAVELY else sc
    return _scenes[key]


def test_defaults():
    o = api.tri_default_options()
    assert T.default_opts() == {f: getattr(o, f) for f, _ in abi.TriOpts._fields_}


@pytest.mark.parametrize("method", list(METHODS))
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_host_parity(shape, model, method):
    sc = scene(shape, MODELS[model])
    e, i = sc.gt_extr, sc.gt_intr
    probe = T.ref_triangulate(sc, e, i, dict(method=METHODS[method], min_angle_deg=0.0))
    target = float(np.nanpercentile(probe["angles"], 10))
    o, ref = T.placed_opts(sc, e, i, angle_target=target, method=METHODS[method])
    s = ref["stats"]
    assert s["n_pt_ok"] >= sc.n_pt // 2 and s["n_pt_angle"] >= 1 and s["n_obs_residual"] >= 1, s
    got = api.triangulate(None, sc.problem(), e, i, T.abi_opts(o))
    T.compare(got, ref, what=f"host {shape} {model} {method}")
    if method == "robust":   # the consensus leaves the gross outliers out: ground truth to the noise
        ok = ref["status"] == T.OK
        err = np.abs(got["X"][ok] - sc.gt_X.reshape(-1, 3)[ok]).max(1)
        print(f"  distance to ground truth: median {np.median(err):.3e}, max {err.max():.3e}")
        assert np.median(err) < 0.01


@pytest.mark.parametrize("model", list(MODELS))
def test_undistortion_round_trip(model):
    sc = scene("band", MODELS[model])
    iw = 6 if sc.model == abi.SFM_CAM_RADIAL3 else 4
    I = sc.gt_intr.reshape(-1, iw)[sc.img_intr[sc.obs_img]]
    uv = sc.obs_uv.reshape(-1, 2)
    b, bad = T.bearings(sc.model, uv, I)
    assert not bad.any()
    err = np.abs(T.redistort(sc.model, b, I) - uv).max()
    print(f"{model}: re-distorted bearings against the pixels, max {err:.3e} px")
    assert err <= 1e-9


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("method", list(METHODS))
def test_noise_free_scene_is_ground_truth(model, method):
    sc = scene("band", MODELS[model], noise=0.0, outliers=0.0)
    o = dict(T.default_opts(), method=METHODS[method], min_angle_deg=0.0)
    got = api.triangulate(None, sc.problem(), sc.gt_extr, sc.gt_intr, T.abi_opts(o))
    err = np.abs(got["X"] - sc.gt_X.reshape(-1, 3)).max()
    print(f"{model} {method}: max |X - ground truth| {err:.3e}, max residual {np.abs(got['residual']).max():.3e}")
    assert (got["status"] == T.OK).all() and got["keep_obs"].all()
    assert err <= 1e-9
    assert got["stats"]["n_pt_ok"] == sc.n_pt and got["stats"]["n_obs_kept"] == sc.n_obs


def _project_px(sc, e, i, img, X):
    R = W.rotations(e)[img]
    P = R @ X + e.reshape(-1, 6)[img, 3:]
    return W.project(sc.model, P[None], i.reshape(1, -1))[0], P


def _hand_built(method):
    """a 6-camera pinhole scene with one special track per point"""
    sc = H.Scene(6, 40, 4, outliers=0.0, lib=abi.load())
    e, i = sc.gt_extr, sc.gt_intr
    tr = T.tracks(sc)
    assert all(len(t) == 4 for t in tr[:12])
    tr[0] = []                                                   # no observation
    tr[1] = tr[1][:1]                                            # one
    tr[2] = tr[2][:2]                                            # two
    if method == "robust":
        # two of one image only: no hypothesis.  (LINEAR would solve for the camera
        # centre, where the projection is 0 / 0 and the verdict a matter of rounding;
        # its one-image case is point 8.)
        tr[3] = [tr[3][0], (tr[3][0][0], tr[3][0][1] + 0.3)]
    tr[4] = tr[4] + [tr[4][0]]                                   # a repeated view
    tr[5] = [(tr[5][0][0], np.array([np.nan, 1.0]))] + tr[5][1:]   # a NaN pixel
    tr[6] = [tr[6][0], (tr[6][1][0], np.array([np.inf, 3.0]))]   # one good observation left
    # parallel rays: two cameras see the same direction in world axes
    Rm = W.rotations(e)
    d = Rm[tr[7][0][0]].T @ np.array([0.01, 0.02, 1.0])
    pp = []
    for im in (tr[7][0][0], tr[7][1][0]):
        c = Rm[im] @ d
        pp.append((im, np.array([i[0] * c[0] / c[2] + i[2], i[1] * c[1] / c[2] + i[3]])))
    tr[7] = pp
    # point 8: two observations of one image, and one by an extra camera (image 6,
    # a half turn about y) that has the point behind it at P = (0.1, 0.2, -5)
    X8 = sc.gt_X.reshape(-1, 3)[8]
    im_a = tr[8][0][0]
    D = np.diag([-1.0, 1.0, -1.0])
    Pb = np.array([0.1, 0.2, -5.0])
    e = np.concatenate([e, [0.0, np.pi, 0.0], Pb - D @ X8])
    assert np.abs(W.rotations(e)[6] - D).max() < 1e-15
    ua, _ = _project_px(sc, e, i, im_a, X8)
    ub, P = _project_px(sc, e, i, 6, X8)
    assert P[2] < 0
    tr[8] = [(im_a, ua), (im_a, ua.copy()), (6, ub)]
    pr = T.Arrays(sc, tr)
    pr.n_cam, pr.img_intr = 7, np.append(sc.img_intr, 0).astype(np.int32)
    return sc, pr, e, i


@pytest.mark.parametrize("method", list(METHODS))
def test_hand_built_tracks(method):
    sc, pr, e, i = _hand_built(method)
    o, ref = T.placed_opts(pr, e, i, angle_target="keep", method=METHODS[method])
    got = api.triangulate(None, pr.problem(), e, i, T.abi_opts(o))
    T.compare(got, ref, what=f"hand-built {method}")
    st = got["status"]
    assert st[0] == st[1] == T.SHORT and st[2] == T.OK and st[6] == T.SHORT
    assert st[4] == T.OK and st[5] == T.OK
    assert got["stats"]["n_obs_bad"] == 2
    o5 = pr.pt_offsets[5]
    assert not got["keep_obs"][o5] and np.isnan(got["residual"][o5]).all() and got["keep_obs"][o5 + 1:o5 + 4].all()
    print(f"{method}: statuses {st[:9].tolist()}")
    if method == "linear":
        # the point behind camera b: the solve takes all three views, the depth rule
        # drops b's, and the two kept rays of one image span an angle of exactly 0
        assert st[8] == T.ANGLE and ref["angles"][8] == 0.0
        o8 = pr.pt_offsets[8]
        assert ref["codes"][o8 + 2] == T.DEPTH
        assert st[7] in (T.INFINITE, T.ANGLE) and st[7] == ref["status"][7]
        # without the cheirality rule nothing is rejected for depth
        o0 = dict(o, cheirality=0)
        ref0 = T.ref_triangulate(pr, e, i, o0)
        got0 = api.triangulate(None, pr.problem(), e, i, T.abi_opts(o0))
        T.compare(got0, ref0, what="hand-built linear, cheirality off")
        assert got0["stats"]["n_obs_depth"] == 0 and got0["status"][8] == T.OK
    else:
        assert st[3] == T.SHORT          # no pair of different images: no hypothesis


@pytest.mark.parametrize("max_hyp", [1, 5])
def test_hypothesis_spread_and_unranking(max_hyp):
    sc = scene("long", abi.SFM_CAM_PINHOLE)
    e, i = sc.gt_extr, sc.gt_intr
    pairs = T.pair_list(sc.obs_img[:16], np.ones(16, bool), max_hyp)
    assert len(pairs) == max_hyp and pairs[0] == (0, 1)
    if max_hyp == 5:
        assert pairs == [(0, 1), (1, 11), (3, 10), (5, 13), (8, 13)]     # 120 pairs: numbers 0, 24, 48, 72, 96
    # 16-tracks whose compared solve is well conditioned in the reference (one
    # hypothesis of two neighbouring cameras can leave a two-view refit)
    probe = T.ref_triangulate(sc, e, i, dict(max_hypotheses=max_hyp, min_angle_deg=0.0))
    tr = [t for t, ex in zip(T.tracks(sc), probe["exclude"]) if not ex][:12]
    assert len(tr) == 12 and all(len(t) == 16 for t in tr)
    pr = T.Arrays(sc, tr)
    o, ref = T.placed_opts(pr, e, i, max_hypotheses=max_hyp, min_angle_deg=0.0)
    got = api.triangulate(None, pr.problem(), e, i, T.abi_opts(o))
    T.compare(got, ref, what=f"max_hypotheses {max_hyp}")
    assert ref["stats"]["n_pt_ok"] >= 1


def test_argument_errors_and_null_outputs():
    lib = abi.load()
    sc = scene("band", abi.SFM_CAM_PINHOLE)
    pr = sc.problem()
    p = abi.ptr
    e, i = sc.gt_extr, sc.gt_intr
    for field, val, word in (("min_track_len", 1, b"min_track_len"), ("max_hypotheses", 0, b"max_hypotheses"),
                             ("method", 2, b"method"), ("max_residual_px", float("nan"), b"NaN")):
        o = api.tri_default_options()
        setattr(o, field, val)
        for rc in (lib.sfm_triangulate_host(None, None, None, C.byref(o), None, None, None, None, None),
                   lib.sfm_triangulate(None, None, None, None, C.byref(o), None, None, None, None, None)):
            assert rc == abi.SFM_ERR_INVALID_ARG and word in lib.sfm_last_error(), (field, lib.sfm_last_error())
    assert lib.sfm_triangulate_host(None, p(e, abi.f64p), p(i, abi.f64p), None, None, None, None, None, None) \
        == abi.SFM_ERR_INVALID_ARG and b"null" in lib.sfm_last_error()
    assert lib.sfm_triangulate(None, C.byref(pr), p(e, abi.f64p), p(i, abi.f64p), None, None, None, None, None,
                               None) == abi.SFM_ERR_INVALID_ARG
    full = api.triangulate(None, pr, e, i)
    st = abi.TriStats()
    assert lib.sfm_triangulate_host(C.byref(pr), p(e, abi.f64p), p(i, abi.f64p), None, None, None, None, None,
                                    C.byref(st)) == 0
    assert {f: getattr(st, f) for f, _ in abi.TriStats._fields_} == full["stats"]
    assert lib.sfm_triangulate_host(C.byref(pr), p(e, abi.f64p), p(i, abi.f64p), None, None, None, None, None,
                                    None) == 0
    ko = np.zeros(sc.n_obs, np.uint8)
    assert lib.sfm_triangulate_host(C.byref(pr), p(e, abi.f64p), p(i, abi.f64p), None, None, None, p(ko, abi.u8p),
                                    None, None) == 0
    np.testing.assert_array_equal(ko.astype(bool), full["keep_obs"])
    bad = sc.problem()
    bad.camera_model = 9
    with pytest.raises(api.SfmError) as ei:
        api.triangulate(None, bad, e, i)
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG
