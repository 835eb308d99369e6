"""CPU: the host side of the post-BA outlier rejection -- the defaults, the
argument checks that run before any device call, and sfm_ba_wash_apply (the
compaction of a problem by the masks a wash returned) against numpy."""
import ctypes as C

import numpy as np
import pytest

import _helpers as H
import _wash_helpers as W

abi, api = H.abi, W.api


@pytest.fixture(scope="module")
def washed():
    """a scene and the reference's masks for it (some of each rule)"""
    sc = H.Scene(12, 600, 4, outliers=0.05, lib=abi.load())
    e, i, x = W.blend(sc, 0.1)
    _, ref = W.placed_opts(sc, e, i, x)
    W.assert_not_vacuous(ref)
    return sc, x, ref


def _arrays(pr):
    off = np.ctypeslib.as_array(pr.pt_offsets, shape=(pr.n_pt + 1,)).copy()
    img = np.ctypeslib.as_array(pr.obs_img, shape=(max(pr.n_obs, 1),))[:pr.n_obs].copy()
    uv = np.ctypeslib.as_array(pr.obs_uv, shape=(max(2 * pr.n_obs, 1),))[:2 * pr.n_obs].copy()
    return off, img, uv


def test_defaults():
    o = api.ba_wash_default_options()
    assert (o.max_residual_px, o.min_angle_deg, o.min_track_len, o.cheirality) == (4.0, 2.0, 2, 1)
    assert W.default_opts() == {f: getattr(o, f) for f, _ in abi.BAWashOpts._fields_}


def test_apply_matches_numpy_compaction(washed):
    sc, x, ref = washed
    pr = sc.problem()
    new, X2, pt_map = api.ba_wash_apply(pr, x, ref["keep_obs"], ref["keep_pt"])
    kept_pts = np.flatnonzero(ref["keep_pt"])
    assert 0 < len(kept_pts) < sc.n_pt
    np.testing.assert_array_equal(pt_map, kept_pts)
    np.testing.assert_array_equal(X2, x.reshape(-1, 3)[kept_pts].reshape(-1))
    off, img, uv = _arrays(new)
    # kept observations of kept points, in their old order
    sel = np.concatenate([np.arange(sc.pt_offsets[p], sc.pt_offsets[p + 1])[ref["keep_obs"][sc.pt_offsets[p]:
                                                                                          sc.pt_offsets[p + 1]]]
                          for p in kept_pts])
    counts = [int(ref["keep_obs"][sc.pt_offsets[p]:sc.pt_offsets[p + 1]].sum()) for p in kept_pts]
    np.testing.assert_array_equal(off, np.concatenate([[0], np.cumsum(counts)]))
    np.testing.assert_array_equal(img, sc.obs_img[sel])
    np.testing.assert_array_equal(uv, sc.obs_uv.reshape(-1, 2)[sel].reshape(-1))
    assert (new.n_pt, new.n_obs) == (ref["stats"]["n_pt_kept"], ref["stats"]["n_obs_kept"])
    assert (new.n_img, new.n_intr, new.const_img, new.camera_model, new.huber_a) == \
        (pr.n_img, pr.n_intr, pr.const_img, pr.camera_model, pr.huber_a)
    # the washed problem is one the planner takes
    assert api.ba_describe(new).n_chunk_pts + api.ba_describe(new).n_general_pts == new.n_pt


def test_apply_all_kept_and_all_removed(washed):
    sc, x, _ = washed
    pr = sc.problem()
    new, X2, pt_map = api.ba_wash_apply(pr, x, np.ones(sc.n_obs, bool), np.ones(sc.n_pt, bool))
    off, img, uv = _arrays(new)
    np.testing.assert_array_equal(off, sc.pt_offsets)
    np.testing.assert_array_equal(img, sc.obs_img)
    np.testing.assert_array_equal(uv, sc.obs_uv)
    np.testing.assert_array_equal(X2, x)
    np.testing.assert_array_equal(pt_map, np.arange(sc.n_pt))
    new, X2, pt_map = api.ba_wash_apply(pr, x, np.zeros(sc.n_obs, bool), np.zeros(sc.n_pt, bool))
    assert (new.n_pt, new.n_obs, len(X2), len(pt_map)) == (0, 0, 0, 0)
    assert _arrays(new)[0].tolist() == [0]


def test_apply_rejects_kept_observation_of_removed_point(washed):
    sc, x, ref = washed
    ko, kp = ref["keep_obs"].copy(), ref["keep_pt"].copy()
    p = int(np.flatnonzero(~kp)[0])
    ko[sc.pt_offsets[p]] = True
    with pytest.raises(api.SfmError) as ei:
        api.ba_wash_apply(sc.problem(), x, ko, kp)
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG and "removed" in str(ei.value)
    with pytest.raises(ValueError):
        api.ba_wash_apply(sc.problem(), x, ko[:-1], kp)


def test_min_track_len_zero_is_invalid():
    """the option check runs before anything else, so it shows without a device"""
    lib = abi.load()
    o = api.ba_wash_default_options()
    o.min_track_len = 0
    rc = lib.sfm_ba_wash(None, None, None, None, None, C.byref(o), None, None, None, None, None)
    assert rc == abi.SFM_ERR_INVALID_ARG and b"min_track_len" in lib.sfm_last_error()
    rc = lib.sfm_ba_plan_wash(None, C.byref(o), None, None, None, None, None)
    assert rc == abi.SFM_ERR_INVALID_ARG and b"min_track_len" in lib.sfm_last_error()
    o.min_track_len = 1
    rc = lib.sfm_ba_wash(None, None, None, None, None, C.byref(o), None, None, None, None, None)
    assert rc == abi.SFM_ERR_INVALID_ARG and b"null" in lib.sfm_last_error()
