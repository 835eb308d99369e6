"""CPU: the dense hand-off's scene (sfm_dense_scene_*) on a track set worked out
by hand, then on the output of the reconstruction's host twin."""
import numpy as np
import pytest

import _recon_helpers as RH
import _resect_helpers as R

abi, api = RH.abi, RH.api

# five images, three intrinsics blocks (block 2 is used by no image), image 2 not registered
IMG_INTR = [0, 1, 0, 1, 0]
REGISTERED = [1, 1, 0, 1, 1]
WH = [640, 480, 320, 240, 640, 480, 320, 240, 640, 480]
INTR = [500.0, 320.0, 240.0, 0.1, 0.01, 0.001, 250.0, 160.0, 120.0, 0.0, 0.0, 0.0, 100.0, 1.0, 2.0, 0.5, 0.0, 0.0]
#   point 0: images 0, 1, 3                  -> views 0, 1, 2
#   point 1: images 4, 0                     -> views 0, 3 (sorted)
#   point 2: image 1 twice, image 4          -> views 1, 3 (an image counts once)
#   point 3: images 0, 2 (2 not registered)  -> one view: short
#   point 4: image 3, image 4 (dead)         -> one view: short
#   point 5: images 0, 1, pt_ok off          -> not looked at
#   point 6: images 3, 1, 0                  -> views 0, 1, 2 (sorted)
OFF = [0, 3, 5, 8, 10, 12, 14, 17]
OBS_IMG = [0, 1, 3, 4, 0, 1, 1, 4, 0, 2, 3, 4, 0, 1, 3, 1, 0]
KEEP = [1] * 11 + [0] + [1] * 5
PT_OK = [1, 1, 1, 1, 1, 0, 1]


def _scene(model=abi.SFM_CAM_RADIAL3, intr=INTR, wh=WH, X=None, extr=None):
    rng = np.random.default_rng(0)
    t = RH.Tracks(5, OFF, OBS_IMG, rng.uniform(0, 300, (17, 2)), IMG_INTR, 3, model)
    if X is None:
        X = rng.uniform(-3, 3, (7, 3))
        X[3] = X[5] = np.nan                       # a short point and a masked one: not read
    if extr is None:
        extr = np.concatenate([rng.uniform(-1.2, 1.2, (5, 3)), rng.uniform(-4, 4, (5, 3))], axis=1)
        extr[0, :3] = 0.0                          # the identity
        extr[2] = np.nan                           # not registered: not read
    return t, X, extr, api.dense_scene(t.problem(), intr, extr, X, wh, REGISTERED, PT_OK, KEEP)


def test_hand_built_scene():
    t, X, extr, s = _scene()
    assert s["K"].tolist() == [[[500, 0, 320], [0, 500, 240], [0, 0, 1]], [[250, 0, 160], [0, 250, 120], [0, 0, 1]],
                               [[100, 0, 1], [0, 100, 2], [0, 0, 1]]]
    assert s["platform_wh"].tolist() == [[640, 480], [320, 240], [0, 0]]
    assert s["image_src"].tolist() == [0, 1, 3, 4]
    assert s["image_platform"].tolist() == [0, 1, 1, 0]
    assert s["image_pose"].tolist() == [0, 0, 1, 1]
    assert s["vert_pt"].tolist() == [0, 1, 2, 6]
    assert s["vert_off"].tolist() == [0, 3, 5, 7, 10]
    assert s["vert_view"].tolist() == [0, 1, 2, 0, 3, 1, 3, 0, 1, 2]
    assert s["n_short"] == 2
    assert s["vert_X"].dtype == np.float32 and s["vert_X"].tobytes() == X[[0, 1, 2, 6]].astype(np.float32).tobytes()
    # poses: a few dozen double roundings of 1.1e-16 each, with a hundredfold margin
    for q, i in enumerate(s["image_src"]):
        Rm = R.rodrigues(extr[i, :3])
        Cc = -Rm.T @ extr[i, 3:]
        assert np.abs(s["R"][q] - Rm).max() <= 1e-12
        assert np.abs(s["C"][q] - Cc).max() <= 1e-12 * max(1.0, np.linalg.norm(Cc))
    assert s["R"][0].tolist() == np.eye(3).tolist()


def test_null_masks_mean_all():
    rng = np.random.default_rng(1)
    t = RH.Tracks(5, OFF, OBS_IMG, rng.uniform(0, 300, (17, 2)), IMG_INTR, 3, abi.SFM_CAM_RADIAL3)
    X, extr = rng.uniform(-3, 3, (7, 3)), rng.uniform(-1, 1, (5, 6))
    s = api.dense_scene(t.problem(), INTR, extr, X, WH)
    assert s["image_src"].tolist() == [0, 1, 2, 3, 4] and s["image_pose"].tolist() == [0, 0, 1, 1, 2]
    assert s["vert_pt"].tolist() == list(range(7)) and s["n_short"] == 0
    assert s["vert_view"].tolist() == [0, 1, 3, 0, 4, 1, 4, 0, 2, 3, 4, 0, 1, 0, 1, 3]


def test_pinhole_k_and_the_checks():
    pin = [500.0, 510.0, 320.0, 240.0, 250.0, 255.0, 160.0, 120.0, 1.0, 2.0, 3.0, 4.0]
    s = _scene(abi.SFM_CAM_PINHOLE, pin)[3]
    assert s["K"][0].tolist() == [[500, 0, 320], [0, 510, 240], [0, 0, 1]] and s["K"][2].tolist() == [[1, 0, 3], [0, 2, 4], [0, 0, 1]]
    with pytest.raises(api.SfmError) as ei:
        _scene(abi.SFM_CAM_SNAVELY, pin)
    assert ei.value.code == abi.SFM_ERR_UNSUPPORTED

    def bad(**kw):
        with pytest.raises(api.SfmError) as ei:
            _scene(**kw)
        assert ei.value.code == abi.SFM_ERR_INVALID_ARG and str(ei.value)

    bad(model=9)
    bad(wh=WH[:8] + [640, 481])                    # images of one block with different sizes
    bad(wh=[0, 480] + WH[2:])
    bad(intr=INTR[:17] + [np.nan])                 # (an unused block is a platform too)
    rng = np.random.default_rng(2)
    X = rng.uniform(-3, 3, (7, 3))
    X[6, 1] = np.inf                               # a kept vertex
    bad(X=X)
    extr = rng.uniform(-1, 1, (5, 6))
    extr[3, 4] = np.nan                            # a registered image
    bad(extr=extr)


@pytest.fixture(scope="module")
def arc():
    sc = RH.ArcScene(abi.SFM_CAM_RADIAL3, lonely=True)
    return sc, sc.run(None, RH.recon_opts(0))


def test_on_a_reconstruction(arc):
    sc, res = arc
    assert res["stats"]["status"] == abi.SFM_RECON_OK and not res["registered"].all()
    s = api.dense_scene(sc.tracks.problem(), res["intr"], res["extr"], res["X"], sc.wh, res["registered"],
                        res["pt_ok"], res["keep_obs"])
    assert res["registered"][s["image_src"]].all() and len(s["image_src"]) == res["registered"].sum()
    assert (np.diff(s["image_src"]) > 0).all()
    lens = np.diff(s["vert_off"])
    assert len(lens) > 100 and (lens >= 2).all() and s["vert_off"][-1] == len(s["vert_view"])
    for a, b in zip(s["vert_off"][:-1], s["vert_off"][1:]):
        assert (np.diff(s["vert_view"][a:b].astype(np.int64)) > 0).all()      # sorted and unique
    assert s["vert_view"].max() < len(s["image_src"])
    assert s["n_short"] + len(s["vert_pt"]) == res["pt_ok"].sum()
    assert res["pt_ok"][s["vert_pt"]].all()
    assert s["vert_X"].tobytes() == res["X"][s["vert_pt"]].astype(np.float32).tobytes()
    # every view of a vertex is a live observation of its point
    t = sc.tracks
    for v in (0, len(lens) // 2, len(lens) - 1):
        p = s["vert_pt"][v]
        o = np.arange(t.pt_offsets[p], t.pt_offsets[p + 1])
        live = set(t.obs_img[o][res["keep_obs"][o] & res["registered"][t.obs_img[o]]].tolist())
        assert set(s["image_src"][s["vert_view"][s["vert_off"][v]:s["vert_off"][v + 1]]].tolist()) == live
    assert s["K"].shape == (1, 3, 3) and s["K"][0, 0, 0] == res["intr"][0] and s["platform_wh"].tolist() == [list(RH.WH)]
