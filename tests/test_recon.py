"""CPU: the incremental reconstruction on the host twins -- the three round
queries against a numpy restatement, sfm_reconstruct_host on a noise-free
scene, the degenerate inputs and the argument checks."""
import numpy as np
import pytest

import _recon_helpers as RH

abi, api = RH.abi, RH.api


# ---- round queries ------------------------------------------------------------------
QUERY_SETS = [
    dict(seed=1, n_img=6, n_pt=40, max_len=5),
    dict(seed=2, n_img=9, n_pt=120, max_len=7, empty_images=(0, 4, 8)),     # images with no observations
    dict(seed=3, n_img=3, n_pt=30, max_len=6, dup=0.6),                     # many points twice in one image
    dict(seed=4, n_img=5, n_pt=0, max_len=3),
    dict(seed=5, n_img=4, n_pt=25, max_len=0),                              # points without observations
    dict(seed=6, n_img=12, n_pt=60, max_len=4, long_track=90),
]


@pytest.mark.parametrize("cfg", QUERY_SETS, ids=lambda c: f"seed{c['seed']}")
def test_host_queries_match_numpy(cfg):
    t = RH.random_tracks(**cfg)
    h = api.ReconTracks(None, t.problem())
    RH.check_queries(h, t, seed=cfg["seed"])
    # dropped observations are gone from every query, for good
    if t.n_obs:
        rng = np.random.default_rng(cfg["seed"])
        dead = rng.random(t.n_obs) < 0.3
        h.drop_obs(np.flatnonzero(dead))
        RH.check_queries(h, t, seed=cfg["seed"] + 50, dead=dead)
    h.close()


def test_host_gather_matches_resect_gather():
    """the device twin's contract: sfm_resect_gather's rows in its order"""
    t = RH.random_tracks(7, 7, 80, 6)
    rng = np.random.default_rng(7)
    X, ok = rng.normal(size=(t.n_pt, 3)), rng.random(t.n_pt) < 0.6
    h = api.ReconTracks(None, t.problem())
    images = [5, 0, 3]
    off, X3, uv, _ = h.gather(X, ok, images)
    off0, X30, uv0 = api.resect_gather(t.problem(), X, ok, images)
    assert off.tobytes() == off0.tobytes() and X3.tobytes() == X30.tobytes() and uv.tobytes() == uv0.tobytes()


def test_query_argument_errors():
    t = RH.random_tracks(8, 4, 10, 3)
    h = api.ReconTracks(None, t.problem())
    ok, reg, X = np.ones(t.n_pt, bool), np.ones(t.n_img, bool), np.zeros((t.n_pt, 3))
    for images in ([4], [-1], [1, 1]):
        with pytest.raises(api.SfmError) as ei:
            h.gather(X, ok, images)
        assert ei.value.code == abi.SFM_ERR_INVALID_ARG
    for mode, ml in ((2, 2), (RH.SOLVED, 0)):
        with pytest.raises(api.SfmError) as ei:
            h.select(reg, ok, mode, ml)
        assert ei.value.code == abi.SFM_ERR_INVALID_ARG
    with pytest.raises(api.SfmError) as ei:
        h.drop_obs([t.n_obs])
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG
    bad = RH.random_tracks(8, 4, 10, 3)
    bad.obs_img[0] = 4
    with pytest.raises(api.SfmError) as ei:
        api.ReconTracks(None, bad.problem())
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG
    bad = RH.random_tracks(8, 4, 10, 3)
    bad.pt_offsets[-1] += 1
    with pytest.raises(api.SfmError) as ei:
        api.ReconTracks(None, bad.problem())
    assert ei.value.code == abi.SFM_ERR_INVALID_ARG


# ---- the driver -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_runs():
    out = {}
    for model in RH.MODELS:
        sc = RH.ArcScene(model)
        out[model] = (sc, sc.run(None, RH.recon_opts(0)))
    return out


@pytest.mark.parametrize("model", RH.MODELS)
def test_host_driver_reconstructs_the_scene(host_runs, model):
    sc, res = host_runs[model]
    sc.check_conditions(res)
    dev = sc.deviation(res)
    st = res["stats"]
    print(f"model {model}: pair {st['initial_pair']}, {st['n_rounds']} rounds, {st['n_points']} points, "
          f"{st['n_obs_kept']} observations kept, deviation {dev:.3e} baselines")
    assert dev <= RH.MARGIN * RH.HOST_DEVIATION
    # the log: round 0 is the pair, every later round lists its candidates in ascending order
    rounds, cands = res["rounds"], res["cands"]
    assert len(rounds) == st["n_rounds"] and len(cands) == st["n_cands"]
    assert rounds[0]["n_cand"] == 2 and [c["image"] for c in cands[:2]] == st["initial_pair"]
    assert sum(r["n_registered"] for r in rounds) == sc.n_cam
    assert sum(r["points_added"] for r in rounds) == st["n_points"]     # (adjust = 0: nothing is removed)
    for k, r in enumerate(rounds[1:], 1):
        cs = cands[r["first_cand"]:r["first_cand"] + r["n_cand"]]
        assert [c["round"] for c in cs] == [k] * len(cs) and sorted(c["image"] for c in cs) == [c["image"] for c in cs]
        best = max(c["count"] for c in cs)
        assert all(c["count"] >= 0.75 * best for c in cs)
        assert r["adjust_repeats"] == 0
    # a second run takes the same decisions and gives the same bytes
    again = sc.run(None, RH.recon_opts(0))
    assert RH.log_integers(again) == RH.log_integers(res)
    assert again["extr"].tobytes() == res["extr"].tobytes() and again["X"].tobytes() == res["X"].tobytes()


def test_no_initial_pair():
    sc = RH.ArcScene(abi.SFM_CAM_PINHOLE)
    # nothing passes: no pairs at all, and a rule no pair can meet
    for res in (sc.run(None, RH.recon_opts(0), pairs=np.zeros((0, 2), np.int32)),
                sc.run(None, RH.recon_opts(0, pair_min_inliers=10 ** 6))):
        st = res["stats"]
        assert res["rc"] == abi.SFM_OK and st["status"] == abi.SFM_RECON_NO_INITIAL_PAIR
        assert not res["registered"].any() and not res["pt_ok"].any() and not res["keep_obs"].any()
        assert st["n_rounds"] == 0 and st["initial_pair"] == [-1, -1] and np.isnan(res["X"]).all()


def test_image_without_tracks_stays_unregistered():
    sc = RH.ArcScene(abi.SFM_CAM_PINHOLE, lonely=True)
    res = sc.run(None, RH.recon_opts(0))
    assert res["rc"] == abi.SFM_OK
    sc.check_conditions(res)
    assert not res["registered"][sc.n_cam] and not res["extr"][sc.n_cam].any()
    assert sc.n_cam not in [c["image"] for c in res["cands"]]


def test_forced_initial_pair(host_runs):
    sc, auto = host_runs[abi.SFM_CAM_PINHOLE]
    pair = (2, 3)
    assert list(pair) != auto["stats"]["initial_pair"]
    res = sc.run(None, RH.recon_opts(0, initial_pair=pair))
    assert res["stats"]["initial_pair"] == list(pair) and not res["extr"][2].any()
    sc.check_conditions(res)
    assert sc.deviation(res) <= RH.MARGIN * RH.HOST_DEVIATION
    # a forced pair that shares no track: no initial pair
    lone = RH.ArcScene(abi.SFM_CAM_PINHOLE, lonely=True)
    res = lone.run(None, RH.recon_opts(0, initial_pair=(0, lone.n_cam)))
    assert res["stats"]["status"] == abi.SFM_RECON_NO_INITIAL_PAIR and not res["registered"].any()


def test_log_capacity_overflow(host_runs):
    sc, full = host_runs[abi.SFM_CAM_PINHOLE]
    res = sc.run(None, RH.recon_opts(0), cap_rounds=1, cap_cands=3)
    assert RH.log_integers(res)[2] == RH.log_integers(full)[2]          # the true counts
    assert res["stats"]["n_rounds"] > 1 and res["stats"]["n_cands"] > 3
    assert len(res["rounds"]) == 1 and len(res["cands"]) == 3
    assert RH.log_integers(res)[0] == RH.log_integers(full)[0][:1] and RH.log_integers(res)[1] == RH.log_integers(full)[1][:3]
    none = sc.run(None, RH.recon_opts(0), cap_rounds=0, cap_cands=0)
    assert none["stats"]["n_rounds"] == full["stats"]["n_rounds"] and none["X"].tobytes() == full["X"].tobytes()


def test_host_twin_has_no_adjustment():
    sc = RH.ArcScene(abi.SFM_CAM_PINHOLE)
    with pytest.raises(api.SfmError) as ei:
        sc.run(None, RH.recon_opts(1))
    assert ei.value.code == abi.SFM_ERR_UNSUPPORTED


def test_driver_argument_errors():
    sc = RH.ArcScene(abi.SFM_CAM_PINHOLE, n_pt=40)

    def fails(code=abi.SFM_ERR_INVALID_ARG, opts=None, **kw):
        with pytest.raises(api.SfmError) as ei:
            sc.run(None, opts or RH.recon_opts(0), **kw)
        assert ei.value.code == code

    fails(pairs=[[0, 8]])
    fails(pairs=[[3, 3]])
    fails(opts=RH.recon_opts(0, initial_pair=(0, 0)))
    fails(opts=RH.recon_opts(0, initial_pair=(0, -1)))
    fails(opts=RH.recon_opts(0, group_ratio=0.0))
    fails(opts=RH.recon_opts(0, max_adjust_repeats=0))
    fails(opts=RH.recon_opts(0, min_track_len=0))
    o = RH.recon_opts(0)
    o.tri.min_track_len = 1
    fails(opts=o)
    o = RH.recon_opts(0)
    o.resect.max_iterations = 0
    fails(opts=o)
    fails(cap_rounds=-1)
    wh = sc.wh.copy()
    sc.wh = wh.copy()
    sc.wh[3] = 0
    fails()
    sc.wh = wh
    sc.tracks.img_intr[2] = 1
    fails()
    sc.tracks.img_intr[2] = 0
    sc.tracks.model = 7
    fails()


def test_cpp_reconstruction_facade():
    import os
    import subprocess
    exe = os.path.join(RH.H.ROOT, "tests", "cpp", "recon_test")
    assert os.path.exists(exe), "run make (builds tests/cpp/recon_test)"
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
