"""GPU: the round queries on the device against the host twin byte for byte, the
driver against its host twin (adjust = 0), the adjusted reconstruction of a
noisy scene against sfm_ba_solve from the truth, and the file-staged run."""
import numpy as np
import pytest

import _recon_helpers as RH

abi, api = RH.abi, RH.api
pytestmark = pytest.mark.gpu

THREADS = 256       # csrc/recon.hip kThreads: lanes per workgroup of the per-point and per-observation kernels
SCAN_TILE = 1024    # csrc/recon.hip kScanTile: 256 threads x 4 elements
TILES_PASS = 256    # tile sums one pass of recon_scan_tiles_kernel takes (kThreads)
VIS_LDS = 4096      # csrc/recon.hip kVisLdsImages: above it the visibility adds straight into global memory


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def sized_tracks(seed, n_img, n_pt, n_obs):
    """exactly n_pt points and n_obs observations"""
    rng = np.random.default_rng(seed)
    lens = rng.multinomial(n_obs, np.full(n_pt, 1.0 / n_pt)) if n_pt else np.zeros(0, int)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    img = rng.integers(0, n_img, n_obs).astype(np.int32)
    rep = rng.random(n_obs) < 0.1
    rep[off[:-1][lens > 0]] = False
    for o in np.flatnonzero(rep):
        img[o] = img[o - 1]
    return RH.Tracks(n_img, off, img, rng.uniform(0, 1000, (n_obs, 2)))


def device_equals_host(ctx, t, seed=0, drop=True):
    prob = t.problem()
    host, dev = api.ReconTracks(None, prob), api.ReconTracks(ctx, prob)
    want = RH.all_queries(host, t, seed)
    got = RH.all_queries(dev, t, seed)
    assert len(got) == len(want) and all(a == b for a, b in zip(got, want))
    assert RH.all_queries(dev, t, seed) == got          # a second device run is identical
    if drop and t.n_obs:
        dead = np.flatnonzero(np.random.default_rng(seed).random(t.n_obs) < 0.25)
        host.drop_obs(dead)
        dev.drop_obs(dead)
        assert RH.all_queries(dev, t, seed + 1) == RH.all_queries(host, t, seed + 1)
    host.close()
    dev.close()


@pytest.mark.parametrize("n", [THREADS - 1, THREADS, THREADS + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_queries_at_tile_edges(ctx, n):
    device_equals_host(ctx, sized_tracks(n, 7, n, 3 * n + 5), seed=n)        # n points
    device_equals_host(ctx, sized_tracks(n + 1, 5, n // 3 + 1, n), seed=n)   # n observations (and gather items)


def test_queries_small_against_numpy(ctx):
    for cfg in (dict(seed=1, n_img=6, n_pt=40, max_len=5), dict(seed=2, n_img=9, n_pt=120, max_len=7, empty_images=(0, 4, 8)),
                dict(seed=3, n_img=3, n_pt=30, max_len=6, dup=0.6)):
        t = RH.random_tracks(**cfg)
        h = api.ReconTracks(ctx, t.problem())
        RH.check_queries(h, t, seed=cfg["seed"])
        h.close()


def test_queries_degenerate(ctx):
    device_equals_host(ctx, RH.random_tracks(4, 5, 0, 3))                       # n_pt = 0
    device_equals_host(ctx, RH.random_tracks(5, 4, 25, 0))                      # points without observations
    device_equals_host(ctx, RH.random_tracks(6, 12, 60, 4, long_track=200))     # a track longer than a wavefront
    device_equals_host(ctx, RH.random_tracks(7, 9, 300, 5, empty_images=(0, 8)))


def test_queries_many_images(ctx):
    """more images than the LDS histogram holds: the visibility's global path"""
    device_equals_host(ctx, sized_tracks(8, VIS_LDS + 3, 600, 3000), drop=False)


def test_queries_multi_pass_scan(ctx):
    """more tiles than one pass of the tile-sum scan takes: observations above 256 x 1024"""
    n_obs = TILES_PASS * SCAN_TILE + 3 * SCAN_TILE + 17
    device_equals_host(ctx, sized_tracks(9, 40, 70001, n_obs), drop=False)


# ---- the driver -------------------------------------------------------------------------
@pytest.mark.parametrize("model", RH.MODELS)
def test_driver_matches_host_twin(ctx, model):
    sc = RH.ArcScene(model)
    host, dev = sc.run(None, RH.recon_opts(0)), sc.run(ctx, RH.recon_opts(0))
    sc.check_conditions(dev)
    assert RH.log_integers(dev) == RH.log_integers(host)
    for f in ("registered", "pt_ok", "keep_obs"):
        np.testing.assert_array_equal(dev[f], host[f])
    ok = host["pt_ok"]
    worst = max(np.abs(dev["extr"] - host["extr"]).max(), np.abs(dev["X"][ok] - host["X"][ok]).max())
    print(f"model {model}: device against host twin {worst:.3e}, against truth {sc.deviation(dev):.3e} baselines")
    assert worst <= RH.HOST_DEVICE_TOL
    assert sc.deviation(dev) <= RH.MARGIN * RH.HOST_DEVIATION
    again = sc.run(ctx, RH.recon_opts(0))
    assert again["extr"].tobytes() == dev["extr"].tobytes() and again["X"].tobytes() == dev["X"].tobytes()


ADJUST_CASES = [(abi.SFM_CAM_PINHOLE, False), (abi.SFM_CAM_SNAVELY, False), (abi.SFM_CAM_RADIAL3, False),
                (abi.SFM_CAM_RADIAL3, True)]


@pytest.mark.parametrize("model,per_image", ADJUST_CASES)
def test_driver_adjusted(ctx, model, per_image):
    sc = RH.ArcScene(model, noise=0.5, per_image_intr=per_image)
    res = sc.run(ctx, RH.recon_opts(1))
    st = res["stats"]
    fin = st["final_adjust"]
    ref = RH.yardstick_rmse(ctx, sc, res)
    print(f"model {model} per-image {per_image}: pair {st['initial_pair']}, {st['n_rounds']} rounds, {st['n_points']} points, "
          f"{st['n_obs_kept']} observations, final rmse {fin['ba']['rmse_final']:.6f}, yardstick {ref:.6f}, "
          f"final wash removed {st['final_removed']}")
    assert st["status"] == abi.SFM_RECON_OK and res["registered"].all()
    assert not res["keep_obs"][sc.bad_obs].any()
    assert st["final_removed"] == 0 and fin["ba_rc"] == 0 and fin["ba"]["usable"]
    assert fin["ba"]["rmse_final"] <= ref * (1.0 + RH.ADJUST_MARGIN)
    if per_image:   # the shape reconstruction() produces takes the dense solve
        assert api.ba_describe(_kept_problem(sc, res)).dense == 1


def _kept_problem(sc, res):
    t, keep = sc.tracks, res["keep_obs"]
    pts = np.flatnonzero(np.bincount(t.obs_pt[keep], minlength=t.n_pt) > 0)
    cnt = np.bincount(t.obs_pt[keep], minlength=t.n_pt)[pts]
    sub = RH.Tracks(t.n_img, np.concatenate([[0], np.cumsum(cnt)]), t.obs_img[keep], t.obs_uv[keep], t.img_intr, t.n_intr,
                    t.model)
    pr = sub.problem()
    pr.const_img = res["stats"]["initial_pair"][0]
    return pr


# ---- file-staged ----------------------------------------------------------------------
def test_sparse_reconstruct_writes_the_ply(ctx, tmp_path):
    from test_mvg_io import write_feat, write_sfm_data
    rng = np.random.default_rng(5)
    n_img, n_pt, f = 6, 300, 700.0
    write_sfm_data(tmp_path / "sfm_data.json", [f"im{k}.jpg" for k in range(n_img)])    # 640 x 480 views
    ang = 0.12 * (np.arange(n_img) - 2.5)
    X = rng.uniform(-1.5, 1.5, (n_pt, 3))
    feats, seen = [], np.full((n_img, n_pt), -1)
    for k, a in enumerate(ang):
        Rm = RH.R.rodrigues([0.0, a, 0.0])
        P = (X - np.array([10 * np.sin(a), 0.0, -10 * np.cos(a)])) @ Rm.T
        uv = f * P[:, :2] / P[:, 2:] + np.array([320.0, 240.0])
        vis = np.flatnonzero((rng.random(n_pt) < 0.8) & (uv[:, 0] > 0) & (uv[:, 0] < 640) & (uv[:, 1] > 0) & (uv[:, 1] < 480))
        vis = rng.permutation(vis)
        seen[k, vis] = np.arange(len(vis))
        kp = np.zeros((len(vis), 4), np.float32)
        kp[:, :2], kp[:, 2] = uv[vis], 2.0
        write_feat(tmp_path / f"im{k}.feat", kp)
        feats.append(kp)
    matches = {}
    for i in range(n_img):
        for j in range(i + 1, n_img):
            both = np.flatnonzero((seen[i] >= 0) & (seen[j] >= 0))
            matches[(i, j)] = np.stack([seen[i, both], seen[j, both]], 1).astype(np.uint32)
    api.mvg_save_matches(str(tmp_path / "matches.f.bin"), matches)
    out = tmp_path / "recon"
    out.mkdir()
    st = api.sparse_reconstruct(ctx, tmp_path, out, focal=f, opts=RH.recon_opts(1))
    assert st["status"] == abi.SFM_RECON_OK and st["n_registered"] == n_img and st["n_points"] > 0.9 * n_pt
    lines = (out / "cloud_and_poses.ply").read_text().splitlines()
    head = lines[:lines.index("end_header") + 1]
    assert head[:3] == ["ply", "format ascii 1.0", f"element vertex {st['n_points'] + st['n_registered']}"]
    assert head[3:] == ["property double x", "property double y", "property double z", "property uchar red",
                        "property uchar green", "property uchar blue", "end_header"]
    body = [ln.split() for ln in lines[len(head):]]
    assert len(body) == st["n_points"] + st["n_registered"] and all(len(b) == 6 for b in body)
    assert all(b[3:] == ["255", "255", "255"] for b in body[:st["n_points"]])
    assert all(b[3:] == ["0", "255", "0"] for b in body[st["n_points"]:])
    # the camera centres lie on the arc: equidistant from the cloud's centre, up to the reconstruction's scale
    C = np.array([[float(v) for v in b[:3]] for b in body[st["n_points"]:]])
    Xr = np.array([[float(v) for v in b[:3]] for b in body[:st["n_points"]]])
    d = np.linalg.norm(C - Xr.mean(0), axis=1)
    assert d.max() / d.min() < 1.05
