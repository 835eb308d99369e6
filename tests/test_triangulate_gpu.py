"""GPU: sfm_triangulate (kernels in csrc/tri.hip) against the numpy fp64
reference of _tri_helpers and against sfm_triangulate_host.  Tolerances and the
threshold placement: _tri_helpers (X 1e-9, residual 1e-9 px at kept
observations, status / keep_obs / stats exact; every threshold in a gap of
the reference's own values)."""
import numpy as np
import pytest

import _helpers as H
import _tri_helpers as T
import _wash_helpers as W

pytestmark = pytest.mark.gpu
abi, api = H.abi, W.api
LINEAR, ROBUST = abi.SFM_TRI_LINEAR, abi.SFM_TRI_ROBUST


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _shuffled(sc, seed=3):
    """every point's observations in a random order"""
    rng = np.random.default_rng(seed)
    perm = np.concatenate([sc.pt_offsets[p] + rng.permutation(sc.pt_offsets[p + 1] - sc.pt_offsets[p])
                           for p in range(sc.n_pt)])
    sc.obs_img = np.ascontiguousarray(sc.obs_img[perm])
    sc.obs_uv = np.ascontiguousarray(sc.obs_uv.reshape(-1, 2)[perm].reshape(-1))
    return sc


SCENES = {
    "band": lambda: H.Scene(12, 200, 4, outliers=0.05),
    "long": lambda: H.Scene(40, 60, 16, outliers=0.05),
    "band_radial3": lambda: H.Scene(12, 200, 4, n_intr=12, model=abi.SFM_CAM_RADIAL3, outliers=0.05),
    "long_radial3": lambda: H.Scene(40, 60, 16, n_intr=40, model=abi.SFM_CAM_RADIAL3, outliers=0.05),
    "band_snavely": lambda: T.flip_z(H.Scene(12, 200, 4, model=abi.SFM_CAM_SNAVELY, outliers=0.05)),
    "long_snavely": lambda: T.flip_z(H.Scene(40, 60, 16, model=abi.SFM_CAM_SNAVELY, outliers=0.05)),
    "random_shuffled": lambda: _shuffled(H.Scene(30, 200, 6, vis_mode=1, outliers=0.05, seed=11)),
}
_cache = {}


def _case(name, method):
    """(scene, placed options, reference) at ground-truth cameras, computed once"""
    if (name, method) not in _cache:
        sc = SCENES[name]()
        e, i = sc.gt_extr, sc.gt_intr
        probe = T.ref_triangulate(sc, e, i, dict(method=method, min_angle_deg=0.0))
        o, ref = T.placed_opts(sc, e, i, angle_target=float(np.nanpercentile(probe["angles"], 10)), method=method)
        _cache[(name, method)] = (sc, o, ref)
    return _cache[(name, method)]


@pytest.mark.parametrize("method", [LINEAR, ROBUST], ids=["linear", "robust"])
@pytest.mark.parametrize("name", list(SCENES))
def test_parity(ctx, name, method):
    sc, o, ref = _case(name, method)
    s = ref["stats"]
    assert s["n_pt_ok"] >= sc.n_pt // 2 and s["n_pt_angle"] >= 1 and s["n_obs_residual"] >= 1, s
    e, i = sc.gt_extr, sc.gt_intr
    got = api.triangulate(ctx, sc.problem(), e, i, T.abi_opts(o))
    T.compare(got, ref, what=f"gpu {name} {method}")
    host = api.triangulate(None, sc.problem(), e, i, T.abi_opts(o))
    np.testing.assert_array_equal(got["status"], host["status"])
    np.testing.assert_array_equal(got["keep_obs"], host["keep_obs"])
    assert got["stats"] == host["stats"]
    ok = host["status"] == T.OK
    assert np.abs(got["X"][ok] - host["X"][ok]).max() <= 1e-9
    again = api.triangulate(ctx, sc.problem(), e, i, T.abi_opts(o))
    for k in ("X", "status", "keep_obs", "residual"):
        np.testing.assert_array_equal(again[k], got[k], err_msg=k)          # bit for bit (NaN == NaN here)
    assert again["stats"] == got["stats"]


@pytest.mark.parametrize("method", [LINEAR, ROBUST], ids=["linear", "robust"])
def test_group_and_wave_boundaries(ctx, method):
    """tracks of 2, 16, 17, 63, 64, 65, 129 and 130 observations next to empty ones"""
    sc = H.Scene(130, 24, 130, outliers=0.05)
    assert (np.diff(sc.pt_offsets) == 130).all()
    e, i = sc.gt_extr, sc.gt_intr
    tr = T.tracks(sc)
    cut = {0: 2, 1: 0, 2: 16, 3: 17, 4: 0, 5: 63, 6: 64, 7: 65, 8: 0, 9: 129, 11: 1, 12: 3, 13: 0, 14: 128}
    for p, n in cut.items():        # n views spread over the orbit (two neighbouring cameras are ill conditioned)
        tr[p] = [tr[p][(j * 130) // (n + 1)] for j in range(n)]
    assert len(tr[10]) == 130
    pr = T.Arrays(sc, tr)
    o, ref = T.placed_opts(pr, e, i, angle_target="keep", method=method)
    assert ref["stats"]["n_pt_ok"] >= 12 and ref["stats"]["n_obs_residual"] >= 1 and ref["stats"]["n_pt_short"] >= 5
    got = api.triangulate(ctx, pr.problem(), e, i, T.abi_opts(o))
    T.compare(got, ref, what=f"boundaries {method}")
    host = api.triangulate(None, pr.problem(), e, i, T.abi_opts(o))
    np.testing.assert_array_equal(got["keep_obs"], host["keep_obs"])
    assert got["stats"] == host["stats"]


def test_long_run_of_points_without_observations(ctx):
    sc = H.Scene(6, 60, 3, outliers=0.05)
    e, i = sc.gt_extr, sc.gt_intr
    tr = T.tracks(sc)
    tr = tr[:20] + [[] for _ in range(300)] + tr[20:]
    pr = T.Arrays(sc, tr)
    o, ref = T.placed_opts(pr, e, i, angle_target="keep")
    assert ref["stats"]["n_pt_short"] >= 300 and ref["stats"]["n_pt_ok"] >= 30
    got = api.triangulate(ctx, pr.problem(), e, i, T.abi_opts(o))
    T.compare(got, ref, what="300 empty points")
    assert (got["status"][20:320] == T.SHORT).all() and np.isnan(got["X"][20:320]).all()


def test_hand_built_tracks(ctx):
    import test_triangulate as C
    for method in ("linear", "robust"):
        sc, pr, e, i = C._hand_built(method)
        o, ref = T.placed_opts(pr, e, i, angle_target="keep", method=C.METHODS[method])
        got = api.triangulate(ctx, pr.problem(), e, i, T.abi_opts(o))
        T.compare(got, ref, what=f"gpu hand-built {method}")


def test_seeds_a_solve(ctx):
    """points triangulated at the perturbed cameras start a solve lower than the
    generator's perturbed points do"""
    sc = H.Scene(12, 600, 4, outliers=0.05)
    pr = sc.problem()
    e, i, x = sc.params()
    tri = api.triangulate(ctx, pr, e, i)
    ok = tri["status"] == T.OK
    assert ok.sum() > sc.n_pt // 2
    Xt = np.where(ok[:, None], tri["X"], 0.0).reshape(-1)
    pr2, x_tri, pt_map = api.ba_wash_apply(pr, Xt, tri["keep_obs"], ok)
    _, x_gen, _ = api.ba_wash_apply(pr, x, tri["keep_obs"], ok)
    assert pr2.n_pt == tri["stats"]["n_pt_ok"] and pr2.n_obs == tri["stats"]["n_obs_kept"]
    rc_a, s_a = api.ba_solve(ctx, pr2, e.copy(), i.copy(), x_tri.copy())
    rc_b, s_b = api.ba_solve(ctx, pr2, e.copy(), i.copy(), x_gen.copy())
    print(f"rmse_initial {s_a.rmse_initial} (triangulated) vs {s_b.rmse_initial} (generator); "
          f"final {s_a.rmse_final} vs {s_b.rmse_final}")
    assert rc_a == 0 and s_a.usable
    assert s_a.rmse_initial < s_b.rmse_initial


def test_every_rank_triangulates_the_whole_problem():
    sc, o, ref = _case("band", ROBUST)
    c2 = api.Context(0, rank=1, world_size=2, flags=abi.SFM_CTX_DIAG_NO_EXCHANGE)
    try:
        T.compare(api.triangulate(c2, sc.problem(), sc.gt_extr, sc.gt_intr, T.abi_opts(o)), ref, what="world 2")
    finally:
        c2.close()


def test_kernel_time_is_reported():
    import ctypes as C
    sc, o, _ = _case("band", ROBUST)
    c = api.Context(0, flags=abi.SFM_CTX_TIME_KERNELS)
    try:
        api.triangulate(c, sc.problem(), sc.gt_extr, sc.gt_intr, T.abi_opts(o))
        ms = C.c_double(-1.0)
        assert c.lib.sfm_ctx_last_kernel_ms(c.h, C.byref(ms)) == 0
        assert 0.0 < ms.value < 1e3
    finally:
        c.close()
