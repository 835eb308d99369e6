"""Depth-map fusion on the CPU: the host twin (sfm_depthmap_fuse_host) against
the numpy restatement of the header's contract (_fuse_helpers.py), byte for
byte; the invariants of the fate rule; accuracy on rendered planes; the pair
lists, the colour pool, capacities, argument checks, the CSR expansion, the PLY
and sfm_densify_host against the three twins chained."""
import numpy as np
import pytest

import _depthmap_helpers as DH
import _fuse_helpers as FH

abi, api = DH.abi, DH.api
F = np.float32
SEED = 3


def fuse_of(fx, flt, est, ctx=None, opts=None, images="fx"):
    return api.depthmap_fuse(ctx, fx.wh, fx.K, fx.R, fx.C, fx.nb_off, fx.nb_view, flt["depth"], est["normal"],
                             images=fx.images if images == "fx" else images, opts=opts)


@pytest.fixture(scope="module")
def case_a():
    fx, est, flt = FH.estimated("plane", 3, 3, SEED)
    ref = FH.fuse_ref(fx.wh, fx.K, fx.R, fx.C, fx.nb_off, fx.nb_view, flt["depth"], est["normal"], fx.images)
    return fx, est, flt, ref


def plane_distance(fx, X):
    return np.abs(np.asarray(X, np.float64)[:, 2] - fx.far)


def test_estimated_fixture_matches_the_restatement(case_a):
    fx, est, flt, ref = case_a
    res = fuse_of(fx, flt, est)
    FH.check_against_ref(res, ref)
    assert res["stats"]["resident_bytes"] > 0 and res["stats"]["seconds"][1] > 0


def test_invariants(case_a):
    fx, est, flt, ref = case_a
    kept = int((flt["depth"] > 0).sum())
    assert ref["n_points"] + ref["n_suppressed"] == kept
    assert 0 < ref["n_suppressed"] and 0 < ref["n_points"]
    # every suppressed pixel's chain of lowest agreeing images ends at an emitted pixel
    for i in range(fx.n):
        for p in np.nonzero(ref["fates"][i] == FH.SUPPRESSED)[0]:
            at, q = i, int(p)
            while ref["fates"][at][q] == FH.SUPPRESSED:
                nxt = int(ref["low_j"][at][q])
                assert nxt < at
                at, q = nxt, int(ref["low_q"][at][q])
            assert ref["fates"][at][q] == FH.EMITTED
    key = ref["src_image"].astype(np.int64) * (1 << 32) + ref["src_pixel"]
    assert (np.diff(key) > 0).all()
    pop = np.array([bin(int(m)).count("1") for m in ref["view_mask"]])
    assert np.array_equal(ref["n_views"], 1 + pop)
    # what DESIGN.md 5l records
    own = np.concatenate([FH.Problem(fx.wh, fx.K, fx.R, fx.C, fx.nb_off, fx.nb_view, flt["depth"], est["normal"])
                          .world_point(i, np.nonzero(flt["depth_maps"][i].reshape(-1) > 0)[0],
                                       flt["depth_maps"][i].reshape(-1)[flt["depth_maps"][i].reshape(-1) > 0])[2]
                          for i in range(fx.n)])
    print("points : kept pixels = %d : %d = %.3f; mean plane distance before %.5f, after %.5f" % (
        ref["n_points"], kept, ref["n_points"] / kept, np.abs(own.astype(np.float64) - fx.far).mean(),
        plane_distance(fx, ref["X"]).mean()))


def rel_tol_scene():
    """(b): exact plane depths; view 1's depths scaled by 1.009 in its left half
    (inside rel_tol 0.01 of its partners) and by 1.011 in its right half (outside)"""
    fx = DH.plane_fixture()
    sc = FH.Scene([fx])
    w = fx.w
    scale = np.where(np.arange(w) < w // 2, F(1.009), F(1.011)).astype(F)
    sc.depth_maps[1] = (sc.depth_maps[1] * scale[None, :]).astype(F)
    return fx, sc


def test_hand_built_plane_tolerance_and_accuracy():
    fx, sc = rel_tol_scene()
    ref = sc.ref()
    res = sc.run(None)
    FH.check_against_ref(res, ref)
    # the offset decides agreement: view 1's right half agrees with nobody, its left half with view 0
    w = fx.w
    f1 = ref["fates"][1].reshape(fx.h, w)
    assert (f1[:, w // 2:] == FH.EMITTED).all() and (f1[:, :w // 2] == FH.SUPPRESSED).sum() > 0
    sel = (ref["src_image"] == 1)
    assert (ref["view_mask"][sel][ref["src_pixel"][sel] % w >= w // 2] == 0).all()
    # accuracy: X is the mean of its contributors' points and the distance to a
    # plane is convex, so a point is at most as far as its farthest contributor.
    # On top, float rounding: a world point is a handful of float operations on
    # numbers of the depth's size (d * ray, three products summed, + C), each
    # off by at most half an ulp of the depth; the m-term sum and the division
    # add at most (m + 1) / 2 ulps more.  16 ulps of the largest depth cover
    # m <= 3 with room: 16 * 2^-23 * 4.1 < 8e-6.
    P = FH.Problem(*sc.args())
    allow = 16 * np.spacing(F(sc.depth.max()))
    worst = np.zeros(ref["n_points"])
    for k in range(ref["n_points"]):
        i, p = int(ref["src_image"][k]), int(ref["src_pixel"][k])
        dist = [abs(float(P.world_point(i, np.array([p]), P.d[i][[p]])[2][0]) - fx.far)]
        for b, j in enumerate(ref["lists"][i]):
            if (int(ref["view_mask"][k]) >> b) & 1:
                A, bb = P.V.nbs[i][b][1], P.V.nbs[i][b][2]
                ap = DH.mul_pixel(A, F(p % w), F(p // w))
                d = P.d[i][p]
                h0, h1, z = d * ap[0] + bb[0], d * ap[1] + bb[1], d * ap[2] + bb[2]
                q = int(np.floor(h1 / z + F(0.5))) * w + int(np.floor(h0 / z + F(0.5)))
                dist.append(abs(float(P.world_point(j, np.array([q]), P.d[j][[q]])[2][0]) - fx.far))
        worst[k] = max(dist)
    assert (plane_distance(fx, res["X"]) <= worst + allow).all()


def test_normal_test_on_either_side_of_the_threshold():
    """(c): cos between view 0's and view 1's normals is set to 0.95 in the left
    half and 0.85 in the right; the threshold 0.9 keeps only the left agreements"""
    fx = DH.plane_fixture()
    sc = FH.Scene([fx])
    w = fx.w
    for cos, cols in ((0.95, slice(0, w // 2)), (0.85, slice(w // 2, w))):
        s = np.sqrt(1 - cos * cos)
        sc.normal_maps[1][:, cols] = np.array([s, 0, -cos], F)   # R is the identity: camera = world
    ref_off, ref_on = sc.ref(), sc.ref(min_normal_cos=0.9)
    assert ref_on["n_points"] > ref_off["n_points"]
    f1 = ref_on["fates"][1].reshape(fx.h, w)
    assert (f1[:, w // 2:] == FH.EMITTED).all() and (f1[:, :w // 2] == FH.SUPPRESSED).any()
    FH.check_against_ref(sc.run(None), ref_off)
    FH.check_against_ref(sc.run(None, FH.fuse_opts(min_normal_cos=0.9)), ref_on)


def test_pair_lists_reverse_only_and_dropped():
    # an image with no neighbours of its own, but listed by the others
    fx = DH.Fixture(24, 20, [(-0.25, 0, 0), (0, 0, 0), (0.3, 0.02, 0)], far=4.0, seed=11, neighbours=[[], [0, 2], [0]])
    sc = FH.Scene([fx])
    ref = sc.ref()
    assert ref["lists"] == [[1, 2], [0, 2], [0, 1]] and ref["n_suppressed"] > 0
    FH.check_against_ref(sc.run(None), ref)
    star = FH.Scene([FH.star_fixture()])
    ref = star.ref()
    assert len(ref["lists"][0]) == 32 and ref["n_pairs_dropped"] == 1 and ref["lists"][0] == list(range(1, 33))
    res = star.run(None)
    FH.check_against_ref(res, ref)
    assert res["stats"]["n_pairs_dropped"] == 1 and int(res["view_mask"].max()) >> 31 == 1


def test_unloaded_channels_and_no_pixels():
    fxs = [FH.group(13, 5, channels=[3, 1, 3]), FH.group(9, 7, channels=[1, 3, 1], seed=7)]
    sc = FH.Scene(fxs, unloaded=(1,))
    ref = sc.ref()
    assert (ref["fates"][1] == FH.NONE).all() and ref["n_suppressed"] > 0
    assert (ref["rgb"][:, 0] != ref["rgb"][:, 2]).any()
    FH.check_against_ref(sc.run(None), ref)
    plain = FH.Scene(fxs, colours=False)
    res = plain.run(None)
    assert res["rgb"] is None
    FH.check_against_ref(res, plain.ref())
    # without pixels rgb is not written
    rc, arrays, st = api.depthmap_fuse_raw(None, *plain.args(), fill=7)
    assert rc == 0 and (arrays["rgb"] == 7).all() and st["n_points"] > 0


def test_cap_points_one_too_small():
    sc = FH.Scene([FH.group(13, 5)])
    need = sc.ref()["n_points"]
    rc, arrays, st = api.depthmap_fuse_raw(None, *sc.args(), images=sc.images, cap_points=need - 1, fill=9)
    assert rc == abi.SFM_ERR_INVALID_ARG and st["n_points"] == need
    assert b"cap_points" in abi.load().sfm_last_error()
    assert all((a == 9).all() for a in arrays.values())
    rc, arrays, st = api.depthmap_fuse_raw(None, *sc.args(), images=sc.images, cap_points=need)
    assert rc == 0 and st["n_points"] == need


def test_argument_checks():
    sc = FH.Scene([FH.group(9, 7)])
    wh, K, R, C, nb_off, nb_view, depth, normal = sc.args()

    def bad(match, code=abi.SFM_ERR_INVALID_ARG, **kw):
        a = dict(wh=wh, K=K, R=R, Cc=C, nb_off=nb_off, nb_view=nb_view, depth=depth, normal=normal, images=sc.images)
        a.update(kw)
        with pytest.raises(api.SfmError, match=match) as e:
            api.depthmap_fuse_host(**a)
        assert e.value.code == code

    w2 = wh.copy()
    w2[0] = 0
    # the sizes change the map length, so the binding's own length check is bypassed with empty maps
    bad("non-positive size", wh=w2, depth=np.zeros(0, F), normal=np.zeros(0, F))
    v = nb_view.copy()
    v[0] = 0
    bad("names the neighbour", nb_view=v)
    v[0] = 3
    bad("names the neighbour", nb_view=v)
    o = nb_off.copy()
    o[0] = 1
    bad("nb_off", nb_off=o)
    bad("more than 8", nb_off=np.array([0, 9, 9, 9]), nb_view=np.array([1, 2] * 4 + [1], np.int32))
    Kb = K.copy()
    Kb[1] = 0
    bad("singular", K=Kb)
    Rb = R.copy()
    Rb[2, 0, 0] = np.nan
    bad("not finite", R=Rb)
    bad("rel_tol", opts=FH.fuse_opts(rel_tol=-1.0))
    bad("rel_tol", opts=FH.fuse_opts(rel_tol=float("nan")))
    bad("min_normal_cos", opts=FH.fuse_opts(min_normal_cos=1.5))
    bad("min_normal_cos", opts=FH.fuse_opts(min_normal_cos=float("nan")))
    bad("device_bytes", opts=FH.fuse_opts(device_bytes=-1))
    bad("resident bytes", code=abi.SFM_ERR_UNSUPPORTED, opts=FH.fuse_opts(device_bytes=64))
    ch, off, px = api._pixel_pool(sc.images)
    ch2 = ch.copy()
    ch2[1] = 2
    bad("channels", images=None, pool=(ch2, off, px))
    lib = abi.load()
    rc = lib.sfm_depthmap_fuse_host(-1, *([None] * 12), 0, *([None] * 8))
    assert rc == abi.SFM_ERR_INVALID_ARG
    rc, _, _ = api.depthmap_fuse_raw(None, *sc.args(), cap_points=-1)
    assert rc == abi.SFM_ERR_INVALID_ARG and b"cap_points" in lib.sfm_last_error()
    # nothing to do
    res = api.depthmap_fuse_host(np.zeros(0, np.int32), np.zeros((0, 3, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)),
                                 np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, F), np.zeros(0, F))
    assert res["stats"]["n_points"] == 0 and len(res["X"]) == 0


def test_cloud_views_and_ply(tmp_path, case_a):
    fx, est, flt, ref = case_a
    res = fuse_of(fx, flt, est)
    off, idx = api.dense_cloud_views(fx.n, fx.nb_off, fx.nb_view, res["src_image"], res["view_mask"])
    roff, ridx = FH.views_ref(ref["lists"], ref["src_image"], ref["view_mask"])
    assert np.array_equal(off, roff) and np.array_equal(idx, ridx)
    assert np.array_equal(np.diff(off), res["n_views"])
    with pytest.raises(api.SfmError, match="beyond"):
        api.dense_cloud_views(fx.n, fx.nb_off, fx.nb_view, [0], [1 << 5])
    with pytest.raises(api.SfmError, match="names image"):
        api.dense_cloud_views(fx.n, fx.nb_off, fx.nb_view, [7], [0])
    n = ref["n_points"]
    for with_n, with_c in ((True, True), (False, True), (True, False), (False, False)):
        path = tmp_path / "cloud.ply"
        api.dense_cloud_write_ply(path, res["X"], res["N"] if with_n else None, res["rgb"] if with_c else None)
        lines, body = FH.read_ply(path)
        want = ["ply", "format binary_little_endian 1.0", "element vertex %d" % n] + [
            "property float " + c for c in ("x", "y", "z") + (("nx", "ny", "nz") if with_n else ())] + [
            "property uchar " + c for c in (("red", "green", "blue") if with_c else ())] + ["end_header"]
        assert lines == want
        cols = [ref["X"][:, 0], ref["X"][:, 1], ref["X"][:, 2]]
        cols += [ref["N"][:, c] for c in range(3)] if with_n else []
        cols += [ref["rgb"][:, c] for c in range(3)] if with_c else []
        for name, col in zip(body.dtype.names, cols):
            assert body[name].tobytes() == np.ascontiguousarray(col).tobytes(), name
    with pytest.raises(api.SfmError, match="cannot open"):
        api.dense_cloud_write_ply(tmp_path / "no" / "dir.ply", res["X"])


def test_densify_host_equals_the_twins_chained():
    fx = DH.small_fixture()
    o = DH.opts(r=2, iterations=1, seed=SEED)
    est = fx.run(None, o)
    flt = fx.filter(None, est)
    cloud = fuse_of(fx, flt, est)
    assert cloud["stats"]["n_points"] > 0
    res = api.densify_host(fx.wh, fx.K, fx.R, fx.C, fx.nb_off, fx.nb_view, fx.drange, fx.images, o)
    FH.same_cloud(res, cloud)
    DH.same_maps(res, est)
    assert res["depth_filtered"].tobytes() == flt["depth"].tobytes() and res["n_agree"].tobytes() == flt["n_agree"].tobytes()
    assert np.array_equal(res["counts"], flt["counts"])
    st = res["stats"]
    assert st["fuse"]["n_points"] == cloud["stats"]["n_points"] and st["filter"]["n_kept"] == flt["stats"]["n_kept"]
    assert st["depthmap"]["n_estimated"] == est["stats"]["n_estimated"]
    lean = api.densify_host(fx.wh, fx.K, fx.R, fx.C, fx.nb_off, fx.nb_view, fx.drange, fx.images, o, maps=False)
    FH.same_cloud(lean, cloud)
