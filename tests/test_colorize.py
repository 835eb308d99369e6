"""CPU: the host twin of the track colouring (sfm_colorize_assign_host,
sfm_colorize_sample, sfm_colorize_host, sfm_colorize_write_ply) against the
recounting restatement of _colorize_helpers.py, exactly, and the argument
checks of include/sfmcore.h ("Track colouring")."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _colorize_helpers as CH

abi, api, RH = CH.abi, CH.api, CH.RH
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = abi.SFM_ERR_INVALID_ARG


def run_host(t, wh, images, pt_ok=None, keep_obs=None):
    """assign, sample and the one-call form on the host twin, each against the restatement"""
    res = api.colorize_assign_host(t.problem(), wh, pt_ok, keep_obs)
    ref = CH.check_against_ref(res, t, wh, pt_ok, keep_obs)
    want = CH.sample_ref(ref["view"], ref["px"], images)
    np.testing.assert_array_equal(api.colorize_sample(res["view"], res["px"], wh, images), want)
    one = api.colorize_host(t.problem(), wh, images, pt_ok, keep_obs)
    np.testing.assert_array_equal(one["rgb"], want)
    np.testing.assert_array_equal(one["view"], ref["view"])
    assert one["stats"]["n_rounds"] == ref["n_rounds"]
    return res, ref, want


@pytest.mark.parametrize("seed", [1, 2])
def test_random_scenes(seed):
    t, wh, images, ok, keep = CH.random_scene(seed)
    res, ref, _ = run_host(t, wh, images, ok, keep)
    assert 1 < ref["n_rounds"] <= t.n_img and (ref["view"][~ok] == -1).all()
    run_host(t, wh, images)              # no masks
    run_host(t, wh, images, ok, None)
    run_host(t, wh, images, None, keep)


def test_null_masks_equal_all_ones():
    t, wh, images, _, _ = CH.random_scene(3, n_img=12, n_pt=300)
    a = api.colorize_assign_host(t.problem(), wh)
    b = api.colorize_assign_host(t.problem(), wh, np.ones(t.n_pt, bool), np.ones(t.n_obs, bool))
    CH.same_assign(a, b)


def test_ties_go_to_the_lowest_index():
    # images 1 and 3 see four points each; image 0 three.  1 goes first, which leaves 3 with two and 0 with three.
    a, b, c, d, e, f, g, h = range(8)
    sees = {1: [a, b, c, d], 3: [c, d, e, f], 0: [g, h, e]}
    lists = [[im for im in (3, 1, 0) if p in sees[im]] for p in range(8)]    # (track order is not image order)
    wh, images = CH.random_images(0, 4)
    t = CH.tracks_from_lists(4, lists, wh)
    res, ref, _ = run_host(t, wh, images)
    counts = CH.initial_counts(t)
    assert counts[1] == counts[3] == 4 and counts[0] == 3 and counts[2] == 0
    assert list(res["order"]) == [1, 0, 3, -1] and res["n_rounds"] == 3
    assert list(res["view"]) == [1, 1, 1, 1, 0, 3, 0, 0]


def test_second_by_initial_count_is_not_second_round():
    # A = 0 sees ten points, B = 1 nine (eight of them A's), C = 2 five of its own
    lists = [[0, 1]] * 8 + [[0]] * 2 + [[1]] + [[2]] * 5
    wh, images = CH.random_images(1, 3)
    t = CH.tracks_from_lists(3, lists, wh)
    counts = CH.initial_counts(t)
    assert list(np.argsort(-counts, kind="stable")) == [0, 1, 2] and list(counts) == [10, 9, 5]
    ref = CH.assign_ref(t, wh)
    assert list(ref["order"]) == [0, 2, 1]       # the restatement: B, second by initial count, goes last
    res, _, _ = run_host(t, wh, images)
    assert list(res["order"]) == [0, 2, 1]


def test_several_observations_in_one_image():
    # point 0: twice in image 0; point 1: three times in image 1, the first dead; point 2: image 1 and twice image 0
    lists = [[0, 0], [1, 1, 1], [1, 0, 0]]
    wh, images = CH.random_images(2, 2)
    t = CH.tracks_from_lists(2, lists, wh)
    keep = np.ones(t.n_obs, bool)
    keep[2] = False
    res, _, _ = run_host(t, wh, images, None, keep)
    assert list(CH.initial_counts(t, None, keep)) == [2, 2]          # each point once per image
    assert list(res["order"]) == [0, 1] and list(res["view"]) == [0, 1, 0]
    assert list(res["obs"]) == [0, 3, 6]        # the first live one: 3 takes over from the dead 2; 6, not 7
    res, _, _ = run_host(t, wh, images)
    assert list(res["obs"]) == [0, 2, 6]


def test_point_without_a_live_observation():
    lists = [[0, 1], [1], [0]]
    wh, images = CH.random_images(3, 2)
    t = CH.tracks_from_lists(2, lists, wh)
    keep = np.array([1, 1, 0, 1], bool)          # point 1's only observation is dead
    res, _, rgb = run_host(t, wh, images, np.ones(3, bool), keep)
    assert res["view"][1] == -1 and res["obs"][1] == -1 and (rgb[1] == 0).all()
    assert res["stats"]["n_to_colour"] == 2 and res["stats"]["n_coloured"] == 2


def test_one_image():
    wh, images = CH.random_images(4, 1)
    t = CH.tracks_from_lists(1, [[0], [0, 0], []], wh)
    res, _, _ = run_host(t, wh, images)
    assert list(res["order"]) == [0] and res["n_rounds"] == 1 and list(res["view"]) == [0, 0, -1]


def test_every_point_masked_off():
    t, wh, images, _, keep = CH.random_scene(5, n_img=6, n_pt=50)
    res, _, rgb = run_host(t, wh, images, np.zeros(t.n_pt, bool), keep)
    assert res["n_rounds"] == 0 and (res["order"] == -1).all() and (res["view"] == -1).all() and (rgb == 0).all()
    assert res["stats"]["n_to_colour"] == 0


def test_empty_problem():
    t = RH.Tracks(0, [0], [], np.zeros((0, 2)))
    res = api.colorize_assign_host(t.problem(), np.zeros(0, np.int32))
    assert res["n_rounds"] == 0 and len(res["view"]) == 0


def test_pixel_rule():
    # two images of different, non-square sizes and channel counts in one pool
    wh = np.array([[7, 4], [5, 9]], np.int32)
    rng = np.random.default_rng(6)
    images = [rng.integers(0, 256, (4, 7, 3), dtype=np.uint8), rng.integers(0, 256, (9, 5), dtype=np.uint8)]
    cases = []                                   # (image, u, v, x, y)
    for im, (w, h) in enumerate(wh):
        for u, x in ((-2.5, 0), (-0.4, 0), (w - 1.0, w - 1), (w - 0.25, w - 1), (float(w), w - 1), (w + 30.0, w - 1),
                     (2.999999, 2), (1.5, 1), (0.7, 0)):
            cases.append((im, u, 1.2, x, 1))
        for v, y in ((-7.0, 0), (h - 1.0, h - 1), (h - 0.25, h - 1), (float(h), h - 1), (h + 2.0, h - 1), (2.5, 2),
                     (1.99, 1), (0.5, 0)):
            cases.append((im, 3.6, v, 3, y))
    t = RH.Tracks(2, np.arange(len(cases) + 1), [c[0] for c in cases], [[c[1], c[2]] for c in cases])
    res, _, rgb = run_host(t, wh, images)
    for p, (im, _, _, x, y) in enumerate(cases):
        assert res["view"][p] == im and tuple(res["px"][p]) == (x, y), cases[p]
        assert tuple(rgb[p]) == (tuple(images[im][y, x]) if im == 0 else (images[im][y, x],) * 3)


def test_sample_with_an_unloaded_image():
    lists = [[0], [0], [1]]
    wh, images = CH.random_images(7, 3)
    t = CH.tracks_from_lists(3, lists, wh)
    res = api.colorize_assign_host(t.problem(), wh)
    want = CH.sample_ref(res["view"], res["px"], images)
    # image 2 colours nothing: it may stay unloaded
    np.testing.assert_array_equal(api.colorize_sample(res["view"], res["px"], wh, images[:2] + [None]), want)
    np.testing.assert_array_equal(api.colorize_host(t.problem(), wh, images[:2] + [None])["rgb"], want)
    # image 1 colours point 2
    with pytest.raises(api.SfmError) as ei:
        api.colorize_sample(res["view"], res["px"], wh, [images[0], None, images[2]])
    assert ei.value.code == INVALID and "not loaded" in str(ei.value)


def _raises_invalid(fn, *a, **kw):
    with pytest.raises(api.SfmError) as ei:
        fn(*a, **kw)
    assert ei.value.code == INVALID, ei.value
    assert len(str(ei.value).split(": ", 1)[1]) > 0      # a message


def test_argument_checks():
    wh, images = CH.random_images(8, 3)
    t = CH.tracks_from_lists(3, [[0, 1], [1, 2], [2]], wh)
    host = api.colorize_assign_host
    host(t.problem(), wh)
    lib = abi.load()
    # the checks of sfm_recon_tracks_create
    n_rounds = C.c_int32()
    assert lib.sfm_colorize_assign_host(None, abi.ptr(wh.reshape(-1), abi.i32p), None, None, None, None, None, None,
                                        C.byref(n_rounds), None) == INVALID
    pr = t.problem(); pr.n_pt = -1
    _raises_invalid(host, pr, wh)
    pr = t.problem(); pr.pt_offsets = None
    _raises_invalid(host, pr, wh)
    bad = RH.Tracks(3, [1, 2, 5, 5], t.obs_img, t.obs_uv)           # does not start at 0
    _raises_invalid(host, bad.problem(), wh)
    bad = RH.Tracks(3, [0, 2, 4, 4], t.obs_img, t.obs_uv)           # does not end at n_obs
    pr = bad.problem(); pr.n_obs = 5
    _raises_invalid(host, pr, wh)
    bad = RH.Tracks(3, t.pt_offsets.copy(), t.obs_img, t.obs_uv)
    bad.pt_offsets[1:3] = [4, 2]                                    # not monotone
    _raises_invalid(host, bad.problem(), wh)
    for im in (-1, 3):
        img = t.obs_img.copy(); img[2] = im
        _raises_invalid(host, RH.Tracks(3, t.pt_offsets, img, t.obs_uv).problem(), wh)
    # null outputs
    pr = t.problem()
    assert lib.sfm_colorize_assign_host(C.byref(pr), abi.ptr(wh.reshape(-1), abi.i32p), None, None, None, None, None,
                                        None, C.byref(n_rounds), None) == INVALID
    # a non-positive image size
    for k, v in ((0, 0), (3, -4)):
        w2 = wh.copy().reshape(-1); w2[k] = v
        _raises_invalid(host, t.problem(), w2)
    # 2^31 points or observations: refused before any array is read
    big_off = np.array([0, 2 ** 31], np.int64)
    pr = t.problem(); pr.n_pt, pr.n_obs, pr.pt_offsets = 1, 2 ** 31, abi.ptr(big_off, abi.i64p)
    assert lib.sfm_colorize_assign_host(C.byref(pr), abi.ptr(wh.reshape(-1), abi.i32p), None, None, None, None, None,
                                        None, C.byref(n_rounds), None) == INVALID
    pr = t.problem(); pr.n_pt = 2 ** 31
    assert lib.sfm_colorize_assign_host(C.byref(pr), abi.ptr(wh.reshape(-1), abi.i32p), None, None, None, None, None,
                                        None, C.byref(n_rounds), None) == INVALID
    assert b"2^31" in lib.sfm_last_error()
    # a non-finite uv: refused on a live observation of a point to colour, not read otherwise
    for val in (np.nan, np.inf, -np.inf):
        uv = t.obs_uv.copy(); uv[3, 1] = val                        # observation 3 belongs to point 1
        nf = RH.Tracks(3, t.pt_offsets, t.obs_img, uv)
        _raises_invalid(host, nf.problem(), wh)
        keep = np.ones(5, bool); keep[3] = False
        host(nf.problem(), wh, None, keep)
        ok = np.ones(3, bool); ok[1] = False
        host(nf.problem(), wh, ok, None)
    # sfm_colorize: channels, and an unloaded image that a point to colour is seen in
    four = [images[0], np.zeros((wh[1, 1], wh[1, 0], 4), np.uint8), images[2]]
    _raises_invalid(api.colorize_host, t.problem(), wh, four)
    two = [images[0], np.zeros((wh[1, 1], wh[1, 0], 2), np.uint8), images[2]]
    _raises_invalid(api.colorize_host, t.problem(), wh, two)
    _raises_invalid(api.colorize_sample, np.zeros(1, np.int32), np.zeros(2, np.int32), wh, two)
    _raises_invalid(api.colorize_host, t.problem(), wh, [images[0], images[1], None])
    ok = np.array([1, 0, 0], bool)                                  # only point 0 (images 0, 1) is to colour
    api.colorize_host(t.problem(), wh, [images[0], images[1], None], ok)
    # sfm_colorize_sample: a view or a pixel out of range
    _raises_invalid(api.colorize_sample, np.array([3], np.int32), np.zeros(2, np.int32), wh, images)
    _raises_invalid(api.colorize_sample, np.array([-2], np.int32), np.zeros(2, np.int32), wh, images)
    _raises_invalid(api.colorize_sample, np.array([0], np.int32), np.array([wh[0, 0], 0], np.int32), wh, images)
    # the device entry points check their context on the host
    assert lib.sfm_colorize_assign(None, C.byref(t.problem()), abi.ptr(wh.reshape(-1), abi.i32p), None, None, None,
                                   None, None, None, C.byref(n_rounds), None) == INVALID
    assert lib.sfm_colorize(None, C.byref(t.problem()), abi.ptr(wh.reshape(-1), abi.i32p), None, None, None, None,
                            None, None, None, None) == INVALID
    assert lib.sfm_sparse_reconstruct_colorize(None, b".", b".", -1.0, None, None, None, None, None, None) == INVALID


def _ply_lines(path):
    lines = open(path).read().splitlines()
    k = lines.index("end_header") + 1
    return lines[:k], lines[k:]


def test_write_ply(tmp_path):
    rng = np.random.default_rng(9)
    n_pt = 7
    X = rng.normal(size=(n_pt, 3)) * 10
    ok = np.array([1, 1, 0, 1, 1, 0, 1], bool)
    X[~ok] = np.nan
    rgb = rng.integers(0, 256, (n_pt, 3), dtype=np.uint8)
    extr = np.zeros((3, 6))
    extr[:, 3:] = rng.normal(size=(3, 3))
    extr[2, :3] = [0.3, -0.2, 0.1]
    reg = np.array([1, 0, 1], bool)
    # the expectation, in cloud_and_poses.ply's shape: the points that are set, ascending, then the registered centres
    head = ["ply", "format ascii 1.0", f"element vertex {ok.sum() + reg.sum()}", "property double x", "property double y",
            "property double z", "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    pts = ["%.16f %.16f %.16f" % tuple(X[p]) for p in np.flatnonzero(ok)]
    cam0 = "%.16f %.16f %.16f 0 255 0" % tuple(-extr[0, 3:])           # no rotation: C = -t
    api.colorize_write_ply(tmp_path / "white.ply", X, ok, None, extr, reg)
    wh_, wb = _ply_lines(tmp_path / "white.ply")
    assert wh_ == head and wb[:len(pts)] == [s + " 255 255 255" for s in pts] and wb[len(pts)] == cam0
    assert len(wb) == len(pts) + 2 and wb[-1].endswith(" 0 255 0")
    api.colorize_write_ply(tmp_path / "colour.ply", X, ok, rgb, extr, reg)
    ch_, cb = _ply_lines(tmp_path / "colour.ply")
    assert ch_ == head and cb[len(pts):] == wb[len(pts):]              # the same camera lines
    assert cb[:len(pts)] == [s + " %d %d %d" % tuple(rgb[p]) for s, p in zip(pts, np.flatnonzero(ok))]
    # no masks: every point and every camera
    api.colorize_write_ply(tmp_path / "all.ply", np.nan_to_num(X), None, rgb, extr, None)
    ah, ab = _ply_lines(tmp_path / "all.ply")
    assert ah[2] == f"element vertex {n_pt + 3}" and len(ab) == n_pt + 3
    with pytest.raises(api.SfmError) as ei:
        api.colorize_write_ply(tmp_path / "no_such_dir" / "x.ply", X, ok, rgb, extr, reg)
    assert ei.value.code == INVALID


def test_cpp_colorize_program(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "colorize_test")
    assert os.path.exists(exe), "run make (builds tests/cpp/colorize_test)"
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path)      # (it writes a small PLY where it runs)
    assert r.returncode == 0 and "colorize ok" in r.stdout, r.stdout + r.stderr
