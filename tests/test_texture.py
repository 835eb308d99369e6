"""CPU: the texturing's host twins (sfm_mesh_face_views_host,
sfm_mesh_texture_bake_host, sfm_mesh_texture_host), sfm_mesh_atlas_fit and
sfm_mesh_write_textured_ply against the numpy restatement of the contract
(_texture_helpers.py): bytes and counts; the coverage partition worked out in
integers, occlusion, back-facing and not drawable faces, ties, skipped images,
constant and ramp images, the fallback, the UV corners, the argument checks."""
import os
import subprocess

import numpy as np
import pytest

import _texture_helpers as TH

abi, api, F = TH.abi, TH.api, TH.F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_both(sc, cell=8, fill=(0, 0, 0)):
    """face views and bake on the host against the restatement; returns (views, bake, ref)"""
    ref = sc.views_ref()
    views = sc.views(None)
    TH.check_views(views, ref)
    o = TH.opts(cell, fill)
    bake = sc.bake(None, views["face_view"], o)
    TH.check_bake(bake, sc.bake_ref(views["face_view"], cell, fill))
    one = sc.texture(None, o)
    TH.same_texture(one, dict(bake, face_view=views["face_view"], face_pixels=views["face_pixels"]))
    return views, bake, ref


@pytest.mark.parametrize("size,diagonal", [((9, 7), 0), ((9, 7), 1), ((8, 8), 0), ((8, 8), 1)])
def test_a_split_quad_partitions_its_pixel_centres(size, diagonal):
    x0, y0, x1, y1 = 2, 2, 2 + size[0], 2 + size[1]
    V, tri = TH.quad(x0, y0, x1, y1, diagonal=diagonal)
    sc = TH.Scene([(16, 12)], [(0, 0, 0)], V, tri)
    views, _, ref = run_both(sc)
    # the quad's own boundary by the tie rule, in integers; the rule keeps two of its four sides
    expect = TH.polygon_centres([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], 16, 12)
    assert expect == size[0] * size[1]
    assert ref["covered"][0].sum() == expect and views["face_pixels"].sum() == expect
    assert (views["face_view"] == 0).all() and (ref["won"] == ref["covered"]).all()


def test_a_fan_of_six_faces_partitions_its_pixel_centres():
    ring = [(12, 6), (10, 10), (6, 10), (4, 6), (6, 2), (10, 2)]
    V = [(8, 6, 4)] + [(x, y, 4) for x, y in ring]
    tri = [(0, 1 + (k + 1) % 6, 1 + k) for k in range(6)]
    sc = TH.Scene([(16, 12)], [(0, 0, 0)], V, tri)
    views, _, ref = run_both(sc)
    expect = TH.polygon_centres(ring, 16, 12)
    assert 0 < expect == ref["covered"][0].sum() == views["stats"]["sum_pixels"]
    assert (views["face_view"] == 0).all()


def test_occlusion_moves_a_hidden_face_to_the_other_view():
    sc = TH.named_scene("occlusion")
    views, _, ref = run_both(sc)
    fv, cov, won = views["face_view"], ref["covered"], ref["won"]
    partly0 = (won[0] < cov[0]) & (cov[0] > 0)
    assert partly0[:24].any()                                  # the near quad hides part of the wall in view 0
    for f in np.flatnonzero(partly0):
        assert fv[f] == (1 if ref["eligible"][1, f] else -1)
    for f in range(len(fv)):
        assert fv[f] < 0 or won[fv[f], f] == cov[fv[f], f]
    assert (fv[24:] >= 0).all()                                # the near quad itself is seen


def test_back_facing_faces_occlude_but_are_never_chosen():
    sc = TH.named_scene("backfacing")
    views, _, ref = run_both(sc)
    assert (views["face_view"][2:] == -1).all() and (ref["covered"][0, 2:] > 0).all()
    assert (ref["won"][0, :2] < ref["covered"][0, :2]).any() and views["stats"]["n_not_drawable"] == 0


def test_faces_that_are_not_drawable_are_counted():
    sc = TH.named_scene("not_drawable")
    views, _, ref = run_both(sc)
    assert views["stats"]["n_not_drawable"] == 4               # two faces, two views
    assert (views["face_view"][2:] == -1).all() and (views["face_view"][:2] >= 0).all()


def test_identical_cameras_give_the_lower_index():
    views, _, _ = run_both(TH.named_scene("tie"))
    assert (views["face_view"] == 0).all() and (views["face_pixels"] > 0).all()


def test_a_skipped_image_is_never_chosen():
    sc = TH.named_scene("skipped")
    views, _, ref = run_both(sc)
    assert (views["face_view"] == 1).all() and ref["covered"][0].sum() == 0
    # with every image loaded the same faces take view 0
    all_loaded = api.mesh_face_views(None, *sc.cam())
    assert (all_loaded["face_view"] == 0).all()


def test_one_channel_beside_three_channels():
    sc = TH.named_scene("mixed")
    views, bake, _ = run_both(sc)
    assert list(views["face_view"]) == [0, 0, 1, 1]
    f = TH.texel_faces(4, 8)[0]
    gray = bake["texture"][(f == 0) | (f == 1)]
    assert (gray[:, 0] == gray[:, 1]).all() and (gray[:, 1] == gray[:, 2]).all()


@pytest.mark.parametrize("cell", [4, 5, 8])
def test_constant_images_give_their_colour_exactly(cell):
    sc = TH.named_scene("occlusion")
    colours = [(200, 30, 7), (9, 250, 128)]
    const = TH.Scene(sc.wh, sc.C, sc.V, sc.tri, images=[np.full((24, 32, 3), c, np.uint8) for c in colours])
    fill = (1, 2, 3)
    views, bake, _ = run_both(const, cell, fill)
    f = TH.texel_faces(len(const.tri), cell)[0]
    expect = np.empty(bake["texture"].shape, np.uint8)
    expect[:] = fill
    for v, c in enumerate(colours):
        expect[(f >= 0) & (views["face_view"][np.maximum(f, 0)] == v)] = c
    assert np.array_equal(bake["texture"], expect)
    assert (views["face_view"] == -1).any() and (views["face_view"] == 0).any() and (views["face_view"] == 1).any()


def test_a_ramp_image_is_reproduced_within_one_grey_level():
    V, tri = TH.quad(3.25, 2.5, 27.75, 20.25)
    ramp = np.tile(np.arange(32, dtype=np.uint8) * 7, (24, 1))
    sc = TH.Scene([(32, 24)], [(0, 0, 0)], V, tri, images=[ramp])
    views, bake, _ = run_both(sc, 8)
    assert (views["face_view"] == 0).all()
    f, half, a, b, l1, l2 = TH.texel_faces(2, 8)
    checked = 0
    for ty, tx in zip(*np.nonzero((f >= 0) & (l1 + l2 <= 1))):        # the texels inside the UV triangle
        P = sc.V[sc.tri[f[ty, tx]]].astype(np.float64)
        x = (P[0] + float(l1[ty, tx]) * (P[1] - P[0]) + float(l2[ty, tx]) * (P[2] - P[0]))[0]   # pixel x = world X here
        # linear interpolation reproduces a linear function; 1 is the rounding of a value that falls on a half
        assert abs(int(bake["texture"][ty, tx, 0]) - 7 * x) <= 1.0
        checked += 1
    assert checked >= 2 * 15


@pytest.mark.parametrize("with_rgb", [False, True])
def test_untextured_faces_take_the_vertex_colours_or_the_fill(with_rgb):
    sc = TH.named_scene("subpixel")
    rgb = np.random.default_rng(11).integers(0, 256, (len(sc.V), 3), dtype=np.uint8) if with_rgb else None
    sc2 = TH.Scene(sc.wh, sc.C, sc.V, sc.tri, vertex_rgb=rgb)
    views, bake, _ = run_both(sc2, 8, (9, 8, 7))
    assert (views["face_view"] == -1).all() and (views["face_pixels"] == 0).all() and views["stats"]["n_untextured"] == 10
    f, half, a, b, l1, l2 = TH.texel_faces(10, 8)
    if with_rgb:
        corner = (f >= 0) & (l1 == 0) & (l2 == 0)                  # a corner texel is its vertex's colour
        assert np.array_equal(bake["texture"][corner], rgb[sc.tri[f[corner], 0]])
    else:
        assert (bake["texture"] == np.array((9, 8, 7), np.uint8)).all()


@pytest.mark.parametrize("cell", [4, 5, 8])
def test_uv_corners_and_the_bilinear_footprint(cell):
    n = 7
    sc = TH.strip_scene(n, two_views=False)
    bake = sc.bake(None, np.full(n, -1, np.int32), TH.opts(cell))
    W, H, cols = TH.atlas_ref(n, cell)
    corners = TH.corners_ref(n, cell)
    f, half, a, b, l1, l2 = TH.texel_faces(n, cell)
    for face in range(n):
        for k in range(3):
            u, v = bake["uv"][face, k]
            assert u == corners[face, k, 0] / F(W) and v == F(1.0) - corners[face, k, 1] / F(H)
            # the corner is the centre of a texel of the face, with the weights of that corner
            tx, ty = int(corners[face, k, 0] - F(0.5)), int(corners[face, k, 1] - F(0.5))
            assert corners[face, k, 0] == tx + 0.5 and corners[face, k, 1] == ty + 0.5 and f[ty, tx] == face
            assert (l1[ty, tx], l2[ty, tx]) == ((0, 0), (1, 0), (0, 1))[k]
    assert TH.footprint_clean(cell)


def test_the_footprint_reaches_the_gutter_and_stops_there():
    # s = 8: the triangle ends at x + y = 6; a fetch just inside it reads the gutter texel (5, 1), never (6, 1)
    assert TH.footprint_touched(8, 5, 1) and not TH.footprint_touched(8, 6, 1)
    assert TH.footprint_touched(8, 0, 0) and not TH.footprint_touched(8, -1, 0)


@pytest.mark.parametrize("n,expect", [(0, (0, 0, 0)), (1, (8, 8, 1)), (2, (8, 8, 1)), (3, (16, 8, 2)), (8, (16, 16, 2)),
                                      (9, (24, 16, 3))])
def test_atlas_fit(n, expect):
    assert api.mesh_atlas_fit(n, 8) == expect == TH.atlas_ref(n, 8)
    assert api.mesh_atlas_fit(n, 5) == TH.atlas_ref(n, 5)


def test_atlas_fit_refuses_what_is_beyond_its_limits():
    n = 2 * (32768 // 8) ** 2
    assert api.mesh_atlas_fit(n, 8) == (32768, 32768, 4096)
    assert api.mesh_atlas_fit_raw(n + 1, 8)[0] == abi.SFM_ERR_UNSUPPORTED
    assert api.mesh_atlas_fit_raw(2 ** 31, 4)[0] == abi.SFM_ERR_UNSUPPORTED
    assert api.mesh_atlas_fit_raw(-1, 8)[0] == abi.SFM_ERR_INVALID_ARG
    for cell in (3, 65, 0):
        assert api.mesh_atlas_fit_raw(4, cell)[0] == abi.SFM_ERR_INVALID_ARG


def test_checks():
    sc = TH.named_scene("tie")
    fv = np.zeros(2, np.int32)
    ok = api.mesh_texture_raw(None, *sc.cam(), images=sc.images)[0]
    assert ok == 0

    def all_three(cam, images=sc.images, opts=None, face_view=fv, vertex_rgb=None):
        return (api.mesh_face_views_raw(None, *cam, images=images, opts=opts)[0],
                api.mesh_texture_bake_raw(None, *cam, face_view, images=images, opts=opts, vertex_rgb=vertex_rgb)[0],
                api.mesh_texture_raw(None, *cam, images=images, opts=opts, vertex_rgb=vertex_rgb)[0])

    bad = abi.SFM_ERR_INVALID_ARG
    wh, K, R, C, V, tri = sc.cam()
    t2 = tri.copy()
    t2[1, 2] = len(V)
    assert all_three((wh, K, R, C, V, t2)) == (bad,) * 3
    t2[1, 2] = -1
    assert all_three((wh, K, R, C, V, t2)) == (bad,) * 3
    for value in (np.nan, np.inf):
        V2, K2, C2 = V.copy(), K.copy(), C.copy()
        V2[3, 1], K2[1, 4], C2[0, 2] = value, value, value
        assert all_three((wh, K, R, C, V2, tri)) == (bad,) * 3
        assert all_three((wh, K2, R, C, V, tri)) == (bad,) * 3
        assert all_three((wh, K, R, C2, V, tri)) == (bad,) * 3
    for cell in (3, 65):
        assert all_three(sc.cam(), opts=TH.opts(cell)) == (bad,) * 3
    assert all_three(sc.cam(), opts=TH.opts(8, device_bytes=-1)) == (bad,) * 3
    wh2 = wh.copy()
    wh2[1, 0] = 0
    assert all_three((wh2, K, R, C, V, tri)) == (bad,) * 3
    # channels other than 1 or 3 on a loaded image
    two = [np.zeros((12, 16, 2), np.uint8), sc.images[1]]
    assert all_three(sc.cam(), images=two) == (bad,) * 3
    # a face_view outside [-1, n_img), or naming a skipped image
    for v in (-2, 2):
        assert api.mesh_texture_bake_raw(None, *sc.cam(), np.array([0, v], np.int32), images=sc.images)[0] == bad
    assert api.mesh_texture_bake_raw(None, *sc.cam(), fv, images=[None, sc.images[1]])[0] == bad
    assert api.mesh_texture_bake_raw(None, *sc.cam(), fv + 1, images=[None, sc.images[1]])[0] == 0
    assert api.mesh_texture_bake_raw(None, *sc.cam(), fv, images=None)[0] == bad
    assert api.mesh_texture_bake_raw(None, *sc.cam(), fv - 1, images=None)[0] == 0
    assert api.mesh_texture_raw(None, *sc.cam(), images=None)[0] == bad
    # null arguments
    lib = abi.load()
    assert lib.sfm_mesh_face_views_host(2, None, None, None, None, None, None, None, 0, None, 0, None, None, None, None,
                                        None) == bad
    assert lib.sfm_mesh_atlas_fit(4, 8, None, None, None) == bad
    assert lib.sfm_mesh_write_textured_ply(None, b"t.ppm", 0, None, 0, None, None) == bad
    # a resident set beyond device_bytes: nothing is written
    for rc, *arrays in (api.mesh_face_views_raw(None, *sc.cam(), images=sc.images, opts=TH.opts(8, device_bytes=64), fill=7)[:3],
                        api.mesh_texture_bake_raw(None, *sc.cam(), fv, images=sc.images, opts=TH.opts(8, device_bytes=64),
                                                  fill=7)[:3],
                        api.mesh_texture_raw(None, *sc.cam(), images=sc.images, opts=TH.opts(8, device_bytes=64), fill=7)[:5]):
        assert rc == abi.SFM_ERR_UNSUPPORTED and all((a == 7).all() for a in arrays)


def test_no_triangles_succeed_and_write_nothing():
    sc = TH.named_scene("tie")
    wh, K, R, C, V, _ = sc.cam()
    none = np.zeros((0, 3), np.int32)
    rc, fv, fp, tex, uv, st = api.mesh_texture_raw(None, wh, K, R, C, V, none, images=sc.images, fill=7)
    assert rc == 0 and (tex == 7).all() and (uv == 7).all() and len(fv) == 0
    assert st["views"]["n_textured"] == 0 and st["bake"]["W"] == 0 and st["bake"]["H"] == 0


def test_the_textured_ply(tmp_path):
    sc = TH.strip_scene(5, two_views=False)
    res = sc.texture(None)
    path = str(tmp_path / "mesh.ply")
    api.mesh_write_textured_ply(path, "mesh_texture.ppm", sc.V, sc.tri, res["uv"])
    lines, V, rec, nf, head = TH.read_textured_ply(path)
    assert lines[:3] == ["ply", "format binary_little_endian 1.0", "comment TextureFile mesh_texture.ppm"]
    assert lines[3:] == [f"element vertex {len(sc.V)}", "property float x", "property float y", "property float z",
                         "element face 5", "property list uchar int vertex_indices", "property list uchar float texcoord", ""]
    assert os.path.getsize(path) == head + 12 * len(sc.V) + 38 * 5 and nf == 5
    assert np.array_equal(V, sc.V) and (rec["n"] == 3).all() and (rec["m"] == 6).all()
    assert np.array_equal(rec["tri"], sc.tri) and rec["uv"].tobytes() == res["uv"].tobytes()
    api.write_pnm(str(tmp_path / "mesh_texture.ppm"), res["texture"])
    assert open(tmp_path / "mesh_texture.ppm", "rb").read(2) == b"P6"


def test_cpp_texture_test(tmp_path):
    exe = os.path.join(ROOT, "tests", "cpp", "texture_test")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "texture ok" in r.stdout
