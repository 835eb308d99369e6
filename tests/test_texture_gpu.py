"""Mesh texturing on the device: sfm_mesh_face_views, sfm_mesh_texture_bake and
sfm_mesh_texture against their host twins and against the numpy restatement
(_texture_helpers.py), bytes and counts, on the smallest shapes that reach
each device-only branch: face counts around the wavefront and the workgroup,
atlas rows that are no multiple of a lane's run, small and odd images, the
wavefront-per-face path and its threshold, faces without a pixel, a budget too
small; and the one-call path against the two calls chained."""
import os
import re

import numpy as np
import pytest

import _depthmap_helpers as DH
import _texture_helpers as TH

abi, api, F = TH.abi, TH.api, TH.F
pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 513]
SCENES = ["occlusion", "backfacing", "not_drawable", "tie", "skipped", "mixed", "large", "subpixel", "threshold"]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def test_constants_mirror_the_header():
    src = open(os.path.join(ROOT, "3dreconstruction_amd", "csrc", "texture_point.h")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kTex\w+) = (\d+);", src)}
    assert got == {"kTexBlock": abi.TEX_BLOCK, "kTexLargeBox": abi.TEX_LARGE_BOX, "kTexRun": abi.TEX_RUN,
                   "kTexSub": abi.TEX_SUB, "kTexMinCell": abi.TEX_MIN_CELL, "kTexMaxCell": abi.TEX_MAX_CELL,
                   "kTexDefaultCell": abi.TEX_DEFAULT_CELL, "kTexMaxAtlas": abi.TEX_MAX_ATLAS}


def three_way(ctx, sc, cell=8, fill=(0, 0, 0)):
    """device, host twin and restatement: face views, bake, and the one call"""
    ref = sc.views_ref()
    dev, host = sc.views(ctx), sc.views(None)
    TH.check_views(dev, ref)
    TH.check_views(host, ref)
    assert dev["stats"]["resident_bytes"] == host["stats"]["resident_bytes"] > 0
    o = TH.opts(cell, fill)
    bref = sc.bake_ref(ref["face_view"], cell, fill)
    bdev, bhost = sc.bake(ctx, ref["face_view"], o), sc.bake(None, ref["face_view"], o)
    TH.check_bake(bdev, bref)
    TH.check_bake(bhost, bref)
    one = sc.texture(ctx, o)
    TH.same_texture(one, dict(bdev, face_view=dev["face_view"], face_pixels=dev["face_pixels"]))
    assert one["stats"]["views"]["n_textured"] == ref["n_textured"]
    return dev, bdev, ref


@pytest.mark.parametrize("n_faces", FACES)
def test_face_counts_around_the_wavefront_and_the_workgroup(ctx, n_faces):
    dev, bake, ref = three_way(ctx, TH.strip_scene(n_faces), 8, (5, 6, 7))
    assert dev["stats"]["n_textured"] > 0
    # an odd count leaves the last half empty: its texels are the fill
    f = TH.texel_faces(n_faces, 8)[0]
    assert (bake["texture"][f < 0] == np.array((5, 6, 7), np.uint8)).all() and ((f < 0).any() or n_faces % 2 == 0)


@pytest.mark.parametrize("cell", [4, 5])
@pytest.mark.parametrize("n_faces", [3, 65, 257])
def test_atlas_rows_that_are_no_multiple_of_a_run(ctx, n_faces, cell):
    three_way(ctx, TH.strip_scene(n_faces), cell, (1, 2, 3))


@pytest.mark.parametrize("size", [(17, 5), (1, 1)])
@pytest.mark.parametrize("n_faces", [3, 65])
def test_small_and_odd_images(ctx, n_faces, size):
    three_way(ctx, TH.strip_scene(n_faces, size))


@pytest.mark.parametrize("name", SCENES)
def test_scenes(ctx, name):
    sc = TH.named_scene(name)
    dev, _, ref = three_way(ctx, sc)
    if name == "large":
        # the pair over the whole image goes one wavefront a face
        assert ref["covered"][0, :2].sum() > 2 * abi.TEX_LARGE_BOX and (dev["face_view"][:2] == 0).all()
        assert (dev["face_view"][2:] == -1).all()
    if name == "threshold":
        boxes = [16 * 16, 17 * 16]
        assert boxes[0] == abi.TEX_LARGE_BOX < boxes[1] and (dev["face_view"] == 0).all()
    if name == "subpixel":
        assert (dev["face_pixels"] == 0).all() and dev["stats"]["n_untextured"] == len(sc.tri)
    if name == "not_drawable":
        assert dev["stats"]["n_not_drawable"] == 4
    if name == "skipped":
        assert (dev["face_view"] == 1).all()


def test_fallback_colours_on_the_device(ctx):
    sc = TH.named_scene("subpixel")
    rgb = np.random.default_rng(11).integers(0, 256, (len(sc.V), 3), dtype=np.uint8)
    three_way(ctx, TH.Scene(sc.wh, sc.C, sc.V, sc.tri, vertex_rgb=rgb), 5, (9, 8, 7))


def test_a_budget_too_small_leaves_everything_untouched(ctx):
    sc = TH.strip_scene(65)
    o = TH.opts(8, device_bytes=1024)
    fv = np.zeros(65, np.int32)
    rc, a, b, st = api.mesh_face_views_raw(ctx, *sc.cam(), images=sc.images, opts=o, fill=7)
    assert rc == abi.SFM_ERR_UNSUPPORTED and (a == 7).all() and (b == 7).all() and st["resident_bytes"] == 0
    rc, tex, uv, _ = api.mesh_texture_bake_raw(ctx, *sc.cam(), fv, images=sc.images, opts=o, fill=7)
    assert rc == abi.SFM_ERR_UNSUPPORTED and (tex == 7).all() and (uv == 7).all()
    rc, a, b, tex, uv, _ = api.mesh_texture_raw(ctx, *sc.cam(), images=sc.images, opts=o, fill=7)
    assert rc == abi.SFM_ERR_UNSUPPORTED and all((x == 7).all() for x in (a, b, tex, uv))
    # the context is still good
    TH.check_views(sc.views(ctx), sc.views_ref())


@pytest.mark.parametrize("views", [False, True])
def test_texture_equals_the_two_calls_chained(ctx, views):
    sc = TH.named_scene("occlusion")
    o = TH.opts(5, (3, 2, 1))
    chosen = sc.views(ctx, o)
    baked = sc.bake(ctx, chosen["face_view"], o)
    one, host = sc.texture(ctx, o, views=views), sc.texture(None, o)
    TH.same_texture(one, baked)
    TH.same_texture(one, host)
    for k in ("n_textured", "n_untextured", "n_not_drawable", "sum_pixels"):
        assert one["stats"]["views"][k] == chosen["stats"][k] == host["stats"]["views"][k]
    assert one["stats"]["views"]["n_textured"] > 0
    if views:
        assert one["face_view"].tobytes() == chosen["face_view"].tobytes()
    else:
        assert "face_view" not in one


def test_end_to_end_from_images_to_a_textured_mesh(ctx):
    fx, opt = DH.small_fixture(), DH.opts(2, 1, 2, 7)
    dense = api.densify(ctx, fx.wh, fx.K, fx.R, fx.C, fx.nb_off, fx.nb_view, fx.drange, fx.images, opt)
    grid = api.mesh_grid_fit(dense["X"], 24, 2)
    mesh = api.mesh_reconstruct(ctx, fx.wh, fx.K, fx.R, fx.C, dense["depth_filtered"], grid, images=fx.images)
    args = (fx.wh, fx.K, fx.R, fx.C, mesh["V"], mesh["tri"])
    dev = api.mesh_texture(ctx, *args, images=fx.images, vertex_rgb=mesh["rgb"])
    host = api.mesh_texture(None, *args, images=fx.images, vertex_rgb=mesh["rgb"])
    TH.same_texture(dev, host)
    assert dev["stats"]["views"]["n_textured"] == host["stats"]["views"]["n_textured"] > 0
    wh = np.asarray(fx.wh).reshape(-1, 2)
    for f in np.flatnonzero(dev["face_view"] >= 0):
        v = int(dev["face_view"][f])
        M, Cf = TH.view_constants(np.asarray(fx.K).reshape(-1, 9)[v], np.asarray(fx.R).reshape(-1, 9)[v],
                                  np.asarray(fx.C).reshape(-1, 3)[v])
        P = mesh["V"][mesh["tri"][f]]
        x, y, z = TH.project(M, Cf, [P[:, c] for c in range(3)])
        assert (z > 0).all() and (x >= 0).all() and (x <= wh[v, 0] - 1).all() and (y >= 0).all() and (y <= wh[v, 1] - 1).all()
