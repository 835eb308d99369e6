"""CPU: the mesh stage's host twins (sfm_tsdf_integrate_host,
sfm_mesh_extract_host, sfm_mesh_reconstruct_host), sfm_mesh_grid_fit and
sfm_mesh_write_ply against the numpy restatement of the contract
(_mesh_helpers.py): bytes and counts, the orientation rule on all 256 corner
configurations, closed manifolds with the right Euler characteristic, an open
mesh, the integration of exact plane depths, the argument checks."""
import os
import subprocess

import numpy as np
import pytest

import _mesh_helpers as MH

abi, api, F = MH.abi, MH.api, MH.F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_all_256_configurations_in_one_call():
    vol = MH.config_volume()
    ref, res = vol.ref(), vol.run(None)
    MH.check_mesh(res, ref)
    assert len(ref["cells"]) == 256 and ref["n_degenerate"] == 0
    # 254 configurations cross; every triangle looks from the inside to the outside
    dots = MH.rule_direction_dots(vol.grid, vol.tsdf, dict(V=res["V"], tri=res["tri"], cells=ref["cells"]))
    assert len(dots) == res["stats"]["n_triangles"] > 254 and (dots > 0).all()
    assert MH.referenced(res)
    # the colours: from the nearer end, or the other one where that end has none
    assert res["rgb"].shape == res["V"].shape and res["rgb"].any()


def test_case_table_is_the_rule():
    table = MH.case_table()
    assert [len(table[t][c]) for t in (0, 5) for c in (0, 1, 3, 7, 15)] == [0, 1, 2, 1, 0] * 2
    # opposite cases have the same triangles, mirrored
    for t in range(6):
        for c in range(16):
            assert sorted(map(sorted, table[t][c])) == sorted(map(sorted, table[t][15 - c]))


@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0)])
def test_closed_surfaces_are_closed_manifolds(name, euler):
    vol = dict(sphere=MH.sphere_volume, torus=MH.torus_volume)[name]()
    assert (vol.tsdf != 0).all()
    res = vol.run(None)
    MH.check_mesh(res, vol.ref())
    topo = MH.mesh_topology(res["tri"])
    assert len(topo["once"]) == 0 and len(topo["more"]) == 0 and len(topo["twice"]) > 0
    assert not topo["directed_repeats"]          # so each edge's two uses run in opposite directions
    assert topo["euler"] == euler and MH.referenced(res)
    assert MH.signed_volume(res["V"], res["tri"]) > 0
    assert res["stats"]["n_degenerate"] == 0


def test_a_slab_of_weight_0_opens_the_sphere():
    vol = MH.sphere_volume(True)
    res = vol.run(None, MH.mesh_opts(2))
    MH.check_mesh(res, vol.ref(2))
    topo = MH.mesh_topology(res["tri"])
    assert len(topo["once"]) > 0 and len(topo["more"]) == 0 and MH.referenced(res)
    # min_weight above every weight: nothing is observed
    none = vol.run(None, MH.mesh_opts(3))
    assert none["stats"]["n_vertices"] == 0 and none["stats"]["n_triangles"] == 0 and len(none["tri"]) == 0


def test_a_zero_sample_gives_counted_degenerate_triangles():
    g = MH.Grid((0.0, 0.0, 0.0), 1.0, (3, 3, 3))
    t = np.full((3, 3, 3), 0.5, F)
    t[1, 1, 1] = 0.0          # outside by the contract
    t[1, 1, 0] = t[1, 0, 0] = -0.5   # two inside corners that share a tetrahedron with it
    vol = MH.Volume(g, t)
    res = vol.run(None)
    MH.check_mesh(res, vol.ref())
    assert res["stats"]["n_degenerate"] > 0


@pytest.mark.parametrize("name,trunc", [("colour", 0.0), ("colour", 0.25), ("plain", 0.0), ("unloaded", 0.0)])
def test_integration_of_exact_plane_depths(name, trunc):
    sc, ref = MH.integration_scene(name), MH.integration_ref(name, trunc)
    res = sc.run(None, MH.tsdf_opts(trunc) if trunc else None)
    MH.check_volume(res, ref)
    g = sc.grid
    z = g.positions()[2].reshape(-1)
    tr = F(trunc) if trunc else F(3.0) * g.voxel
    # further than trunc behind the plane: never integrated; in front of it, inside the frusta: seen
    assert (res["weight"][z - F(sc.far) > tr] == 0).all() and res["stats"]["n_observed"] > g.n // 3
    assert (res["weight"] <= (2 if name == "unloaded" else 3)).all() and res["weight"].max() >= 2
    if name == "plain":
        assert res["rgb"] is None
    else:
        assert res["has_rgb"].any() and (res["rgb"][res["has_rgb"] == 0] == 0).all()
    # the zero crossing lies on the plane.  Every camera has R = I and C_z = 0, so z = h2 is the
    # lattice point's own z and sd = 4 - z exactly (the lattice's z planes are exact in float);
    # t = sd / trunc is one rounding, the sum of at most 3 equal terms and its division add at most 3 more,
    # so ta and tb carry at most 4 half-ulps each, ta - tb one more, u = ta / (ta - tb) one more: below
    # 12 half-ulps of relative error in u.  A vertex's z is za + u * (zb - za): the product is at most a
    # voxel, so u's error moves it by less than voxel * 6 * 2^-23, the product's own rounding by half an ulp
    # of a voxel and the final sum by half an ulp of the depth.
    mesh = api.mesh_extract(None, g.c(), res["tsdf"], res["weight"])
    assert mesh["stats"]["n_vertices"] > 0 and mesh["stats"]["n_degenerate"] == 0
    allow = float(g.voxel) * 6 * 2.0 ** -23 + 0.5 * float(np.spacing(g.voxel)) + 0.5 * float(np.spacing(F(sc.far + float(g.voxel))))
    worst = float(np.abs(mesh["V"][:, 2].astype(np.float64) - sc.far).max())
    print(f"{name} trunc {trunc}: worst |z - {sc.far}| = {worst:.3g}, allowance {allow:.3g}")
    assert worst <= allow


def test_reconstruct_host_equals_the_two_calls_chained():
    sc = MH.integration_scene("colour")
    vol = sc.run(None)
    mesh = api.mesh_extract(None, sc.grid.c(), vol["tsdf"], vol["weight"], vol["rgb"], vol["has_rgb"])
    one = api.mesh_reconstruct(None, *sc.args(), images=sc.sc.images, volume=True)
    MH.same_mesh(one, mesh)
    assert one["tsdf"].tobytes() == vol["tsdf"].tobytes() and one["weight"].tobytes() == vol["weight"].tobytes()
    assert one["stats"]["mesh"]["n_triangles"] == mesh["stats"]["n_triangles"] > 0
    assert one["stats"]["tsdf"]["n_observed"] == vol["stats"]["n_observed"]
    assert one["rgb"] is not None and one["rgb"].any()


def _raises(code, text, fn, *a, **k):
    with pytest.raises(api.SfmError) as ei:
        fn(*a, **k)
    assert ei.value.code == code and text in str(ei.value), str(ei.value)


def test_argument_checks():
    vol = MH.sphere_volume()
    g, t, w = vol.grid, vol.tsdf, vol.weight
    ex = lambda grid, **k: api.mesh_extract(None, grid, t, w, **k)
    _raises(abi.SFM_ERR_INVALID_ARG, "voxel", ex, api.mesh_grid(g.origin, 0.0, g.dims))
    _raises(abi.SFM_ERR_INVALID_ARG, "voxel", ex, api.mesh_grid(g.origin, -1.0, g.dims))
    _raises(abi.SFM_ERR_INVALID_ARG, "dims", ex, api.mesh_grid(g.origin, g.voxel, (17, 0, 13)))
    _raises(abi.SFM_ERR_INVALID_ARG, "cap", ex, g.c(), cap_vertices=-1, cap_triangles=10)
    _raises(abi.SFM_ERR_INVALID_ARG, "min_weight", ex, g.c(), opts=MH.mesh_opts(0))
    _raises(abi.SFM_ERR_UNSUPPORTED, "2^31", ex, api.mesh_grid(g.origin, g.voxel, (2048, 1024, 1024)))
    sc = MH.integration_scene("plain")
    _raises(abi.SFM_ERR_INVALID_ARG, "trunc", sc.run, None, MH.tsdf_opts(float("nan")))
    _raises(abi.SFM_ERR_INVALID_ARG, "trunc", sc.run, None, MH.tsdf_opts(-1.0))
    _raises(abi.SFM_ERR_UNSUPPORTED, "device_bytes", sc.run, None, MH.tsdf_opts(0.0, 1000))
    args = list(sc.args())
    args[5] = api.mesh_grid(sc.grid.origin, float("nan"), sc.grid.dims)
    _raises(abi.SFM_ERR_INVALID_ARG, "voxel", api.tsdf_integrate, None, *args)
    _raises(abi.SFM_ERR_INVALID_ARG, "min_weight", api.mesh_reconstruct, None, *sc.args(), mesh_opts=MH.mesh_opts(256))


def test_caps_too_small_write_nothing_and_report_the_needs():
    vol, ref = MH.sphere_volume(), MH.sphere_volume().ref()
    nv, nt = ref["n_vertices"], ref["n_triangles"]
    for cv, ct in ((nv - 1, nt), (nv, nt - 1), (0, 0)):
        rc, arrays, st = api.mesh_extract_raw(None, vol.grid.c(), vol.tsdf, vol.weight, cap_vertices=cv, cap_triangles=ct,
                                              fill=7)
        assert rc == abi.SFM_ERR_INVALID_ARG and (st["n_vertices"], st["n_triangles"]) == (nv, nt)
        assert "cap_vertices" in abi.load().sfm_last_error().decode()
        assert (arrays["V"] == 7).all() and (arrays["tri"] == 7).all() and (arrays["rgb"] == 7).all()
    rc, arrays, st2 = api.mesh_extract_raw(None, vol.grid.c(), vol.tsdf, vol.weight, cap_vertices=st["n_vertices"],
                                           cap_triangles=st["n_triangles"])
    assert rc == abi.SFM_OK
    MH.check_mesh(dict(V=arrays["V"].reshape(-1, 3), rgb=None, tri=arrays["tri"].reshape(-1, 3), stats=st2), ref)


def test_grid_fit_on_a_hand_made_cloud():
    X = np.array([[0, 0, 0], [4, 1, 0.5], [1, 2, 1], [3, 0.25, 0.75]], F)
    g = api.mesh_grid_fit(X, 8, 2)
    assert g.voxel == 0.5 and list(g.origin) == [-1.0, -1.0, -1.0] and list(g.dims) == [14, 10, 8]
    g = api.mesh_grid_fit(X + F(10), 4, 0)
    assert g.voxel == 1.0 and list(g.origin) == [10.0, 10.0, 10.0] and list(g.dims) == [6, 4, 3]
    # every point lies inside the lattice, the margin on either side
    hi = np.array(g.origin) + g.voxel * (np.array(g.dims) - 1)
    assert (X + 10 <= hi).all()
    _raises(abi.SFM_ERR_INVALID_ARG, "extent", api.mesh_grid_fit, X[:1], 8)
    _raises(abi.SFM_ERR_INVALID_ARG, "resolution", api.mesh_grid_fit, X, 0)
    _raises(abi.SFM_ERR_INVALID_ARG, "finite", api.mesh_grid_fit, np.array([[0, 0, np.inf], [1, 1, 1]], F), 8)
    _raises(abi.SFM_ERR_UNSUPPORTED, "limits", api.mesh_grid_fit, X, 4000)


def test_ply_reads_back(tmp_path):
    vol = MH.config_volume()
    res = vol.run(None)
    path = str(tmp_path / "mesh.ply")
    api.mesh_write_ply(path, res["V"], res["tri"], res["rgb"])
    lines, verts, faces = MH.read_mesh_ply(path)
    assert lines[2] == f"element vertex {len(res['V'])}" and "property uchar red" in lines
    assert np.stack([verts["x"], verts["y"], verts["z"]], -1).tobytes() == res["V"].tobytes()
    assert np.stack([verts["red"], verts["green"], verts["blue"]], -1).tobytes() == res["rgb"].tobytes()
    assert faces.astype(np.int32).tobytes() == res["tri"].tobytes()
    api.mesh_write_ply(path, res["V"], res["tri"])
    lines, verts, faces = MH.read_mesh_ply(path)
    assert "property uchar red" not in lines and len(faces) == len(res["tri"])
    bad = res["tri"].copy()
    bad[0, 0] = len(res["V"])
    _raises(abi.SFM_ERR_INVALID_ARG, "names vertex", api.mesh_write_ply, path, res["V"], bad)


def test_cpp_mesh_program(tmp_path):
    """the stand-alone host program (host twins and façade compiled in): the one a sanitizer build runs"""
    exe = os.path.join(ROOT, "tests", "cpp", "mesh_test")
    assert os.path.exists(exe), "run make (builds tests/cpp/mesh_test)"
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0 and "mesh ok" in r.stdout, r.stdout + r.stderr
