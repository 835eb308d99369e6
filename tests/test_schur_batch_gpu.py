"""GPU parity of the 64-row Schur kernel's wave batches (csrc/ba_schur.hip:
6 points / 60 observations per batch for the pinhole model) against the CPU
oracle, on small scenes cut so that the batch walk meets its boundaries:

- tracks of exactly 10 (6 full points per batch), in chunks of 16, 13, 1, ...
  points: a chunk of one point, chunks that are no multiple of 6
- tracks of 11 (6 x 11 passes the cap: batches of 5), every point seeing the
  constant camera (`crow < 0` inside the window)
- mixed track lengths 2..11 in one chunk, and 2..10 over sliding windows
- two intrinsics blocks in one chunk (the run-boundary sums of phase C2)
- a solve that rejects steps (the first pass forms the point scales, later
  passes and relinearisations reuse them)
- a point of exactly the cap (60) and of one above it (61): both leave the
  chunk path and the rest still solves on 64-row tiles

What a 64-row chunk can hold bounds the tracks that reach the kernel: a tile
row block per optimised camera (6 rows) plus the intrinsics block, so at most
10 optimised cameras, and a chunk stages at most 14 cameras (kCamSlots), so
no track above 14 and never a cap-sized one.  A problem of the C ABI has one
constant image (sfm_ba_problem.const_img), so the scenes here reach tracks of
11; tracks of 12 to 14 would need further constant images, which these
scenes cannot state.  The batch rule itself is walked for every track length
up to the cap + 1 on the host (tests/test_schur_batch.py).  Every scene
asserts through the plan that it ran on 64-row chunk tiles."""
import importlib

import numpy as np
import pytest

import _helpers as H

pytestmark = pytest.mark.gpu
abi = H.abi
api = importlib.import_module("3dreconstruction_amd.api")

RTOL_COST = 1e-6
# points taken per visibility window (24 cameras, 10 views: 15 windows); the
# planner cuts a window's points into chunks of at most 16
COUNTS = [32, 33, 17, 32, 16, 38, 32, 1, 32, 29, 32, 16, 32, 45, 32]


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _pick(sc, pts, lens):
    """sc reduced to its points `pts`, each cut to its first lens[j] observations"""
    obs, off = [], [0]
    for p, n in zip(pts, lens):
        a = int(sc.pt_offsets[p])
        assert a + n <= sc.pt_offsets[p + 1]
        obs.extend(range(a, a + int(n)))
        off.append(off[-1] + int(n))
    obs, pts = np.array(obs), np.array(pts)
    sc.obs_img = np.ascontiguousarray(sc.obs_img[obs])
    sc.obs_uv = np.ascontiguousarray(sc.obs_uv.reshape(-1, 2)[obs].reshape(-1))
    sc.pt_offsets = np.array(off, np.int64)
    for name in ("X", "gt_X"):
        setattr(sc, name, np.ascontiguousarray(getattr(sc, name).reshape(-1, 3)[pts].reshape(-1)))
    sc.n_pt, sc.n_obs = len(pts), len(obs)
    return sc


def _windows(n_base, counts):
    """base point indices: counts[w] points of window w (n_base / len(counts) points each)"""
    per = n_base // len(counts)
    return [w * per + j for w, c in enumerate(counts) for j in range(c)]


def _compare(ctx, sc, opts=None, n_general=0, check_trace=True):
    """GPU solve against the oracle (as tests/test_ba_gpu.py), on 64-row chunk tiles"""
    sh = api.ba_describe(sc.problem())
    assert sh.tile_rows == 64 and sh.n_general_pts == n_general and sh.n_chunk_pts == sc.n_pt - n_general, \
        (sh.tile_rows, sh.n_chunk_pts, sh.n_general_pts)
    orc_rc, os_, _, (oe, oi, ox) = H.oracle_solve(sc, opts, threads=8)
    e, i, x = sc.params()
    plan = api.BAPlan(ctx, sc.problem(), e, i, x)
    assert plan.info().tile_rows == 64 and plan.info().n_chunks == sh.n_chunks
    rc, gs = plan.run(opts)
    e, i, x = plan.download()
    plan.close()
    assert rc == orc_rc == 0, (rc, api.abi.load().sfm_last_error())
    assert gs.termination == os_.termination and gs.usable == os_.usable == 1
    assert abs(gs.initial_cost / os_.initial_cost - 1) < 1e-12
    print(f"final cost gpu {gs.final_cost!r} oracle {os_.final_cost!r}; steps gpu "
          f"{gs.successful_steps}+{gs.unsuccessful_steps} oracle {os_.successful_steps}+{os_.unsuccessful_steps}")
    assert abs(gs.final_cost / os_.final_cost - 1) < RTOL_COST, (gs.final_cost, os_.final_cost)
    assert abs(gs.rmse_final / os_.rmse_final - 1) < RTOL_COST
    if check_trace:
        assert (gs.iterations, gs.successful_steps, gs.unsuccessful_steps) == \
               (os_.iterations, os_.successful_steps, os_.unsuccessful_steps)
    c = H.oracle_cost(sc, e, i, x)   # the written-back parameters carry the reported cost
    assert abs(c / gs.final_cost - 1) < 1e-9, (c, gs.final_cost)
    return gs, sh


def test_tracks_of_10_full_batches_and_chunk_lengths(ctx):
    pts = _windows(1500, COUNTS)
    sc = _pick(H.Scene(24, 1500, 10, seed=41), pts, [10] * len(pts))
    # a chunk of one point: the one point of window 7 shares a 64-row tile with
    # no other point (with any, the optimised cameras need more than 64 rows),
    # and _compare asserts that every point is a chunk point on 64-row tiles
    lone = sum(COUNTS[:7])
    cams = [set(sc.obs_img[sc.pt_offsets[p]:sc.pt_offsets[p + 1]]) for p in range(sc.n_pt)]
    assert COUNTS[7] == 1 and all(6 * len((cams[lone] | cams[p]) - {sc.const_img}) + 4 > 64
                                  for p in range(sc.n_pt) if p != lone)
    _, sh = _compare(ctx, sc)
    assert sh.n_chunks >= sum((c + 15) // 16 for c in COUNTS) - 2


def test_tracks_of_11_batches_of_5_with_constant_camera(ctx):
    sc = _pick(H.Scene(11, 300, 11, seed=42), range(300), [11] * 300)
    assert sc.const_img == 1 and np.all(sc.obs_img.reshape(-1, 11) == np.arange(11))
    _compare(ctx, sc)


def test_mixed_tracks_2_to_11_in_one_chunk(ctx):
    rng = np.random.default_rng(5)
    lens = rng.integers(2, 12, 300)
    assert set(lens) == set(range(2, 12))
    _compare(ctx, _pick(H.Scene(11, 300, 11, seed=43), range(300), lens))


def test_mixed_tracks_2_to_10_sliding_windows(ctx):
    rng = np.random.default_rng(6)
    pts = _windows(1500, COUNTS)
    lens = rng.integers(2, 11, len(pts))
    lens[::7] = 10   # full tracks keep the windows' far cameras tied in
    _compare(ctx, _pick(H.Scene(24, 1500, 10, seed=44), pts, lens))


def test_two_intrinsics_blocks_in_one_chunk(ctx):
    # 9 optimised cameras + 2 intrinsics blocks = 62 rows; images alternate between the blocks
    pts = _windows(1600, COUNTS + [8])
    sc = _pick(H.Scene(24, 1600, 9, n_intr=2, seed=45), pts, [9] * len(pts))
    assert set(sc.img_intr[:2]) == {0, 1}
    _compare(ctx, sc)


def test_rejected_steps(ctx):
    # large perturbations, 10 % outliers and a wide first trust region: the
    # oracle rejects 6 of 21 steps
    pts = _windows(1500, COUNTS)
    sc = _pick(H.Scene(24, 1500, 10, seed=48, perturb=(0.5, 2.0, 2.0, 200.0), outliers=0.1), pts, [10] * len(pts))
    opts = abi.default_options()
    opts.initial_trust_region_radius = 1e8
    gs, _ = _compare(ctx, sc, opts)
    assert gs.unsuccessful_steps > 0 and gs.successful_steps > 1


@pytest.mark.parametrize("track", [60, 61])
def test_track_at_and_above_the_cap_leaves_the_chunk_path(ctx, track):
    # 61 views per base point; one point keeps `track` of them, the rest 8
    sc = _pick(H.Scene(64, 200, 61, seed=46), range(200), [track] + [8] * 199)
    _compare(ctx, sc, n_general=1)
