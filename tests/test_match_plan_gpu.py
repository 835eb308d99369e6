"""GPU tests of the match plan's launch batches and of plan reuse (the kernels'
parity with the oracle is test_match_gpu.py's)."""
import importlib

import numpy as np
import pytest

import _helpers as H
from test_match_gpu import _rootsift_f32, ctx  # noqa: F401  (ctx: the module-scoped context fixture)

pytestmark = pytest.mark.gpu
abi = H.abi
api = importlib.import_module("3dreconstruction_amd.api")


# The mutual pass and the digest put the pair on grid.y / grid.x and so run in
# batches of 65535 pairs.  A tiny collection under a pair list of 65539 pairs
# runs a second batch of both; what the batches must get right is the offset
# into the pair list and the outputs, and the global pair index of the digest.

_LONG = 65539
_SIZES = [5, 0, 4]
_OFF = np.concatenate([[0], np.cumsum(_SIZES)]).astype(np.int64)
_BATCH = 65535      # pairs per mutual / digest launch
# the exhaustive pairs of three images, in both orientations; (0, 2) first, so
# that the second batch (pairs 65535 .. 65538 = 3, 4, 5, 0 of this list) holds
# the one pair whose mutual pass has something to remove (row 4 of image 0)
_SHORT = np.array([[0, 2], [0, 1], [1, 2], [2, 1], [2, 0], [1, 0]], np.int32)
_LAUNCHES = {abi.SFM_MATCH_RATIO: (1, 1),     # (short list, long list): one nearest-neighbour launch
             abi.SFM_MATCH_MUTUAL: (3, 4)}    # two nearest-neighbour passes + one / two mutual batches


def _tiny_collection(kind):
    """Images of 5, 0 and 4 rows; the last repeats rows of the first up to
    small noise, so real matches survive the ratio test."""
    rng = np.random.default_rng(2024)
    if kind == "u8":
        a = rng.integers(4, 250, size=(5, 128)).astype(np.int32)
        c = a[:4] + rng.integers(-2, 3, size=(4, 128))
        return np.concatenate([a, c]).astype(np.uint8)
    a = _rootsift_f32(rng, 5)
    c = a[:4] + rng.uniform(0.05, 0.3, size=(4, 128)).astype(np.float32)
    desc = np.concatenate([a, c])
    assert (desc != np.round(desc)).any()          # stays on the f32 kernel
    return desc


def _long_pairs():
    return np.tile(_SHORT, (-(-_LONG // len(_SHORT)), 1))[:_LONG]


def _tiled(counts, v):
    """Per-match array v of the short list -> that of the long (tiled) list."""
    reps, rem = divmod(_LONG, len(counts))
    return np.concatenate([np.tile(v, reps), v[:int(counts[:rem].sum())]])


_short_cache = {}


def _short_run(ctx, kind, mode):
    """(total, counts, i, j, d, digest) of a fresh plan over the short list."""
    if (kind, mode) not in _short_cache:
        plan = api.MatchPlan(ctx, _tiny_collection(kind), _OFF)
        total = plan.run(_SHORT, mode)
        assert plan.last_ms()[1] == _LAUNCHES[mode][0]
        r = (total,) + plan.fetch() + (plan.digest(),)
        plan.close()
        for a in r[1:5]:
            a.setflags(write=False)
        _short_cache[(kind, mode)] = r
    return _short_cache[(kind, mode)]


@pytest.mark.parametrize("mode", [abi.SFM_MATCH_RATIO, abi.SFM_MATCH_MUTUAL])
@pytest.mark.parametrize("kind", ["u8", "f32"])
def test_plan_second_launch_batch(ctx, kind, mode):
    total_s, cs, is_, js, ds, _ = _short_run(ctx, kind, mode)
    assert total_s == cs.sum()
    nonempty = [k for k, (I, J) in enumerate(_SHORT) if _SIZES[I] and _SIZES[J]]
    assert cs[nonempty].max() > 0 and cs.sum() == cs[nonempty].sum()
    # the second batch holds matches (the digest's pair index counts there) ...
    tail = sorted({k % len(_SHORT) for k in range(_BATCH, _LONG)})
    assert cs[tail].max() > 0
    if mode == abi.SFM_MATCH_MUTUAL:
        # ... and a pair where the mutual pass removed a row of I: without it every
        # row of I keeps its nearest neighbour in a non-empty J
        assert any(_SIZES[_SHORT[k][1]] > 0 and cs[k] < _SIZES[_SHORT[k][0]] for k in tail)
    plan = api.MatchPlan(ctx, _tiny_collection(kind), _OFF)
    total = plan.run(_long_pairs(), mode)
    assert plan.last_ms()[1] == _LAUNCHES[mode][1]
    counts, i, j, d = plan.fetch()
    assert d.dtype == (np.int32 if kind == "u8" else np.float32)
    np.testing.assert_array_equal(counts, np.tile(cs, -(-_LONG // len(cs)))[:_LONG])
    np.testing.assert_array_equal(i, _tiled(cs, is_))
    np.testing.assert_array_equal(j, _tiled(cs, js))
    np.testing.assert_array_equal(d.view(np.uint32), _tiled(cs, ds).view(np.uint32))
    assert total == counts.sum()
    if kind == "u8":
        assert plan.digest() == api.match_digest(counts, i, j, d)
    plan.close()


@pytest.mark.parametrize("first", [abi.SFM_MATCH_RATIO, abi.SFM_MATCH_MUTUAL])
def test_plan_reuse_after_longer_run(ctx, first):
    # the output buffers only grow: after a short run nothing of the long one shows
    second = abi.SFM_MATCH_MUTUAL if first == abi.SFM_MATCH_RATIO else abi.SFM_MATCH_RATIO
    total_s, cs, is_, js, ds, dg = _short_run(ctx, "u8", second)
    plan = api.MatchPlan(ctx, _tiny_collection("u8"), _OFF)
    plan.run(_long_pairs(), first)
    assert plan.run(_SHORT, second) == total_s
    assert plan.last_ms()[1] == _LAUNCHES[second][0]
    counts, i, j, d = plan.fetch()
    np.testing.assert_array_equal(counts, cs)
    np.testing.assert_array_equal(i, is_)
    np.testing.assert_array_equal(j, js)
    np.testing.assert_array_equal(d, ds)
    assert plan.digest() == dg == api.match_digest(counts, i, j, d)
    plan.close()
