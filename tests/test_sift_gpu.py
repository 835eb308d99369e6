"""GPU: SIFT extraction (sfm_sift) against its host twin bit for bit, against
the reference's goldens within the CPU test's bounds, downstream through the
matcher, and the constant image, overflow and batch independence on the
device."""
import json
import os

import numpy as np
import pytest

import _sift_helpers as S

abi, api = S.abi, S.api
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def views(ctx):
    """the three 640 x 480 views in one batch, on the device (computed once)"""
    return api.sift(ctx, np.stack([S.image(v) for v in S.VIEWS]))


def test_views_batch_equals_host(views):
    out, n, sm = views
    for k, v in enumerate(S.VIEWS):
        (xyso, desc), cnt = S.host(v)
        assert n[k] == cnt
        assert out[k][0].tobytes() == xyso.tobytes()
        np.testing.assert_array_equal(out[k][1], desc)
    assert sm["n_features"] == int(n.sum()) and sm["n_overflow"] == 0


@pytest.mark.parametrize("name", S.SMALL)
def test_small_sizes_equal_host(ctx, name):
    """160 x 120, 96 x 64 and the odd 161 x 97 (odd sides halve by dropping the last row / column)"""
    out, n, _ = api.sift(ctx, S.image(name))
    (xyso, desc), cnt = S.host(name)
    assert n[0] == cnt and out[0][0].tobytes() == xyso.tobytes()
    np.testing.assert_array_equal(out[0][1], desc)


def test_batch_of_seeds_equals_host_and_is_independent(ctx):
    batch = np.stack([S.seed_image(160, 120, s) for s in (21, 22, 23, 24, 25)])
    dev = api.sift(ctx, batch)
    S.same(dev, api.sift(None, batch))
    S.same(dev, api.sift(ctx, batch))   # run against run
    alone = api.sift(ctx, batch[3])
    assert alone[1][0] == dev[1][3] and alone[0][0][0].tobytes() == dev[0][3][0].tobytes()
    np.testing.assert_array_equal(alone[0][0][1], dev[0][3][1])


def test_device_against_reference(ctx, views):
    out, n, _ = views
    for k, v in enumerate(S.VIEWS):
        S.against_golden(v, out[k][0], out[k][1], int(n[k]))
    for name in S.SMALL:
        o, m, _ = api.sift(ctx, S.image(name))
        S.against_golden(name, o[0][0], o[0][1], int(m[0]))


def test_matches_downstream(ctx, views):
    """sfm_match_dense on the device's descriptors of views 0-1 and 0-2 gives
    the golden match lists wherever the descriptors equal the golden ones"""
    out, _, _ = views
    exp = json.load(open(os.path.join(S.GOLDEN, "vlfeat_matches.json")))
    for j in (1, 2):
        equal = all(np.array_equal(out[k][1], S.golden(S.VIEWS[k])[1]) for k in (0, j))
        for mode in (0, 1):
            e = exp["pairs"][f"0-{j}-{mode}"]
            gi, gd = api.match_dense(ctx, out[0][1], out[j][1], mode)
            differ = int((np.asarray(gi) != np.asarray(e["idx"])).sum())
            print(f"views 0-{j} mode {mode}: {differ} matches differ (descriptors equal the golden ones: {equal})")
            if equal:
                np.testing.assert_array_equal(gi, e["idx"])
                np.testing.assert_array_equal(gd, e["d2"])


def test_constant_overflow_and_empty(ctx):
    out, n, sm = api.sift(ctx, np.full((2, 48, 64), 90, np.uint8))
    assert n.tolist() == [0, 0] and sm["n_keypoints"] == 0
    (xyso, desc), cnt = S.host("vlfeat_sift_160x120")
    out, nf, sm = api.sift(ctx, S.image("vlfeat_sift_160x120"), cap_per_img=10)
    assert nf[0] == cnt and sm["n_overflow"] == 1 and sm["n_written"] == 10
    assert out[0][0].tobytes() == xyso[:10].tobytes()
    np.testing.assert_array_equal(out[0][1], desc[:10])
    _, nf0, _ = api.sift(ctx, S.image("vlfeat_sift_160x120"), cap_per_img=0)
    assert nf0[0] == cnt
    out, n, _ = api.sift(ctx, np.zeros((0, 8, 8), np.uint8))
    assert out == [] and len(n) == 0
    _, n, _ = api.sift(ctx, np.zeros((1, 2, 9), np.uint8))
    assert n.tolist() == [0]
    o = api.sift_default_options()
    o.first_octave = -1
    with pytest.raises(api.SfmError) as ei:
        api.sift(ctx, S.image("vlfeat_sift_96x64"), o)
    assert ei.value.code == abi.SFM_ERR_UNSUPPORTED


def test_high_preset_and_upright_equal_host(ctx):
    o = api.sift_default_options()
    o.peak_threshold = 0.01
    o.orientation = 0
    g = S.image("vlfeat_sift_161x97")
    S.same(api.sift(ctx, g, o), api.sift(None, g, o))


def test_kernel_time_is_reported():
    c = api.Context(0, flags=abi.SFM_CTX_TIME_KERNELS)
    try:
        _, _, sm = api.sift(c, S.image("vlfeat_sift_96x64"))
        assert sm["kernel_ms"] > 0
    finally:
        c.close()
