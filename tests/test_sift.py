"""CPU: SIFT extraction on the host (sfm_sift_host) against the reference's own
features and descriptors (tests/golden, written by the reference's VLFeat on
the images sfm_synth_image rebuilds), its properties, the capacity
convention, the feature file round trip and the C++ façade."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _helpers as H
import _sift_helpers as S

abi, api = S.abi, S.api


@pytest.mark.parametrize("name", list(S.CASES))
def test_host_against_reference(name):
    (xyso, desc), n = S.host(name)
    S.against_golden(name, xyso, desc, n)


def test_constant_image_has_no_features():
    out, n, sm = api.sift(None, np.full((2, 48, 64), 131, np.uint8))
    assert n.tolist() == [0, 0] and sm["n_keypoints"] == 0 and len(out[0][0]) == 0


def test_lower_peak_threshold_finds_a_superset_count():
    o = api.sift_default_options()
    o.peak_threshold = 0.01   # the HIGH preset
    _, n, _ = api.sift(None, S.image("vlfeat_sift_160x120"), o)
    assert n[0] > S.host("vlfeat_sift_160x120")[1]


def test_capacity_overflow_reports_the_true_count():
    """at most cap rows, in canonical order; n_feat stays the true count; SFM_OK"""
    (xyso, desc), n = S.host("vlfeat_sift_160x120")
    out, nf, sm = api.sift(None, S.image("vlfeat_sift_160x120"), cap_per_img=10)
    assert nf[0] == n == 40 and sm["n_overflow"] == 1 and sm["n_written"] == 10 and sm["n_features"] == 40
    assert out[0][0].tobytes() == xyso[:10].tobytes()
    np.testing.assert_array_equal(out[0][1], desc[:10])
    _, nf0, _ = api.sift(None, S.image("vlfeat_sift_160x120"), cap_per_img=0)   # the size query
    assert nf0[0] == 40


def test_unsupported_and_bad_arguments():
    g = S.image("vlfeat_sift_96x64")
    for field, value, code in (("first_octave", -1, abi.SFM_ERR_UNSUPPORTED), ("first_octave", 1, abi.SFM_ERR_UNSUPPORTED),
                               ("n_scales", 9, abi.SFM_ERR_UNSUPPORTED), ("n_scales", 0, abi.SFM_ERR_INVALID_ARG),
                               ("n_octaves", -1, abi.SFM_ERR_INVALID_ARG), ("edge_threshold", 0.0, abi.SFM_ERR_INVALID_ARG),
                               ("peak_threshold", -1.0, abi.SFM_ERR_INVALID_ARG)):
        o = api.sift_default_options()
        setattr(o, field, value)
        with pytest.raises(api.SfmError) as ei:
            api.sift(None, g, o)
        assert ei.value.code == code, field
    lib = abi.load()
    nf = np.zeros(1, np.int64)
    assert lib.sfm_sift_host(None, 1, 96, 64, None, 0, None, None, abi.ptr(nf, abi.i64p), None) == abi.SFM_ERR_INVALID_ARG
    assert lib.sfm_sift_host(abi.ptr(g, abi.u8p), 1, 0, 64, None, 0, None, None, abi.ptr(nf, abi.i64p),
                             None) == abi.SFM_ERR_INVALID_ARG
    assert lib.sfm_sift_host(abi.ptr(g, abi.u8p), 1, 96, 64, None, 5, None, None, abi.ptr(nf, abi.i64p),
                             None) == abi.SFM_ERR_INVALID_ARG
    assert lib.sfm_sift(None, abi.ptr(g, abi.u8p), 1, 96, 64, None, 0, None, None, abi.ptr(nf, abi.i64p),
                        None) == abi.SFM_ERR_INVALID_ARG   # null context, before any device call


def test_empty_batch_and_tiny_images():
    out, n, sm = api.sift(None, np.zeros((0, 8, 8), np.uint8))
    assert out == [] and len(n) == 0 and sm["n_images"] == 0
    for h, w in ((1, 1), (2, 9), (3, 3), (5, 4)):   # below an octave's 3 x 3, and just at it
        _, n, _ = api.sift(None, np.arange(h * w, dtype=np.uint8).reshape(1, h, w) * 37)
        assert n.tolist() == [0]


def test_image_in_a_batch_equals_the_image_alone():
    names = ["vlfeat_sift_160x120"]
    a = S.seed_image(160, 120, 11)
    b = S.seed_image(160, 120, 12)
    batch = np.stack([a, S.image(names[0]), b])
    out, n, _ = api.sift(None, batch)
    (xyso, desc), cnt = S.host(names[0])
    assert n[1] == cnt and out[1][0].tobytes() == xyso.tobytes()
    np.testing.assert_array_equal(out[1][1], desc)
    assert n[0] > 0 and n[2] > 0 and out[0][0].tobytes() != out[2][0].tobytes()


def test_upright_features_keep_the_keypoints():
    o = api.sift_default_options()
    o.orientation = 0
    out, n, sm = api.sift(None, S.image("vlfeat_sift_160x120"), o)
    assert n[0] == sm["n_keypoints"] and (out[0][0][:, 3] == 0).all()


def test_feat_file_round_trip(tmp_path):
    (xyso, _), n = S.host("vlfeat_sift_160x120")
    p = str(tmp_path / "a.feat")
    api.mvg_write_feat(p, xyso)
    back = api.mvg_read_feat(p)
    assert back.shape == (n, 4) and back.tobytes() == xyso.tobytes()
    api.mvg_write_feat(p, np.zeros((0, 4), np.float32))
    assert len(api.mvg_read_feat(p)) == 0
    assert abi.load().sfm_mvg_write_feat(None, None, 0) == abi.SFM_ERR_INVALID_ARG


def test_synth_image_is_deterministic_and_views_differ():
    a = api.synth_image(96, 64, 7)
    np.testing.assert_array_equal(a, S.image("vlfeat_sift_96x64"))
    assert a.std() > 10 and (api.synth_image(96, 64, 7, 0.2, 3.0, -2.0, 1.1) != a).any()
    assert abi.load().sfm_synth_image(0, 4, 1, 0.0, 0.0, 0.0, 1.0, None) == abi.SFM_ERR_INVALID_ARG


def test_cpp_sift_facade(tmp_path):
    """sfm::HostSIFT_Image_describer and detectFeature(): the C++ program's own
    checks, then its files through the Python readers the matcher tests use"""
    exe = os.path.join(H.ROOT, "tests", "cpp", "sift_test")
    assert os.path.exists(exe), "run make (builds tests/cpp/sift_test)"
    out = subprocess.run([exe, S.GOLDEN, str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sift_test ok" in out.stdout
    assert abi.load().sfm_mvg_check_describer(str(tmp_path / "image_describer.json").encode()) == abi.SFM_OK
    (xyso, desc), n = S.host("vlfeat_sift_160x120")
    assert api.mvg_read_feat(str(tmp_path / "a.feat")).tobytes() == xyso.tobytes()
    np.testing.assert_array_equal(api.mvg_read_desc(str(tmp_path / "c.desc")), desc)
    assert len(api.mvg_read_desc(str(tmp_path / "b.desc"))) == 14
