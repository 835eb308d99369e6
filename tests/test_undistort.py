"""CPU: the undistortion's host twin (sfm_undistort_host) against the numpy
restatement of the per-pixel contract (_undistort_helpers.py), byte for byte
and count for count; the argument checks; the PNM writer."""
import os
import subprocess

import numpy as np
import pytest

import _undistort_helpers as UH

abi, api = UH.abi, UH.api
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _raises(code, fn, *a, **kw):
    with pytest.raises(api.SfmError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert str(ei.value)


def _with(b, **kw):
    for k, v in kw.items():
        setattr(b, k, v)
    return b


@pytest.mark.parametrize("ch", [3, 1])
@pytest.mark.parametrize("name", ["strong", "barrel", "mixed_k", "tiny", "one_pixel"])
def test_host_twin_equals_the_restatement(name, ch):
    b = UH.case(name, ch)
    res = b.run(None)
    b.check(res)
    assert res["stats"]["n_chunks"] == 1 and res["stats"]["n_copied"] == 0


def test_strong_case_reaches_every_branch():
    """the 67 x 41, k1 = 0.8 input has pixels outside, pixels of low weight, and
    pixels sampled in the one-pixel strips left of column 0 and right of column w - 1"""
    b = UH.case("strong", 3)
    info, w = b.refs[0], 67
    assert info["n_outside"] > 0 and info["n_low_weight"] > 0
    filled = info["inside"] & ~info["low"]
    assert (filled & (info["x"] < 0)).any() and (filled & (info["x"] > w - 1)).any()
    st = b.run(None)["stats"]
    assert st["n_outside"] == info["n_outside"] > 0 and st["n_low_weight"] == info["n_low_weight"] > 0


@pytest.mark.parametrize("ch", [3, 1])
def test_zero_distortion_is_the_identity(ch):
    b = UH.case("identity", ch)
    res = b.run(None)
    b.check(res)
    assert res["images"][0].tobytes() == b.images[0].tobytes()
    assert res["stats"]["n_outside"] == res["stats"]["n_low_weight"] == 0


def test_pinhole_is_a_byte_copy_and_snavely_unsupported():
    rng = np.random.default_rng(8)
    images = [UH.random_image(rng, 13, 9, 3), None, UH.random_image(rng, 6, 11, 1)]
    sizes = [13, 9, 4, 4, 6, 11]
    b = UH.Batch(images, sizes, [0, 0, 0], [50.0, 50.0, 6.0, 4.0], gaps=[1, 0, 3, 2], model=UH.PINHOLE)
    res = b.run(None)
    b.check(res)
    assert res["stats"]["n_copied"] == 2 and res["stats"]["n_pixels"] == 0 and res["stats"]["n_chunks"] == 0
    s = UH.Batch(images, sizes, [0, 0, 0], [50.0, 0.0, 0.0, 0.0], model=UH.PINHOLE)
    s.model = UH.SNAVELY
    _raises(abi.SFM_ERR_UNSUPPORTED, s.run, None)


def test_mixed_batch_in_one_call():
    b = UH.mixed_batch()
    res = b.run(None)
    b.check(res)                      # (the sentinels between and after the images included)
    assert res["images"][2] is None and res["stats"]["n_images"] == 4
    assert (b.want == UH.UNTOUCHED).sum() >= 3 + 5 + 7 + 1 + 9


def test_fill_colour():
    b = UH.mixed_batch(fill=(200, 17, 96))
    b.check(b.run(None))
    info = b.refs[0]
    got = b.run(None)["images"][0]
    assert (got[~info["inside"]] == np.array([200, 17, 96], np.uint8)).all()
    assert (got[info["low"]] == 0).all() and info["low"].any()          # T(), not the fill
    gray = b.run(None)["images"][3]
    assert (gray[~b.refs[3]["inside"]] == 200).all()


def test_chunk_plan_is_reported_and_checked():
    """the host twin reports the plan the device would run, with the same checks"""
    rng = np.random.default_rng(9)
    images = [UH.random_image(rng, 64, 48, c) for c in (3, 1, 3)]
    b = UH.Batch(images, [64, 48] * 3, [0, 0, 0], [70.0, 31.5, 23.5, 0.2, 0.0, 0.0])
    assert b.run(None)["stats"]["n_chunks"] == 1
    split = b.run(None, chunk_bytes=20000)       # an RGB image is 2 * 48 * 192 = 18432 pitched bytes
    b.check(split)
    assert split["stats"]["n_chunks"] == 3
    rows = b.run(None, chunk_bytes=6000)         # no image fits: bands of rows
    b.check(rows)
    assert rows["stats"]["n_chunks"] > 3
    _raises(abi.SFM_ERR_INVALID_ARG, b.run, None, chunk_bytes=100)
    _raises(abi.SFM_ERR_INVALID_ARG, b.run, None, chunk_bytes=-1)


def test_argument_checks():
    img = UH.random_image(np.random.default_rng(10), 8, 6, 3)
    k = [10.0, 4.0, 3.0, 0.1, 0.0, 0.0]
    ok = lambda **kw: UH.Batch([img], kw.get("sizes", [8, 6]), kw.get("img_intr", [0]), kw.get("intr", k))
    ok().check(ok().run(None))
    bad = abi.SFM_ERR_INVALID_ARG
    for sizes in ([0, 6], [8, -1]):
        _raises(bad, _with(ok(), wh=np.array(sizes, np.int32)).run, None)
    for ch in (2, 4, 0):
        b = ok()
        b.pool = (np.array([ch], np.int32), b.pool[1], b.pool[2])
        _raises(bad, b.run, None)
    for ii in (-1, 1):
        _raises(bad, _with(ok(), img_intr=np.array([ii], np.int32)).run, None)
    _raises(bad, _with(ok(), model=7).run, None)
    for at, v in ((0, np.nan), (3, np.inf), (5, -np.inf), (0, 0.0)):
        kk = list(k)
        kk[at] = v
        _raises(bad, _with(ok(), intr=np.array(kk)).run, None)
    # a block that no loaded image uses is not read; an unloaded image's channels neither
    two = UH.Batch([img, None], [8, 6, 8, 6], [0, 1], k + [np.nan] * 6)
    two.pool = (np.array([3, 9], np.int32), two.pool[1], two.pool[2])
    two.check(two.run(None))
    # nothing to do
    none = UH.Batch([None], [8, 6], [0], k)
    st = none.run(None)["stats"]
    assert st["n_images"] == st["n_pixels"] == st["n_chunks"] == 0
    empty = api.undistort_host(UH.RADIAL3, [], [], [], images=[])
    assert empty["stats"]["n_images"] == 0


def test_default_options():
    o = api.undistort_default_options()
    assert o.chunk_bytes == 0 and list(o.fill) == [0, 0, 0]


@pytest.mark.parametrize("ch", [1, 3])
def test_write_pnm_round_trip(tmp_path, ch):
    im = UH.random_image(np.random.default_rng(11), 7, 5, ch)
    path = tmp_path / ("a.pgm" if ch == 1 else "a.ppm")
    api.write_pnm(path, im)
    raw = path.read_bytes()
    head = b"P%d\n7 5\n255\n" % (5 if ch == 1 else 6)
    assert raw[:len(head)] == head and raw[len(head):] == im.tobytes()
    _raises(abi.SFM_ERR_INVALID_ARG, api.write_pnm, tmp_path / "no" / "dir.pgm", im)
    _raises(abi.SFM_ERR_INVALID_ARG, api.write_pnm, path, np.zeros((2, 2, 2), np.uint8))


def test_cpp_undistort_program(tmp_path):
    """the stand-alone host program (host twin, scene and façade compiled in): the one a sanitizer build runs"""
    exe = os.path.join(ROOT, "tests", "cpp", "undistort_test")
    assert os.path.exists(exe), "run make (builds tests/cpp/undistort_test)"
    r = subprocess.run([exe], capture_output=True, text=True, cwd=tmp_path)      # (it writes two small PNMs where it runs)
    assert r.returncode == 0 and "undistort ok" in r.stdout, r.stdout + r.stderr
