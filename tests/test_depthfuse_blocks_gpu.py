"""Depth-map fusion on the device, one image a call: rasters of 1, 64, 65, 256,
257 and 513 pixels, that is one, two and three blocks with a partial last one,
so the scan (csrc/dense_scan.h) sees one array of 1, 2 and 3 counts and every
rank is a block base + a rank inside the block; and one of 66 000 pixels, 258
blocks, which takes the scan into its second step.  Bytes against the host twin and
the numpy restatement (_fuse_helpers.py), as test_depthfuse_gpu.py does for
calls of several images."""
import numpy as np
import pytest

import _depthmap_helpers as DH
import _fuse_helpers as FH

api = DH.api
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


# the last case is 258 blocks: the scan takes 256 counts a step, so a second step of two counts on top of a carry
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (13, 5), (16, 16), (257, 1), (27, 19), (300, 220)])
def test_one_image_block_bases(ctx, w, h):
    n = w * h
    assert n in (1, 64, 65, 256, 257, 513, 66000)
    sc = FH.Scene([DH.Fixture(w, h, [(0, 0, 0)], far=4.0, seed=31 + n, neighbours=[[]])])
    keep = np.unique(np.r_[np.arange(0, n, 3), n - 1])   # every third pixel and the last: ranks differ from indices
    sc.keep_only(0, keep)
    ref = sc.ref()
    FH.check_against_ref(sc.run(None), ref)
    FH.check_against_ref(sc.run(ctx), ref)
    assert ref["n_points"] == len(keep) and ref["n_suppressed"] == 0
    assert np.array_equal(ref["src_pixel"], keep) and (ref["src_image"] == 0).all()
