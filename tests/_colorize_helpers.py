"""Reference for the track colouring tests (test_colorize.py,
test_colorize_gpu.py): a small seeded scene maker (tracks, masks, random 1- and
3-channel images of different sizes) and an independent restatement of the
semantics in include/sfmcore.h ("Track colouring"), written the slow way: every
round recounts every remaining point, with dicts keyed by image.  The library
keeps its counts incrementally; a mistake in a decrement shows here as a
different order.  Everything is integral: the comparisons are exact."""
import numpy as np

import _recon_helpers as RH

abi, api = RH.abi, RH.api


# ---- the restatement ------------------------------------------------------------------
def assign_ref(t, wh, pt_ok=None, keep_obs=None):
    """dict(view, obs, px, order (padded with -1 to n_img), n_rounds, n_to_colour)"""
    wh = np.asarray(wh).reshape(-1, 2)
    ok = np.ones(t.n_pt, bool) if pt_ok is None else np.asarray(pt_ok, bool)
    live = np.ones(t.n_obs, bool) if keep_obs is None else np.asarray(keep_obs, bool)
    seen = []                                   # per point: image -> its first live observation there
    for p in range(t.n_pt):
        d = {}
        if ok[p]:
            for o in range(int(t.pt_offsets[p]), int(t.pt_offsets[p + 1])):
                if live[o]:
                    d.setdefault(int(t.obs_img[o]), o)
        seen.append(d)
    left = [p for p in range(t.n_pt) if seen[p]]
    n_to_colour = len(left)
    view = np.full(t.n_pt, -1, np.int32)
    obs = np.full(t.n_pt, -1, np.int64)
    px = np.zeros((t.n_pt, 2), np.int32)
    order = []
    while left:
        count = {}
        for p in left:                          # the recount
            for im in seen[p]:
                count[im] = count.get(im, 0) + 1
        best = max(count.values())
        v = min(im for im, c in count.items() if c == best)
        order.append(v)
        for p in left:
            if v in seen[p]:
                o = seen[p][v]
                view[p], obs[p] = v, o
                for a in (0, 1):
                    px[p, a] = int(min(max(float(t.obs_uv[o, a]), 0.0), float(wh[v, a] - 1)))   # clamp, then truncate
        left = [p for p in left if v not in seen[p]]
    n_rounds = len(order)
    return dict(view=view, obs=obs, px=px, order=np.array(order + [-1] * (t.n_img - n_rounds), np.int32),
                n_rounds=n_rounds, n_to_colour=n_to_colour)


def sample_ref(view, px, images):
    rgb = np.zeros((len(view), 3), np.uint8)
    for p, v in enumerate(view):
        if v >= 0:
            rgb[p] = images[v][px[p, 1], px[p, 0]]   # (a gray value broadcasts to g g g)
    return rgb


def initial_counts(t, pt_ok=None, keep_obs=None):
    """count[v] before the first round, recounted"""
    ok = np.ones(t.n_pt, bool) if pt_ok is None else np.asarray(pt_ok, bool)
    live = np.ones(t.n_obs, bool) if keep_obs is None else np.asarray(keep_obs, bool)
    pairs = {(int(t.obs_img[o]), int(t.obs_pt[o])) for o in range(t.n_obs) if live[o] and ok[t.obs_pt[o]]}
    return np.bincount([im for im, _ in pairs], minlength=t.n_img)[:t.n_img]


# ---- scenes ---------------------------------------------------------------------------------
def random_images(seed, n_img, w_range=(17, 40), h_range=(11, 30)):
    """(wh [n_img, 2], images): non-square, different sizes, channels 1 and 3 in turn"""
    rng = np.random.default_rng(seed)
    wh = np.stack([rng.integers(*w_range, n_img), rng.integers(*h_range, n_img)], 1).astype(np.int32)
    images = [rng.integers(0, 256, (h, w) if i % 2 else (h, w, 3), dtype=np.uint8) for i, (w, h) in enumerate(wh)]
    return wh, images


def tracks_from_lists(n_img, lists, wh, seed=0):
    """lists[p]: the images of point p's observations, in track order; uv random,
    some outside the image (negative, and past the right / lower edge)"""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    img = np.array([i for x in lists for i in x], np.int32)
    wh = np.asarray(wh).reshape(-1, 2)
    uv = rng.uniform(-3.0, 1.0, (len(img), 2)) + rng.uniform(0, 1, (len(img), 2)) * (wh[img] + 5.0) if len(img) \
        else np.zeros((0, 2))
    return RH.Tracks(n_img, off, img, uv)


def random_scene(seed, n_img=40, n_pt=2000, min_len=2, max_len=12, dead=1 / 3, masked=1 / 5, dup=0.15,
                 empty_images=()):
    """(tracks, wh, images, pt_ok, keep_obs): tracks of min_len .. max_len
    observations over random images (with probability dup an observation repeats
    the image of the one before it), `dead` of the observations dead, `masked`
    of the points masked off"""
    rng = np.random.default_rng(seed)
    wh, images = random_images(seed + 1, n_img)
    usable = np.array([i for i in range(n_img) if i not in set(empty_images)])
    lists = []
    for _ in range(n_pt):
        x = list(usable[rng.integers(0, len(usable), rng.integers(min_len, max_len + 1))])
        for k in range(1, len(x)):
            if rng.random() < dup:
                x[k] = x[k - 1]
        lists.append(x)
    t = tracks_from_lists(n_img, lists, wh, seed + 2)
    return t, wh, images, rng.random(n_pt) >= masked, rng.random(t.n_obs) >= dead


def same_assign(a, b):
    """two results of api.colorize_assign (or one and assign_ref's): every output, exactly"""
    for f in ("view", "obs", "px", "order"):
        x, y = np.asarray(a[f]), np.asarray(b[f])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    assert a["n_rounds"] == b["n_rounds"]


def check_against_ref(res, t, wh, pt_ok=None, keep_obs=None):
    ref = assign_ref(t, wh, pt_ok, keep_obs)
    same_assign(res, ref)
    st = res["stats"]
    assert st["n_rounds"] == ref["n_rounds"] and st["n_to_colour"] == ref["n_to_colour"]
    assert st["n_coloured"] == int((ref["view"] >= 0).sum()) == ref["n_to_colour"]
    return ref


# ---- the file-staged scene of test_recon_gpu.py's sparse_reconstruct test ----------------------
def stage_sparse_scene(tmp_path, n_img=6, n_pt=300, f=700.0):
    """sfm_data.json (640 x 480 views), im<k>.feat and matches.f.bin in tmp_path; returns (n_img, f)"""
    from test_mvg_io import write_feat, write_sfm_data
    rng = np.random.default_rng(5)
    write_sfm_data(tmp_path / "sfm_data.json", [f"im{k}.jpg" for k in range(n_img)])
    ang = 0.12 * (np.arange(n_img) - 2.5)
    X = rng.uniform(-1.5, 1.5, (n_pt, 3))
    seen = np.full((n_img, n_pt), -1)
    for k, a in enumerate(ang):
        Rm = RH.R.rodrigues([0.0, a, 0.0])
        P = (X - np.array([10 * np.sin(a), 0.0, -10 * np.cos(a)])) @ Rm.T
        uv = f * P[:, :2] / P[:, 2:] + np.array([320.0, 240.0])
        vis = np.flatnonzero((rng.random(n_pt) < 0.8) & (uv[:, 0] > 0) & (uv[:, 0] < 640) & (uv[:, 1] > 0) & (uv[:, 1] < 480))
        vis = rng.permutation(vis)
        seen[k, vis] = np.arange(len(vis))
        kp = np.zeros((len(vis), 4), np.float32)
        kp[:, :2], kp[:, 2] = uv[vis], 2.0
        write_feat(tmp_path / f"im{k}.feat", kp)
    matches = {}
    for i in range(n_img):
        for j in range(i + 1, n_img):
            both = np.flatnonzero((seen[i] >= 0) & (seen[j] >= 0))
            matches[(i, j)] = np.stack([seen[i, both], seen[j, both]], 1).astype(np.uint32)
    api.mvg_save_matches(str(tmp_path / "matches.f.bin"), matches)
    return n_img, f
