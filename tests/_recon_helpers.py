"""Reference for the incremental reconstruction tests (test_recon.py,
test_recon_gpu.py): plain numpy restatements of the three round queries from
the semantics in include/sfmcore.h ("Incremental reconstruction"), random track
sets for them, and the synthetic scene of the driver tests: 8 images on an arc
of radius 10 around 400 points in a cube of side 4, every point seen by 3 to 8
consecutive images, exact projections (plus Gaussian pixel noise where a test
asks for it), and in 8 tracks of four or more views one observation moved by
at least 150 px (the corrupted observations).

Measured values.
  Host twin, adjust = 0, noise-free scene (x86-64 host, the machine the CPU
  suite runs on), worst deviation of a pose or a point from ground truth in
  the gauge of the result (first image of the pair at the identity, baseline 1):
  PINHOLE 1.6e-14, SNAVELY 3.6e-14, RADIAL3 1.4e-13 baselines with the pair the
  rule picks (images 1 and 7), and 5.9e-13 (PINHOLE) from the forced pair (2, 3),
  whose short baseline conditions the gauge worse.  HOST_DEVIATION is the
  largest; the tests allow MARGIN = 100 x it, as the relpose tests do for their
  rounding-level figures (rounding differs between hosts).
  Device, adjust = 1, 0.5 px noise, measured on an MI355X: final RMSE of the
  driver / of sfm_ba_solve started from the true parameters on the same kept
  observations (ADJUST_RMSE): PINHOLE 0.298865 / 0.298867, SNAVELY 0.299300 /
  0.299300, RADIAL3 0.299717 / 0.299717, RADIAL3 with a block per image
  0.297229 / 0.297229.  They agree to 7e-6 relative; the solver stops on a
  relative cost decrease of 1e-6 per iteration, so two descents to one minimum
  may end a few such steps apart.  ADJUST_MARGIN = 1e-3 relative is 100 x the
  largest difference seen.  On the same machine the device driver with
  adjust = 0 was within 2.8e-14 of the host twin's poses and points.
"""
import ctypes as C

import numpy as np

import _helpers as H
import _resect_helpers as R
import _wash_helpers as W

abi, api = H.abi, W.api
MODELS = R.MODELS
WH = R.WH
NEW, SOLVED = abi.SFM_RECON_NEW, abi.SFM_RECON_SOLVED

HOST_DEVIATION = 5.9e-13
MARGIN = 100.0
# host against device: the resect tests' margin for doubles (compare_results)
HOST_DEVICE_TOL = 1e-9
# adjust = 1 on the MI355X, 0.5 px noise, seed 11: final RMSE of the driver and
# of sfm_ba_solve started from the true parameters on the same kept observations
# (model: driver, yardstick); the driver may exceed the yardstick by ADJUST_MARGIN
# (relative).  Keys: (camera model, a block per image).
ADJUST_RMSE = {(0, False): (0.298865, 0.298867), (1, False): (0.299300, 0.299300), (2, False): (0.299717, 0.299717),
               (2, True): (0.297229, 0.297229)}
ADJUST_MARGIN = 1e-3


class Tracks:
    """pt_offsets / obs_img / obs_uv as numpy arrays and a BAProblem view"""

    def __init__(self, n_img, pt_offsets, obs_img, obs_uv, img_intr=None, n_intr=1, model=0, huber=4.0):
        self.n_img = int(n_img)
        self.pt_offsets = np.ascontiguousarray(pt_offsets, np.int64)
        self.obs_img = np.ascontiguousarray(obs_img, np.int32)
        self.obs_uv = np.ascontiguousarray(np.asarray(obs_uv, np.float64).reshape(-1, 2))
        self.n_pt, self.n_obs = len(self.pt_offsets) - 1, len(self.obs_img)
        self.img_intr = np.ascontiguousarray(np.zeros(max(n_img, 1), np.int32) if img_intr is None else img_intr,
                                             np.int32)
        self.n_intr, self.model, self.huber = n_intr, model, huber
        self.obs_pt = np.repeat(np.arange(self.n_pt), np.diff(self.pt_offsets))
        # never-null arrays for the C side
        self._img = self.obs_img if self.n_obs else np.zeros(1, np.int32)
        self._uv = self.obs_uv if self.n_obs else np.zeros((1, 2))

    def problem(self):
        pr = abi.BAProblem()
        pr.n_img, pr.n_intr, pr.n_pt, pr.n_obs = self.n_img, self.n_intr, self.n_pt, self.n_obs
        pr.pt_offsets = abi.ptr(self.pt_offsets, abi.i64p)
        pr.obs_img = abi.ptr(self._img, abi.i32p)
        pr.obs_uv = abi.ptr(self._uv, abi.f64p)
        pr.img_intr = abi.ptr(self.img_intr, abi.i32p)
        pr.const_img, pr.camera_model, pr.huber_a = -1, self.model, self.huber
        pr._keep = self
        return pr


def random_tracks(seed, n_img, n_pt, max_len, dup=0.2, empty_images=(), long_track=0):
    """n_pt tracks of 0 .. max_len observations over the images outside
    empty_images; with probability dup an observation repeats the image of the
    one before it (a point seen twice in one image); long_track > 0 makes the
    first track that long."""
    rng = np.random.default_rng(seed)
    imgs = np.array([i for i in range(n_img) if i not in set(empty_images)], np.int32)
    lens = rng.integers(0, max_len + 1, n_pt) if len(imgs) else np.zeros(n_pt, int)
    if long_track and n_pt:
        lens[0] = long_track
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(off[-1])
    img = imgs[rng.integers(0, max(len(imgs), 1), n)] if n else np.zeros(0, np.int32)
    rep = rng.random(n) < dup
    rep[off[:-1][lens > 0]] = False          # (a track's first observation has none before it)
    for o in np.flatnonzero(rep):
        img[o] = img[o - 1]
    uv = rng.uniform(0, 1000, (n, 2))
    return Tracks(n_img, off, img, uv)


# ---- the three queries, restated ---------------------------------------------------
def visibility_ref(t, pt_ok, dead=None):
    alive = np.ones(t.n_obs, bool) if dead is None else ~dead
    use = alive & np.asarray(pt_ok, bool)[t.obs_pt]
    seen = np.unique(np.stack([t.obs_img[use], t.obs_pt[use]], 1), axis=0) if use.any() else np.zeros((0, 2), int)
    return np.bincount(seen[:, 0], minlength=t.n_img).astype(np.int32)[:t.n_img]


def gather_ref(t, X, pt_ok, images, dead=None):
    alive = np.ones(t.n_obs, bool) if dead is None else ~dead
    use = alive & np.asarray(pt_ok, bool)[t.obs_pt]
    X = np.asarray(X, float).reshape(-1, 3)
    rows = [np.flatnonzero(use & (t.obs_img == im)) for im in images]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    obs = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
    return off, X[t.obs_pt[obs]], t.obs_uv[obs], obs


def select_ref(t, registered, pt_ok, mode, min_track_len=2, dead=None):
    alive = np.ones(t.n_obs, bool) if dead is None else ~dead
    registered, pt_ok = np.asarray(registered, bool), np.asarray(pt_ok, bool)
    kept = alive & registered[t.obs_img] if t.n_obs else np.zeros(0, bool)
    sel = np.zeros(t.n_pt, bool)
    for p in range(t.n_pt):
        k = kept[t.pt_offsets[p]:t.pt_offsets[p + 1]]
        im = t.obs_img[t.pt_offsets[p]:t.pt_offsets[p + 1]][k]
        if mode == NEW:
            sel[p] = not pt_ok[p] and len(set(im.tolist())) >= 2
        else:
            sel[p] = pt_ok[p] and len(im) >= max(min_track_len, 1)
    obs = np.flatnonzero(kept & sel[t.obs_pt]) if t.n_obs else np.zeros(0, int)
    pts = np.flatnonzero(sel)
    cnt = np.bincount(t.obs_pt[obs], minlength=t.n_pt)[pts] if t.n_pt else np.zeros(0, int)
    return dict(pt_offsets=np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64), obs_img=t.obs_img[obs],
                obs_uv=t.obs_uv[obs], pt_map=pts.astype(np.int64), obs_map=obs.astype(np.int64))


def same_select(a, b):
    for f in ("pt_offsets", "obs_img", "obs_uv", "pt_map", "obs_map"):
        x, y = np.asarray(a[f]), np.asarray(b[f])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f


def same_gather(a, b):
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.shape == y.shape and x.astype(y.dtype).tobytes() == y.tobytes()


def states(t, seed):
    """(registered, pt_ok) pairs: nothing / everything registered, pt_ok all 0 /
    all 1, and two random ones"""
    rng = np.random.default_rng(seed)
    z = lambda n: np.zeros(n, bool)
    o = lambda n: np.ones(n, bool)
    out = [(z(t.n_img), z(t.n_pt)), (o(t.n_img), o(t.n_pt)), (o(t.n_img), z(t.n_pt)), (z(t.n_img), o(t.n_pt))]
    for _ in range(2):
        out.append((rng.random(t.n_img) < 0.6, rng.random(t.n_pt) < 0.5))
    return out


def check_queries(h, t, seed=0, dead=None):
    """every query of handle h against the numpy restatement, over states(t)"""
    rng = np.random.default_rng(seed + 1)
    X = rng.normal(size=(t.n_pt, 3))
    for reg, ok in states(t, seed):
        np.testing.assert_array_equal(h.visibility(ok), visibility_ref(t, ok, dead))
        lists = [[], list(range(t.n_img)), list(rng.permutation(t.n_img)[:max(t.n_img // 2, 1)]) if t.n_img else []]
        for images in lists:
            same_gather(h.gather(X, ok, images), gather_ref(t, X, ok, images, dead))
        for mode, ml in ((NEW, 2), (SOLVED, 2), (SOLVED, 3)):
            same_select(h.select(reg, ok, mode, ml), select_ref(t, reg, ok, mode, ml, dead))


def all_queries(h, t, seed=0):
    """what check_queries asks, as bytes (for run-to-run and host/device comparisons)"""
    rng = np.random.default_rng(seed + 1)
    X = rng.normal(size=(t.n_pt, 3))
    out = []
    for reg, ok in states(t, seed):
        out.append(h.visibility(ok).tobytes())
        for images in ([], list(range(t.n_img)), list(rng.permutation(t.n_img)[:max(t.n_img // 2, 1)]) if t.n_img else []):
            out += [np.asarray(a).tobytes() for a in h.gather(X, ok, images)]
        for mode, ml in ((NEW, 2), (SOLVED, 2), (SOLVED, 3)):
            s = h.select(reg, ok, mode, ml)
            out += [np.asarray(s[f]).tobytes() for f in sorted(s)]
    return out


# ---- the driver's scene --------------------------------------------------------------
class ArcScene:
    def __init__(self, model, seed=11, n_img=8, n_pt=400, noise=0.0, n_bad=8, per_image_intr=False, lonely=False):
        """lonely: one more image, last, that shares no track"""
        rng = np.random.default_rng(seed)
        self.model, self.n_cam = model, n_img
        ang = 0.12 * (np.arange(n_img) - 0.5 * (n_img - 1))
        flip = np.diag([1.0, -1.0, -1.0]) if model == abi.SFM_CAM_SNAVELY else np.eye(3)   # SNAVELY looks down -z
        self.Rs, self.ts = [], []
        for a in ang:
            Rm = flip @ R.rodrigues([0.0, a, 0.0])
            Cc = np.array([10 * np.sin(a), 0.0, -10 * np.cos(a)])
            self.Rs.append(Rm)
            self.ts.append(-Rm @ Cc)
        self.gt_X = rng.uniform(-2, 2, (n_pt, 3))
        lens = rng.integers(3, 9, n_pt).clip(max=n_img)
        start = np.array([rng.integers(0, n_img - k + 1) for k in lens])
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        img = np.concatenate([np.arange(s, s + k) for s, k in zip(start, lens)]).astype(np.int32)
        pt = np.repeat(np.arange(n_pt), lens)
        base = R.intrinsics(model)
        n_intr = n_img if per_image_intr else 1
        self.gt_intr = np.tile(base, n_intr)
        img_intr = np.arange(n_img, dtype=np.int32) if per_image_intr else np.zeros(n_img, np.int32)
        P = np.stack([self.Rs[i] @ self.gt_X[p] + self.ts[i] for i, p in zip(img, pt)])
        uv = W.project(model, P, np.tile(base, (len(P), 1))) + noise * rng.normal(size=(len(P), 2))
        # the corrupted observations: one per track, in n_bad tracks of four or more views
        self.bad_obs = np.zeros(len(img), bool)
        for p in rng.permutation(np.flatnonzero(lens >= 4))[:n_bad]:
            o = off[p] + rng.integers(0, lens[p])
            d = rng.normal(size=2)
            uv[o] += d / np.linalg.norm(d) * rng.uniform(150, 400)
            self.bad_obs[o] = True
        self.clean_pt = ~np.bincount(pt[self.bad_obs], minlength=n_pt).astype(bool)
        if lonely:
            n_img += 1
            img_intr = np.append(img_intr, 0).astype(np.int32)
        self.n_img = n_img
        self.tracks = Tracks(n_img, off, img, uv, img_intr, n_intr, model)
        self.wh = np.tile(np.array(WH, np.int32), n_img)
        self.pairs = api.exhaustive_pairs(n_img)

    def run(self, ctx, opts=None, pairs=None, **kw):
        return api.reconstruct(ctx, self.tracks.problem(), self.gt_intr, self.wh, self.pairs if pairs is None else pairs,
                               opts, **kw)

    def deviation(self, res):
        """largest deviation of a registered pose or a reconstructed point from
        ground truth after the similarity that puts the pair's first image at the
        identity and its baseline at length 1, in baselines"""
        a, b = res["stats"]["initial_pair"]
        Ra, ta = self.Rs[a], self.ts[a]
        rel = lambda i: (self.Rs[i] @ Ra.T, self.ts[i] - self.Rs[i] @ Ra.T @ ta)
        s = np.linalg.norm(rel(b)[1])
        worst = 0.0
        for i in np.flatnonzero(res["registered"]):
            Rr, tr = rel(i)
            worst = max(worst, np.abs(R.rodrigues(res["extr"][i, :3]) - Rr).max(), np.abs(res["extr"][i, 3:] - tr / s).max())
        Xa = (self.gt_X @ Ra.T + ta) / s
        ok = res["pt_ok"]
        return max(worst, np.abs(res["X"][ok] - Xa[ok]).max())

    def check_conditions(self, res, n_reg=None):
        """the required conditions of the driver tests"""
        assert res["stats"]["status"] == abi.SFM_RECON_OK
        assert res["registered"][:self.n_cam].all() and res["registered"].sum() == (n_reg or self.n_cam)
        assert not res["keep_obs"][self.bad_obs].any()
        assert res["pt_ok"][self.clean_pt].all()
        assert np.isnan(res["X"][~res["pt_ok"]]).all() and np.isfinite(res["X"][res["pt_ok"]]).all()
        t = self.tracks
        want = res["pt_ok"][t.obs_pt] & res["registered"][t.obs_img]
        assert not (res["keep_obs"] & ~want).any()


def recon_opts(adjust=0, iters=256, **kw):
    o = api.recon_default_options()
    o.adjust = adjust
    o.relpose.max_iterations = o.resect.max_iterations = iters
    for k, v in kw.items():
        if k == "initial_pair":
            o.initial_pair[0], o.initial_pair[1] = v
        else:
            setattr(o, k, v)
    return o


def log_integers(res):
    """the round log's integers (and the decisions they record)"""
    r = [(x["first_cand"], x["n_cand"], x["n_registered"], x["adjust_repeats"], x["points_added"], x["obs_dropped"],
          x["points_removed"]) for x in res["rounds"]]
    c = [(x["round"], x["image"], x["count"], x["status"], x["n_inliers"]) for x in res["cands"]]
    st = res["stats"]
    return r, c, (st["status"], tuple(st["initial_pair"]), st["n_rounds"], st["n_cands"], st["n_registered"],
                  st["n_points"], st["n_obs_kept"])


def rot_to_aa(Rm):
    """angle-axis of a rotation matrix, also near pi (SNAVELY's cameras): the
    axis is the eigenvector of eigenvalue 1, its sign the one that reproduces Rm"""
    w, v = np.linalg.eig(Rm)
    ax = np.real(v[:, int(np.argmin(np.abs(w - 1.0)))])
    ax = ax / np.linalg.norm(ax) * np.arccos(np.clip((np.trace(Rm) - 1) / 2, -1, 1))
    return ax if np.abs(R.rodrigues(ax) - Rm).max() <= np.abs(R.rodrigues(-ax) - Rm).max() else -ax


def yardstick_rmse(ctx, sc, res):
    """sfm_ba_solve from the true parameters on the observations the driver kept"""
    t = sc.tracks
    keep = res["keep_obs"]
    pts = np.flatnonzero(np.bincount(t.obs_pt[keep], minlength=t.n_pt) > 0)
    cnt = np.bincount(t.obs_pt[keep], minlength=t.n_pt)[pts]
    sub = Tracks(t.n_img, np.concatenate([[0], np.cumsum(cnt)]), t.obs_img[keep], t.obs_uv[keep], t.img_intr, t.n_intr,
                 t.model)
    pr = sub.problem()
    pr.const_img = res["stats"]["initial_pair"][0]
    extr = np.zeros((t.n_img, 6))
    for i in range(sc.n_cam):
        extr[i] = np.concatenate([rot_to_aa(sc.Rs[i]), sc.ts[i]])
    extr, intr, X = extr.reshape(-1).copy(), sc.gt_intr.copy(), sc.gt_X[pts].reshape(-1).copy()
    rc, s = api.ba_solve(ctx, pr, extr, intr, X)
    assert rc == 0 and s.usable
    return s.rmse_final
