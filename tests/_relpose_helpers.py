"""Reference for the relative pose tests (test_relpose.py, test_relpose_gpu.py):
plain numpy fp64, written from the semantics in include/sfmcore.h ("Relative
pose") and independently of the C++ -- the two-view generator, the
point-to-line error of a correspondence under E (through the undistorted pixels
and F, as the header words it), the a-contrario NFA of a model over every k,
Horn's decomposition check, the cheirality count by an SVD triangulation and
the median ray angle.  Nothing here searches: every check takes the model the
library reports and recomputes what follows from it.

Tolerances.  min_nfa 1e-9 (the project's).  Everything else was measured once
on the host twin (x86-64) and is allowed 100 x the worst value seen, as
rounding differs between hosts.  The five-point solver on the 200 noise-free
samples per model of fivept_samples(): the ten cubic constraints at a returned
E 1.6e-07 (bound 1.6e-05), |b_J' E b_I| at the five pairs 2.5e-16 (bound
2.5e-14), the nearest returned E to the true one up to sign 7.9e-07 (bound
7.9e-05); the worst cases are samples whose polynomial has two nearby roots.
Recovery (300 correspondences, 30 % outliers, 0.5 px noise, 256 iterations):
rotation within 3.9e-03 rad and the direction of t within 9.4e-03 rad of truth
(bounds 0.39 and 0.94 rad).  Noise-free 60-point pairs: rotation and direction
within 1.1e-12 rad (bound 1.1e-10).  The chain (relpose -> triangulate ->
resect on a noise-free scene, chain() below) lands within 2.4e-14 baselines of
ground truth in the result's gauge (bound 2.4e-12)."""
import numpy as np

import _helpers as H
import _resect_helpers as R
import _tri_helpers as T
import _wash_helpers as W

abi, api = H.abi, W.api
OK, FEW, NO_MODEL, AMBIGUOUS = 0, 1, 2, 3
MODELS = R.MODELS
FLT_EPS = R.FLT_EPS
WH = R.WH
WH4 = WH + WH
intrinsics, rodrigues, rot_to_aa = R.intrinsics, R.rodrigues, R.rot_to_aa

# measured on the host twin (docstring); the bounds are 100 x these
FIVEPT_CONSTRAINT, FIVEPT_EPIPOLAR, FIVEPT_TRUE_E = 1.6e-07, 2.5e-16, 7.9e-07
RECOVERY_ROT, RECOVERY_DIR, NOISE_FREE_POSE, CHAIN = 3.9e-03, 9.4e-03, 1.1e-12, 2.4e-14
MARGIN = 100.0


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0.0]])


def essential(Rm, t):
    """[t]x R at Frobenius norm sqrt(2)"""
    E = skew(t) @ Rm
    return E * np.sqrt(2.0) / np.linalg.norm(E)


def undistorted(model, intr):
    """the block with its distortion coefficients taken as zero"""
    z = np.array(intr, float)
    if model == abi.SFM_CAM_SNAVELY:
        z[1:3] = 0.0
    elif model == abi.SFM_CAM_RADIAL3:
        z[3:6] = 0.0
    return z


def calibration(model, intr):
    """K with u^ (homogeneous) proportional to K b"""
    if model == abi.SFM_CAM_PINHOLE:
        return np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1.0]])
    if model == abi.SFM_CAM_SNAVELY:
        return np.diag([intr[0], intr[0], -1.0])
    return np.array([[intr[0], 0, intr[1]], [0, intr[0], intr[2]], [0, 0, 1.0]])


def errors(model, E, intrI, intrJ, xy):
    """squared distance in px of u^_J from the line F u^_I; +inf without two
    finite bearings or when not finite"""
    n = len(xy)
    with np.errstate(all="ignore"):
        bi, badi = T.bearings(model, xy[:, :2], np.tile(intrI, (n, 1)))
        bj, badj = T.bearings(model, xy[:, 2:], np.tile(intrJ, (n, 1)))
        ui = W.project(model, bi, np.tile(undistorted(model, intrI), (n, 1)))
        uj = W.project(model, bj, np.tile(undistorted(model, intrJ), (n, 1)))
        F = np.linalg.inv(calibration(model, intrJ)).T @ E @ np.linalg.inv(calibration(model, intrI))
        line = np.concatenate([ui, np.ones((n, 1))], 1) @ F.T
        d = (line[:, :2] * uj).sum(1) + line[:, 2]
        e = d * d / (line[:, 0] ** 2 + line[:, 1] ** 2)
    e[badi | badj | ~np.isfinite(e)] = np.inf
    return e


def camera_points(model, rng, n, depth=(4, 8)):
    P = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.1, 1.1, n), rng.uniform(*depth, n)], 1)
    return -P if model == abi.SFM_CAM_SNAVELY else P


def make_pair(model, n, outliers, seed, sigma=0.5, w=None, t=None):
    """n correspondences of one image pair: P_J = R P_I + t, both in front.
    Outlier pixels of image J are uniform in the image, redrawn until they lie
    at least 50 px from the true epipolar line."""
    rng = np.random.default_rng(seed)
    intr = intrinsics(model)
    if w is None:
        w = rng.normal(size=3)
        w *= rng.uniform(0.05, 0.25) / np.linalg.norm(w)
    if t is None:
        t = rng.normal(size=3) * np.array([1.0, 0.5, 0.3])
        t /= np.linalg.norm(t)
    w, t = np.asarray(w, float), np.asarray(t, float)
    Rm = rodrigues(w)
    PI = camera_points(model, rng, n)
    PJ = PI @ Rm.T + t
    I = np.tile(intr, (max(n, 1), 1))[:n]
    xy = np.concatenate([W.project(model, PI, I), W.project(model, PJ, I)], 1) if n else np.zeros((0, 4))
    xy = xy + sigma * rng.normal(size=(n, 4))
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outliers * n))]] = True
    tn = np.linalg.norm(t)
    Et = essential(Rm, t) if tn > 0 else None
    lo, hi = R.image_box(model)
    for k in np.flatnonzero(out):
        while True:
            xy[k, 2:] = rng.uniform(lo, hi)
            if Et is None or errors(model, Et, intr, intr, xy[k:k + 1])[0] >= 50.0 ** 2:
                break
    return dict(model=model, n=n, xy=xy, intr=intr, R=Rm, w=w, t=t, outlier=out)


def opts(precision=4.0, max_iterations=4096, front_ratio=0.7):
    o = abi.RelposeOpts()
    o.precision, o.max_iterations, o.front_ratio = precision, max_iterations, front_ratio
    return o


def run(ctx, pairs, o=None, pair_intr=None, intr=None):
    """api.relpose over pairs of one camera model (each with its own
    intrinsics block for both images unless pair_intr / intr are given)"""
    model = pairs[0]["model"]
    if intr is None:
        intr = np.concatenate([p["intr"] for p in pairs])
        pair_intr = np.repeat(np.arange(len(pairs)), 2)
    return api.relpose(ctx, model, [p["xy"] for p in pairs], pair_intr, intr, [WH4] * len(pairs), o)


# ---- the semantics, restated ----------------------------------------------------
def logcombi_tables(n):
    """(logcombi(k, n), logcombi(5, k)) for k = 0..n, rounded to float as OpenMVG's"""
    i = np.arange(1, n + 1)
    cs = np.concatenate([[0.0], np.cumsum(np.log10(n - i + 1.0) - np.log10(i))])
    k = np.arange(n + 1)
    ln = np.where((k > 0) & (k < n), cs[np.minimum(k, n - k)], 0.0)
    lk = np.zeros(n + 1)
    for kk in range(6, n + 1):
        s = 0.0
        for j in range(1, min(5, kk - 5) + 1):
            s += np.log10(kk - j + 1.0) - np.log10(j)
        lk[kk] = s
    return ln.astype(np.float32).astype(np.float64), lk.astype(np.float32).astype(np.float64)


def nfa_scan(err, precision=4.0):
    """order (ascending (error, index) of the errors under the bound) and
    NFA(k) for k = 6..m as an array indexed by k (inf below 6)"""
    n = len(err)
    bound = precision ** 2 if 0 < precision < np.inf else np.finfo(float).max
    cand = np.flatnonzero(err <= bound)
    order = cand[np.lexsort((cand, err[cand]))]
    m = len(order)
    nfa = np.full(m + 1, np.inf)
    if m >= 6:
        ln, lk = logcombi_tables(n)
        k = np.arange(6, m + 1)
        logalpha = np.log10(2.0 * np.hypot(*WH) / (WH[0] * WH[1])) + 0.5 * np.log10(err[order[k - 1]] + FLT_EPS)
        nfa[6:] = np.log10(10.0 * (n - 5)) + logalpha * (k - 5) + ln[k] + lk[k]
    return order, nfa


def pair_intrinsics(p):
    return p.get("intrI", p["intr"]), p.get("intrJ", p["intr"])


def check_model(p, r, precision=4.0, min_gap=1e-6):
    """n_inliers, min_nfa, error_max and the inliers follow from E"""
    assert r["status"] in (OK, AMBIGUOUS)
    assert abs(np.linalg.norm(r["E"]) - np.sqrt(2.0)) <= 1e-12
    iI, iJ = pair_intrinsics(p)
    err = errors(p["model"], r["E"], iI, iJ, p["xy"])
    order, nfa = nfa_scan(err, precision)
    k = int(np.argmin(nfa))
    gap = np.delete(nfa, k).min() - nfa[k]
    print(f"n {p['n']}: argmin k {k} (reported {r['n_inliers']}), min_nfa {nfa[k]:.6f} (reported {r['min_nfa']:.6f}), "
          f"gap to the second best {gap:.3e}")
    assert gap >= min_gap, "the seed puts two NFA values within 1e-6: choose another"
    assert r["n_inliers"] == k and k > 12
    assert abs(r["min_nfa"] - nfa[k]) <= 1e-9
    assert abs(r["error_max"] - np.sqrt(err[order[k - 1]])) <= 1e-9
    # the inliers are that prefix in order wherever this reference can tell two
    # errors apart: it knows a distance to D = 1e-9 px (as _resect_helpers), so
    # an error e = d^2 to 2 sqrt(e) D + D^2; the five correspondences of the
    # model's own sample have errors of pure rounding
    inl = r["inliers"]
    np.testing.assert_array_equal(np.sort(inl), np.sort(order[:k]))
    D = 1e-9
    differ = np.flatnonzero(inl != order[:k])
    tol = 2 * np.sqrt(np.maximum(err[inl[differ]], err[order[differ]])) * D + D * D
    assert (np.abs(err[inl[differ]] - err[order[differ]]) <= tol).all(), (inl[differ], order[differ])


def motions(E):
    """Horn's four (R, t) of E: the header's formulas"""
    G = E @ E.T
    T2 = 0.5 * np.trace(G) * np.eye(3) - G
    i = int(np.argmax(np.diag(T2)))
    t = T2[i] / np.sqrt(T2[i, i])
    C = np.stack([np.cross(E[1], E[2]), np.cross(E[2], E[0]), np.cross(E[0], E[1])])
    Ra, Rb = (C - skew(t) @ E) / (t @ t), (C + skew(t) @ E) / (t @ t)
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


def in_front(model, Rm, t, bi, bj):
    """the two-view linear triangulation of every bearing pair under [I | 0]
    and [R | t] (smallest singular vector of the stacked (I - b b') [R | t]),
    and whether it is in front of both cameras"""
    out = np.zeros(len(bi), bool)
    PJm = np.concatenate([Rm, t[:, None]], 1)
    PIm = np.eye(3, 4)
    for k in range(len(bi)):
        A = np.concatenate([(np.eye(3) - np.outer(bi[k], bi[k])) @ PIm, (np.eye(3) - np.outer(bj[k], bj[k])) @ PJm])
        v = np.linalg.svd(A)[2][-1]
        if abs(v[3]) <= 1e-12:
            continue
        X = v[:3] / v[3]
        zi, zj = X[2], (Rm @ X + t)[2]
        out[k] = (zi < 0 and zj < 0) if model == abi.SFM_CAM_SNAVELY else (zi > 0 and zj > 0)
    return out


def check_motion(p, r, front_ratio=0.7):
    """status, pose, n_front and angle_median follow from E and the inliers"""
    iI, iJ = pair_intrinsics(p)
    xy = p["xy"][r["inliers"]]
    n = len(xy)
    bi, _ = T.bearings(p["model"], xy[:, :2], np.tile(iI, (n, 1)))
    bj, _ = T.bearings(p["model"], xy[:, 2:], np.tile(iJ, (n, 1)))
    ms = motions(r["E"])
    fronts = [in_front(p["model"], Rm, t, bi, bj) for Rm, t in ms]
    cnt = np.array([f.sum() for f in fronts])
    b = int(np.argmax(cnt))
    second = np.delete(cnt, b).max()
    print(f"cheirality counts {cnt.tolist()}, reported n_front {r['n_front']}, status {r['status']}")
    wins = cnt[b] > 0 and second / cnt[b] < front_ratio
    assert r["status"] == (OK if wins else AMBIGUOUS)
    if not wins:
        assert not r["pose"].any() and r["n_front"] == 0 and r["angle_median"] == 0.0
        return
    Rm, t = ms[b]
    assert r["n_front"] == cnt[b]
    assert np.abs(rodrigues(r["pose"][:3]) - Rm).max() <= 1e-9 and np.abs(r["pose"][3:] - t).max() <= 1e-9
    assert abs(np.linalg.norm(t) - 1.0) <= 1e-9 and np.abs(Rm.T @ Rm - np.eye(3)).max() <= 1e-9
    Et = skew(t) @ Rm
    assert min(np.abs(r["E"] - Et).max(), np.abs(r["E"] + Et).max()) <= 1e-9
    a, c = bi[fronts[b]], bj[fronts[b]] @ Rm         # b_I and R' b_J
    ang = np.degrees(np.arctan2(np.linalg.norm(np.cross(a, c), axis=1), (a * c).sum(1)))
    med = np.sort(ang)[len(ang) // 2]
    print(f"median ray angle {med:.6f} deg (reported {r['angle_median']:.6f})")
    assert abs(r["angle_median"] - med) <= 1e-9


def pose_errors(p, r):
    """(rotation error in rad, angle between t and the true direction in rad)"""
    dR = rodrigues(r["pose"][:3]) @ p["R"].T
    ax = np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    rot = np.arctan2(np.linalg.norm(ax) / 2, (np.trace(dR) - 1) / 2)
    tt = p["t"] / np.linalg.norm(p["t"])
    return rot, np.arctan2(np.linalg.norm(np.cross(r["pose"][3:], tt)), r["pose"][3:] @ tt)


# ---- the five-point solver -------------------------------------------------------
def fivept_samples(model, count=200, seed=9):
    """noise-free samples: five bearing pairs of a random two-view geometry"""
    rng = np.random.default_rng(seed + 100 * model)
    out = []
    for _ in range(count):
        w = rng.normal(size=3)
        w *= rng.uniform(0.05, 0.4) / np.linalg.norm(w)
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        Rm = rodrigues(w)
        PI = camera_points(model, rng, 5)
        PJ = PI @ Rm.T + t
        out.append((PI / np.linalg.norm(PI, axis=1)[:, None], PJ / np.linalg.norm(PJ, axis=1)[:, None],
                    essential(Rm, t)))
    return out


def constraint_residual(E):
    """the ten cubic constraints at E"""
    return max(abs(np.linalg.det(E)), np.abs(2 * E @ E.T @ E - np.trace(E @ E.T) * E).max())


def compare_results(a, b, tol=1e-9):
    """integers and inliers exactly, doubles to tol"""
    assert len(a) == len(b)
    worst = 0.0
    for x, y in zip(a, b):
        for f in ("status", "n_inliers", "n_front", "iterations"):
            assert x[f] == y[f], (f, x[f], y[f])
        np.testing.assert_array_equal(x["inliers"], y["inliers"])
        for f in ("E", "pose", "error_max", "min_nfa", "angle_median"):
            u, v = np.atleast_1d(x[f]).ravel(), np.atleast_1d(y[f]).ravel()
            assert (np.isfinite(u) == np.isfinite(v)).all() and (u[~np.isfinite(u)] == v[~np.isfinite(v)]).all(), f
            fin = np.isfinite(u)
            if fin.any():
                worst = max(worst, np.abs(u[fin] - v[fin]).max())
    print(f"largest difference of a double: {worst:.3e}")
    assert worst <= tol


identical = R.identical

SHAPES = (5, 6, 12, 13, 63, 64, 65, 255, 256, 257, 1000)


def shape_pairs(model, seed=150):
    """pairs of SHAPES sizes: outlier-free up to 13, 30 % outliers above"""
    return [make_pair(model, n, 0.0 if n <= 13 else 0.3, seed + i) for i, n in enumerate(SHAPES)]


def check_shapes(pairs, res):
    for p, r in zip(pairs, res):
        want = FEW if p["n"] <= 5 else NO_MODEL if p["n"] <= 12 else OK
        assert r["status"] == want, (p["n"], r["status"])
        if want == OK:
            check_model(p, r)
            check_motion(p, r)
            assert not p["outlier"][r["inliers"]].any()
        else:
            assert r["n_inliers"] == 0 and not r["pose"].any() and not r["E"].any()
            assert r["error_max"] == 0.0 and len(r["inliers"]) == 0 and r["n_front"] == 0


# ---- the chain relpose -> triangulate -> resect ------------------------------------
def chain(ctx):
    """Bootstraps a noise-free scene from nothing (ctx None: on the host twins):
    the relative pose of the two images that share the most tracks, the
    triangulation of those tracks with the poses (identity, result), the
    resection of the image that sees the most of the new points.  Returns the
    largest deviation of the three poses and the points from ground truth after
    the similarity that puts the first image at the identity and the baseline
    at length 1 (the gauge relative pose leaves open), in units of the baseline."""
    import copy
    sc = H.Scene(12, 600, 4, seed=4321, noise=0.0, outliers=0.0)
    uv = sc.obs_uv.reshape(-1, 2)
    pt_of = np.repeat(np.arange(sc.n_pt), np.diff(sc.pt_offsets))
    seen = np.full((sc.n_cam, sc.n_pt), -1)
    seen[sc.obs_img, pt_of] = np.arange(sc.n_obs)
    common = (seen[:, None, :] >= 0) & (seen[None, :, :] >= 0)
    cnt = np.triu(common.sum(2), 1)
    a, b = np.unravel_index(int(np.argmax(cnt)), cnt.shape)
    pts = np.flatnonzero(common[a, b])
    xy = np.concatenate([uv[seen[a, pts]], uv[seen[b, pts]]], 1)
    rp = api.relpose(ctx, sc.model, [xy], [sc.img_intr[a], sc.img_intr[b]], sc.gt_intr, [WH4],
                     opts(max_iterations=64))[0]
    assert rp["status"] == OK and rp["n_front"] == len(pts), (rp["status"], rp["n_front"], len(pts))
    # the two views of the common tracks, every point keeping its index
    two = copy.copy(sc)
    keep = np.zeros(sc.n_obs, bool)
    keep[seen[a, pts]] = keep[seen[b, pts]] = True
    two.pt_offsets = np.concatenate([[0], np.cumsum(np.bincount(pt_of[keep], minlength=sc.n_pt))]).astype(np.int64)
    two.obs_img = np.ascontiguousarray(sc.obs_img[keep])
    two.obs_uv = np.ascontiguousarray(uv[keep].reshape(-1))
    two.n_obs = int(keep.sum())
    extr = np.zeros((sc.n_cam, 6))
    extr[b] = rp["pose"]
    tri = api.triangulate(ctx, two.problem(), extr.reshape(-1), sc.gt_intr)
    ok = tri["status"] == T.OK
    assert ok.sum() >= 0.9 * len(pts), (ok.sum(), len(pts))
    others = [c for c in range(sc.n_cam) if c not in (a, b)]
    c = others[int(np.argmax([(seen[c, ok] >= 0).sum() for c in others]))]
    off, X3, uv3 = api.resect_gather(sc.problem(), tri["X"], ok, [c])
    rs = api.resect(ctx, sc.model, [X3], [uv3], [sc.img_intr[c]], sc.gt_intr, [WH], R.opts(max_iterations=64))[0]
    assert rs["status"] == R.OK
    # ground truth in the gauge of the result
    gt = sc.gt_extr.reshape(-1, 6)
    Ra, ta = rodrigues(gt[a, :3]), gt[a, 3:]
    rel = {}
    for im in (b, c):
        Rr = rodrigues(gt[im, :3]) @ Ra.T
        rel[im] = (Rr, gt[im, 3:] - Rr @ ta)
    s = np.linalg.norm(rel[b][1])
    worst = 0.0
    for im, pose in ((b, rp["pose"]), (c, rs["pose"])):
        worst = max(worst, np.abs(rodrigues(pose[:3]) - rel[im][0]).max(), np.abs(pose[3:] - rel[im][1] / s).max())
    Xa = (sc.gt_X.reshape(-1, 3) @ Ra.T + ta) / s
    worst = max(worst, np.abs(tri["X"][ok] - Xa[ok]).max())
    print(f"chain: images {a}, {b} ({len(pts)} common tracks, {ok.sum()} points), then image {c} "
          f"({off[1]} correspondences, {rs['n_inliers']} inliers): largest deviation {worst:.3e} baselines")
    return worst
