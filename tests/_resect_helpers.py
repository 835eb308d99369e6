"""Reference for the camera resection tests (test_resect.py, test_resect_gpu.py):
plain numpy fp64, written from the semantics in include/sfmcore.h ("Camera
resection") and independently of the C++ -- the generator, the error of a
correspondence (_wash_helpers.project), the a-contrario NFA of a model over
every k, and a Gauss-Newton refit whose Jacobian comes from complex-step
differentiation of that projection.  Nothing here searches: every check takes
the model the library reports and recomputes what follows from it.

Tolerances: min_nfa 1e-9 (sums of <= n log10 terms, 1e-13), pose against the
reference refit 1e-9 (the project's host/reference tolerance for X).  P3P, on
the 200 triplets per model of p3p_triplets(): the host twin's worst
|R'R - I| or |det R - 1| is 1.4e-15 (bound 1e-12), its worst
|unit(R X + t) x b| 8.2e-15 (bound 1e-9), and the nearest returned model is
within 8.2e-12 of the true pose (bound 1e-7), measured once on an x86-64 host:
the issue's starting values hold as they are."""
import numpy as np

import _helpers as H
import _tri_helpers as T
import _wash_helpers as W

abi, api = H.abi, W.api
OK, FEW, NO_MODEL = 0, 1, 2
MODELS = (abi.SFM_CAM_PINHOLE, abi.SFM_CAM_SNAVELY, abi.SFM_CAM_RADIAL3)
FLT_EPS = float(np.finfo(np.float32).eps)
WH = (2832, 2128)


def intrinsics(model):
    if model == abi.SFM_CAM_PINHOLE:
        return np.array([2900.0, 2890.0, 1416.0, 1064.0])
    if model == abi.SFM_CAM_SNAVELY:
        return np.array([2900.0, -0.05, 0.01, 0.0])
    return np.array([2900.0, 1416.0, 1064.0, -0.05, 0.01, -0.001])


def rodrigues(w):
    return W.rotations(np.concatenate([np.asarray(w, float), np.zeros(3)]))[0]


def rot_to_aa(R):
    """angle-axis of a rotation matrix (angles away from 0 and pi)"""
    ang = np.arccos(np.clip((np.trace(R) - 1) / 2, -1, 1))
    ax = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    nrm = np.linalg.norm(ax)
    return ax / nrm * ang if nrm > 0 else np.zeros(3)


def random_pose(rng):
    w = rng.normal(size=3)
    w *= rng.uniform(0.1, 0.6) / np.linalg.norm(w)
    return rodrigues(w), rng.uniform(-1, 1, size=3), w


def camera_points(model, rng, n):
    """points in a box in front of the camera (SNAVELY looks down -z)"""
    P = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.1, 1.1, n), rng.uniform(4, 8, n)], 1)
    return -P if model == abi.SFM_CAM_SNAVELY else P


def image_box(model):
    """the pixel rectangle of the image (SNAVELY pixels are centred)"""
    if model == abi.SFM_CAM_SNAVELY:
        return np.array([-WH[0] / 2, -WH[1] / 2]), np.array([WH[0] / 2, WH[1] / 2])
    return np.zeros(2), np.array(WH, float)


def make_problem(model, n, outliers, seed, sigma=0.5):
    """n correspondences of one image: X [n, 3], uv [n, 2], the true pose and
    the outlier mask.  Outlier pixels are uniform in the image, redrawn until
    they lie at least 50 px from the true projection."""
    rng = np.random.default_rng(seed)
    intr = intrinsics(model)
    R, t, w = random_pose(rng)
    P = camera_points(model, rng, n)
    X = (P - t) @ R                    # R' (P - t)
    true_uv = W.project(model, P, np.tile(intr, (n, 1))) if n else np.zeros((0, 2))
    uv = true_uv + sigma * rng.normal(size=(n, 2))
    out = np.zeros(n, bool)
    out[rng.permutation(n)[:int(round(outliers * n))]] = True
    lo, hi = image_box(model)
    for k in np.flatnonzero(out):
        while True:
            p = rng.uniform(lo, hi)
            if np.linalg.norm(p - true_uv[k]) >= 50.0:
                break
        uv[k] = p
    return dict(model=model, n=n, X=X, uv=uv, intr=intr, R=R, t=t, pose=np.concatenate([w, t]), outlier=out)


def opts(precision=0.0, max_iterations=4096, refine_iterations=10):
    o = abi.ResectOpts()
    o.precision, o.max_iterations, o.refine_iterations = precision, max_iterations, refine_iterations
    return o


def run(ctx, problems, o=None, img_intr=None, intr=None):
    """api.resect over problems of one camera model (each with its own
    intrinsics block unless img_intr / intr are given)"""
    model = problems[0]["model"]
    if intr is None:
        intr = np.concatenate([p["intr"] for p in problems])
        img_intr = np.arange(len(problems))
    return api.resect(ctx, model, [p["X"] for p in problems], [p["uv"] for p in problems], img_intr, intr,
                      [WH] * len(problems), o)


# ---- the semantics, restated ----------------------------------------------------
def errors(model, pose, intr, X, uv):
    """squared pixel error of every correspondence under pose (angle-axis, t):
    +inf without a finite bearing, behind the camera, or not finite"""
    n = len(X)
    I = np.tile(intr, (n, 1))
    with np.errstate(all="ignore"):
        P = X @ rodrigues(pose[:3]).T + pose[3:]
        r = W.project(model, P, I) - uv
        e = r[:, 0] ** 2 + r[:, 1] ** 2
        front = P[:, 2] < 0 if model == abi.SFM_CAM_SNAVELY else P[:, 2] > 0
        _, bad = T.bearings(model, uv, I)
    e[~front | ~np.isfinite(r).all(1) | ~np.isfinite(e) | bad] = np.inf
    return e


def logcombi_tables(n):
    """(logcombi(k, n), logcombi(3, k)) for k = 0..n, rounded to float as OpenMVG's"""
    i = np.arange(1, n + 1)
    cs = np.concatenate([[0.0], np.cumsum(np.log10(n - i + 1.0) - np.log10(i))])
    k = np.arange(n + 1)
    ln = np.where((k > 0) & (k < n), cs[np.minimum(k, n - k)], 0.0)
    lk = np.zeros(n + 1)
    for kk in range(4, n + 1):
        s = 0.0
        for j in range(1, min(3, kk - 3) + 1):
            s += np.log10(kk - j + 1.0) - np.log10(j)
        lk[kk] = s
    return ln.astype(np.float32).astype(np.float64), lk.astype(np.float32).astype(np.float64)


def nfa_scan(err, precision=0.0):
    """order (ascending (error, index) of the errors under the bound) and
    NFA(k) for k = 4..m as an array indexed by k (inf below 4)"""
    n = len(err)
    bound = precision ** 2 if 0 < precision < np.inf else np.finfo(float).max
    cand = np.flatnonzero(err <= bound)
    order = cand[np.lexsort((cand, err[cand]))]
    m = len(order)
    nfa = np.full(m + 1, np.inf)
    if m >= 4:
        ln, lk = logcombi_tables(n)
        k = np.arange(4, m + 1)
        logalpha = np.log10(np.pi / (WH[0] * WH[1])) + np.log10(err[order[k - 1]] + FLT_EPS)
        nfa[4:] = np.log10(4.0 * (n - 3)) + logalpha * (k - 3) + ln[k] + lk[k]
    return order, nfa


def check_model(p, r, precision=0.0, min_gap=1e-6):
    """check 2: n_inliers, min_nfa, error_max and inliers follow from pose_model"""
    assert r["status"] == OK
    err = errors(p["model"], r["pose_model"], p["intr"], p["X"], p["uv"])
    order, nfa = nfa_scan(err, precision)
    k = int(np.argmin(nfa))
    rest = np.delete(nfa, k)
    gap = rest.min() - nfa[k]
    print(f"n {p['n']}: argmin k {k} (reported {r['n_inliers']}), min_nfa {nfa[k]:.6f} (reported {r['min_nfa']:.6f}), "
          f"gap to the second best {gap:.3e}")
    assert gap >= min_gap, "the seed puts two NFA values within 1e-6: choose another"
    assert r["n_inliers"] == k
    assert abs(r["min_nfa"] - nfa[k]) <= 1e-9
    assert abs(r["error_max"] - np.sqrt(err[order[k - 1]])) <= 1e-9
    # inliers is exactly that prefix in order, wherever this reference can tell
    # two errors apart: it knows a residual to D = 1e-9 px (eps * 3000 px over
    # some twenty operations is 1.3e-11 px; 75 times that), so an error e = |r|^2
    # to 2 sqrt(e) D + D^2.  The three correspondences of the model's own
    # minimal sample have errors of 1e-24 px^2, pure rounding: their order is
    # the library's to choose.  Everywhere else the order must be the same.
    inl = r["inliers"]
    np.testing.assert_array_equal(np.sort(inl), np.sort(order[:k]))
    D = 1e-9
    differ = np.flatnonzero(inl != order[:k])
    tol = 2 * np.sqrt(np.maximum(err[inl[differ]], err[order[differ]])) * D + D * D
    assert len(differ) <= 3 and (np.abs(err[inl[differ]] - err[order[differ]]) <= tol).all(), \
        (inl[differ], order[differ], err[inl[differ]], err[order[differ]])


def refit(p, pose0, inliers, iterations=10):
    """the issue's Gauss-Newton on (R <- exp[d]x R, t += d_t) over `inliers`
    from pose0; the Jacobian by complex-step differentiation of the projection"""
    model, intr = p["model"], p["intr"]
    X, uv = p["X"][inliers], p["uv"][inliers]
    R, t = rodrigues(pose0[:3]), pose0[3:].copy()
    I = np.tile(intr, (len(X), 1))
    h = 1e-30
    for _ in range(iterations):
        RX = X @ R.T
        P = RX + t
        front = P[:, 2] < 0 if model == abi.SFM_CAM_SNAVELY else P[:, 2] > 0
        r = W.project(model, P, I) - uv
        use = front & np.isfinite(r).all(1)
        JP = np.zeros((len(X), 2, 3))
        for a in range(3):
            Pc = P.astype(complex)
            Pc[:, a] += 1j * h
            JP[:, :, a] = W.project(model, Pc, I).imag / h
        S = np.zeros((len(X), 3, 3))      # -[R X]x
        S[:, 0, 1], S[:, 0, 2] = RX[:, 2], -RX[:, 1]
        S[:, 1, 0], S[:, 1, 2] = -RX[:, 2], RX[:, 0]
        S[:, 2, 0], S[:, 2, 1] = RX[:, 1], -RX[:, 0]
        J = np.concatenate([JP @ S, JP], 2)[use].reshape(-1, 6)
        try:
            d = np.linalg.solve(J.T @ J, -J.T @ r[use].reshape(-1))
        except np.linalg.LinAlgError:
            return pose0
        R = rodrigues(d[:3]) @ R
        t = t + d[3:]
        if d @ d < 1e-24:
            break
    return np.concatenate([rot_to_aa(R), t])


def cost(p, pose, inliers):
    e = errors(p["model"], pose, p["intr"], p["X"], p["uv"])[inliers]
    return e.sum()


def check_refit(p, r, tol=1e-9):
    """check 3"""
    ref = refit(p, r["pose_model"], r["inliers"])
    d = np.abs(r["pose"] - ref).max()
    c0, c1 = cost(p, r["pose_model"], r["inliers"]), cost(p, r["pose"], r["inliers"])
    print(f"refit: |pose - reference| {d:.3e}, inlier cost {c0:.6f} -> {c1:.6f}")
    assert d <= tol
    assert c1 <= c0


def pose_error(p, pose):
    return max(np.abs(rodrigues(pose[:3]) - p["R"]).max(), np.abs(pose[3:] - p["t"]).max())


# ---- P3P -----------------------------------------------------------------------
def p3p_triplets(model, count=200, seed=7):
    """well-conditioned triplets: bearings at least 5 degrees apart and a world
    triangle whose angle at the first point is between 20 and 160 degrees"""
    rng = np.random.default_rng(seed + 100 * model)
    out = []
    while len(out) < count:
        R, t, _ = random_pose(rng)
        P = camera_points(model, rng, 3)
        b = P / np.linalg.norm(P, axis=1)[:, None]
        cosb = [b[0] @ b[1], b[0] @ b[2], b[1] @ b[2]]
        e1, e2 = P[1] - P[0], P[2] - P[0]
        s = np.linalg.norm(np.cross(e1, e2)) / (np.linalg.norm(e1) * np.linalg.norm(e2))
        if max(cosb) > np.cos(np.radians(5)) or s < np.sin(np.radians(20)):
            continue
        out.append((b, (P - t) @ R, R, t))
    return out


def compare_results(a, b, tol=1e-9):
    """check 5: integers and inliers exactly, doubles to tol"""
    assert len(a) == len(b)
    worst = 0.0
    for x, y in zip(a, b):
        for f in ("status", "n_inliers", "iterations"):
            assert x[f] == y[f], (f, x[f], y[f])
        np.testing.assert_array_equal(x["inliers"], y["inliers"])
        for f in ("pose", "pose_model", "error_max", "min_nfa"):
            u, v = np.atleast_1d(x[f]), np.atleast_1d(y[f])
            assert (np.isfinite(u) == np.isfinite(v)).all() and (u[~np.isfinite(u)] == v[~np.isfinite(v)]).all(), f
            fin = np.isfinite(u)
            if fin.any():
                worst = max(worst, np.abs(u[fin] - v[fin]).max())
    print(f"largest difference of a double: {worst:.3e}")
    assert worst <= tol


def identical(a, b):
    """bit for bit"""
    for x, y in zip(a, b):
        for f in x:
            assert np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes(), f


SHAPES = (0, 3, 4, 7, 8, 9, 64, 255, 256, 257, 1000)


def shape_problems(model, seed=50):
    """problems of SHAPES sizes: outlier-free up to 9, 30 % outliers above"""
    return [make_problem(model, n, 0.0 if n <= 9 else 0.3, seed + i) for i, n in enumerate(SHAPES)]


def check_shapes(problems, res):
    for p, r in zip(problems, res):
        want = FEW if p["n"] <= 3 else NO_MODEL if p["n"] <= 7 else OK
        assert r["status"] == want, (p["n"], r["status"])
        if want == OK:
            check_model(p, r)
            check_refit(p, r)
            assert not p["outlier"][r["inliers"]].any()
        else:
            assert r["n_inliers"] == 0 and not r["pose"].any() and not r["pose_model"].any()
            assert r["error_max"] == 0.0 and len(r["inliers"]) == 0
