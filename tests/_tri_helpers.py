"""Reference for the track triangulation tests (test_triangulate.py,
test_triangulate_gpu.py): a plain numpy fp64 restatement of the semantics in
include/sfmcore.h ("Track triangulation") -- np.linalg.eigh for the solves,
_wash_helpers.rotations / project for the residual -- plus the threshold
placement that keeps every decision off a borderline.

Tolerances (compare()): X 1e-9 absolute (eps * |M| / lambda2 <= 2.2e-16 * 100 *
tens of operations ~ 1e-12 at |X| <= 4 with lambda2 / lambda4 >= 0.01: three
decades of margin), residual 1e-9 px at kept observations (as the wash),
status, keep_obs and every stats field exact."""
import numpy as np

import _helpers as H
import _wash_helpers as W

abi, api = H.abi, W.api
OK, SHORT, ANGLE, INFINITE = 0, 1, 2, 3
KEEP, DEPTH, RESIDUAL, BAD, NOPOINT = 0, 1, 2, 3, 4
UNDISTORT_ITERS = 20


def default_opts():
    return dict(method=abi.SFM_TRI_ROBUST, max_hypotheses=64, max_residual_px=4.0, min_angle_deg=2.0,
                min_track_len=2, cheirality=1)


def abi_opts(o):
    a = abi.TriOpts()
    for f, _ in abi.TriOpts._fields_:
        setattr(a, f, o[f])
    return a


def radial(model, intr, r2):
    if model == abi.SFM_CAM_RADIAL3:
        return 1 + intr[:, 3] * r2 + intr[:, 4] * r2 ** 2 + intr[:, 5] * r2 ** 3
    return 1 + r2 * (intr[:, 1] + intr[:, 2] * r2)


def bearings(model, uv, intr):
    """unit bearings [n, 3] of pixels uv [n, 2] (intr [n, iw]) and the bad mask"""
    with np.errstate(all="ignore"):
        z = np.ones(len(uv))
        if model == abi.SFM_CAM_PINHOLE:
            p = np.stack([(uv[:, 0] - intr[:, 2]) / intr[:, 0], (uv[:, 1] - intr[:, 3]) / intr[:, 1]], 1)
        else:
            if model == abi.SFM_CAM_RADIAL3:
                pd = (uv - intr[:, 1:3]) / intr[:, :1]
            else:
                pd = uv / intr[:, :1]
                z = -z
            p = pd.copy()
            for _ in range(UNDISTORT_ITERS):
                p = pd / radial(model, intr, (p ** 2).sum(1))[:, None]
        b = np.concatenate([p, z[:, None]], 1)
        b = b / np.sqrt((p ** 2).sum(1) + 1.0)[:, None]
    return b, ~np.isfinite(b).all(1)


def redistort(model, b, intr):
    """pixels of camera-frame bearings b (the model's projection)"""
    return W.project(model, b, intr)


def _solve(G):
    """(X or None, lambda2 / lambda4) of the 4x4 Gram sum G"""
    w, v = np.linalg.eigh(G)
    vec = v[:, 0]
    ratio = w[1] / w[3] if w[3] > 0 else 0.0
    with np.errstate(all="ignore"):
        if not abs(vec[3]) > 1e-12:
            return None, ratio
        X = vec[:3] / vec[3]
    return (X if np.isfinite(X).all() else None), ratio


def pair_list(imgs, good, max_hyp):
    """the hypotheses' (a, b) of a track: images per observation, good mask"""
    idx = [i for i in range(len(imgs)) if good[i]]
    pairs = [(a, b) for ia, a in enumerate(idx) for b in idx[ia + 1:] if imgs[a] != imgs[b]]
    if len(pairs) > max_hyp:
        pairs = [pairs[(h * len(pairs)) // max_hyp] for h in range(max_hyp)]
    return pairs


def ref_triangulate(sc, extr, intr, opts=None):
    """The rules of sfm_triangulate on `sc` (a _helpers.Scene or anything with its
    arrays) at the cameras (extr, intr).  Besides the outputs: `norms` (every
    residual norm any judgement evaluated), `angles` (the widest kept angle of
    each point that got that far) and `exclude` (points whose X comparison is
    unsafe: a tie between the two best hypotheses, or an ill-conditioned
    compared solve)."""
    o = dict(default_opts(), **(opts or {}))
    model = sc.model
    iw = 6 if model == abi.SFM_CAM_RADIAL3 else 4
    img = sc.obs_img
    uv = sc.obs_uv.reshape(-1, 2)
    R = W.rotations(extr)
    t = extr.reshape(-1, 6)[:, 3:]
    I = intr.reshape(-1, iw)[sc.img_intr[img]] if sc.n_obs else np.zeros((0, iw))
    b, bad = bearings(model, uv, I)
    Rt = np.concatenate([R, t[:, :, None]], 2)[img]                       # [n, 3, 4]
    with np.errstate(all="ignore"):
        Cm = np.einsum("nij,njk->nik", np.eye(3)[None] - b[:, :, None] * b[:, None, :], Rt)
        G = np.einsum("nji,njk->nik", Cm, Cm)                             # [n, 4, 4]
        ray = np.einsum("nji,nj->ni", R[img], b)                          # R' b
    norms = []

    def judge(X, sel):
        """codes and residuals of observations sel at X"""
        with np.errstate(all="ignore"):
            P = np.einsum("nij,j->ni", R[img[sel]], X) + t[img[sel]]
            r = W.project(model, P, I[sel]) - uv[sel]
            nrm = np.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2)
            front = P[:, 2] < 0 if model == abi.SFM_CAM_SNAVELY else P[:, 2] > 0
            code = np.zeros(len(sel), np.int32)
            dep = ~np.isfinite(r).all(1)
            if o["cheirality"]:
                dep |= ~front
            code[dep] = DEPTH
            if o["max_residual_px"] > 0:
                code[(code == 0) & (nrm > o["max_residual_px"])] = RESIDUAL
        norms.extend(nrm[np.isfinite(nrm)].tolist())
        return code, r

    n_pt = sc.n_pt
    X_out = np.full((n_pt, 3), np.nan)
    status = np.zeros(n_pt, np.uint8)
    keep_obs = np.zeros(sc.n_obs, bool)
    residual = np.full((sc.n_obs, 2), np.nan)
    codes = np.full(sc.n_obs, BAD, np.int32)
    angles = np.full(n_pt, np.nan)
    exclude = np.zeros(n_pt, bool)
    min_ratio = np.inf
    for p in range(n_pt):
        a0, a1 = int(sc.pt_offsets[p]), int(sc.pt_offsets[p + 1])
        good = ~bad[a0:a1]
        gi = a0 + np.flatnonzero(good)
        X = None
        early_short = False
        if len(gi) < 2:
            early_short = True
        elif o["method"] == abi.SFM_TRI_LINEAR:
            X, ratio = _solve(np.add.reduce(G[gi], 0))
            final_ratio = ratio
        else:
            pairs = pair_list(img[a0:a1], good, o["max_hypotheses"])
            if not pairs:
                early_short = True
            else:
                scores = []
                for h, (a, c) in enumerate(pairs):
                    Xh, _ = _solve(G[a0 + a] + G[a0 + c])
                    if Xh is None:
                        scores.append((0, 0.0, h, None))
                        continue
                    code, r = judge(Xh, gi)
                    inl = code == KEEP
                    ssq = 0.0
                    for k in np.flatnonzero(inl):
                        ssq += r[k, 0] ** 2 + r[k, 1] ** 2
                    scores.append((int(inl.sum()), ssq, h, Xh))
                order = sorted(scores, key=lambda s: (-s[0], s[1], s[2]))
                best = order[0]
                # a tie between two different points (two hypotheses from identical
                # observations give the same X bit for bit: no ambiguity)
                if len(order) > 1 and order[1][0] == best[0] and best[3] is not None and \
                        abs(order[1][1] - best[1]) <= 1e-6 * max(abs(best[1]), abs(order[1][1])) and \
                        not np.array_equal(order[1][3], best[3]):
                    exclude[p] = True
                if best[0] < 2:
                    early_short = True
                else:
                    code, _ = judge(best[3], gi)
                    X, final_ratio = _solve(np.add.reduce(G[gi[code == KEEP]], 0))
        if early_short:
            status[p] = SHORT
            codes[gi] = NOPOINT
            continue
        if X is None:
            status[p] = INFINITE
            codes[gi] = NOPOINT
            continue
        if final_ratio < 0.01:
            exclude[p] = True
        min_ratio = min(min_ratio, final_ratio)
        code, r = judge(X, gi)
        codes[gi] = code
        residual[gi] = r
        kept = gi[code == KEEP]
        if len(kept) < o["min_track_len"]:
            status[p] = SHORT
            continue
        d = ray[kept]
        cr = np.cross(d[:, None, :], d[None, :, :])
        ang = np.degrees(np.arctan2(np.sqrt((cr ** 2).sum(2)), d @ d.T))
        angles[p] = ang[~np.eye(len(kept), dtype=bool)].max()
        if o["min_angle_deg"] > 0 and angles[p] < o["min_angle_deg"]:
            status[p] = ANGLE
            continue
        X_out[p] = X
        keep_obs[kept] = True
    solved = np.isin(codes, (KEEP, DEPTH, RESIDUAL))
    stats = dict(n_pt_ok=int((status == OK).sum()), n_pt_short=int((status == SHORT).sum()),
                 n_pt_angle=int((status == ANGLE).sum()), n_pt_infinite=int((status == INFINITE).sum()),
                 n_obs_kept=int(keep_obs.sum()), n_obs_bad=int(bad.sum()),
                 n_obs_depth=int((codes[solved] == DEPTH).sum()), n_obs_residual=int((codes[solved] == RESIDUAL).sum()))
    return dict(X=X_out, status=status, keep_obs=keep_obs, residual=residual, stats=stats, codes=codes,
                norms=np.array(norms), angles=angles, exclude=exclude, min_ratio=min_ratio, opts=o)


def placed_opts(sc, extr, intr, angle_target=None, **over):
    """Options whose thresholds sit in gaps (> 1e-6) of the reference's own
    values: max_residual_px nearest its given value among every residual norm
    the reference evaluates (every hypothesis's included), min_angle_deg
    nearest angle_target (default: its given value; "keep": the given value
    itself, checked) among the widest kept angles.  Returns (opts, reference).  Asserts that at most 1 % of the
    points are excluded from the X comparison."""
    o = dict(default_opts(), **over)
    if o["max_residual_px"] > 0:
        want = o["max_residual_px"]
        for _ in range(6):        # the refit's residuals move with the threshold: place, then check
            ref = ref_triangulate(sc, extr, intr, dict(o, min_angle_deg=0.0))
            if len(ref["norms"]) == 0 or np.abs(ref["norms"] - o["max_residual_px"]).min() > 0.5e-6:
                break
            o["max_residual_px"] = W.gap_threshold(ref["norms"], want)
        else:
            raise AssertionError("no residual threshold clear of every evaluated residual")
    if o["min_angle_deg"] > 0:
        ref = ref_triangulate(sc, extr, intr, dict(o, min_angle_deg=0.0))
        ang = ref["angles"][np.isfinite(ref["angles"])]
        if len(ang):
            if angle_target == "keep":      # the given threshold, if it is clear of every angle
                assert np.abs(ang - o["min_angle_deg"]).min() > 0.5e-6
            else:
                o["min_angle_deg"] = W.gap_threshold(ang, o["min_angle_deg"] if angle_target is None else angle_target)
    ref = ref_triangulate(sc, extr, intr, o)
    if len(ref["norms"]) and o["max_residual_px"] > 0:
        assert np.abs(ref["norms"] - o["max_residual_px"]).min() > 0.5e-6
    left_out = int((ref["exclude"] & (ref["status"] == OK)).sum())      # of the points whose X is compared at all
    assert left_out <= 0.01 * sc.n_pt, (left_out, sc.n_pt)
    return o, ref


def compare(got, ref, tol=1e-9, what="triangulation"):
    np.testing.assert_array_equal(got["status"], ref["status"])
    np.testing.assert_array_equal(got["keep_obs"], ref["keep_obs"])
    assert got["stats"] == ref["stats"], (got["stats"], ref["stats"])
    ok = ref["status"] == OK
    assert np.isnan(got["X"][~ok]).all() and np.isfinite(got["X"][ok]).all()
    cmp = ok & ~ref["exclude"]
    err_x = np.abs(got["X"][cmp] - ref["X"][cmp]).max() if cmp.any() else 0.0
    k = ref["keep_obs"]
    err_r = np.abs(got["residual"][k] - ref["residual"][k]).max() if k.any() else 0.0
    print(f"{what}: X err {err_x:.3e}, residual err {err_r:.3e} px, excluded {int(ref['exclude'].sum())}, "
          f"min lambda2/lambda4 {ref['min_ratio']:.3g}, stats {got['stats']}")
    assert err_x <= tol
    assert err_r <= tol


class Arrays:
    """a problem assembled from per-point observation lists [(image, (u, v)), ...]"""

    def __init__(self, sc, tracks):
        self.n_cam, self.n_intr, self.model = sc.n_cam, sc.n_intr, sc.model
        self.img_intr, self.const_img, self.huber = sc.img_intr, sc.const_img, sc.huber
        self.n_pt = len(tracks)
        self.pt_offsets = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.int64)
        self.n_obs = int(self.pt_offsets[-1])
        flat = [ob for t in tracks for ob in t]
        self.obs_img = np.array([ob[0] for ob in flat], np.int32)
        self.obs_uv = np.array([ob[1] for ob in flat], np.float64).reshape(-1)

    problem = H.Scene.problem


def tracks(sc):
    uv = sc.obs_uv.reshape(-1, 2)
    return [[(int(sc.obs_img[o]), uv[o].copy()) for o in range(sc.pt_offsets[p], sc.pt_offsets[p + 1])]
            for p in range(sc.n_pt)]


def flip_z(sc):
    """the same scene seen by cameras looking down -z (X -> -X, t -> -t negates
    every P = R X + t, which SFM_CAM_SNAVELY's p = -P / P2 does not see): the
    generator's cameras look down +z, SNAVELY's cheirality wants -z"""
    for a in (sc.X, sc.gt_X):
        a *= -1.0
    for a in (sc.extr, sc.gt_extr):
        a.reshape(-1, 6)[:, 3:] *= -1.0
    return sc
