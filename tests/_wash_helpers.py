"""Reference for the post-BA outlier rejection tests (test_ba_wash.py,
test_ba_wash_gpu.py): plain numpy fp64 -- the Rodrigues rotation, the three
projections of include/sfmcore.h and the rejection rules of sfm_ba_wash --
plus the threshold placement that keeps every comparison off a borderline."""
import importlib

import numpy as np

import _helpers as H

abi = H.abi
api = importlib.import_module("3dreconstruction_amd.api")

DEPTH, RESIDUAL = 1, 2          # observation reject codes
SHORT, ANGLE = 1, 2             # point removal codes
EPS = np.finfo(np.float64).eps


def rotations(extr):
    """R [n, 3, 3] of the angle-axis blocks (ceres::AngleAxisRotatePoint:
    Rodrigues, or I + [w]x when |w|^2 <= eps)."""
    w = extr.reshape(-1, 6)[:, :3]
    R = np.zeros((len(w), 3, 3))
    for i, wi in enumerate(w):
        th2 = wi @ wi
        K = np.array([[0, -wi[2], wi[1]], [wi[2], 0, -wi[0]], [-wi[1], wi[0], 0]])
        if th2 > EPS:
            th = np.sqrt(th2)
            k = K / th
            R[i] = np.eye(3) + np.sin(th) * k + (1 - np.cos(th)) * (k @ k)
        else:
            R[i] = np.eye(3) + K
    return R


def project(model, P, intr):
    """pixel (u, v) [n, 2] of camera-frame points P [n, 3]; intr [n, iw]"""
    with np.errstate(all="ignore"):
        if model == abi.SFM_CAM_PINHOLE:
            x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
            return np.stack([intr[:, 0] * x + intr[:, 2], intr[:, 1] * y + intr[:, 3]], 1)
        if model == abi.SFM_CAM_SNAVELY:
            x, y = -P[:, 0] / P[:, 2], -P[:, 1] / P[:, 2]
            r2 = x * x + y * y
            d = 1 + r2 * (intr[:, 1] + intr[:, 2] * r2)
            return np.stack([intr[:, 0] * d * x, intr[:, 0] * d * y], 1)
        x, y = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
        r2 = x * x + y * y
        c = 1 + intr[:, 3] * r2 + intr[:, 4] * r2 ** 2 + intr[:, 5] * r2 ** 3
        return np.stack([intr[:, 1] + intr[:, 0] * x * c, intr[:, 2] + intr[:, 0] * y * c], 1)


def default_opts():
    return dict(max_residual_px=4.0, min_angle_deg=2.0, min_track_len=2, cheirality=1)


def abi_opts(o):
    a = abi.BAWashOpts()
    a.max_residual_px, a.min_angle_deg = o["max_residual_px"], o["min_angle_deg"]
    a.min_track_len, a.cheirality = o["min_track_len"], o["cheirality"]
    return a


def ref_wash(sc, extr, intr, X, opts=None):
    """The rules of sfm_ba_wash on scene `sc` (a _helpers.Scene or anything with
    its arrays) at (extr, intr, X)."""
    o = dict(default_opts(), **(opts or {}))
    iw = 6 if sc.model == abi.SFM_CAM_RADIAL3 else 4
    pt_of = np.repeat(np.arange(sc.n_pt), np.diff(sc.pt_offsets))
    img = sc.obs_img
    R = rotations(extr)
    t = extr.reshape(-1, 6)[:, 3:]
    Xp = X.reshape(-1, 3)[pt_of]
    P = np.einsum("nij,nj->ni", R[img], Xp) + t[img]
    r = project(sc.model, P, intr.reshape(-1, iw)[sc.img_intr[img]]) - sc.obs_uv.reshape(-1, 2)
    with np.errstate(all="ignore"):
        norm = np.sqrt(r[:, 0] ** 2 + r[:, 1] ** 2)
        front = P[:, 2] < 0 if sc.model == abi.SFM_CAM_SNAVELY else P[:, 2] > 0
        code = np.zeros(sc.n_obs, np.int32)
        bad = ~np.isfinite(r).all(1)
        if o["cheirality"]:
            bad |= ~front
        code[bad] = DEPTH
        if o["max_residual_px"] > 0:
            code[(code == 0) & (norm > o["max_residual_px"])] = RESIDUAL
    d = np.einsum("nji,nj->ni", R[img], P)      # R' P
    max_angle = np.zeros(sc.n_pt)
    removed = np.zeros(sc.n_pt, np.int32)
    for p in range(sc.n_pt):
        a, b = sc.pt_offsets[p], sc.pt_offsets[p + 1]
        alive = d[a:b][code[a:b] == 0]
        if len(alive) >= 2:
            cr = np.cross(alive[:, None, :], alive[None, :, :])
            ang = np.degrees(np.arctan2(np.sqrt((cr ** 2).sum(2)), alive @ alive.T))
            max_angle[p] = ang[~np.eye(len(alive), dtype=bool)].max()
        if len(alive) < o["min_track_len"]:
            removed[p] = SHORT
        elif o["min_angle_deg"] > 0 and max_angle[p] < o["min_angle_deg"]:
            removed[p] = ANGLE
    keep_pt = removed == 0
    keep_obs = (code == 0) & keep_pt[pt_of]
    stats = dict(n_obs_depth=int((code == DEPTH).sum()), n_obs_residual=int((code == RESIDUAL).sum()),
                 n_pt_short=int((removed == SHORT).sum()), n_pt_angle=int((removed == ANGLE).sum()),
                 n_obs_kept=int(keep_obs.sum()), n_pt_kept=int(keep_pt.sum()))
    return dict(residual=r, norm=norm, depth=P[:, 2], code=code, max_angle=max_angle, removed=removed,
                keep_obs=keep_obs, keep_pt=keep_pt, stats=stats)


def gap_threshold(values, target, min_gap=1e-6):
    """The midpoint of the gap wider than min_gap, between consecutive sorted
    values, whose midpoint is nearest `target`: a threshold no value is
    within min_gap / 2 of."""
    v = np.sort(np.asarray(values)[np.isfinite(values)])
    v = np.concatenate([[v[0] - 1.0], v, [v[-1] + 1.0]])
    gaps = np.diff(v)
    mids = (v[:-1] + v[1:]) / 2
    ok = gaps > min_gap
    assert ok.any()
    k = np.argmin(np.where(ok, np.abs(mids - target), np.inf))
    return float(mids[k])


def placed_opts(sc, extr, intr, X, **over):
    """Options whose thresholds sit in gaps of the reference's own values: the
    residual threshold nearest 4 px, the angle threshold nearest the median of
    the reference's max angles (at that residual threshold).  Returns (opts
    dict, the reference result with them)."""
    o = dict(default_opts(), **over)
    first = ref_wash(sc, extr, intr, X, dict(o, max_residual_px=0.0, min_angle_deg=0.0))
    o["max_residual_px"] = gap_threshold(first["norm"], 4.0)
    second = ref_wash(sc, extr, intr, X, dict(o, min_angle_deg=0.0))
    o["min_angle_deg"] = gap_threshold(second["max_angle"], float(np.median(second["max_angle"])))
    return o, ref_wash(sc, extr, intr, X, o)


def assert_not_vacuous(ref):
    s = ref["stats"]
    assert s["n_obs_residual"] >= 1 and s["n_pt_short"] >= 1 and s["n_pt_angle"] >= 1, s
    assert s["n_pt_kept"] >= 1, s


def blend(sc, alpha):
    """ground truth + alpha * (the scene's perturbed start - ground truth)"""
    return (sc.gt_extr + alpha * (sc.extr - sc.gt_extr), sc.gt_intr + alpha * (sc.intr - sc.gt_intr),
            sc.gt_X + alpha * (sc.X - sc.gt_X))


def compare(got, ref, tol=1e-9):
    """residual / max_angle to `tol`, masks and every stats field exactly"""
    with np.errstate(invalid="ignore"):
        rr, gr = ref["residual"], got["residual"]
        fin = np.isfinite(rr)
        assert (np.isfinite(gr) == fin).all()
        err_r = np.abs(gr[fin] - rr[fin]).max() if fin.any() else 0.0
    err_a = np.abs(got["max_angle"] - ref["max_angle"]).max() if len(ref["max_angle"]) else 0.0
    print(f"wash parity: residual err {err_r:.3e} px, angle err {err_a:.3e} deg, stats {got['stats']}")
    assert err_r <= tol
    assert err_a <= tol
    np.testing.assert_array_equal(got["keep_obs"], ref["keep_obs"])
    np.testing.assert_array_equal(got["keep_pt"], ref["keep_pt"])
    assert got["stats"] == ref["stats"]
