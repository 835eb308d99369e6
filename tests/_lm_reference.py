"""One Levenberg-Marquardt iteration of the bundle adjuster, computed by a
method that shares no structure with oracle/ba_oracle.cpp or the HIP solver:
the full normal equations H y = g over every parameter column, formed densely
in np.longdouble (64-bit mantissa) and solved to a backward error of 2^-60.
No Schur complement, no blocks, no bands.

Past DENSE_MAX unknowns H is not formed: the residual g - H y of the same
certificate comes from the Jacobian rows (Operator, longdouble), and y from
iterative refinement with an fp64 direct solve of a sparse fp64 copy of H as
the preconditioner (SchurFactor).  y is accepted by its residual alone,
however it was found, so the reference still shares no structure with the
code under test; test_matrix_free_reference_agrees_with_the_dense_one holds
the two paths against each other on every scene small enough for both.

What is taken from the oracle: the per-observation residual and Jacobian
(orc_ba_jacobian_model, mode 0 -- pinned to dual numbers and finite
differences by test_oracle_ba / test_snavely / test_radial3; the fp64 values
promote exactly) and the cost of a parameter set (orc_ba_cost, a plain sum).
Everything downstream -- loss correction, Jacobi scale, clamped LM diagonal,
normal equations, solve, model cost change, step norm, step quality, radius
rule, gradient norm -- is restated here from the definitions in the header of
ba_oracle.cpp.
"""
import ctypes as C
import math

import numpy as np
import scipy.linalg as sl
import scipy.sparse as sp
import scipy.sparse.linalg as spl

import _helpers as H

abi = H.abi
LD = np.longdouble

LONGDOUBLE_OK = np.finfo(LD).nmant >= 63
SKIP_REASON = (f"np.longdouble has a {np.finfo(LD).nmant}-bit mantissa here; the LM reference needs "
               "the 64-bit mantissa of the x87 extended format (nmant >= 63)")
BACKWARD_ERROR_MAX = 2.0 ** -60
U = 2.0 ** -53
DENSE_MAX = 2500    # unknowns up to which H is formed densely in longdouble; past it the matrix-free path


def pack(params):
    """(extr, intr, X) -> one flat fp64 vector."""
    return np.concatenate([np.asarray(a, np.float64).reshape(-1) for a in params])


def unpack(scene, p):
    ne, ni = len(scene.extr), len(scene.intr)
    return p[:ne].copy(), p[ne:ne + ni].copy(), p[ne + ni:].copy()


class Layout:
    """The parameter columns of a scene: 6 per observed non-gauge camera, the
    model's width per observed intrinsics block (3 for SNAVELY: the 4th double
    is not a parameter), 3 per point.  `cols` indexes pack(params); `idx[o]`
    maps the oracle's Jacobian row layout (intrinsics | extr | X) of
    observation o to columns, with n (one dummy column) where the Jacobian
    entry belongs to no parameter."""

    def __init__(self, sc):
        iw = 6 if sc.model == abi.SFM_CAM_RADIAL3 else 4
        iwp = 3 if sc.model == abi.SFM_CAM_SNAVELY else iw
        ne, ni = 6 * sc.n_cam, iw * sc.n_intr
        assert len(sc.extr) == ne and len(sc.intr) == ni and len(sc.X) == 3 * sc.n_pt
        obs_img = np.asarray(sc.obs_img[:sc.n_obs], np.int64)
        obs_pt = np.repeat(np.arange(sc.n_pt), np.diff(sc.pt_offsets))
        cam_used = np.zeros(sc.n_cam, bool)
        cam_used[obs_img] = True
        intr_used = np.zeros(sc.n_intr, bool)
        intr_used[sc.img_intr[obs_img]] = True
        where = np.full(ne + ni + 3 * sc.n_pt, -1, np.int64)    # flat parameter -> column
        cols = []
        for i in range(sc.n_cam):
            if cam_used[i] and i != sc.const_img:
                cols.extend(range(6 * i, 6 * i + 6))
        for q in range(sc.n_intr):
            if intr_used[q]:
                cols.extend(range(ne + iw * q, ne + iw * q + iwp))
        cols.extend(range(ne + ni, ne + ni + 3 * sc.n_pt))
        self.cols = np.array(cols, np.int64)
        self.n = n = len(cols)
        where[self.cols] = np.arange(n)
        flat = np.concatenate([ne + iw * sc.img_intr[obs_img][:, None] + np.arange(iw)[None, :],
                               6 * obs_img[:, None] + np.arange(6)[None, :],
                               ne + ni + 3 * obs_pt[:, None] + np.arange(3)[None, :]], axis=1)
        idx = where[flat]
        idx[idx < 0] = n
        self.idx = idx
        self.iw, self.w = iw, iw + 9
        self.obs_img, self.obs_pt = obs_img, obs_pt
        self.free = np.ones(len(where), bool)
        self.free[self.cols] = False    # flat entries that are no parameter: never moved


def _key(sc, *parts):
    return (id(sc),) + tuple(a.tobytes() if isinstance(a, np.ndarray) else a for a in parts)


_layouts, _lin, _steps = {}, {}, {}


def layout(sc):
    if id(sc) not in _layouts:
        _layouts[id(sc)] = (sc, Layout(sc))     # (the scene is kept alive: its id stays its own)
    return _layouts[id(sc)][1]


def linearize(sc, p):
    """Loss-corrected residuals f [n_obs, 2] and Jacobian rows Jc [n_obs, 2, w]
    in longdouble at the flat parameters p, the unscaled gradient g = Jc' f over
    the columns, and the Huber branch counts."""
    key = _key(sc, p)
    if key in _lin:
        return _lin[key]
    assert LONGDOUBLE_OK, SKIP_REASON
    lay = layout(sc)
    lib = H.oracle()
    e, i, x = unpack(sc, p)
    uv = np.ascontiguousarray(sc.obs_uv, np.float64)
    r = np.zeros((sc.n_obs, 2))
    J = np.zeros((sc.n_obs, 2, lay.w))
    f64 = C.sizeof(C.c_double)
    pe, pi, px, puv, pr, pj = (a.ctypes.data for a in (e, i, x, uv, r, J))
    cast = lambda addr: C.cast(addr, abi.f64p)   # noqa: E731
    for o in range(sc.n_obs):
        img = int(lay.obs_img[o])
        rc = lib.orc_ba_jacobian_model(sc.model, 0, cast(pi + f64 * lay.iw * int(sc.img_intr[img])),
                                       cast(pe + f64 * 6 * img), cast(px + f64 * 3 * int(lay.obs_pt[o])),
                                       cast(puv + f64 * 2 * o), cast(pr + f64 * 2 * o),
                                       cast(pj + f64 * 2 * lay.w * o))
        assert rc == 0
    r, J = r.astype(LD), J.astype(LD)
    # rho(s) = s (s <= a^2), 2 a sqrt(s) - a^2 otherwise; r and J scaled by sqrt(rho'(s))
    s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
    a = LD(sc.huber)
    outer = (s > a * a) if sc.huber > 0 else np.zeros(len(s), bool)
    wgt = np.ones(len(s), LD)
    wgt[outer] = np.sqrt(a / np.sqrt(s[outer]))
    f = r * wgt[:, None]
    Jc = J * wgt[:, None, None]
    g = np.zeros(lay.n + 1, LD)
    np.add.at(g, lay.idx, Jc[:, 0, :] * f[:, 0, None] + Jc[:, 1, :] * f[:, 1, None])
    out = dict(f=f, Jc=Jc, g=g[:lay.n], n_inner=int((~outer).sum()), n_outer=int(outer.sum()))
    if len(_lin) > 8:       # a few points stay hot (x0 of each scene in use); the rest is recomputed
        _lin.pop(next(iter(_lin)))
    _lin[key] = out
    return out


def colnorm2(lay, Jrows):
    cn = np.zeros(lay.n + 1, LD)
    np.add.at(cn, lay.idx, Jrows[:, 0, :] * Jrows[:, 0, :] + Jrows[:, 1, :] * Jrows[:, 1, :])
    return cn[:lay.n]


def jacobi_scale(sc, p0, opts):
    """1 / (1 + sqrt(|J col|^2)) of the corrected Jacobian at p0; 1 without scaling."""
    lay = layout(sc)
    if not opts.jacobi_scaling:
        return np.ones(lay.n, LD)
    return 1 / (1 + np.sqrt(colnorm2(lay, linearize(sc, p0)["Jc"])))


def gradient_max_norm(sc, p):
    """|x - (x - g)|_inf in fp64 with the longdouble gradient at p, max|g| and max|x| over the columns."""
    lay = layout(sc)
    g = linearize(sc, p)["g"].astype(np.float64)
    x = p[lay.cols]
    return float(np.abs(x - (x - g)).max()), float(np.abs(g).max()), float(np.abs(x).max())


def cost(sc, p):
    return H.oracle_cost(sc, *unpack(sc, p))


def _solve(Hm, g):
    """H y = g: fp64 Cholesky factor, iterative refinement on longdouble
    residuals until the normwise backward error is <= 2^-60 (asserted)."""
    H64 = Hm.astype(np.float64)
    Li = np.linalg.inv(np.linalg.cholesky(H64))
    hn, gn = np.abs(Hm).sum(axis=1).max(), np.abs(g).max()
    y = np.zeros(len(g), LD)
    be = np.inf
    for _ in range(12):
        res = g - Hm @ y
        be = float(np.abs(res).max() / (hn * np.abs(y).max() + gn))
        if be <= BACKWARD_ERROR_MAX / 4:
            break
        y = y + (Li.T @ (Li @ res.astype(np.float64))).astype(LD)
    assert be <= BACKWARD_ERROR_MAX, f"reference solve: backward error 2^{math.log2(be):.1f} > 2^-60"
    return y, be, H64


def scaled_rows(sc, x0, x, radius, opts):
    """(J_s rows, f, scale, colnorm^2 of J_s, clamp(colnorm^2) / radius, g = J_s' f) at x, in longdouble."""
    lay = layout(sc)
    n = lay.n
    lin = linearize(sc, x)
    scale = jacobi_scale(sc, x0, opts)
    sx = np.concatenate([scale, [LD(0)]])
    Js = lin["Jc"] * sx[lay.idx][:, None, :]
    f = lin["f"]
    cn = colnorm2(lay, Js)
    diag = np.clip(cn, LD(opts.min_lm_diagonal), LD(opts.max_lm_diagonal)) / LD(radius)
    g = np.zeros(n + 1, LD)
    np.add.at(g, lay.idx, Js[:, 0, :] * f[:, 0, None] + Js[:, 1, :] * f[:, 1, None])
    return Js, f, scale, cn, diag, g[:n]


def normal_equations(sc, x0, x, radius, opts):
    """(H, g, J_s rows, f, scale, colnorm^2 of J_s) at x: H = J_s' J_s + clamp(colnorm^2) / radius
    accumulated observation by observation in longdouble, g = J_s' f."""
    lay = layout(sc)
    n = lay.n
    assert n <= DENSE_MAX
    Js, f, scale, cn, diag, g = scaled_rows(sc, x0, x, radius, opts)
    Hm = np.zeros((n + 1, n + 1), LD)
    np.add.at(Hm, (lay.idx[:, :, None], lay.idx[:, None, :]),
              Js[:, 0, :, None] * Js[:, 0, None, :] + Js[:, 1, :, None] * Js[:, 1, None, :])
    Hm = Hm[:n, :n]
    Hm[np.arange(n), np.arange(n)] += diag
    return Hm, g, Js, f, scale, cn


class Operator:
    """y -> H y = J_s' (J_s y) + (clamp(colnorm^2) / radius) y in longdouble, straight from the Jacobian rows
    (gather by lay.idx, scatter by np.add.at): H is never formed, so the layout may be of any size.  This is
    the residual of the certificate.  |H|_inf, the certificate's scale, and the preconditioner come from a
    sparse fp64 copy of H (J' J of the fp64 rows: every observation couples its own 9 + iw columns only)."""

    def __init__(self, lay, Js, diag):
        self.lay, self.Js, self.diag, self.n = lay, Js, diag, lay.n
        self._h64 = None

    def __call__(self, y):
        lay, Js = self.lay, self.Js
        s = np.concatenate([y, [LD(0)]])
        m = (Js * s[lay.idx][:, None, :]).sum(axis=2)
        out = np.zeros(self.n + 1, LD)
        np.add.at(out, lay.idx, Js[:, 0, :] * m[:, 0, None] + Js[:, 1, :] * m[:, 1, None])
        return out[:self.n] + self.diag * y

    def h64(self):
        """H rounded to fp64 row by row, sparse (CSR)."""
        if self._h64 is None:
            n, (no, _, w) = self.n, self.Js.shape
            rows = np.repeat(np.arange(2 * no), w)
            cols = np.repeat(self.lay.idx[:, None, :], 2, axis=1).reshape(-1)
            J = sp.csr_matrix((self.Js.astype(np.float64).reshape(-1), (rows, cols)), shape=(2 * no, n + 1))[:, :n]
            self._h64 = (J.T @ J + sp.diags(self.diag.astype(np.float64))).tocsr()
        return self._h64

    def norm_inf(self):
        return float(abs(self.h64()).sum(axis=1).max())

    def backward_error(self, y, g):
        """|g - H y|_inf / (|H|_inf |y|_inf + |g|_inf), the residual in longdouble."""
        return float(np.abs(g - self(y)).max() / (LD(self.norm_inf()) * np.abs(y).max() + np.abs(g).max()))


class SchurFactor:
    """An fp64 direct solve with the sparse fp64 H, used as a preconditioner only: the 3 x 3 point blocks (the
    trailing n_e columns; the layout puts the points last) eliminated, the reduced system dense, factored by
    scipy.linalg.cho_factor.  Whatever it returns only speeds the refinement up or slows it down: y is
    accepted by the longdouble residual alone."""

    def __init__(self, H64, n_e):
        n = H64.shape[0]
        nf = n - n_e
        coo = H64[nf:, nf:].tocoo()
        assert np.array_equal(coo.row // 3, coo.col // 3), "the point block of H is block diagonal"
        V = np.zeros((n_e // 3, 3, 3))
        V[coo.row // 3, coo.row % 3, coo.col % 3] = coo.data
        k = np.arange(n_e // 3)
        self.Vi = sp.bsr_matrix((np.linalg.inv(V), k, np.arange(n_e // 3 + 1)), shape=(n_e, n_e)).tocsr()
        self.W = H64[:nf, nf:].tocsr()
        S = (H64[:nf, :nf] - self.W @ self.Vi @ self.W.T).toarray()
        self.cf = sl.cho_factor(S, lower=True, overwrite_a=True, check_finite=False)
        self.nf = nf

    def __call__(self, r):
        rf, re = r[:self.nf], r[self.nf:]
        yf = sl.cho_solve(self.cf, rf - self.W @ (self.Vi @ re), check_finite=False)
        return np.concatenate([yf, self.Vi @ (re - self.W.T @ yf)])


def solve_matrix_free(op, g, n_e):
    """H y = g for an Operator: SchurFactor as the preconditioner, iterative refinement on longdouble
    residuals until the normwise backward error is <= 2^-60 (asserted, as _solve does); kappa = lambda_max /
    lambda_min of the fp64 H by Lanczos (eigsh: the largest directly, the smallest in shift-invert mode
    about 0 with the factor as the inverse).  Returns (y, backward error, kappa)."""
    H64 = op.h64()
    pre = SchurFactor(H64, n_e)
    hn, gn = LD(op.norm_inf()), np.abs(g).max()
    y = np.zeros(len(g), LD)
    be = np.inf
    for _ in range(12):
        res = g - op(y)
        be = float(np.abs(res).max() / (hn * np.abs(y).max() + gn))
        if be <= BACKWARD_ERROR_MAX / 4:
            break
        y = y + pre(res.astype(np.float64)).astype(LD)
    assert be <= BACKWARD_ERROR_MAX, f"reference solve: backward error 2^{math.log2(be):.1f} > 2^-60"
    n = len(g)
    A = spl.LinearOperator((n, n), matvec=lambda v: H64 @ v, dtype=np.float64)
    v0 = np.ones(n)
    top = spl.eigsh(A, k=1, which="LA", v0=v0, tol=1e-9, return_eigenvectors=False)[0]
    low = spl.eigsh(A, k=1, sigma=0.0, which="LM", v0=v0, tol=1e-9, return_eigenvectors=False,
                    OPinv=spl.LinearOperator((n, n), matvec=pre, dtype=np.float64))[0]
    return y, be, float(top / low)


def gradient_classes(sc, p):
    """max|g| (unscaled gradient at p) over the camera, intrinsics and point columns, and the class of the largest."""
    lay = layout(sc)
    g = np.abs(linearize(sc, p)["g"].astype(np.float64))
    ne, ni = len(sc.extr), len(sc.intr)
    cls = np.where(lay.cols < ne, 0, np.where(lay.cols < ne + ni, 1, 2))
    mx = [float(g[cls == k].max()) if (cls == k).any() else 0.0 for k in range(3)]
    return ("cam", "intr", "pt")[int(np.argmax(mx))], mx


def lm_step(sc, x0, x, radius, opts, decrease_factor=2.0):
    """One LM iteration from the flat parameters x at trust-region radius
    `radius`; x0 fixes the Jacobi scale.  decrease_factor: 2^(1 + number of
    rejected steps directly before this one)."""
    key = _key(sc, x0, x, float(radius), float(decrease_factor), bytes(opts))
    if key in _steps:
        return _steps[key]
    lay = layout(sc)
    lin = linearize(sc, x)
    if lay.n <= DENSE_MAX:
        Hm, g, Js, f, scale, _ = normal_equations(sc, x0, x, radius, opts)
        y, be, H64 = _solve(Hm, g)
        ev = np.linalg.eigvalsh(H64)    # H is symmetric positive definite: cond_2 = lambda_max / lambda_min
        cond = float(ev[-1] / ev[0])
    else:
        Js, f, scale, _, diag, g = scaled_rows(sc, x0, x, radius, opts)
        y, be, cond = solve_matrix_free(Operator(lay, Js, diag), g, 3 * sc.n_pt)
    s = np.concatenate([-y, [LD(0)]])
    m = (Js * s[lay.idx][:, None, :]).sum(axis=2)               # J_s s per residual row
    model_cost_change = -(m * (f + m / 2)).sum()
    delta = -scale * y
    cand = x.copy()
    cand[lay.cols] = (x[lay.cols].astype(LD) + delta).astype(np.float64)
    x_cost, cand_cost = cost(sc, x), cost(sc, cand)
    out = dict(y=y, scale=scale, delta=delta, cond=cond, backward_error=be, g_scaled=g,
               model_cost_change=float(model_cost_change), step_is_valid=bool(model_cost_change > 0),
               x_cost=x_cost, candidate_cost=cand_cost, candidate=cand,
               step_norm=float(np.sqrt((delta * delta).sum())), cost_change=x_cost - cand_cost,
               n_inner=lin["n_inner"], n_outer=lin["n_outer"])
    out["relative_decrease"] = rd = out["cost_change"] / out["model_cost_change"]
    out["step_is_successful"] = ok = bool(out["step_is_valid"] and rd > opts.min_relative_decrease)
    out["trust_region_radius"] = next_radius(radius, rd, ok, decrease_factor, opts)
    out["gradient_max_norm"] = gradient_max_norm(sc, x)[0]
    out["gradient_max_norm_new"] = gradient_max_norm(sc, cand)[0] if ok else out["gradient_max_norm"]
    _steps[key] = out
    return out


def next_radius(radius, relative_decrease, accepted, decrease_factor, opts):
    """The accept / reject radius rule, in fp64 as both implementations run it."""
    if accepted:
        return min(opts.max_trust_region_radius,
                   radius / max(1.0 / 3.0, 1.0 - math.pow(2.0 * relative_decrease - 1.0, 3)))
    return radius / decrease_factor
