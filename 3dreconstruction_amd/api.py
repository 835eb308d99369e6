"""Thin numpy wrappers over libsfmcore.so (ctypes) for tests and bench.py.

Every call goes through the C-ABI in include/sfmcore.h; there is no Python
compute path and no fallback: if the library or a gfx950 device is missing,
these raise.
"""
import ctypes as C

import numpy as np

from . import _abi as abi


class SfmError(RuntimeError):
    def __init__(self, code, where):
        lib = abi.load()
        msg = lib.sfm_last_error().decode(errors="replace")
        super().__init__(f"{where} failed with {code}: {msg}")
        self.code = code


def _check(rc, where):
    if rc != abi.SFM_OK:
        raise SfmError(rc, where)


class Context:
    """sfm_ctx: one HIP device (+ RCCL communicator when world_size > 1).

    allreduce: optional callable (numpy float64 array, op) -> None reducing the
    array in place across ranks (op 0 sum, 1 max); replaces RCCL, e.g. with a
    torch.distributed gloo group."""

    def __init__(self, device=0, rank=0, world_size=1, comm_id=None, allreduce=None, flags=0):
        self.lib = abi.load()
        o = abi.CtxOpts()
        o.device, o.rank, o.world_size, o.flags = device, rank, world_size, flags
        self._id = None
        self._hook = None
        if comm_id is not None:
            self._id = (C.c_uint8 * 128).from_buffer_copy(bytes(comm_id))
            o.comm_id = C.cast(self._id, abi.u8p)
        if allreduce is not None:
            import numpy as np

            def hook(user, buf, n, op):
                try:
                    allreduce(np.ctypeslib.as_array(buf, shape=(n,)), int(op))
                    return 0
                except Exception:
                    return -1

            self._hook = abi.ALLREDUCE_HOOK(hook)
            o.allreduce = C.cast(self._hook, C.c_void_p)
        h = C.c_void_p()
        _check(self.lib.sfm_ctx_create(C.byref(o), C.byref(h)), "sfm_ctx_create")
        self.h = h
        self._children = []

    def _adopt(self, child):
        import weakref
        self._children.append(weakref.ref(child))

    def synchronize(self):
        _check(self.lib.sfm_ctx_synchronize(self.h), "sfm_ctx_synchronize")

    def close(self):
        if self.h:
            for r in self._children:  # plans must die before their context
                c = r()
                if c is not None:
                    c.close()
            self.lib.sfm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def comm_unique_id():
    lib = abi.load()
    buf = (C.c_uint8 * 128)()
    _check(lib.sfm_comm_unique_id(buf), "sfm_comm_unique_id")
    return bytes(buf)


# descriptor dtype -> (C suffix, descriptor pointer, distance dtype, distance pointer)
_MATCH_KINDS = {np.uint8: ("", abi.u8p, np.int32, abi.i32p),
                np.float32: ("_f32", abi.f32p, np.float32, abi.f32p)}


def _match_dense(ctx, a, b, mode, ratio, dtype):
    sfx, dp, dist, distp = _MATCH_KINDS[dtype]
    a = np.ascontiguousarray(a, dtype).reshape(-1, 128)
    b = np.ascontiguousarray(b, dtype).reshape(-1, 128)
    n_out = len(a) if mode == abi.SFM_MATCH_MUTUAL else len(b)
    idx = np.zeros(max(n_out, 1), np.int32)
    d2 = np.zeros(max(n_out, 1), dist)
    o = abi.MatchOptions(mode, ratio)
    name = "sfm_match_dense" + sfx
    _check(getattr(ctx.lib, name)(ctx.h, abi.ptr(a, dp), len(a), abi.ptr(b, dp), len(b), C.byref(o),
                                  abi.ptr(idx, abi.i32p), abi.ptr(d2, distp)), name)
    return idx[:n_out], d2[:n_out]


def match_dense(ctx, a, b, mode=abi.SFM_MATCH_RATIO, ratio=0.8):
    return _match_dense(ctx, a, b, mode, ratio, np.uint8)


def match_dense_f32(ctx, a, b, mode=abi.SFM_MATCH_RATIO, ratio=0.8):
    """sfm_match_dense_f32: float descriptors (cv::Mat CV_32F); returns
    (idx, squared distance as float32, -1 where unmatched)."""
    return _match_dense(ctx, a, b, mode, ratio, np.float32)


class MatchPlan:
    """Resident descriptor collection for all-pairs matching (uint8, or float32
    through sfm_match_plan_create_f32: fetch() then returns float distances)."""

    def __init__(self, ctx, desc, offsets):
        self.ctx = ctx
        self.f32 = np.asarray(desc).dtype == np.float32
        self._sfx, dp, self._dist, self._distp = _MATCH_KINDS[np.float32 if self.f32 else np.uint8]
        desc = np.ascontiguousarray(desc, np.float32 if self.f32 else np.uint8).reshape(-1, 128)
        offsets = np.ascontiguousarray(offsets, np.int64)
        self.n_img = len(offsets) - 1
        h = C.c_void_p()
        name = "sfm_match_plan_create" + self._sfx
        _check(getattr(ctx.lib, name)(ctx.h, abi.ptr(desc, dp), abi.ptr(offsets, abi.i64p), self.n_img,
                                      C.byref(h)), name)
        self.h = h
        self.n_pairs = 0
        ctx._adopt(self)

    def run(self, pairs, mode=abi.SFM_MATCH_RATIO, ratio=0.8, count=True):
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self.n_pairs = len(pairs)
        o = abi.MatchOptions(mode, ratio)
        tot = C.c_int64()
        _check(self.ctx.lib.sfm_match_plan_run(self.h, abi.ptr(pairs, abi.i32p), len(pairs),
                                               C.byref(o), C.byref(tot) if count else None),
               "sfm_match_plan_run")
        return tot.value if count else None

    def fetch(self):
        name = "sfm_match_plan_fetch" + self._sfx
        fetch = getattr(self.ctx.lib, name)
        counts = np.zeros(max(self.n_pairs, 1), np.int64)
        _check(fetch(self.h, abi.ptr(counts, abi.i64p), None, None, None), name)
        counts = counts[:self.n_pairs]
        tot = int(counts.sum())
        i = np.zeros(max(tot, 1), np.uint32)
        j = np.zeros(max(tot, 1), np.uint32)
        d = np.zeros(max(tot, 1), self._dist)
        _check(fetch(self.h, abi.ptr(counts, abi.i64p), abi.ptr(i, abi.u32p), abi.ptr(j, abi.u32p),
                     abi.ptr(d, self._distp)), name)
        return counts, i[:tot], j[:tot], d[:tot]

    def cascade_index(self, pairs):
        """Hash tables for the images of `pairs` (SFM_MATCH_CASCADE); later
        cascade runs over any part of that list reuse them."""
        pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        _check(self.ctx.lib.sfm_match_plan_cascade_index(self.h, abi.ptr(pairs, abi.i32p),
                                                         len(pairs)), "sfm_match_plan_cascade_index")

    def digest(self):
        v = C.c_uint64()
        _check(self.ctx.lib.sfm_match_plan_digest(self.h, C.byref(v)), "sfm_match_plan_digest")
        return v.value

    def last_ms(self):
        ms = C.c_double()
        n = C.c_int64()
        _check(self.ctx.lib.sfm_match_plan_get_last_ms(self.h, C.byref(ms), C.byref(n)),
               "sfm_match_plan_get_last_ms")
        return ms.value, n.value

    def close(self):
        if self.h:
            self.ctx.lib.sfm_match_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _mix64(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def match_digest(counts, i, j, d):
    """Host restatement of the device digest (order-independent)."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    key = (np.asarray(i[:n], np.uint64) << np.uint64(32)) | np.asarray(j[:n], np.uint64)
    m = _mix64(key ^ (np.asarray(d[:n]).astype(np.uint32).astype(np.uint64) << np.uint64(21)))
    # per-pair sums modulo 2^64 (an empty pair sums to 0)
    h = np.zeros(len(counts), np.uint64)
    np.add.at(h, np.repeat(np.arange(len(counts)), counts), m)
    with np.errstate(over="ignore"):
        pair_id = np.arange(1, len(counts) + 1, dtype=np.uint64)
        return int(_mix64(h + np.uint64(0x9E3779B97F4A7C15) * pair_id).sum(dtype=np.uint64))


def exhaustive_pairs(n):
    lib = abi.load()
    m = n * (n - 1) // 2
    out = np.zeros(max(2 * m, 2), np.int32)
    _check(lib.sfm_exhaustive_pairs(n, abi.ptr(out, abi.i32p)), "sfm_exhaustive_pairs")
    return out[:2 * m].reshape(-1, 2)


def synth_descriptors(n_img, n_kp, seed=0xC3):
    lib = abi.load()
    d = np.zeros(max(n_img * n_kp * 128, 1), np.uint8)
    _check(lib.sfm_synth_descriptors(n_img, n_kp, seed, abi.ptr(d, abi.u8p)),
           "sfm_synth_descriptors")
    return d[:n_img * n_kp * 128].reshape(-1, 128)


def ba_describe(problem, rank=0, world=1):
    """[cpu] The planner's structure for a problem (sfm_ba_describe)."""
    lib = abi.load()
    out = abi.BAPlanShape()
    _check(lib.sfm_ba_describe(C.byref(problem), rank, world, C.byref(out)), "sfm_ba_describe")
    return out


def ba_grown_digest(prev, problem):
    """[cpu] (fresh digest, grown digest, reused sorted points) of `problem`
    planned from scratch and grown from `prev`'s plan (sfm_ba_grown_digest)."""
    lib = abi.load()
    df, dg, r = C.c_uint64(), C.c_uint64(), C.c_int64()
    _check(lib.sfm_ba_grown_digest(C.byref(prev), C.byref(problem), C.byref(df), C.byref(dg), C.byref(r)),
           "sfm_ba_grown_digest")
    return df.value, dg.value, r.value


def ba_dense_schedule(problem):
    """[cpu] The dense dataflow solve's schedule for `problem`
    (sfm_ba_dense_schedule): (shape dict, int32 array); the array is empty
    when the dataflow solve does not run."""
    lib = abi.load()
    n = C.c_int64()
    shape = np.zeros(7, np.int32)
    _check(lib.sfm_ba_dense_schedule(C.byref(problem), None, 0, C.byref(n), shape.ctypes.data_as(abi.i32p)),
           "sfm_ba_dense_schedule")
    meta = np.zeros(max(n.value, 1), np.int32)
    _check(lib.sfm_ba_dense_schedule(C.byref(problem), meta.ctypes.data_as(abi.i32p), n.value, C.byref(n),
                                     shape.ctypes.data_as(abi.i32p)), "sfm_ba_dense_schedule")
    keys = ("nt", "chains", "tasks", "flow", "nF", "nb", "D")
    return dict(zip(keys, (int(v) for v in shape))), meta[:n.value]


class BAPlan:
    """Resident BA problem (sfm_ba_plan): upload once, run many times."""

    def __init__(self, ctx, problem, extr, intr, X):
        self.ctx = ctx
        self._keep = (problem, extr, intr, X)
        h = C.c_void_p()
        _check(ctx.lib.sfm_ba_plan_create(ctx.h, C.byref(problem), abi.ptr(extr, abi.f64p),
                                          abi.ptr(intr, abi.f64p), abi.ptr(X, abi.f64p),
                                          C.byref(h)), "sfm_ba_plan_create")
        self.h = h
        self.shape = (len(extr), len(intr), len(X))
        ctx._adopt(self)

    def run(self, opts=None, check=True):
        o = opts or abi.default_options()
        s = abi.BASummary()
        rc = self.ctx.lib.sfm_ba_plan_run(self.h, C.byref(o), C.byref(s))
        if check and rc not in (abi.SFM_OK, abi.SFM_ERR_SOLVER):
            _check(rc, "sfm_ba_plan_run")
        return rc, s

    def download(self):
        e, i, x = (np.zeros(n) for n in self.shape)
        _check(self.ctx.lib.sfm_ba_plan_download(self.h, abi.ptr(e, abi.f64p), abi.ptr(i, abi.f64p),
                                                 abi.ptr(x, abi.f64p)), "sfm_ba_plan_download")
        return e, i, x

    def wash(self, opts=None):
        """sfm_ba_plan_wash at the plan's current parameters: dict(residual
        [n_obs, 2], max_angle [n_pt], keep_obs, keep_pt (bool), stats), in the
        problem's own order."""
        pr = self._keep[0]
        out = _wash_outputs(pr.n_obs, pr.n_pt)
        st = abi.BAWashStats()
        _check(self.ctx.lib.sfm_ba_plan_wash(self.h, C.byref(opts) if opts is not None else None,
                                             *_wash_ptrs(out), C.byref(st)), "sfm_ba_plan_wash")
        return _wash_result(out, st)

    def wash_last_ms(self):
        """(observation pass, point pass) device ms of the last wash(); -1
        unless the context was created with SFM_CTX_TIME_KERNELS."""
        a, b = C.c_double(), C.c_double()
        _check(self.ctx.lib.sfm_ba_plan_wash_last_ms(self.h, C.byref(a), C.byref(b)),
               "sfm_ba_plan_wash_last_ms")
        return a.value, b.value

    def info(self):
        inf = abi.BAPlanInfo()
        _check(self.ctx.lib.sfm_ba_plan_get_info(self.h, C.byref(inf)), "sfm_ba_plan_get_info")
        return inf

    def trace(self, cap=256):
        tr = (abi.BAIter * cap)()
        n = C.c_int32()
        _check(self.ctx.lib.sfm_ba_plan_get_trace(self.h, tr, cap, C.byref(n)),
               "sfm_ba_plan_get_trace")
        return [tr[k] for k in range(n.value)]

    def close(self):
        if self.h:
            self.ctx.lib.sfm_ba_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ba_solve(ctx, problem, extr, intr, X, opts=None):
    """sfm_ba_solve: in-place update of extr/intr/X when the solution is usable."""
    o = opts or abi.default_options()
    s = abi.BASummary()
    rc = ctx.lib.sfm_ba_solve(ctx.h, C.byref(problem), abi.ptr(extr, abi.f64p),
                              abi.ptr(intr, abi.f64p), abi.ptr(X, abi.f64p), C.byref(o),
                              C.byref(s))
    return rc, s


def ba_wash_default_options():
    o = abi.BAWashOpts()
    abi.load().sfm_ba_wash_default_options(C.byref(o))
    return o


def _wash_outputs(n_obs, n_pt):
    return (np.zeros(2 * max(n_obs, 1)), np.zeros(max(n_pt, 1)), np.zeros(max(n_obs, 1), np.uint8),
            np.zeros(max(n_pt, 1), np.uint8), n_obs, n_pt)


def _wash_ptrs(out):
    r, a, ko, kp = out[:4]
    return abi.ptr(r, abi.f64p), abi.ptr(a, abi.f64p), abi.ptr(ko, abi.u8p), abi.ptr(kp, abi.u8p)


def _wash_result(out, st):
    r, a, ko, kp, n_obs, n_pt = out
    return dict(residual=r[:2 * n_obs].reshape(-1, 2), max_angle=a[:n_pt], keep_obs=ko[:n_obs].astype(bool),
                keep_pt=kp[:n_pt].astype(bool), stats={f: getattr(st, f) for f, _ in abi.BAWashStats._fields_})


def ba_wash(ctx, problem, extr, intr, X, opts=None):
    """sfm_ba_wash (post-BA outlier rejection) at (extr, intr, X):
    dict(residual [n_obs, 2], max_angle [n_pt] in degrees, keep_obs, keep_pt
    (bool), stats), in the problem's own order.  opts: BAWashOpts (None: the
    defaults, ba_wash_default_options())."""
    out = _wash_outputs(problem.n_obs, problem.n_pt)
    st = abi.BAWashStats()
    _check(ctx.lib.sfm_ba_wash(ctx.h, C.byref(problem), abi.ptr(extr, abi.f64p), abi.ptr(intr, abi.f64p),
                               abi.ptr(X, abi.f64p), C.byref(opts) if opts is not None else None,
                               *_wash_ptrs(out), C.byref(st)), "sfm_ba_wash")
    return _wash_result(out, st)


def ba_wash_apply(problem, X, keep_obs, keep_pt):
    """[cpu] sfm_ba_wash_apply: (washed BAProblem, X of its points, pt_map).
    The new problem keeps its arrays alive and shares img_intr with `problem`,
    which has to outlive it."""
    lib = abi.load()
    ko = np.ascontiguousarray(keep_obs, np.uint8)
    kp = np.ascontiguousarray(keep_pt, np.uint8)
    X = np.ascontiguousarray(X, np.float64)
    if len(ko) != problem.n_obs or len(kp) != problem.n_pt or len(X) != 3 * problem.n_pt:
        raise ValueError("ba_wash_apply: mask / X sizes do not match the problem")
    # the sizes the wash's stats give (the library writes the kept observations of kept points only,
    # and rejects a kept observation of a removed point)
    n_pt = int(np.count_nonzero(kp))
    n_obs = int(np.count_nonzero(ko))
    off = np.zeros(n_pt + 1, np.int64)
    img = np.zeros(max(n_obs, 1), np.int32)
    uv = np.zeros(2 * max(n_obs, 1))
    Xo = np.zeros(3 * max(n_pt, 1))
    pm = np.zeros(max(n_pt, 1), np.int64)
    _check(lib.sfm_ba_wash_apply(C.byref(problem), abi.ptr(X, abi.f64p), abi.ptr(ko, abi.u8p), abi.ptr(kp, abi.u8p),
                                 abi.ptr(off, abi.i64p), abi.ptr(img, abi.i32p), abi.ptr(uv, abi.f64p),
                                 abi.ptr(Xo, abi.f64p), abi.ptr(pm, abi.i64p)), "sfm_ba_wash_apply")
    pr = abi.BAProblem()
    pr.n_img, pr.n_intr, pr.n_pt, pr.n_obs = problem.n_img, problem.n_intr, n_pt, n_obs
    pr.pt_offsets = abi.ptr(off, abi.i64p)
    pr.obs_img = abi.ptr(img, abi.i32p)
    pr.obs_uv = abi.ptr(uv, abi.f64p)
    pr.img_intr = problem.img_intr
    pr.const_img, pr.camera_model, pr.huber_a = problem.const_img, problem.camera_model, problem.huber_a
    pr._keep = (off, img, uv, problem)
    return pr, Xo[:3 * n_pt], pm[:n_pt]


def tri_default_options():
    o = abi.TriOpts()
    abi.load().sfm_tri_default_options(C.byref(o))
    return o


def triangulate(ctx, problem, extr, intr, opts=None):
    """sfm_triangulate (ctx None: sfm_triangulate_host, on the CPU): every point
    of `problem` from its track and the cameras (extr, intr).  dict(X [n_pt, 3]
    (NaN where the point is not OK), status [n_pt] (SFM_TRI_*), keep_obs [n_obs]
    (bool), residual [n_obs, 2], stats), in the problem's own order.  opts:
    TriOpts (None: the defaults, tri_default_options())."""
    n_pt, n_obs = problem.n_pt, problem.n_obs
    X = np.zeros(3 * max(n_pt, 1))
    st = np.zeros(max(n_pt, 1), np.uint8)
    ko = np.zeros(max(n_obs, 1), np.uint8)
    r = np.zeros(2 * max(n_obs, 1))
    stats = abi.TriStats()
    args = (C.byref(problem), abi.ptr(extr, abi.f64p), abi.ptr(intr, abi.f64p),
            C.byref(opts) if opts is not None else None, abi.ptr(X, abi.f64p), abi.ptr(st, abi.u8p),
            abi.ptr(ko, abi.u8p), abi.ptr(r, abi.f64p), C.byref(stats))
    if ctx is None:
        _check(abi.load().sfm_triangulate_host(*args), "sfm_triangulate_host")
    else:
        _check(ctx.lib.sfm_triangulate(ctx.h, *args), "sfm_triangulate")
    return dict(X=X[:3 * n_pt].reshape(-1, 3), status=st[:n_pt], keep_obs=ko[:n_obs].astype(bool),
                residual=r[:2 * n_obs].reshape(-1, 2),
                stats={f: getattr(stats, f) for f, _ in abi.TriStats._fields_})


def resect_default_options():
    o = abi.ResectOpts()
    abi.load().sfm_resect_default_options(C.byref(o))
    return o


def resect(ctx, camera_model, X_list, uv_list, img_intr, intr, wh, opts=None):
    """sfm_resect (ctx None: sfm_resect_host, on the CPU) over a list of images:
    X_list[q] (n_q, 3) world points and uv_list[q] (n_q, 2) pixels, img_intr[q]
    the image's block of intr, wh[q] = (w, h).  One dict per image: pose,
    pose_model (angle-axis, t), error_max, min_nfa, n_inliers, iterations,
    status (SFM_RESECT_*), inliers.  opts: ResectOpts (None: the defaults)."""
    n_img = len(X_list)
    off = np.zeros(n_img + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in X_list])
    n = int(off[-1])
    X = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in X_list])
                             if n else np.zeros((1, 3)))
    uv = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64).reshape(-1, 2) for x in uv_list])
                              if n else np.zeros((1, 2)))
    img_intr = np.ascontiguousarray(np.asarray(img_intr, np.int32).reshape(-1))
    intr = np.ascontiguousarray(np.asarray(intr, np.float64).reshape(-1))
    iw = abi.load().sfm_ba_intr_width(camera_model)
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    assert len(img_intr) == n_img and len(wh) == 2 * n_img
    res = (abi.ResectResult * max(n_img, 1))()
    inl = np.full(max(n, 1), -1, np.int32)
    args = (camera_model, n_img, abi.ptr(off, abi.i64p), abi.ptr(X, abi.f64p), abi.ptr(uv, abi.f64p),
            abi.ptr(img_intr, abi.i32p), abi.ptr(intr, abi.f64p), len(intr) // iw if iw else 0,
            abi.ptr(wh, abi.i32p), C.byref(opts) if opts is not None else None, res, abi.ptr(inl, abi.i32p))
    if ctx is None:
        _check(abi.load().sfm_resect_host(*args), "sfm_resect_host")
    else:
        _check(ctx.lib.sfm_resect(ctx.h, *args), "sfm_resect")
    out = []
    for q in range(n_img):
        r = res[q]
        out.append({"pose": np.array(r.pose[:]), "pose_model": np.array(r.pose_model[:]), "error_max": r.error_max,
                    "min_nfa": r.min_nfa, "n_inliers": r.n_inliers, "iterations": r.iterations, "status": r.status,
                    "inliers": inl[off[q]:off[q] + r.n_inliers].copy()})
    return out


def resect_p3p(b, X):
    """sfm_resect_p3p: the models [(R (3, 3), t (3,)), ...] that map the world
    points X (3, 3) onto the unit bearings b (3, 3)."""
    b = np.ascontiguousarray(b, np.float64).reshape(9)
    X = np.ascontiguousarray(X, np.float64).reshape(9)
    Rt = np.zeros(48)
    n = C.c_int32()
    _check(abi.load().sfm_resect_p3p(abi.ptr(b, abi.f64p), abi.ptr(X, abi.f64p), abi.ptr(Rt, abi.f64p),
                                     C.byref(n)), "sfm_resect_p3p")
    return [(Rt[12 * m:12 * m + 9].reshape(3, 3).copy(), Rt[12 * m + 9:12 * m + 12].copy()) for m in range(n.value)]


def resect_gather(problem, X, pt_ok, images, counts_only=False):
    """sfm_resect_gather: for each image of `images`, its observations whose
    point is flagged in pt_ok, in the problem's order: (off, X3 [n, 3],
    uv [n, 2]), or off alone with counts_only."""
    images = np.ascontiguousarray(np.asarray(images, np.int32).reshape(-1))
    pt_ok = np.ascontiguousarray(np.asarray(pt_ok).astype(np.uint8).reshape(-1))
    X = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
    off = np.zeros(len(images) + 1, np.int64)
    lib = abi.load()
    head = (C.byref(problem), abi.ptr(X, abi.f64p), abi.ptr(pt_ok, abi.u8p), abi.ptr(images, abi.i32p), len(images),
            abi.ptr(off, abi.i64p))
    _check(lib.sfm_resect_gather(*head, None, None), "sfm_resect_gather")
    if counts_only:
        return off
    X3 = np.zeros((max(int(off[-1]), 1), 3))
    uv = np.zeros((max(int(off[-1]), 1), 2))
    _check(lib.sfm_resect_gather(*head, abi.ptr(X3, abi.f64p), abi.ptr(uv, abi.f64p)), "sfm_resect_gather")
    return off, X3[:off[-1]], uv[:off[-1]]


def relpose_default_options():
    o = abi.RelposeOpts()
    abi.load().sfm_relpose_default_options(C.byref(o))
    return o


def relpose(ctx, camera_model, xy_list, pair_intr, intr, wh, opts=None):
    """sfm_relpose (ctx None: sfm_relpose_host, on the CPU) over a list of image
    pairs: xy_list[q] (n_q, 4) matched pixels (x_I, y_I, x_J, y_J), pair_intr[q]
    = (block of image I, block of image J) in intr, wh[q] = (w_I, h_I, w_J, h_J).
    One dict per pair: E (3, 3), pose (angle-axis, t), error_max, min_nfa,
    angle_median, n_inliers, n_front, iterations, status (SFM_RELPOSE_*),
    inliers.  opts: RelposeOpts (None: the defaults)."""
    n_pairs = len(xy_list)
    off = np.zeros(n_pairs + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in xy_list])
    n = int(off[-1])
    xy = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64).reshape(-1, 4) for x in xy_list])
                              if n else np.zeros((1, 4)))
    pair_intr = np.ascontiguousarray(np.asarray(pair_intr, np.int32).reshape(-1))
    intr = np.ascontiguousarray(np.asarray(intr, np.float64).reshape(-1))
    iw = abi.load().sfm_ba_intr_width(camera_model)
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    assert len(pair_intr) == 2 * n_pairs and len(wh) == 4 * n_pairs
    res = (abi.RelposeResult * max(n_pairs, 1))()
    inl = np.full(max(n, 1), -1, np.int32)
    args = (camera_model, n_pairs, abi.ptr(off, abi.i64p), abi.ptr(xy, abi.f64p), abi.ptr(pair_intr, abi.i32p),
            abi.ptr(intr, abi.f64p), len(intr) // iw if iw else 0, abi.ptr(wh, abi.i32p),
            C.byref(opts) if opts is not None else None, res, abi.ptr(inl, abi.i32p))
    if ctx is None:
        _check(abi.load().sfm_relpose_host(*args), "sfm_relpose_host")
    else:
        _check(ctx.lib.sfm_relpose(ctx.h, *args), "sfm_relpose")
    out = []
    for q in range(n_pairs):
        r = res[q]
        out.append({"E": np.array(r.E[:]).reshape(3, 3), "pose": np.array(r.pose[:]), "error_max": r.error_max,
                    "min_nfa": r.min_nfa, "angle_median": r.angle_median, "n_inliers": r.n_inliers,
                    "n_front": r.n_front, "iterations": r.iterations, "status": r.status,
                    "inliers": inl[off[q]:off[q] + r.n_inliers].copy()})
    return out


def relpose_5pt(bI, bJ):
    """sfm_relpose_5pt: the essential matrices [(3, 3), ...] with bJ[i]' E bI[i] = 0
    for the five unit bearing pairs bI, bJ (5, 3)."""
    bI = np.ascontiguousarray(bI, np.float64).reshape(15)
    bJ = np.ascontiguousarray(bJ, np.float64).reshape(15)
    E = np.zeros(90)
    n = C.c_int32()
    _check(abi.load().sfm_relpose_5pt(abi.ptr(bI, abi.f64p), abi.ptr(bJ, abi.f64p), abi.ptr(E, abi.f64p),
                                      C.byref(n)), "sfm_relpose_5pt")
    return [E[9 * m:9 * m + 9].reshape(3, 3).copy() for m in range(n.value)]


def sift_default_options():
    o = abi.SiftOptions()
    abi.load().sfm_sift_options_default(C.byref(o))
    return o


def sift(ctx, gray, opts=None, cap_per_img=8192):
    """sfm_sift (ctx None: sfm_sift_host, on the CPU) over gray (n_img, h, w)
    uint8 images of one size.  Returns ([(xyso (n, 4) float32, desc (n, 128)
    uint8), ...] per image, holding min(n_feat, cap_per_img) rows, n_feat
    (n_img,) int64 the true counts, and the summary as a dict."""
    g = np.ascontiguousarray(gray, np.uint8)
    if g.ndim == 2:
        g = g[None]
    n_img, h, w = g.shape
    cap = int(cap_per_img)
    xyso = np.zeros((max(n_img, 1), max(cap, 1), 4), np.float32)
    desc = np.zeros((max(n_img, 1), max(cap, 1), 128), np.uint8)
    n_feat = np.zeros(max(n_img, 1), np.int64)
    sm = abi.SiftSummary()
    args = (abi.ptr(g, abi.u8p), n_img, w, h, C.byref(opts) if opts is not None else None, cap,
            abi.ptr(xyso, abi.f32p) if cap else None, abi.ptr(desc, abi.u8p) if cap else None,
            abi.ptr(n_feat, abi.i64p), C.byref(sm))
    if ctx is None:
        _check(abi.load().sfm_sift_host(*args), "sfm_sift_host")
    else:
        _check(ctx.lib.sfm_sift(ctx.h, *args), "sfm_sift")
    n_feat = n_feat[:n_img]
    out = [(xyso[i, :min(int(n_feat[i]), cap)].copy(), desc[i, :min(int(n_feat[i]), cap)].copy())
           for i in range(n_img)]
    return out, n_feat, {f: getattr(sm, f) for f, _ in abi.SiftSummary._fields_}


def synth_image(w, h, seed, angle=0.0, tx=0.0, ty=0.0, scale=1.0):
    """sfm_synth_image: the (h, w) uint8 blob-field view the golden SIFT fixtures were taken from."""
    g = np.zeros((h, w), np.uint8)
    _check(abi.load().sfm_synth_image(w, h, seed, angle, tx, ty, scale, abi.ptr(g, abi.u8p)), "sfm_synth_image")
    return g


def mvg_write_feat(path, xyso):
    f = np.ascontiguousarray(xyso, np.float32).reshape(-1, 4)
    _check(abi.load().sfm_mvg_write_feat(_b(path), abi.ptr(f, abi.f32p), f.shape[0]), "sfm_mvg_write_feat")


def tracks_default_options():
    o = abi.TracksOpts()
    abi.load().sfm_tracks_default_options(C.byref(o))
    return o


def _match_arrays(matches):
    """{(I, J): [n, 2] of (i, j)} in the dict's own order, or (pairs, counts, i, j)
    arrays in sfm_mvg_save_matches' layout -> those four arrays, contiguous."""
    if isinstance(matches, dict):
        keys = list(matches)
        pairs = np.array(keys, np.int32).reshape(-1, 2)
        counts = np.array([len(matches[k]) for k in keys], np.int64)
        ij = np.concatenate([np.asarray(matches[k], np.uint32).reshape(-1, 2) for k in keys]) \
            if keys else np.zeros((0, 2), np.uint32)
        i, j = ij[:, 0], ij[:, 1]
    else:
        pairs, counts, i, j = matches
    return (np.ascontiguousarray(pairs, np.int32).reshape(-1, 2), np.ascontiguousarray(counts, np.int64),
            np.ascontiguousarray(i, np.uint32), np.ascontiguousarray(j, np.uint32))


class Tracks:
    """sfm_tracks: the tracks of a set of pairwise matches, in canonical order
    (sfm_tracks_build on ctx; ctx None: sfm_tracks_build_host, on the CPU).
    feat_off[n_img + 1]: image I owns the node ids feat_off[I] .. feat_off[I+1]-1;
    matches: {(I, J): [n, 2] of (i, j)} or (pairs, counts, i, j) arrays; xy
    (optional): [feat_off[n_img], 2] positions, gathered into obs_uv."""

    def __init__(self, ctx, n_img, feat_off, matches, xy=None, opts=None):
        self.lib = abi.load()
        self.n_img = int(n_img)
        off = np.ascontiguousarray(feat_off, np.int64)
        if len(off) != self.n_img + 1:
            raise ValueError("Tracks: feat_off must have n_img + 1 entries")
        pairs, counts, i, j = _match_arrays(matches)
        # (the library rejects a negative count or 2^31 matches before it reads a match)
        total = int(counts.sum()) if len(counts) and (counts >= 0).all() else 0
        if len(counts) != len(pairs) or len(i) != len(j) or (total < 2**31 and len(i) < total):
            raise ValueError("Tracks: match arrays do not agree in size")
        if xy is not None:
            xy = np.ascontiguousarray(xy, np.float64).reshape(-1)
            if len(xy) < 2 * max(int(off[-1]), 0):
                raise ValueError("Tracks: xy needs a position per node id")
            if len(xy) == 0:
                xy = np.zeros(2)
        h = C.c_void_p()
        args = (self.n_img, abi.ptr(off, abi.i64p), len(pairs), abi.ptr(pairs, abi.i32p), abi.ptr(counts, abi.i64p),
                abi.ptr(i, abi.u32p), abi.ptr(j, abi.u32p), abi.ptr(xy, abi.f64p),
                C.byref(opts) if opts is not None else None, C.byref(h))
        if ctx is None:
            _check(self.lib.sfm_tracks_build_host(*args), "sfm_tracks_build_host")
        else:
            _check(self.lib.sfm_tracks_build(ctx.h, *args), "sfm_tracks_build")
        self._own(h, ctx)

    def _own(self, h, ctx):
        self.h = h
        if ctx is not None:
            ctx._adopt(self)

    @classmethod
    def _from_handle(cls, h, ctx, n_img):
        t = cls.__new__(cls)
        t.lib = abi.load()
        t.n_img = n_img
        t._own(h, ctx)
        return t

    def stats(self):
        st = abi.TracksStats()
        _check(self.lib.sfm_tracks_get_stats(self.h, C.byref(st)), "sfm_tracks_get_stats")
        return {f: getattr(st, f) for f, _ in abi.TracksStats._fields_}

    def fetch(self, uv=True):
        """dict(pt_offsets [n_tracks + 1], obs_img, obs_feat [n_obs], obs_uv
        [n_obs, 2]); uv False leaves obs_uv out (tracks built without xy have
        none: asking is an error)."""
        st = self.stats()
        n_trk, n_obs = st["n_tracks"], st["n_obs"]
        off = np.zeros(n_trk + 1, np.int64)
        img = np.zeros(max(n_obs, 1), np.int32)
        feat = np.zeros(max(n_obs, 1), np.uint32)
        xy = np.zeros(2 * max(n_obs, 1)) if uv else None
        _check(self.lib.sfm_tracks_fetch(self.h, abi.ptr(off, abi.i64p), abi.ptr(img, abi.i32p),
                                         abi.ptr(feat, abi.u32p), abi.ptr(xy, abi.f64p)), "sfm_tracks_fetch")
        return dict(pt_offsets=off, obs_img=img[:n_obs], obs_feat=feat[:n_obs],
                    obs_uv=xy[:2 * n_obs].reshape(-1, 2) if uv else None)

    def problem(self, img_intr, camera_model=abi.SFM_CAM_PINHOLE):
        """The tracks as a BAProblem (what triangulate, ba_solve and ba_wash
        take): img_intr[n_img] maps every image to its intrinsics block.  The
        problem keeps its arrays alive; no image is held constant."""
        f = self.fetch()
        ii = np.ascontiguousarray(img_intr, np.int32)
        if len(ii) != self.n_img:
            raise ValueError("Tracks.problem: img_intr must have n_img entries")
        off = f["pt_offsets"]
        img = np.ascontiguousarray(f["obs_img"]) if len(f["obs_img"]) else np.zeros(1, np.int32)
        uv = np.ascontiguousarray(f["obs_uv"].reshape(-1)) if len(f["obs_uv"]) else np.zeros(2)
        pr = abi.BAProblem()
        pr.n_img, pr.n_intr = self.n_img, int(ii.max()) + 1 if len(ii) else 0
        pr.n_pt, pr.n_obs = len(off) - 1, int(off[-1])
        pr.pt_offsets = abi.ptr(off, abi.i64p)
        pr.obs_img = abi.ptr(img, abi.i32p)
        pr.obs_uv = abi.ptr(uv, abi.f64p)
        pr.img_intr = abi.ptr(ii, abi.i32p)
        pr.const_img, pr.camera_model, pr.huber_a = -1, camera_model, 0.0
        pr._keep = (off, img, uv, ii)
        return pr

    def close(self):
        if self.h:
            self.lib.sfm_tracks_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sparse_tracks(ctx, matches_dir, matches_file=None, opts=None):
    """sfm_sparse_tracks: the Tracks of <matches_dir>/matches.f.bin (or
    matches_file) over the views of its sfm_data.json and their <stem>.feat."""
    h = C.c_void_p()
    _check(ctx.lib.sfm_sparse_tracks(ctx.h, _b(matches_dir), _b(matches_file) if matches_file else None,
                                     C.byref(opts) if opts is not None else None, C.byref(h)),
           "sfm_sparse_tracks")
    return Tracks._from_handle(h, ctx, len(mvg_load_views(str(matches_dir).rstrip("/") + "/sfm_data.json")))


def ba_cache_stats(ctx):
    """(reused, grown, fresh) plan counts of sfm_ba_solve on this context."""
    r, g, f = C.c_int64(), C.c_int64(), C.c_int64()
    _check(ctx.lib.sfm_ba_cache_stats(ctx.h, C.byref(r), C.byref(g), C.byref(f)), "sfm_ba_cache_stats")
    return r.value, g.value, f.value


def ba_cache_clear(ctx):
    _check(ctx.lib.sfm_ba_cache_clear(ctx.h), "sfm_ba_cache_clear")


def ba_partition(problem, world_size):
    lib = abi.load()
    order = np.zeros(max(problem.n_pt, 1), np.int64)
    bounds = np.zeros(world_size + 1, np.int64)
    _check(lib.sfm_ba_partition(C.byref(problem), world_size, abi.ptr(order, abi.i64p),
                                abi.ptr(bounds, abi.i64p)), "sfm_ba_partition")
    return order[:problem.n_pt], bounds


# ---------------------------------------------------------------------------
# incremental SequentialActuator loop (config C5)
# ---------------------------------------------------------------------------
def seq_default_options():
    o = abi.SeqOptions()
    abi.load().sfm_seq_default_options(C.byref(o))
    return o


class OrbitSequence:
    """[cpu] The synthetic closed-orbit image sequence (sfm_synth_orbit_image)."""

    def __init__(self, n_img=300, n_landmarks=60000, n_clutter=1000, track_mean=10.0,
                 detect_prob=0.95, noise_px=0.5, desc_noise_dims=24, desc_noise_amp=3,
                 prior_rot=2e-4, prior_t=1e-3, seed=0x5F3D0005):
        c = abi.SynthOrbitConfig()
        c.n_img, c.n_clutter, c.n_landmarks = n_img, n_clutter, n_landmarks
        c.track_mean, c.detect_prob, c.noise_px = track_mean, detect_prob, noise_px
        c.desc_noise_dims, c.desc_noise_amp = desc_noise_dims, desc_noise_amp
        c.prior_rot, c.prior_t, c.seed = prior_rot, prior_t, seed
        self.cfg = c
        self.n_img = n_img

    def image(self, k, gt=False):
        """dict(kp [n,2] f64, desc [n,128] u8, prior [6], landmark [n] (gt))"""
        lib = abi.load()
        n = C.c_int32()
        _check(lib.sfm_synth_orbit_image(C.byref(self.cfg), k, C.byref(n), None, None, None, None,
                                         None), "sfm_synth_orbit_image")
        kp = np.zeros((n.value, 2))
        d = np.zeros((max(n.value, 1), 128), np.uint8)
        prior = np.zeros(6)
        lm = np.zeros(max(n.value, 1), np.int64)
        _check(lib.sfm_synth_orbit_image(C.byref(self.cfg), k, C.byref(n), abi.ptr(kp, abi.f64p),
                                         abi.ptr(d, abi.u8p), abi.ptr(prior, abi.f64p),
                                         abi.ptr(lm, abi.i64p), None), "sfm_synth_orbit_image")
        out = {"kp": kp, "desc": d[:n.value], "prior": prior}
        if gt:
            out["landmark"] = lm[:n.value]
        return out

    def gt_points(self):
        lib = abi.load()
        n = C.c_int32()
        X = np.zeros(3 * max(self.cfg.n_landmarks, 1))
        _check(lib.sfm_synth_orbit_image(C.byref(self.cfg), 0, C.byref(n), None, None, None, None,
                                         abi.ptr(X, abi.f64p)), "sfm_synth_orbit_image")
        return X[:3 * self.cfg.n_landmarks].reshape(-1, 3)


def seq_image(img):
    """numpy image dict -> SeqImage (keeps the arrays referenced)."""
    si = abi.SeqImage()
    kp = np.ascontiguousarray(img["kp"], np.float64)
    d = np.ascontiguousarray(img["desc"], np.uint8)
    si.n_kp = len(kp)
    si.kp_xy = abi.ptr(kp, abi.f64p)
    si.desc = abi.ptr(d, abi.u8p)
    for a in range(6):
        si.pose_prior[a] = float(img["prior"][a])
    si._keep = (kp, d)
    return si


class _SeqCalls:
    """init / add / bundle_adjust / step / matches / world over the sfm_seq_*
    (product) or orc_seq_* (oracle, tests only) entry points."""

    def _f(self, name):
        return getattr(self.lib, self.prefix + name)

    def init(self, a, b):
        _check(self._f("init")(self.h, C.byref(seq_image(a)), C.byref(seq_image(b))), self.prefix + "init")

    def add(self, img):
        kept = C.c_int32()
        _check(self._f("add_image")(self.h, C.byref(seq_image(img)), C.byref(kept)), self.prefix + "add_image")
        return bool(kept.value)

    def bundle_adjust(self):
        s = abi.BASummary()
        _check(self._f("bundle_adjust")(self.h, C.byref(s)), self.prefix + "bundle_adjust")
        return s

    def step(self):
        st = abi.SeqStep()
        _check(self._f("last_step")(self.h, C.byref(st)), self.prefix + "last_step")
        return st

    def matches(self, which):
        n = C.c_int64()
        self._f("matches")(self.h, which, None, None, None, 0, C.byref(n))
        q = np.zeros(max(n.value, 1), np.int32)
        t = np.zeros_like(q)
        d = np.zeros(len(q), np.float32)
        _check(self._f("matches")(self.h, which, abi.ptr(q, abi.i32p), abi.ptr(t, abi.i32p),
                                  abi.ptr(d, abi.f32p), n.value, C.byref(n)), self.prefix + "matches")
        return q[:n.value], t[:n.value], d[:n.value]

    def world(self):
        n_pts, n_img = C.c_int64(), C.c_int32()
        self._f("world")(self.h, None, None, 0, C.byref(n_pts), None, 0, C.byref(n_img), None)
        X = np.zeros(3 * max(n_pts.value, 1))
        nobs = np.zeros(max(n_pts.value, 1), np.int64)
        poses = np.zeros(6 * max(n_img.value, 1))
        intr = np.zeros(4)
        _check(self._f("world")(self.h, abi.ptr(X, abi.f64p), abi.ptr(nobs, abi.i64p), n_pts.value,
                                C.byref(n_pts), abi.ptr(poses, abi.f64p), n_img.value, C.byref(n_img),
                                abi.ptr(intr, abi.f64p)), self.prefix + "world")
        return {"X": X[:3 * n_pts.value].reshape(-1, 3), "n_obs": nobs[:n_pts.value],
                "poses": poses[:6 * n_img.value].reshape(-1, 6), "intr": intr}

    def observations(self):
        """(image sequence index [n], uv [n, 2]) of every observation, points
        in index order (counts: world()["n_obs"])"""
        n = C.c_int64()
        self._f("observations")(self.h, None, None, 0, C.byref(n))
        img = np.zeros(max(n.value, 1), np.int32)
        uv = np.zeros((max(n.value, 1), 2))
        _check(self._f("observations")(self.h, abi.ptr(img, abi.i32p), abi.ptr(uv, abi.f64p), n.value,
                                       C.byref(n)), self.prefix + "observations")
        return img[:n.value], uv[:n.value]

    def close(self):
        if self.h:
            self._f("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SeqLoop(_SeqCalls):
    """SequentialActuator on the GPU (sfm_seq_*)."""

    def __init__(self, ctx, opts=None):
        self.ctx, self.lib, self.prefix = ctx, ctx.lib, "sfm_seq_"
        o = opts or seq_default_options()
        h = C.c_void_p()
        _check(self.lib.sfm_seq_create(ctx.h, C.byref(o), C.byref(h)), "sfm_seq_create")
        self.h = h
        ctx._adopt(self)


# ---------------------------------------------------------------------------
# file-staged sparseBuilder flow (OpenMVG stage-boundary formats)
# ---------------------------------------------------------------------------
def _b(path):
    return str(path).encode()


def mvg_load_views(path):
    """sfm_data.json VIEWS -> list of dicts sorted by id_view."""
    lib = abi.load()
    n = C.c_int32()
    _check(lib.sfm_mvg_load_views(_b(path), None, 0, C.byref(n)), "sfm_mvg_load_views")
    v = (abi.MvgView * max(n.value, 1))()
    _check(lib.sfm_mvg_load_views(_b(path), v, n.value, C.byref(n)), "sfm_mvg_load_views")
    return [{"id_view": x.id_view, "id_intrinsic": x.id_intrinsic, "id_pose": x.id_pose,
             "width": x.width, "height": x.height, "img_path": x.img_path.decode()}
            for x in v[:n.value]]


def mvg_check_describer(path):
    _check(abi.load().sfm_mvg_check_describer(_b(path)), "sfm_mvg_check_describer")


def mvg_read_desc(path):
    lib = abi.load()
    n = C.c_int64()
    _check(lib.sfm_mvg_read_desc(_b(path), None, 0, C.byref(n)), "sfm_mvg_read_desc")
    d = np.zeros((max(n.value, 1), 128), np.uint8)
    _check(lib.sfm_mvg_read_desc(_b(path), abi.ptr(d, abi.u8p), n.value, C.byref(n)),
           "sfm_mvg_read_desc")
    return d[:n.value]


def mvg_write_desc(path, desc):
    d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 128)
    _check(abi.load().sfm_mvg_write_desc(_b(path), abi.ptr(d, abi.u8p), d.shape[0]),
           "sfm_mvg_write_desc")


def mvg_read_feat(path):
    lib = abi.load()
    n = C.c_int64()
    _check(lib.sfm_mvg_read_feat(_b(path), None, 0, C.byref(n)), "sfm_mvg_read_feat")
    f = np.zeros((max(n.value, 1), 4), np.float32)
    _check(lib.sfm_mvg_read_feat(_b(path), f.ctypes.data_as(C.POINTER(C.c_float)), n.value,
                                 C.byref(n)), "sfm_mvg_read_feat")
    return f[:n.value]


def mvg_load_pairs(path, n_views):
    lib = abi.load()
    n = C.c_int64()
    _check(lib.sfm_mvg_load_pairs(_b(path), n_views, None, 0, C.byref(n)), "sfm_mvg_load_pairs")
    p = np.zeros((max(n.value, 1), 2), np.int32)
    _check(lib.sfm_mvg_load_pairs(_b(path), n_views, abi.ptr(p, abi.i32p), n.value, C.byref(n)),
           "sfm_mvg_load_pairs")
    return p[:n.value]


def mvg_save_pairs(path, pairs):
    p = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    _check(abi.load().sfm_mvg_save_pairs(_b(path), abi.ptr(p, abi.i32p), p.shape[0]),
           "sfm_mvg_save_pairs")


def mvg_save_matches(path, matches):
    """matches: {(I, J): int array [n, 2] of (i, j)} -> PairWiseMatches file."""
    keys = sorted(matches)
    pairs = np.array(keys, np.int32).reshape(-1, 2)
    counts = np.array([len(matches[k]) for k in keys], np.int64)
    ij = np.concatenate([np.asarray(matches[k], np.uint32).reshape(-1, 2) for k in keys]) \
        if keys else np.zeros((0, 2), np.uint32)
    i = np.ascontiguousarray(ij[:, 0])
    j = np.ascontiguousarray(ij[:, 1])
    _check(abi.load().sfm_mvg_save_matches(_b(path), abi.ptr(pairs, abi.i32p), len(keys),
                                           abi.ptr(counts, abi.i64p), abi.ptr(i, abi.u32p),
                                           abi.ptr(j, abi.u32p)), "sfm_mvg_save_matches")


def mvg_load_matches(path):
    """PairWiseMatches file -> {(I, J): uint32 array [n, 2]} (map order)."""
    lib = abi.load()
    npair, nm = C.c_int64(), C.c_int64()
    _check(lib.sfm_mvg_load_matches(_b(path), None, None, None, None, 0, 0, C.byref(npair),
                                    C.byref(nm)), "sfm_mvg_load_matches")
    pairs = np.zeros((max(npair.value, 1), 2), np.int32)
    counts = np.zeros(max(npair.value, 1), np.int64)
    i = np.zeros(max(nm.value, 1), np.uint32)
    j = np.zeros(max(nm.value, 1), np.uint32)
    _check(lib.sfm_mvg_load_matches(_b(path), abi.ptr(pairs, abi.i32p), abi.ptr(counts, abi.i64p),
                                    abi.ptr(i, abi.u32p), abi.ptr(j, abi.u32p), npair.value,
                                    nm.value, C.byref(npair), C.byref(nm)), "sfm_mvg_load_matches")
    out, off = {}, 0
    for k in range(npair.value):
        c = int(counts[k])
        out[(int(pairs[k, 0]), int(pairs[k, 1]))] = np.stack([i[off:off + c], j[off:off + c]], 1)
        off += c
    return out


def sparse_match_pair(matches_dir):
    """sparseBuilder::matchPair(): writes <matches_dir>/pairs.bin."""
    _check(abi.load().sfm_sparse_match_pair(_b(matches_dir)), "sfm_sparse_match_pair")


def sparse_match(ctx, matches_dir, mode=abi.SFM_MATCH_CASCADE, ratio=0.8, force=False, dedup_xy=True):
    """sparseBuilder::match(), file-staged, on the GPU matcher.  The default
    mode is the reference's "AUTO" (cascade hashing, sparseBuilder.cpp:814,
    911-914); SFM_MATCH_RATIO is its "BRUTEFORCEL2" (:919-921)."""
    o = abi.SparseMatchOpts()
    o.mode, o.ratio, o.force, o.dedup_xy = mode, ratio, int(force), int(dedup_xy)
    st = abi.SparseMatchStats()
    _check(ctx.lib.sfm_sparse_match(ctx.h, _b(matches_dir), C.byref(o), C.byref(st)),
           "sfm_sparse_match")
    return {"n_views": st.n_views, "n_pairs_in": st.n_pairs_in, "n_pairs_out": st.n_pairs_out,
            "n_matches": st.n_matches, "reloaded": bool(st.reloaded)}


# ---- geometric filter (GeometricFilter_FMatrix_AC) ----------
def fmatrix_opts(precision=4.0, max_iterations=2048):
    o = abi.FMatrixOpts()
    o.precision, o.max_iterations = precision, max_iterations
    return o


def _fmatrix_inputs(xy_list, wh):
    counts = np.array([len(x) for x in xy_list], np.int64)
    off = np.zeros(len(xy_list) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    xy = np.ascontiguousarray(np.concatenate([np.asarray(x, np.float64).reshape(-1, 4) for x in xy_list])
                              if len(xy_list) and off[-1] else np.zeros((1, 4)), np.float64)
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1, 4))
    return off, xy, wh


def _fmatrix_outputs(off, res, inl):
    out = []
    for q in range(len(off) - 1):
        r = res[q]
        out.append({"F": np.array(r.F[:]).reshape(3, 3), "error_max": r.error_max, "min_nfa": r.min_nfa,
                    "n_inliers": r.n_inliers, "iterations": r.iterations,
                    "inliers": inl[off[q]:off[q] + r.n_inliers].copy()})
    return out


def fmatrix_ac(ctx, xy_list, wh, opts=None):
    """sfm_fmatrix_ac over a list of pairs: xy_list[q] is an (n_q, 4) array of
    (x_I, y_I, x_J, y_J) pixels, wh[q] = (w_I, h_I, w_J, h_J).  Returns one
    dict per pair (F, error_max, min_nfa, n_inliers, iterations, inliers)."""
    lib = abi.load()
    off, xy, wh = _fmatrix_inputs(xy_list, wh)
    n_pairs = len(off) - 1
    res = (abi.FMatrixResult * max(n_pairs, 1))()
    inl = np.full(max(int(off[-1]), 1), -1, np.int32)
    _check(lib.sfm_fmatrix_ac(ctx.h, n_pairs, abi.ptr(off, abi.i64p), abi.ptr(xy, abi.f64p),
                              abi.ptr(wh, abi.i32p), C.byref(opts or fmatrix_opts()), res,
                              abi.ptr(inl, abi.i32p)), "sfm_fmatrix_ac")
    return _fmatrix_outputs(off, res, inl)


def sparse_filter(ctx, matches_dir, opts=None):
    lib = abi.load()
    st = abi.SparseFilterStats()
    _check(lib.sfm_sparse_filter(ctx.h, _b(matches_dir), C.byref(opts or fmatrix_opts()), C.byref(st)),
           "sfm_sparse_filter")
    return st


# ---- incremental reconstruction -----------------------------------------------------
def recon_default_options():
    o = abi.ReconOpts()
    abi.load().sfm_recon_default_options(C.byref(o))
    return o


class ReconTracks:
    """sfm_recon_tracks: a problem's tracks held resident (ctx None: the host
    twin) for the three round queries.  Every query returns what the device or
    the host walk wrote, compacted, as numpy arrays."""

    def __init__(self, ctx, problem):
        self.lib = abi.load()
        self.n_img, self.n_pt, self.n_obs = problem.n_img, problem.n_pt, problem.n_obs
        # the rows a gather of an image can have at most
        img = np.ctypeslib.as_array(problem.obs_img, shape=(max(self.n_obs, 1),))[:self.n_obs]
        self._per_img = np.bincount(img, minlength=max(self.n_img, 1)) if self.n_obs else np.zeros(max(self.n_img, 1), int)
        h = C.c_void_p()
        if ctx is None:
            _check(self.lib.sfm_recon_tracks_create_host(C.byref(problem), C.byref(h)), "sfm_recon_tracks_create_host")
        else:
            _check(self.lib.sfm_recon_tracks_create(ctx.h, C.byref(problem), C.byref(h)), "sfm_recon_tracks_create")
            ctx._adopt(self)
        self.h = h

    def _ok(self, pt_ok):
        a = np.ascontiguousarray(np.asarray(pt_ok).astype(np.uint8).reshape(-1))
        assert len(a) == self.n_pt
        return a if self.n_pt else np.zeros(1, np.uint8)

    def drop_obs(self, obs):
        obs = np.ascontiguousarray(np.asarray(obs, np.int64).reshape(-1))
        _check(self.lib.sfm_recon_tracks_drop_obs(self.h, abi.ptr(obs, abi.i64p), len(obs)), "sfm_recon_tracks_drop_obs")

    def visibility(self, pt_ok):
        count = np.zeros(max(self.n_img, 1), np.int32)
        _check(self.lib.sfm_recon_visibility(self.h, abi.ptr(self._ok(pt_ok), abi.u8p), abi.ptr(count, abi.i32p)),
               "sfm_recon_visibility")
        return count[:self.n_img]

    def gather(self, X, pt_ok, images):
        """(off [n_images + 1], X3 [n, 3], uv [n, 2], obs [n])"""
        images = np.ascontiguousarray(np.asarray(images, np.int32).reshape(-1))
        X = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
        if not len(X):
            X = np.zeros(3)
        off = np.zeros(len(images) + 1, np.int64)
        ok_img = images[(images >= 0) & (images < self.n_img)]
        cap = int(self._per_img[ok_img].sum()) if len(ok_img) else 0
        X3 = np.zeros((max(cap, 1), 3))
        uv = np.zeros((max(cap, 1), 2))
        obs = np.zeros(max(cap, 1), np.int64)
        _check(self.lib.sfm_recon_gather(self.h, abi.ptr(X, abi.f64p), abi.ptr(self._ok(pt_ok), abi.u8p),
                                         abi.ptr(images, abi.i32p), len(images), abi.ptr(off, abi.i64p),
                                         abi.ptr(X3, abi.f64p), abi.ptr(uv, abi.f64p), abi.ptr(obs, abi.i64p), cap),
               "sfm_recon_gather")
        return off, X3[:off[-1]].copy(), uv[:off[-1]].copy(), obs[:off[-1]].copy()

    def select(self, registered, pt_ok, mode, min_track_len=2):
        """dict(pt_offsets, obs_img, obs_uv [n, 2], pt_map, obs_map)"""
        reg = np.ascontiguousarray(np.asarray(registered).astype(np.uint8).reshape(-1))
        assert len(reg) == self.n_img
        if not self.n_img:
            reg = np.zeros(1, np.uint8)
        n_pt, n_obs = C.c_int64(), C.c_int64()
        off = np.zeros(self.n_pt + 1, np.int64)
        img = np.zeros(max(self.n_obs, 1), np.int32)
        uv = np.zeros((max(self.n_obs, 1), 2))
        pm = np.zeros(max(self.n_pt, 1), np.int64)
        om = np.zeros(max(self.n_obs, 1), np.int64)
        _check(self.lib.sfm_recon_select(self.h, abi.ptr(reg, abi.u8p), abi.ptr(self._ok(pt_ok), abi.u8p), mode,
                                         min_track_len, C.byref(n_pt), C.byref(n_obs), abi.ptr(off, abi.i64p),
                                         abi.ptr(img, abi.i32p), abi.ptr(uv, abi.f64p), abi.ptr(pm, abi.i64p),
                                         abi.ptr(om, abi.i64p), self.n_pt, self.n_obs), "sfm_recon_select")
        n_pt, n_obs = n_pt.value, n_obs.value
        return dict(pt_offsets=off[:n_pt + 1].copy(), obs_img=img[:n_obs].copy(), obs_uv=uv[:n_obs].copy(),
                    pt_map=pm[:n_pt].copy(), obs_map=om[:n_obs].copy())

    def close(self):
        if getattr(self, "h", None):
            self.lib.sfm_recon_tracks_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _struct_dict(s):
    out = {}
    for f, t in s._fields_:
        v = getattr(s, f)
        out[f] = _struct_dict(v) if isinstance(v, C.Structure) else (list(v) if isinstance(v, C.Array) else v)
    return out


def reconstruct(ctx, problem, intr, wh, pairs, opts=None, cap_rounds=256, cap_cands=1024):
    """sfm_reconstruct (ctx None: sfm_reconstruct_host, on the CPU) over the
    tracks of `problem`: dict(rc, extr [n_img, 6], intr (refined copy),
    X [n_pt, 3], registered, pt_ok, keep_obs (bool), rounds, cands (lists of
    dicts, what fitted the capacities), stats (dict))."""
    lib = abi.load()
    n_img, n_pt, n_obs = problem.n_img, problem.n_pt, problem.n_obs
    intr = np.ascontiguousarray(np.asarray(intr, np.float64).reshape(-1)).copy()
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1))
    assert len(wh) == 2 * n_img
    extr = np.zeros(6 * max(n_img, 1))
    X = np.zeros(3 * max(n_pt, 1))
    reg = np.zeros(max(n_img, 1), np.uint8)
    ok = np.zeros(max(n_pt, 1), np.uint8)
    keep = np.zeros(max(n_obs, 1), np.uint8)
    rounds = (abi.ReconRound * max(cap_rounds, 1))()
    cands = (abi.ReconCand * max(cap_cands, 1))()
    st = abi.ReconStats()
    args = (C.byref(problem), abi.ptr(intr, abi.f64p), abi.ptr(wh, abi.i32p), abi.ptr(pairs, abi.i32p), len(pairs) // 2,
            C.byref(opts) if opts is not None else None, abi.ptr(extr, abi.f64p), abi.ptr(X, abi.f64p),
            abi.ptr(reg, abi.u8p), abi.ptr(ok, abi.u8p), abi.ptr(keep, abi.u8p), rounds, cap_rounds, cands, cap_cands,
            C.byref(st))
    rc = lib.sfm_reconstruct_host(*args) if ctx is None else lib.sfm_reconstruct(ctx.h, *args)
    _check(rc, "sfm_reconstruct_host" if ctx is None else "sfm_reconstruct")
    return dict(rc=rc, extr=extr[:6 * n_img].reshape(-1, 6), intr=intr, X=X[:3 * n_pt].reshape(-1, 3),
                registered=reg[:n_img].astype(bool), pt_ok=ok[:n_pt].astype(bool), keep_obs=keep[:n_obs].astype(bool),
                rounds=[_struct_dict(rounds[k]) for k in range(min(st.n_rounds, cap_rounds))],
                cands=[_struct_dict(cands[k]) for k in range(min(st.n_cands, cap_cands))], stats=_struct_dict(st))


def sparse_reconstruct(ctx, matches_dir, out_dir, focal=-1.0, opts=None):
    """sfm_sparse_reconstruct: sparseBuilder::reconstruction(), file-staged;
    writes <out_dir>/cloud_and_poses.ply and returns the stats dict."""
    st = abi.ReconStats()
    _check(abi.load().sfm_sparse_reconstruct(ctx.h, _b(matches_dir), _b(out_dir), focal,
                                             C.byref(opts) if opts is not None else None, C.byref(st)),
           "sfm_sparse_reconstruct")
    return _struct_dict(st)


# ---- track colouring ------------------------------------------------------------------
def _mask(a, n):
    """an optional uint8 mask of n entries (None stays None: all)"""
    if a is None:
        return None
    a = np.ascontiguousarray(np.asarray(a).astype(np.uint8).reshape(-1))
    assert len(a) == n
    return a if n else np.zeros(1, np.uint8)


def colorize_assign(ctx, problem, wh, pt_ok=None, keep_obs=None):
    """sfm_colorize_assign (ctx None: sfm_colorize_assign_host): which view
    colours each point.  dict(view [n_pt], obs [n_pt], px [n_pt, 2],
    order [n_img] (-1 from n_rounds on), n_rounds, stats)."""
    lib = abi.load()
    n_img, n_pt = problem.n_img, problem.n_pt
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    assert len(wh) == 2 * n_img
    ok, keep = _mask(pt_ok, n_pt), _mask(keep_obs, problem.n_obs)
    view = np.full(max(n_pt, 1), -7, np.int32)
    obs = np.full(max(n_pt, 1), -7, np.int64)
    px = np.full(2 * max(n_pt, 1), -7, np.int32)
    order = np.full(max(n_img, 1), -7, np.int32)
    n_rounds = C.c_int32(-7)
    st = abi.ColorizeStats()
    args = (C.byref(problem), abi.ptr(wh, abi.i32p), abi.ptr(ok, abi.u8p), abi.ptr(keep, abi.u8p),
            abi.ptr(view, abi.i32p), abi.ptr(obs, abi.i64p), abi.ptr(px, abi.i32p), abi.ptr(order, abi.i32p),
            C.byref(n_rounds), C.byref(st))
    if ctx is None:
        _check(lib.sfm_colorize_assign_host(*args), "sfm_colorize_assign_host")
    else:
        _check(lib.sfm_colorize_assign(ctx.h, *args), "sfm_colorize_assign")
    return dict(view=view[:n_pt], obs=obs[:n_pt], px=px[:2 * n_pt].reshape(-1, 2), order=order[:n_img],
                n_rounds=n_rounds.value, stats=_struct_dict(st))


def colorize_assign_host(problem, wh, pt_ok=None, keep_obs=None):
    return colorize_assign(None, problem, wh, pt_ok, keep_obs)


def _pixel_pool(images):
    """images: per view a uint8 array [h, w] / [h, w, 1] / [h, w, 3], or None
    (not loaded) -> (channels, img_off, pixels) as sfm_colorize_sample reads them"""
    channels = np.ones(max(len(images), 1), np.int32)
    img_off = np.full(max(len(images), 1), -1, np.int64)
    parts, at = [], 0
    for i, im in enumerate(images):
        if im is None:
            continue
        im = np.ascontiguousarray(im, np.uint8)
        channels[i] = 1 if im.ndim == 2 else im.shape[2]
        img_off[i] = at
        parts.append(im.reshape(-1))
        at += im.size
    pixels = np.concatenate(parts) if parts else np.zeros(1, np.uint8)
    return channels, img_off, pixels


def colorize_sample(view, px, wh, images=None, pool=None):
    """sfm_colorize_sample: rgb [n_pt, 3] from the images (a list, see
    _pixel_pool) or a ready (channels, img_off, pixels) pool."""
    view = np.ascontiguousarray(np.asarray(view, np.int32).reshape(-1))
    px = np.ascontiguousarray(np.asarray(px, np.int32).reshape(-1))
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    n_pt, n_img = len(view), len(wh) // 2
    assert len(px) == 2 * n_pt
    channels, img_off, pixels = pool if pool is not None else _pixel_pool(images)
    rgb = np.full(3 * max(n_pt, 1), 77, np.uint8)
    _check(abi.load().sfm_colorize_sample(n_pt, abi.ptr(view if n_pt else np.zeros(1, np.int32), abi.i32p),
                                          abi.ptr(px if n_pt else np.zeros(2, np.int32), abi.i32p), n_img,
                                          abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p),
                                          abi.ptr(channels, abi.i32p), abi.ptr(img_off, abi.i64p),
                                          abi.ptr(pixels, abi.u8p), abi.ptr(rgb, abi.u8p)), "sfm_colorize_sample")
    return rgb[:3 * n_pt].reshape(-1, 3)


def colorize(ctx, problem, wh, images=None, pt_ok=None, keep_obs=None, pool=None):
    """sfm_colorize (ctx None: sfm_colorize_host): assign and sample in one
    call.  dict(rgb [n_pt, 3], view [n_pt], stats)."""
    lib = abi.load()
    n_img, n_pt = problem.n_img, problem.n_pt
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    assert len(wh) == 2 * n_img
    ok, keep = _mask(pt_ok, n_pt), _mask(keep_obs, problem.n_obs)
    channels, img_off, pixels = pool if pool is not None else _pixel_pool(images)
    rgb = np.full(3 * max(n_pt, 1), 77, np.uint8)
    view = np.full(max(n_pt, 1), -7, np.int32)
    st = abi.ColorizeStats()
    args = (C.byref(problem), abi.ptr(wh, abi.i32p), abi.ptr(ok, abi.u8p), abi.ptr(keep, abi.u8p),
            abi.ptr(channels, abi.i32p), abi.ptr(img_off, abi.i64p), abi.ptr(pixels, abi.u8p), abi.ptr(rgb, abi.u8p),
            abi.ptr(view, abi.i32p), C.byref(st))
    if ctx is None:
        _check(lib.sfm_colorize_host(*args), "sfm_colorize_host")
    else:
        _check(lib.sfm_colorize(ctx.h, *args), "sfm_colorize")
    return dict(rgb=rgb[:3 * n_pt].reshape(-1, 3), view=view[:n_pt], stats=_struct_dict(st))


def colorize_host(problem, wh, images=None, pt_ok=None, keep_obs=None, pool=None):
    return colorize(None, problem, wh, images, pt_ok, keep_obs, pool)


def colorize_write_ply(path, X, pt_ok=None, rgb=None, extr=None, registered=None):
    """sfm_colorize_write_ply: the points with pt_ok (None: all) in their
    colours (None: white), then the registered (None: all) camera centres."""
    X = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1, 3))
    extr = np.ascontiguousarray(np.zeros((0, 6)) if extr is None else np.asarray(extr, np.float64).reshape(-1, 6))
    n_pt, n_img = len(X), len(extr)
    if rgb is not None:
        rgb = np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1))
        assert len(rgb) == 3 * n_pt
    _check(abi.load().sfm_colorize_write_ply(_b(path), n_pt, abi.ptr(X if n_pt else np.zeros(3), abi.f64p),
                                             abi.ptr(_mask(pt_ok, n_pt), abi.u8p), abi.ptr(rgb, abi.u8p), n_img,
                                             abi.ptr(extr if n_img else np.zeros(6), abi.f64p),
                                             abi.ptr(_mask(registered, n_img), abi.u8p)), "sfm_colorize_write_ply")


def sparse_reconstruct_colorize(ctx, matches_dir, out_dir, images, focal=-1.0, opts=None):
    """sfm_sparse_reconstruct_colorize: reconstruction() + colorize(),
    file-staged; images in the view order of sfm_data.json (see _pixel_pool).
    Writes <out_dir>/cloud_and_poses.ply and <out_dir>/colorized.ply and
    returns (reconstruction stats, colouring stats)."""
    channels, img_off, pixels = _pixel_pool(images)
    st, cs = abi.ReconStats(), abi.ColorizeStats()
    _check(abi.load().sfm_sparse_reconstruct_colorize(ctx.h, _b(matches_dir), _b(out_dir), focal,
                                                      C.byref(opts) if opts is not None else None,
                                                      abi.ptr(channels, abi.i32p), abi.ptr(img_off, abi.i64p),
                                                      abi.ptr(pixels, abi.u8p), C.byref(st), C.byref(cs)),
           "sfm_sparse_reconstruct_colorize")
    return _struct_dict(st), _struct_dict(cs)


# ---- dense hand-off -------------------------------------------------------------------
def undistort_default_options():
    o = abi.UndistortOpts()
    abi.load().sfm_undistort_default_options(C.byref(o))
    return o


def undistort(ctx, camera_model, img_intr, intr, wh, images=None, opts=None, pool=None, out=None):
    """sfm_undistort (ctx None: sfm_undistort_host): every loaded image
    undistorted.  images: a list as in _pixel_pool, or a ready (channels,
    img_off, pixels) pool.  out: the byte pool to write into (as large as
    pixels; by default a zeroed one).  dict(out (the pool), images (views of
    it, one per image, None where not loaded), stats)."""
    lib = abi.load()
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    n_img = len(wh) // 2
    img_intr = np.ascontiguousarray(np.asarray(img_intr, np.int32).reshape(-1))
    assert len(img_intr) == n_img
    iw = max(lib.sfm_ba_intr_width(camera_model), 1)
    intr = np.ascontiguousarray(np.asarray(intr, np.float64).reshape(-1))
    assert len(intr) % iw == 0
    n_intr = len(intr) // iw
    channels, img_off, pixels = pool if pool is not None else _pixel_pool(images)
    if out is None:
        out = np.zeros(len(pixels), np.uint8)
    assert out.dtype == np.uint8 and out.flags.c_contiguous and len(out) >= len(pixels)
    st = abi.UndistortStats()
    args = (camera_model, n_img, n_intr, abi.ptr(img_intr if n_img else np.zeros(1, np.int32), abi.i32p),
            abi.ptr(intr if n_intr else np.zeros(1), abi.f64p), abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p),
            abi.ptr(channels, abi.i32p), abi.ptr(img_off, abi.i64p), abi.ptr(pixels, abi.u8p),
            C.byref(opts) if opts is not None else None, abi.ptr(out, abi.u8p), C.byref(st))
    if ctx is None:
        _check(lib.sfm_undistort_host(*args), "sfm_undistort_host")
    else:
        _check(lib.sfm_undistort(ctx.h, *args), "sfm_undistort")
    views = []
    for i in range(n_img):
        if img_off[i] < 0:
            views.append(None)
            continue
        w, h, ch = int(wh[2 * i]), int(wh[2 * i + 1]), int(channels[i])
        v = out[img_off[i]:img_off[i] + w * h * ch]
        views.append(v.reshape(h, w) if ch == 1 else v.reshape(h, w, ch))
    return dict(out=out, images=views, stats=_struct_dict(st))


def undistort_host(camera_model, img_intr, intr, wh, images=None, opts=None, pool=None, out=None):
    return undistort(None, camera_model, img_intr, intr, wh, images, opts, pool, out)


def write_pnm(path, image):
    """sfm_undistort_write_pnm: a uint8 [h, w] / [h, w, 1] image as binary P5, [h, w, 3] as P6."""
    im = np.ascontiguousarray(image, np.uint8)
    ch = 1 if im.ndim == 2 else im.shape[2]
    _check(abi.load().sfm_undistort_write_pnm(_b(path), im.shape[1], im.shape[0], ch, abi.ptr(im.reshape(-1), abi.u8p)),
           "sfm_undistort_write_pnm")


def dense_scene(problem, intr, extr, X, wh, registered=None, pt_ok=None, keep_obs=None):
    """sfm_dense_scene_build + get_info + fetch + destroy: the scene of
    openMVG2openMVS as a dict of arrays: K [n_platforms, 3, 3], platform_wh,
    image_src, image_platform, image_pose, R [n_images, 3, 3], C [n_images, 3],
    vert_X (float32) [n_vertices, 3], vert_off, vert_view, vert_pt, n_short."""
    lib = abi.load()
    n_img, n_pt = problem.n_img, problem.n_pt
    intr = np.ascontiguousarray(np.asarray(intr, np.float64).reshape(-1))
    extr = np.ascontiguousarray(np.asarray(extr, np.float64).reshape(-1))
    X = np.ascontiguousarray(np.asarray(X, np.float64).reshape(-1))
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    assert len(extr) == 6 * n_img and len(X) == 3 * n_pt and len(wh) == 2 * n_img
    h = C.c_void_p()
    _check(lib.sfm_dense_scene_build(C.byref(problem), abi.ptr(intr if len(intr) else np.zeros(1), abi.f64p),
                                     abi.ptr(extr if n_img else np.zeros(6), abi.f64p),
                                     abi.ptr(X if n_pt else np.zeros(3), abi.f64p),
                                     abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p),
                                     abi.ptr(_mask(registered, n_img), abi.u8p), abi.ptr(_mask(pt_ok, n_pt), abi.u8p),
                                     abi.ptr(_mask(keep_obs, problem.n_obs), abi.u8p), C.byref(h)),
           "sfm_dense_scene_build")
    try:
        info = abi.DenseSceneInfo()
        _check(lib.sfm_dense_scene_get_info(h, C.byref(info)), "sfm_dense_scene_get_info")
        npl, ni, nv, nw = info.n_platforms, info.n_images, info.n_vertices, info.n_views
        out = dict(K=np.zeros((npl, 3, 3)), platform_wh=np.zeros((npl, 2), np.int32), image_src=np.zeros(ni, np.int32),
                   image_platform=np.zeros(ni, np.int32), image_pose=np.zeros(ni, np.int32), R=np.zeros((ni, 3, 3)),
                   C=np.zeros((ni, 3)), vert_X=np.zeros((nv, 3), np.float32), vert_off=np.zeros(nv + 1, np.int64),
                   vert_view=np.zeros(nw, np.uint32), vert_pt=np.zeros(nv, np.int64))
        types = dict(K=abi.f64p, platform_wh=abi.i32p, image_src=abi.i32p, image_platform=abi.i32p,
                     image_pose=abi.i32p, R=abi.f64p, C=abi.f64p, vert_X=abi.f32p, vert_off=abi.i64p,
                     vert_view=abi.u32p, vert_pt=abi.i64p)
        _check(lib.sfm_dense_scene_fetch(h, *[abi.ptr(out[k], types[k]) if out[k].size else None for k in types]),
               "sfm_dense_scene_fetch")
        out["n_short"] = info.n_short
        return out
    finally:
        lib.sfm_dense_scene_destroy(h)


# ---- dense depth maps -----------------------------------------------------------------
def depth_views_default_options():
    o = abi.DepthViewsOpts()
    abi.load().sfm_depth_views_default_options(C.byref(o))
    return o


def depth_views_select(scene, opts=None):
    """sfm_depth_views_select over the dict of dense_scene(): dict(nb_off,
    nb_view, nb_score, drange [n_images, 2] float32)."""
    lib = abi.load()
    o = opts if opts is not None else depth_views_default_options()
    K = np.ascontiguousarray(np.asarray(scene["K"], np.float64).reshape(-1))
    plat = np.ascontiguousarray(np.asarray(scene["image_platform"], np.int32).reshape(-1))
    R = np.ascontiguousarray(np.asarray(scene["R"], np.float64).reshape(-1))
    Cc = np.ascontiguousarray(np.asarray(scene["C"], np.float64).reshape(-1))
    X = np.ascontiguousarray(np.asarray(scene["vert_X"], np.float32).reshape(-1))
    off = np.ascontiguousarray(np.asarray(scene["vert_off"], np.int64).reshape(-1))
    view = np.ascontiguousarray(np.asarray(scene["vert_view"], np.uint32).reshape(-1))
    n_img, n_vert = len(plat), len(off) - 1
    cap = max(n_img * max(o.max_neighbors, 0), 1)
    nb_off, nb_view = np.zeros(n_img + 1, np.int64), np.zeros(cap, np.int32)
    nb_score, drange = np.zeros(cap), np.zeros((max(n_img, 1), 2), np.float32)
    one = np.zeros(9)
    _check(lib.sfm_depth_views_select(len(K) // 9, n_img, n_vert, abi.ptr(K if len(K) else one, abi.f64p),
                                      abi.ptr(plat if n_img else np.zeros(1, np.int32), abi.i32p),
                                      abi.ptr(R if n_img else one, abi.f64p), abi.ptr(Cc if n_img else one, abi.f64p),
                                      abi.ptr(X if n_vert else np.zeros(3, np.float32), abi.f32p), abi.ptr(off, abi.i64p),
                                      abi.ptr(view if len(view) else np.zeros(1, np.uint32), abi.u32p), C.byref(o),
                                      abi.ptr(nb_off, abi.i64p), abi.ptr(nb_view, abi.i32p), abi.ptr(nb_score, abi.f64p),
                                      abi.ptr(drange, abi.f32p)), "sfm_depth_views_select")
    n = int(nb_off[-1])
    return dict(nb_off=nb_off, nb_view=nb_view[:n].copy(), nb_score=nb_score[:n].copy(), drange=drange[:n_img])


def depthmap_default_options():
    o = abi.DepthmapOpts()
    abi.load().sfm_depthmap_default_options(C.byref(o))
    return o


def depthmap_filter_default_options():
    o = abi.DepthmapFilterOpts()
    abi.load().sfm_depthmap_filter_default_options(C.byref(o))
    return o


def _depth_cameras(wh, K, R, Cc, nb_off, nb_view):
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    n_img = len(wh) // 2
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(-1))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1))
    Cc = np.ascontiguousarray(np.asarray(Cc, np.float64).reshape(-1))
    nb_off = np.ascontiguousarray(np.asarray(nb_off, np.int64).reshape(-1))
    nb_view = np.ascontiguousarray(np.asarray(nb_view, np.int32).reshape(-1))
    assert len(K) == 9 * n_img and len(R) == 9 * n_img and len(Cc) == 3 * n_img and len(nb_off) == n_img + 1
    n_map = int((wh[0::2].astype(np.int64) * wh[1::2]).sum()) if n_img and (wh > 0).all() else 0
    one = np.zeros(9)
    ptrs = (abi.ptr(K if n_img else one, abi.f64p), abi.ptr(R if n_img else one, abi.f64p),
            abi.ptr(Cc if n_img else one, abi.f64p), abi.ptr(nb_off, abi.i64p),
            abi.ptr(nb_view if len(nb_view) else np.zeros(1, np.int32), abi.i32p))
    keep = (wh, K, R, Cc, nb_off, nb_view, one)
    return wh, n_img, n_map, ptrs, keep


def _map_views(wh, arr, comps=1):
    out, at = [], 0
    for i in range(len(wh) // 2):
        w, h = int(wh[2 * i]), int(wh[2 * i + 1])
        v = arr[comps * at:comps * (at + w * h)]
        out.append(v.reshape(h, w) if comps == 1 else v.reshape(h, w, comps))
        at += w * h
    return out


def depthmap(ctx, wh, K, R, Cc, nb_off, nb_view, drange, images=None, opts=None, pool=None, init_depth=None,
             init_normal=None):
    """sfm_depthmap (ctx None: sfm_depthmap_host).  K, R [n_img, 3, 3], Cc
    [n_img, 3]; images as in undistort(); init_depth / init_normal: flat
    float32 arrays laid out as the maps.  dict(depth, normal, cost (flat),
    depth_maps / normal_maps / cost_maps (views per image), stats)."""
    lib = abi.load()
    wh, n_img, n_map, cams, keep = _depth_cameras(wh, K, R, Cc, nb_off, nb_view)
    channels, img_off, pixels = pool if pool is not None else _pixel_pool(images)
    drange = np.ascontiguousarray(np.asarray(drange, np.float32).reshape(-1))
    assert len(drange) == 2 * n_img
    depth, normal, cost = (np.zeros(max(k * n_map, 1), np.float32) for k in (1, 3, 1))
    if init_depth is not None:
        init_depth = np.ascontiguousarray(np.asarray(init_depth, np.float32).reshape(-1))
        assert len(init_depth) == n_map
    if init_normal is not None:
        init_normal = np.ascontiguousarray(np.asarray(init_normal, np.float32).reshape(-1))
        assert len(init_normal) == 3 * n_map
    st = abi.DepthmapStats()
    args = (n_img, abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p), abi.ptr(channels, abi.i32p),
            abi.ptr(img_off, abi.i64p), abi.ptr(pixels, abi.u8p), cams[0], cams[1], cams[2], cams[3], cams[4],
            abi.ptr(drange if n_img else np.zeros(2, np.float32), abi.f32p), abi.ptr(init_depth, abi.f32p),
            abi.ptr(init_normal, abi.f32p), C.byref(opts) if opts is not None else None, abi.ptr(depth, abi.f32p),
            abi.ptr(normal, abi.f32p), abi.ptr(cost, abi.f32p), C.byref(st))
    if ctx is None:
        _check(lib.sfm_depthmap_host(*args), "sfm_depthmap_host")
    else:
        _check(lib.sfm_depthmap(ctx.h, *args), "sfm_depthmap")
    depth, normal, cost = depth[:n_map], normal[:3 * n_map], cost[:n_map]
    return dict(depth=depth, normal=normal, cost=cost, depth_maps=_map_views(wh, depth),
                normal_maps=_map_views(wh, normal, 3), cost_maps=_map_views(wh, cost), stats=_struct_dict(st))


def depthmap_host(wh, K, R, Cc, nb_off, nb_view, drange, images=None, opts=None, pool=None, init_depth=None,
                  init_normal=None):
    return depthmap(None, wh, K, R, Cc, nb_off, nb_view, drange, images, opts, pool, init_depth, init_normal)


def depthmap_filter(ctx, wh, K, R, Cc, nb_off, nb_view, depth, cost, opts=None):
    """sfm_depthmap_filter (ctx None: sfm_depthmap_filter_host) over the flat
    maps of depthmap().  dict(depth (flat), n_agree (flat uint8), depth_maps,
    counts [n_img, 2] (candidates, kept), stats)."""
    lib = abi.load()
    wh, n_img, n_map, cams, keep = _depth_cameras(wh, K, R, Cc, nb_off, nb_view)
    depth = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(-1))
    cost = np.ascontiguousarray(np.asarray(cost, np.float32).reshape(-1))
    assert len(depth) == len(cost) and (n_map == 0 or len(depth) == n_map)
    out, agree = np.zeros(max(n_map, 1), np.float32), np.zeros(max(n_map, 1), np.uint8)
    counts = np.zeros((max(n_img, 1), 2), np.int64)
    st = abi.DepthmapFilterStats()
    args = (n_img, abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p), cams[0], cams[1], cams[2], cams[3], cams[4],
            abi.ptr(depth if n_map else np.zeros(1, np.float32), abi.f32p),
            abi.ptr(cost if n_map else np.zeros(1, np.float32), abi.f32p), C.byref(opts) if opts is not None else None,
            abi.ptr(out, abi.f32p), abi.ptr(agree, abi.u8p), abi.ptr(counts, abi.i64p), C.byref(st))
    if ctx is None:
        _check(lib.sfm_depthmap_filter_host(*args), "sfm_depthmap_filter_host")
    else:
        _check(lib.sfm_depthmap_filter(ctx.h, *args), "sfm_depthmap_filter")
    out, agree = out[:n_map], agree[:n_map]
    return dict(depth=out, n_agree=agree, depth_maps=_map_views(wh, out), counts=counts[:n_img],
                stats=_struct_dict(st))


def depthmap_filter_host(wh, K, R, Cc, nb_off, nb_view, depth, cost, opts=None):
    return depthmap_filter(None, wh, K, R, Cc, nb_off, nb_view, depth, cost, opts)


# ---- dense fusion ---------------------------------------------------------------------
def depthmap_fuse_default_options():
    o = abi.DepthmapFuseOpts()
    abi.load().sfm_depthmap_fuse_default_options(C.byref(o))
    return o


def _cloud_arrays(cap, fill=0):
    n = max(cap, 1)
    return dict(X=np.full(3 * n, fill, np.float32), N=np.full(3 * n, fill, np.float32), rgb=np.full(3 * n, fill, np.uint8),
                n_views=np.full(n, fill, np.uint8), view_mask=np.full(n, fill, np.uint32),
                src_image=np.full(n, fill, np.int32), src_pixel=np.full(n, fill, np.int32))


def _cloud_ptrs(cap, a):
    return (cap, abi.ptr(a["X"], abi.f32p), abi.ptr(a["N"], abi.f32p), abi.ptr(a["rgb"], abi.u8p),
            abi.ptr(a["n_views"], abi.u8p), abi.ptr(a["view_mask"], abi.u32p), abi.ptr(a["src_image"], abi.i32p),
            abi.ptr(a["src_pixel"], abi.i32p))


def _cloud_dict(a, n, colours, stats):
    return dict(X=a["X"][:3 * n].reshape(-1, 3), N=a["N"][:3 * n].reshape(-1, 3),
                rgb=a["rgb"][:3 * n].reshape(-1, 3) if colours else None, n_views=a["n_views"][:n],
                view_mask=a["view_mask"][:n], src_image=a["src_image"][:n], src_pixel=a["src_pixel"][:n], stats=stats)


def depthmap_fuse_raw(ctx, wh, K, R, Cc, nb_off, nb_view, depth, normal, images=None, opts=None, pool=None,
                      cap_points=None, fill=0):
    """sfm_depthmap_fuse (ctx None: sfm_depthmap_fuse_host) without the check of
    its return code: (rc, the cloud's arrays at their full capacity, pre-filled
    with `fill`, the stats dict).  cap_points None: the pixels with depth > 0."""
    lib = abi.load()
    wh, n_img, n_map, cams, keep = _depth_cameras(wh, K, R, Cc, nb_off, nb_view)
    depth = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(-1))
    normal = np.ascontiguousarray(np.asarray(normal, np.float32).reshape(-1))
    assert n_map == 0 or (len(depth) == n_map and len(normal) == 3 * n_map)
    colours = images is not None or pool is not None
    channels, img_off, pixels = (pool if pool is not None else _pixel_pool(images)) if colours else (None, None, None)
    cap = int((depth[:n_map] > 0).sum()) if cap_points is None else int(cap_points)
    arrays = _cloud_arrays(cap, fill)
    st = abi.DepthmapFuseStats()
    args = (n_img, abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p), abi.ptr(channels, abi.i32p),
            abi.ptr(img_off, abi.i64p), abi.ptr(pixels, abi.u8p), cams[0], cams[1], cams[2], cams[3], cams[4],
            abi.ptr(depth if n_map else np.zeros(1, np.float32), abi.f32p),
            abi.ptr(normal if n_map else np.zeros(3, np.float32), abi.f32p),
            C.byref(opts) if opts is not None else None) + _cloud_ptrs(cap, arrays) + (C.byref(st),)
    rc = lib.sfm_depthmap_fuse_host(*args) if ctx is None else lib.sfm_depthmap_fuse(ctx.h, *args)
    return rc, arrays, _struct_dict(st)


def depthmap_fuse(ctx, wh, K, R, Cc, nb_off, nb_view, depth, normal, images=None, opts=None, pool=None):
    """sfm_depthmap_fuse (ctx None: sfm_depthmap_fuse_host) over the filter's
    depth and depthmap()'s normal (flat); images as in undistort(), None: no
    colours.  dict(X, N [n, 3] float32, rgb [n, 3] uint8 or None, n_views
    (uint8), view_mask (uint32), src_image, src_pixel (int32), stats)."""
    rc, arrays, st = depthmap_fuse_raw(ctx, wh, K, R, Cc, nb_off, nb_view, depth, normal, images, opts, pool)
    _check(rc, "sfm_depthmap_fuse_host" if ctx is None else "sfm_depthmap_fuse")
    return _cloud_dict(arrays, st["n_points"], images is not None or pool is not None, st)


def depthmap_fuse_host(wh, K, R, Cc, nb_off, nb_view, depth, normal, images=None, opts=None, pool=None):
    return depthmap_fuse(None, wh, K, R, Cc, nb_off, nb_view, depth, normal, images, opts, pool)


def densify(ctx, wh, K, R, Cc, nb_off, nb_view, drange, images=None, opts=None, filter_opts=None, fuse_opts=None,
            pool=None, init_depth=None, init_normal=None, maps=True):
    """sfm_densify (ctx None: sfm_densify_host): depth maps, filter and fusion in
    one call.  The cloud as depthmap_fuse() returns it, plus, with maps=True,
    depth, normal, cost, depth_filtered (flat float32), n_agree (uint8) and
    counts [n_img, 2]; maps=False leaves the maps on the device."""
    lib = abi.load()
    wh, n_img, n_map, cams, keep = _depth_cameras(wh, K, R, Cc, nb_off, nb_view)
    channels, img_off, pixels = pool if pool is not None else _pixel_pool(images)
    drange = np.ascontiguousarray(np.asarray(drange, np.float32).reshape(-1))
    assert len(drange) == 2 * n_img
    if init_depth is not None:
        init_depth = np.ascontiguousarray(np.asarray(init_depth, np.float32).reshape(-1))
        assert len(init_depth) == n_map
    if init_normal is not None:
        init_normal = np.ascontiguousarray(np.asarray(init_normal, np.float32).reshape(-1))
        assert len(init_normal) == 3 * n_map
    arrays = _cloud_arrays(n_map)
    m = dict(depth=np.zeros(max(n_map, 1), np.float32), normal=np.zeros(max(3 * n_map, 1), np.float32),
             cost=np.zeros(max(n_map, 1), np.float32), depth_filtered=np.zeros(max(n_map, 1), np.float32),
             n_agree=np.zeros(max(n_map, 1), np.uint8), counts=np.zeros((max(n_img, 1), 2), np.int64)) if maps else {}
    st = abi.DensifyStats()
    opt = lambda o: C.byref(o) if o is not None else None
    args = (n_img, abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p), abi.ptr(channels, abi.i32p),
            abi.ptr(img_off, abi.i64p), abi.ptr(pixels, abi.u8p), cams[0], cams[1], cams[2], cams[3], cams[4],
            abi.ptr(drange if n_img else np.zeros(2, np.float32), abi.f32p), abi.ptr(init_depth, abi.f32p),
            abi.ptr(init_normal, abi.f32p), opt(opts), opt(filter_opts), opt(fuse_opts)) + _cloud_ptrs(n_map, arrays) + (
            abi.ptr(m.get("depth"), abi.f32p), abi.ptr(m.get("normal"), abi.f32p), abi.ptr(m.get("cost"), abi.f32p),
            abi.ptr(m.get("depth_filtered"), abi.f32p), abi.ptr(m.get("n_agree"), abi.u8p),
            abi.ptr(m.get("counts"), abi.i64p), C.byref(st))
    if ctx is None:
        _check(lib.sfm_densify_host(*args), "sfm_densify_host")
    else:
        _check(lib.sfm_densify(ctx.h, *args), "sfm_densify")
    sd = _struct_dict(st)
    out = _cloud_dict(arrays, sd["fuse"]["n_points"], True, sd)
    if maps:
        out.update(depth=m["depth"][:n_map], normal=m["normal"][:3 * n_map], cost=m["cost"][:n_map],
                   depth_filtered=m["depth_filtered"][:n_map], n_agree=m["n_agree"][:n_map], counts=m["counts"][:n_img])
    return out


def densify_host(wh, K, R, Cc, nb_off, nb_view, drange, images=None, opts=None, filter_opts=None, fuse_opts=None,
                 pool=None, init_depth=None, init_normal=None, maps=True):
    return densify(None, wh, K, R, Cc, nb_off, nb_view, drange, images, opts, filter_opts, fuse_opts, pool, init_depth,
                   init_normal, maps)


def dense_cloud_views(n_img, nb_off, nb_view, src_image, view_mask):
    """sfm_dense_cloud_views: (view_off [n + 1] int64, view_idx int32), the
    images that see each point: its own first, then its agreeing fusion pairs."""
    lib = abi.load()
    nb_off = np.ascontiguousarray(np.asarray(nb_off, np.int64).reshape(-1))
    nb_view = np.ascontiguousarray(np.asarray(nb_view, np.int32).reshape(-1))
    src = np.ascontiguousarray(np.asarray(src_image, np.int32).reshape(-1))
    mask = np.ascontiguousarray(np.asarray(view_mask, np.uint32).reshape(-1))
    n = len(src)
    assert len(mask) == n and len(nb_off) == n_img + 1
    off = np.zeros(n + 1, np.int64)
    args = (n_img, abi.ptr(nb_off, abi.i64p), abi.ptr(nb_view if len(nb_view) else np.zeros(1, np.int32), abi.i32p), n,
            abi.ptr(src if n else np.zeros(1, np.int32), abi.i32p), abi.ptr(mask if n else np.zeros(1, np.uint32), abi.u32p),
            abi.ptr(off, abi.i64p))
    _check(lib.sfm_dense_cloud_views(*args, None), "sfm_dense_cloud_views")
    idx = np.zeros(max(int(off[-1]), 1), np.int32)
    _check(lib.sfm_dense_cloud_views(*args, abi.ptr(idx, abi.i32p)), "sfm_dense_cloud_views")
    return off, idx[:int(off[-1])]


def dense_cloud_write_ply(path, X, N=None, rgb=None):
    """sfm_dense_cloud_write_ply: binary little-endian x y z [nx ny nz] [red green blue]"""
    X = np.ascontiguousarray(np.asarray(X, np.float32).reshape(-1, 3))
    n = len(X)
    N = None if N is None else np.ascontiguousarray(np.asarray(N, np.float32).reshape(-1, 3))
    rgb = None if rgb is None else np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3))
    assert (N is None or len(N) == n) and (rgb is None or len(rgb) == n)
    pad = lambda a, t: a if a is None or n else np.zeros(3, t)
    _check(abi.load().sfm_dense_cloud_write_ply(_b(path), n, abi.ptr(X if n else np.zeros(3, np.float32), abi.f32p),
                                               abi.ptr(pad(N, np.float32), abi.f32p), abi.ptr(pad(rgb, np.uint8), abi.u8p)),
           "sfm_dense_cloud_write_ply")


# ---- mesh -----------------------------------------------------------------------------
def tsdf_default_options():
    o = abi.TsdfOpts()
    abi.load().sfm_tsdf_default_options(C.byref(o))
    return o


def mesh_default_options():
    o = abi.MeshOpts()
    abi.load().sfm_mesh_default_options(C.byref(o))
    return o


def mesh_grid(origin, voxel, dims):
    """an sfm_mesh_grid from origin [3], voxel and dims (nx, ny, nz)"""
    g = abi.MeshGrid()
    g.origin[:] = [float(v) for v in origin]
    g.voxel = float(voxel)
    g.dims[:] = [int(v) for v in dims]
    return g


def mesh_grid_fit(X, resolution, margin_voxels=2):
    """sfm_mesh_grid_fit: the grid (abi.MeshGrid) around the cloud X [n, 3]"""
    X = np.ascontiguousarray(np.asarray(X, np.float32).reshape(-1))
    g = abi.MeshGrid()
    _check(abi.load().sfm_mesh_grid_fit(len(X) // 3, abi.ptr(X if len(X) else np.zeros(3, np.float32), abi.f32p),
                                        int(resolution), int(margin_voxels), C.byref(g)), "sfm_mesh_grid_fit")
    return g


def _tsdf_inputs(wh, K, R, Cc, depth, images, pool):
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    n_img = len(wh) // 2
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(-1))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1))
    Cc = np.ascontiguousarray(np.asarray(Cc, np.float64).reshape(-1))
    assert len(K) == 9 * n_img and len(R) == 9 * n_img and len(Cc) == 3 * n_img
    n_map = int((wh[0::2].astype(np.int64) * wh[1::2]).sum()) if n_img and (wh > 0).all() else 0
    depth = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(-1))
    assert n_map == 0 or len(depth) == n_map
    colours = images is not None or pool is not None
    channels, img_off, pixels = (pool if pool is not None else _pixel_pool(images)) if colours else (None, None, None)
    one = np.zeros(9)
    keep = (wh, K, R, Cc, depth, channels, img_off, pixels, one)
    args = (n_img, abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p), abi.ptr(channels, abi.i32p),
            abi.ptr(img_off, abi.i64p), abi.ptr(pixels, abi.u8p), abi.ptr(K if n_img else one, abi.f64p),
            abi.ptr(R if n_img else one, abi.f64p), abi.ptr(Cc if n_img else one, abi.f64p),
            abi.ptr(depth if n_map else np.zeros(1, np.float32), abi.f32p))
    return args, colours, keep


def _grid_points(grid):
    d = [int(v) for v in grid.dims]
    return d[0] * d[1] * d[2] if min(d) > 0 and d[0] * d[1] * d[2] < 2 ** 31 else 0


def tsdf_integrate(ctx, wh, K, R, Cc, depth, grid, images=None, opts=None, pool=None):
    """sfm_tsdf_integrate (ctx None: sfm_tsdf_integrate_host) over the filter's
    depth (flat); images as in undistort(), None: no colours.  dict(tsdf
    (float32), weight (uint8), rgb [n, 3] and has_rgb (uint8) or None, flat over
    the lattice's raster; stats)."""
    lib = abi.load()
    args, colours, keep = _tsdf_inputs(wh, K, R, Cc, depth, images, pool)
    n = max(_grid_points(grid), 1)
    tsdf, weight = np.zeros(n, np.float32), np.zeros(n, np.uint8)
    rgb, has = (np.zeros(3 * n, np.uint8), np.zeros(n, np.uint8)) if colours else (None, None)
    st = abi.TsdfStats()
    args = args + (C.byref(grid), C.byref(opts) if opts is not None else None, abi.ptr(tsdf, abi.f32p),
                   abi.ptr(weight, abi.u8p), abi.ptr(rgb, abi.u8p), abi.ptr(has, abi.u8p), C.byref(st))
    if ctx is None:
        _check(lib.sfm_tsdf_integrate_host(*args), "sfm_tsdf_integrate_host")
    else:
        _check(lib.sfm_tsdf_integrate(ctx.h, *args), "sfm_tsdf_integrate")
    return dict(tsdf=tsdf, weight=weight, rgb=rgb.reshape(-1, 3) if colours else None, has_rgb=has,
                stats=_struct_dict(st))


def _mesh_arrays(cap_v, cap_t, fill=0):
    return dict(V=np.full(3 * max(cap_v, 1), fill, np.float32), rgb=np.full(3 * max(cap_v, 1), fill, np.uint8),
                tri=np.full(3 * max(cap_t, 1), fill, np.int32))


def _mesh_ptrs(cap_v, cap_t, a):
    return (cap_v, cap_t, abi.ptr(a["V"], abi.f32p), abi.ptr(a["rgb"], abi.u8p), abi.ptr(a["tri"], abi.i32p))


def _mesh_dict(a, st, colours, stats):
    nv, nt = st["n_vertices"], st["n_triangles"]
    return dict(V=a["V"][:3 * nv].reshape(-1, 3), rgb=a["rgb"][:3 * nv].reshape(-1, 3) if colours else None,
                tri=a["tri"][:3 * nt].reshape(-1, 3), stats=stats)


def mesh_extract_raw(ctx, grid, tsdf, weight, rgb=None, has_rgb=None, opts=None, cap_vertices=0, cap_triangles=0,
                     fill=0):
    """sfm_mesh_extract (ctx None: sfm_mesh_extract_host) without the check of
    its return code: (rc, the mesh's arrays at their full capacity, pre-filled
    with `fill`, the stats dict)."""
    lib = abi.load()
    tsdf = np.ascontiguousarray(np.asarray(tsdf, np.float32).reshape(-1))
    weight = np.ascontiguousarray(np.asarray(weight, np.uint8).reshape(-1))
    n = _grid_points(grid)
    assert n == 0 or (len(tsdf) == n and len(weight) == n)
    if rgb is not None:
        rgb = np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1))
        has_rgb = np.ascontiguousarray(np.asarray(has_rgb, np.uint8).reshape(-1))
        assert n == 0 or (len(rgb) == 3 * n and len(has_rgb) == n)
    arrays = _mesh_arrays(int(cap_vertices), int(cap_triangles), fill)
    st = abi.MeshStats()
    args = (C.byref(grid), abi.ptr(tsdf, abi.f32p), abi.ptr(weight, abi.u8p), abi.ptr(rgb, abi.u8p),
            abi.ptr(has_rgb if rgb is not None else None, abi.u8p), C.byref(opts) if opts is not None else None
            ) + _mesh_ptrs(int(cap_vertices), int(cap_triangles), arrays) + (C.byref(st),)
    rc = lib.sfm_mesh_extract_host(*args) if ctx is None else lib.sfm_mesh_extract(ctx.h, *args)
    return rc, arrays, _struct_dict(st)


def mesh_extract(ctx, grid, tsdf, weight, rgb=None, has_rgb=None, opts=None, cap_vertices=None, cap_triangles=None):
    """sfm_mesh_extract (ctx None: sfm_mesh_extract_host).  Without caps the
    call is made twice: once to learn the needs, once with them.  dict(V [n, 3]
    float32, rgb [n, 3] uint8 or None, tri [m, 3] int32, stats)."""
    where = "sfm_mesh_extract_host" if ctx is None else "sfm_mesh_extract"
    cv, ct = (0, 0) if cap_vertices is None else (cap_vertices, cap_triangles)
    rc, arrays, st = mesh_extract_raw(ctx, grid, tsdf, weight, rgb, has_rgb, opts, cv, ct)
    if cap_vertices is None and rc == abi.SFM_ERR_INVALID_ARG and st["n_vertices"] > 0:
        rc, arrays, st = mesh_extract_raw(ctx, grid, tsdf, weight, rgb, has_rgb, opts, st["n_vertices"], st["n_triangles"])
    _check(rc, where)
    return _mesh_dict(arrays, st, rgb is not None, st)


def mesh_reconstruct_raw(ctx, wh, K, R, Cc, depth, grid, images=None, tsdf_opts=None, mesh_opts=None, pool=None,
                         cap_vertices=0, cap_triangles=0, volume=False, fill=0):
    """sfm_mesh_reconstruct (ctx None: sfm_mesh_reconstruct_host) without the
    check of its return code: (rc, arrays, stats dict, tsdf, weight); the volume
    is fetched only with volume=True."""
    lib = abi.load()
    args, colours, keep = _tsdf_inputs(wh, K, R, Cc, depth, images, pool)
    n = max(_grid_points(grid), 1)
    tsdf, weight = (np.zeros(n, np.float32), np.zeros(n, np.uint8)) if volume else (None, None)
    arrays = _mesh_arrays(int(cap_vertices), int(cap_triangles), fill)
    st = abi.MeshReconstructStats()
    opt = lambda o: C.byref(o) if o is not None else None
    args = args + (C.byref(grid), opt(tsdf_opts), opt(mesh_opts)) + _mesh_ptrs(int(cap_vertices), int(cap_triangles), arrays) + (
        abi.ptr(tsdf, abi.f32p), abi.ptr(weight, abi.u8p), C.byref(st))
    rc = lib.sfm_mesh_reconstruct_host(*args) if ctx is None else lib.sfm_mesh_reconstruct(ctx.h, *args)
    return rc, arrays, _struct_dict(st), tsdf, weight


def mesh_reconstruct(ctx, wh, K, R, Cc, depth, grid, images=None, tsdf_opts=None, mesh_opts=None, pool=None,
                     cap_vertices=None, cap_triangles=None, volume=False):
    """sfm_mesh_reconstruct (ctx None: sfm_mesh_reconstruct_host): integration
    and extraction in one call.  The mesh as mesh_extract() returns it, plus,
    with volume=True, tsdf and weight.  Without caps the call is made twice."""
    where = "sfm_mesh_reconstruct_host" if ctx is None else "sfm_mesh_reconstruct"
    call = lambda cv, ct: mesh_reconstruct_raw(ctx, wh, K, R, Cc, depth, grid, images, tsdf_opts, mesh_opts, pool, cv, ct,
                                               volume)
    rc, arrays, st, tsdf, weight = call(*((0, 0) if cap_vertices is None else (cap_vertices, cap_triangles)))
    if cap_vertices is None and rc == abi.SFM_ERR_INVALID_ARG and st["mesh"]["n_vertices"] > 0:
        rc, arrays, st, tsdf, weight = call(st["mesh"]["n_vertices"], st["mesh"]["n_triangles"])
    _check(rc, where)
    out = _mesh_dict(arrays, st["mesh"], images is not None or pool is not None, st)
    if volume:
        out.update(tsdf=tsdf, weight=weight)
    return out


def mesh_write_ply(path, V, tri, rgb=None):
    """sfm_mesh_write_ply: binary little-endian x y z [red green blue], then the faces"""
    V = np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3))
    tri = np.ascontiguousarray(np.asarray(tri, np.int32).reshape(-1, 3))
    rgb = None if rgb is None else np.ascontiguousarray(np.asarray(rgb, np.uint8).reshape(-1, 3))
    assert rgb is None or len(rgb) == len(V)
    n, m = len(V), len(tri)
    _check(abi.load().sfm_mesh_write_ply(_b(path), n, abi.ptr(V if n else np.zeros(3, np.float32), abi.f32p),
                                        abi.ptr(rgb if rgb is None or n else np.zeros(3, np.uint8), abi.u8p), m,
                                        abi.ptr(tri if m else np.zeros(3, np.int32), abi.i32p)), "sfm_mesh_write_ply")


# ---- mesh texture ---------------------------------------------------------------------
def mesh_texture_default_options():
    o = abi.MeshTextureOpts()
    abi.load().sfm_mesh_texture_default_options(C.byref(o))
    return o


def mesh_atlas_fit_raw(n_triangles, cell=abi.TEX_DEFAULT_CELL):
    """sfm_mesh_atlas_fit without the check of its return code: (rc, W, H, cols)"""
    W, H, cols = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    rc = abi.load().sfm_mesh_atlas_fit(int(n_triangles), int(cell), C.byref(W), C.byref(H), C.byref(cols))
    return rc, W.value, H.value, cols.value


def mesh_atlas_fit(n_triangles, cell=abi.TEX_DEFAULT_CELL):
    """sfm_mesh_atlas_fit: (W, H, cols) of the atlas of n_triangles faces"""
    rc, W, H, cols = mesh_atlas_fit_raw(n_triangles, cell)
    _check(rc, "sfm_mesh_atlas_fit")
    return W, H, cols


def _texture_inputs(wh, K, R, Cc, V, tri, images, pool, vertex_rgb=None):
    wh = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    n_img = len(wh) // 2
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(-1))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(-1))
    Cc = np.ascontiguousarray(np.asarray(Cc, np.float64).reshape(-1))
    assert len(K) == 9 * n_img and len(R) == 9 * n_img and len(Cc) == 3 * n_img
    V = np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1))
    tri = np.ascontiguousarray(np.asarray(tri, np.int32).reshape(-1))
    n_v, n_t = len(V) // 3, len(tri) // 3
    colours = images is not None or pool is not None
    channels, img_off, pixels = (pool if pool is not None else _pixel_pool(images)) if colours else (None, None, None)
    if vertex_rgb is not None:
        vertex_rgb = np.ascontiguousarray(np.asarray(vertex_rgb, np.uint8).reshape(-1))
        assert len(vertex_rgb) == 3 * n_v
    one = np.zeros(9)
    keep = (wh, K, R, Cc, V, tri, channels, img_off, pixels, vertex_rgb, one)
    img = (n_img, abi.ptr(wh if n_img else np.zeros(2, np.int32), abi.i32p), abi.ptr(channels, abi.i32p),
           abi.ptr(img_off, abi.i64p), abi.ptr(pixels, abi.u8p), abi.ptr(K if n_img else one, abi.f64p),
           abi.ptr(R if n_img else one, abi.f64p), abi.ptr(Cc if n_img else one, abi.f64p))
    Vp = (n_v, abi.ptr(V if n_v else np.zeros(3, np.float32), abi.f32p))
    tp = (n_t, abi.ptr(tri if n_t else np.zeros(3, np.int32), abi.i32p))
    return img, Vp, abi.ptr(vertex_rgb, abi.u8p), tp, n_t, keep


def _texture_cell(opts):
    return int(opts.cell) if opts is not None else abi.TEX_DEFAULT_CELL


def _atlas_arrays(n_t, opts, fill):
    rc, W, H, _ = mesh_atlas_fit_raw(max(n_t, 0), _texture_cell(opts))
    if rc != 0:
        W = H = 0
    return np.full(max(3 * W * H, 1), fill, np.uint8), np.full(max(6 * n_t, 1), fill, np.float32), W, H


def mesh_face_views_raw(ctx, wh, K, R, Cc, V, tri, images=None, opts=None, pool=None, fill=0):
    """sfm_mesh_face_views (ctx None: sfm_mesh_face_views_host) without the
    check of its return code: (rc, face_view, face_pixels, stats dict); the
    arrays are pre-filled with `fill`."""
    lib = abi.load()
    img, Vp, _, tp, n_t, keep = _texture_inputs(wh, K, R, Cc, V, tri, images, pool)
    fv, fp = np.full(max(n_t, 1), fill, np.int32), np.full(max(n_t, 1), fill, np.int32)
    st = abi.MeshFaceViewsStats()
    args = img + Vp + tp + (C.byref(opts) if opts is not None else None, abi.ptr(fv, abi.i32p), abi.ptr(fp, abi.i32p),
                            C.byref(st))
    rc = lib.sfm_mesh_face_views_host(*args) if ctx is None else lib.sfm_mesh_face_views(ctx.h, *args)
    return rc, fv[:n_t], fp[:n_t], _struct_dict(st)


def mesh_face_views(ctx, wh, K, R, Cc, V, tri, images=None, opts=None, pool=None):
    """sfm_mesh_face_views (ctx None: the host twin): dict(face_view, face_pixels
    [n_triangles] int32, stats).  images as in undistort(): None entries are
    skipped views; images None: every view counts."""
    rc, fv, fp, st = mesh_face_views_raw(ctx, wh, K, R, Cc, V, tri, images, opts, pool)
    _check(rc, "sfm_mesh_face_views_host" if ctx is None else "sfm_mesh_face_views")
    return dict(face_view=fv, face_pixels=fp, stats=st)


def mesh_texture_bake_raw(ctx, wh, K, R, Cc, V, tri, face_view, images=None, vertex_rgb=None, opts=None, pool=None,
                          fill=0):
    """sfm_mesh_texture_bake (ctx None: the host twin) without the check of its
    return code: (rc, texture (flat), uv (flat), stats dict)."""
    lib = abi.load()
    img, Vp, vrgb, tp, n_t, keep = _texture_inputs(wh, K, R, Cc, V, tri, images, pool, vertex_rgb)
    fv = np.ascontiguousarray(np.asarray(face_view, np.int32).reshape(-1))
    assert len(fv) == n_t
    tex, uv, W, H = _atlas_arrays(n_t, opts, fill)
    st = abi.MeshBakeStats()
    args = img + Vp + (vrgb,) + tp + (abi.ptr(fv if n_t else np.zeros(1, np.int32), abi.i32p),
                                      C.byref(opts) if opts is not None else None, abi.ptr(tex, abi.u8p),
                                      abi.ptr(uv, abi.f32p), C.byref(st))
    rc = lib.sfm_mesh_texture_bake_host(*args) if ctx is None else lib.sfm_mesh_texture_bake(ctx.h, *args)
    return rc, tex, uv, _struct_dict(st)


def _texture_dict(tex, uv, n_t, st, W, H):
    return dict(texture=tex[:3 * W * H].reshape(H, W, 3), uv=uv[:6 * n_t].reshape(-1, 3, 2), stats=st)


def mesh_texture_bake(ctx, wh, K, R, Cc, V, tri, face_view, images=None, vertex_rgb=None, opts=None, pool=None):
    """sfm_mesh_texture_bake (ctx None: the host twin) with the caller's
    face_view: dict(texture [H, W, 3] uint8, top row first, uv [n, 3, 2], stats)."""
    rc, tex, uv, st = mesh_texture_bake_raw(ctx, wh, K, R, Cc, V, tri, face_view, images, vertex_rgb, opts, pool)
    _check(rc, "sfm_mesh_texture_bake_host" if ctx is None else "sfm_mesh_texture_bake")
    return _texture_dict(tex, uv, len(np.asarray(tri).reshape(-1)) // 3, st, st["W"], st["H"])


def mesh_texture_raw(ctx, wh, K, R, Cc, V, tri, images=None, vertex_rgb=None, opts=None, pool=None, fill=0,
                     views=True):
    """sfm_mesh_texture (ctx None: the host twin) without the check of its
    return code: (rc, face_view, face_pixels, texture, uv, stats dict);
    views=False: face_view and face_pixels are not fetched (None)."""
    lib = abi.load()
    img, Vp, vrgb, tp, n_t, keep = _texture_inputs(wh, K, R, Cc, V, tri, images, pool, vertex_rgb)
    fv, fp = (np.full(max(n_t, 1), fill, np.int32), np.full(max(n_t, 1), fill, np.int32)) if views else (None, None)
    tex, uv, W, H = _atlas_arrays(n_t, opts, fill)
    st = abi.MeshTextureStats()
    args = img + Vp + (vrgb,) + tp + (C.byref(opts) if opts is not None else None, abi.ptr(fv, abi.i32p),
                                      abi.ptr(fp, abi.i32p), abi.ptr(tex, abi.u8p), abi.ptr(uv, abi.f32p), C.byref(st))
    rc = lib.sfm_mesh_texture_host(*args) if ctx is None else lib.sfm_mesh_texture(ctx.h, *args)
    return rc, (fv[:n_t] if views else None), (fp[:n_t] if views else None), tex, uv, _struct_dict(st)


def mesh_texture(ctx, wh, K, R, Cc, V, tri, images=None, vertex_rgb=None, opts=None, pool=None, views=True):
    """sfm_mesh_texture (ctx None: the host twin): face views and bake in one
    call.  dict(texture, uv, stats, and with views=True face_view, face_pixels)."""
    rc, fv, fp, tex, uv, st = mesh_texture_raw(ctx, wh, K, R, Cc, V, tri, images, vertex_rgb, opts, pool, views=views)
    _check(rc, "sfm_mesh_texture_host" if ctx is None else "sfm_mesh_texture")
    out = _texture_dict(tex, uv, len(np.asarray(tri).reshape(-1)) // 3, st, st["bake"]["W"], st["bake"]["H"])
    if views:
        out.update(face_view=fv, face_pixels=fp)
    return out


def mesh_write_textured_ply(path, texture_name, V, tri, uv):
    """sfm_mesh_write_textured_ply: x y z, then per face the indices and six texture coordinates"""
    V = np.ascontiguousarray(np.asarray(V, np.float32).reshape(-1, 3))
    tri = np.ascontiguousarray(np.asarray(tri, np.int32).reshape(-1, 3))
    uv = np.ascontiguousarray(np.asarray(uv, np.float32).reshape(-1, 6))
    assert len(uv) == len(tri)
    n, m = len(V), len(tri)
    _check(abi.load().sfm_mesh_write_textured_ply(_b(path), _b(texture_name),
                                                  n, abi.ptr(V if n else np.zeros(3, np.float32), abi.f32p), m,
                                                  abi.ptr(tri if m else np.zeros(3, np.int32), abi.i32p),
                                                  abi.ptr(uv if m else np.zeros(6, np.float32), abi.f32p)),
           "sfm_mesh_write_textured_ply")
