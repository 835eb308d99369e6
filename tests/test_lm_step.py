"""CPU: single Levenberg-Marquardt iterations of oracle/ba_oracle.cpp against
the extended-precision reference tests/_lm_reference.py (H dense in
longdouble up to 2500 unknowns, matrix-free past that; the same 2^-60
certificate either way).

For every scene and threads in {1, 2, 3, 8} (the three many-tile scenes of
LARGE: 8 only) the oracle runs with
max_num_iterations = n (n = 1, 2, 3; all tolerances 0, so it takes exactly n
iterations).  The reference is fed the oracle's own x_{n-1} (the parameters
the n-1 run wrote back) and trace[n-1].trust_region_radius, so every
iteration is an independent single-step check: x_n - x_{n-1} and every
sfm_ba_iter field of iteration n are compared.  Nothing compounds.

Tolerances (u = 2^-53, kappa = cond_2(H) of the reference's fp64 copy of H,
B = C_STEP kappa u; y the step in the Jacobi-scaled space, g = J_s' f):
  step                 |y - y_ref|_2 <= B |y_ref|_2 + |ulp(x) / scale|_2
                       (a backward-stable fp64 formation and solve; the ulp
                       term is the fp64 subtraction x_n - x_{n-1});  after a
                       rejected step x_n == x_{n-1} bit for bit
  cost (at x_0)        1e-12 relative (a plain sum; the bar of initial_cost)
  cost (candidate),    1e-12 relative + |g|_2 |y_ref|_2 B   (first-order
  model_cost_change    propagation of the step bound);  cost_change: the sum
                       of the bounds of its two costs
  step_norm            max(scale) B |y_ref|_2 + |ulp(x)|_2   (the step bound
                       carried to the unscaled space, delta = -scale y)
  relative_decrease    (tol(cost_change) + |q| tol(model)) / (|model| - tol(model))
  trust_region_radius  recomputed in fp64 from the implementation's own
                       relative_decrease (accept: r / max(1/3, 1 - (2q-1)^3),
                       capped; reject: r / 2^k): 1e-15 relative
  gradient_max_norm    the reference's longdouble g (unscaled) at the
                       implementation's own x_n through |x - (x - g)| in
                       fp64: 1e-12 max|g| + ulp(max|x|)
  iteration, step_is_valid, step_is_successful: equal; the reference's
  relative_decrease is asserted to lie further than its tolerance from
  min_relative_decrease, so the decision is not a coin toss.
Cap: B <= 1e-6 for every scene but no_gauge, so the step bound cannot hide a
dropped block.  kappa grows with the trust-region radius (one fixed pose
leaves the scale of the scene free: J'J is singular along it and H is held up
there by diag / radius alone), so a scene that would miss the cap starts from
a smaller radius; C_STEP is never loosened.

C_STEP is measured against the reference only, never against the GPU: the
largest |y_orc - y_ref|_2 / (kappa u |y_ref|_2) of the oracle over every
scene, iteration and thread count below, times 8 (the GPU's different but
equally valid summation orders and FMA contraction), rounded up to a power
of two.  Measured on the run that filled this table (max over threads and
iterations; kappa and B at the last iteration, where the radius is largest):

  scene            unknowns  max ratio   kappa     B = C_STEP kappa u
  one_block           226   0.078       4.2e5     9.3e-11
  band_c4            1582   0.049       4.6e5     1.0e-10
  band_c4_pt         1582   0.068       1.8e6     4.1e-10
  band_arrow4        1594   0.235       4.6e5     1.0e-10
  dense_random       1078   0.075       3.5e5     7.7e-11
  dense_random_pt    1078   0.049       1.1e6     2.4e-10
  mixed              1498   0.154       5.3e5     1.2e-10
  long_track         1036   0.142       9.1e5     2.0e-10
  repeats             718   0.104       5.0e5     1.1e-10
  two_chains          688   0.070       6.0e5     1.3e-10
  snavely             693   0.031       4.6e5     1.0e-10
  snavely_intr        693   0.030       4.5e5     1.0e-10
  radial3             786   0.013       5.0e8     1.1e-7
  per_cam_pinhole    1094   0.130       1.4e6     3.1e-10
  plain               688   6.6e-7      3.1e9     6.9e-7    (radius 1e3)
  no_gauge            712   0.098       5.1e5     1.1e-10   (exempt from the cap; it meets it all the same)
  clamped             220   3.6e-4      1.8e9     4.0e-7    (radius 1e1)
  rejecting           520   0.027       1.2e7     2.6e-9    (radius 1e7, n = 1..4)
  dense_flow_wrap       10282   0.039    4.5e5     1.0e-10   (8 threads; matrix-free reference)
  percam_radial3_band    2250   0.011    3.4e9     7.6e-7    (8 threads)
  dense_chain_101       24406   0.146    5.5e5     1.2e-10   (8 threads; matrix-free reference)

  maximum ratio 0.235 (band_arrow4, 1 thread, n = 1)  ->  8 x = 1.88  ->  C_STEP = 2
  (test_c_step_is_eight_times_the_oracle_worst_ratio regenerates the table and asserts the choice)

The many-tile dense scenes (LARGE) are each the smallest that reaches its
mechanism in csrc/ba_bcr.hip, asserted through sfm_ba_dense_schedule together
with the next smaller scene that does not:
  dense_flow_wrap      214 cameras, random visibility: the dataflow solve on
                       one chain, 21 block columns, 270 tasks -- more than the
                       255 workers a 256-CU device can give, so workers take
                       several tasks in order (213 cameras: 20 columns, 247)
  percam_radial3_band  47 cameras, RADIAL3, one intrinsics block each: the
                       Cuthill-McKee tile order split over two chains, an
                       intrinsics tile among the first nt / 2 (46: one chain)
  dense_chain_101      1068 cameras: 6406 rows, 101 block columns, past the
                       dataflow limit: panel / update launches in groups of
                       four columns, then dense_back_all_kernel (1067: 100
                       columns, dataflow)
Their ratios stay below band_arrow4's, so C_STEP = 2 covers them.  CPU cost
measured on an 8-core x86 host: this module 50 s before the three scenes,
about 2 min with them (dense_chain_101 runs twice, once more for the C_STEP
table); dense_chain_101 takes 13 s for its three
reference steps (4 s each: sparse fp64 H, the 6406-row reduced system's
factor, two Lanczos runs, 2-3 refinements) and 30 s for the oracle's six
iterations (5 s each; 48 s each before the oracle's band factor went by
panels over the threads); dense_flow_wrap 2 s + 1 s, percam_radial3_band
(dense reference) 6 s + 0.4 s; the dense / matrix-free cross-check of the 18
older scenes under 1.5 s each.

gradient_max_norm is a maximum over all columns, so one trace entry witnesses
only the column class that holds the largest |g| entry.  With the generator's
default perturbation that is a camera column nearly everywhere (rotation
columns are ~10 x the point columns, and a camera sums ~60 observations), so
band_c4_pt, dense_random_pt (the length unit shrunk 100 x, points perturbed
far more than poses: point columns at x_1..x_3) and snavely_intr (l1 off: an
intrinsics column at x_0) move the maximum; GRADIENT_CLASS pins the class at
every checked point of every scene.

two_chains: 65 cameras is the smallest count for which 14-view tracks plan
two chains (64 cameras: one); it stays (688 unknowns).
rejecting: a first radius of 1e16 (Ceres' max_trust_region_radius) cannot
meet the cap (kappa ~ 1.6 radius there), so the scene starts from 1e7:
the generator's default perturbation is then rejected twice (radius / 2,
/ 4) and accepted at the third and fourth iteration; a stronger perturbation
leaves no residual in the quadratic Huber branch.
"""
import math

import numpy as np
import pytest

import _helpers as H
import _lm_reference as R

abi, api = H.abi, H.api
LD = R.LD
pytestmark = pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.SKIP_REASON)

C_STEP = 2.0
STEP_BOUND_CAP = 1e-6
THREADS = (1, 2, 3, 8)
STARRED = ("band_c4", "dense_random", "band_c4_pt", "dense_random_pt")   # run under every engine shape


# ---- scenes ---------------------------------------------------------------------
def _merge(base, extra):
    """`extra`'s points appended to `base` (same cameras: same seed and n_cam)."""
    assert base.n_cam == extra.n_cam and np.array_equal(base.extr, extra.extr)
    base.pt_offsets = np.concatenate([base.pt_offsets, base.n_obs + extra.pt_offsets[1:]])
    base.obs_img = np.concatenate([base.obs_img, extra.obs_img])
    base.obs_uv = np.concatenate([base.obs_uv, extra.obs_uv])
    base.X = np.concatenate([base.X, extra.X])
    base.gt_X = np.concatenate([base.gt_X, extra.gt_X])
    base.n_pt += extra.n_pt
    base.n_obs += extra.n_obs
    return base


def _with_repeats(sc, every=7, shift=0.3):
    """Every `every`-th point observes its first image a second time (as
    test_ba_general_gpu._with_repeats, which a CPU module cannot import)."""
    uv = sc.obs_uv.reshape(-1, 2)
    imgs, uvs, off = [], [], [0]
    for p in range(sc.n_pt):
        a, b = int(sc.pt_offsets[p]), int(sc.pt_offsets[p + 1])
        imgs.extend(sc.obs_img[a:b])
        uvs.extend(uv[a:b])
        if p % every == 0:
            imgs.append(sc.obs_img[a])
            uvs.append(uv[a] + shift)
        off.append(len(imgs))
    sc.obs_img = np.array(imgs, np.int32)
    sc.obs_uv = np.ascontiguousarray(np.array(uvs).reshape(-1))
    sc.pt_offsets = np.array(off, np.int64)
    sc.n_obs = len(imgs)
    return sc


def _flip_z(sc):
    """Cameras looking down -z, as SFM_CAM_SNAVELY's p = -P / P2 wants (X -> -X, t -> -t)."""
    for a in (sc.X, sc.gt_X):
        a *= -1.0
    for a in (sc.extr, sc.gt_extr):
        a.reshape(-1, 6)[:, 3:] *= -1.0
    return sc


def _point_heavy(sc, unit=0.01, every=40, shift=0.1):
    """Every `every`-th point displaced by `shift`, then the scene's length
    unit shrunk (X and t times `unit`; no residual changes): the point and
    translation columns of J grow by 1 / unit over the rotation columns, and
    with poses perturbed far less than points (POINT_HEAVY) the largest
    gradient entry lies in a point column."""
    sc.X.reshape(-1, 3)[::every] += shift
    for a in (sc.X, sc.gt_X):
        a *= unit
    for a in (sc.extr, sc.gt_extr):
        a.reshape(-1, 6)[:, 3:] *= unit
    return sc


POINT_HEAVY = (0.0005, 0.0002, 0.005, 5.0)     # perturb: rotation, translation, points, focal


def _rotation(w):
    th = np.linalg.norm(w)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def _clamped():
    """one_block plus: an intrinsics block and a camera nothing observes, a
    track with no observation (zero columns: the diagonal is min_lm_diagonal)
    and a single-observation track pushed 1e6 times further along its ray (the
    residual stays, its columns shrink below the clamp with a gradient on them)."""
    sc = H.Scene(8, 60, 3, n_intr=2, outliers=0.2)
    sc.img_intr[:] = 0                                     # intrinsics block 1: no image
    dead = 5
    assert dead != sc.const_img
    keep, off = [], [0]
    for p in range(sc.n_pt):
        ids = [o for o in range(sc.pt_offsets[p], sc.pt_offsets[p + 1]) if sc.obs_img[o] != dead]
        if p == 0:
            ids = ids[:1]
        if p == 1:
            ids = []
        keep.extend(ids)
        off.append(len(keep))
    keep = np.array(keep, np.int64)
    sc.obs_img = np.ascontiguousarray(sc.obs_img[keep])
    sc.obs_uv = np.ascontiguousarray(sc.obs_uv.reshape(-1, 2)[keep].reshape(-1))
    sc.pt_offsets = np.array(off, np.int64)
    sc.n_obs = len(keep)
    img = int(sc.obs_img[0])
    assert img != sc.const_img
    Rm, t = _rotation(sc.extr[6 * img:6 * img + 3]), sc.extr[6 * img + 3:6 * img + 6]
    centre = -Rm.T @ t
    sc.X[0:3] = centre + 1e6 * (sc.X[0:3] - centre)
    return sc


def _two_chains():
    sc = H.Scene(65, 100, 14, outliers=0.2)
    assert api.ba_dense_schedule(sc.problem())[0]["chains"] == 2
    fewer = H.Scene(64, 100, 14, outliers=0.2)     # (one camera fewer: a single chain)
    assert api.ba_dense_schedule(fewer.problem())[0]["chains"] == 1
    return sc


def _schedule(sc):
    """The dense dataflow schedule's shape, and whether an intrinsics tile (natural index >= nb / 64) stands
    among the first nt // 2 positions of its order (test_dense_schedule_banded_arrow's condition)."""
    sh, meta = api.ba_dense_schedule(sc.problem())
    nt = sh["nt"]
    sh["intr_early"] = bool(len(meta)) and any(int(p) >= sh["nb"] // 64 for p in meta[:nt // 2])
    return sh


def _dense_flow_wrap():
    """Random visibility, the dataflow solve on one chain with more tasks than a 256-CU device has workers
    (workers = min(tasks, CUs - chains)): every worker takes several tasks in order.  214 cameras are 21
    block columns and 270 tasks; 213 are 20 columns and 247 tasks."""
    def wraps(sh):
        return sh["flow"] == 1 and sh["chains"] == 1 and sh["tasks"] > 256
    sc = H.Scene(214, 3000, 6, vis_mode=1, outliers=0.2)
    assert wraps(_schedule(sc)), _schedule(sc)
    fewer = H.Scene(213, 3000, 6, vis_mode=1, outliers=0.2)
    assert not wraps(_schedule(fewer)), _schedule(fewer)
    return sc


def _percam_radial3_band():
    """RADIAL3 with one intrinsics block per camera on an open orbit: 47 cameras is the smallest count for
    which the tiles take the Cuthill-McKee order and split over two chains (46: image order, one chain)."""
    def banded(sh):
        return sh["flow"] == 1 and sh["chains"] == 2 and sh["intr_early"]
    sc = H.Scene(47, 564, 4, n_intr=47, model=abi.SFM_CAM_RADIAL3, outliers=0.2)
    assert banded(_schedule(sc)), _schedule(sc)
    fewer = H.Scene(46, 552, 4, n_intr=46, model=abi.SFM_CAM_RADIAL3, outliers=0.2)
    assert not banded(_schedule(fewer)), _schedule(fewer)
    return sc


def _dense_chain_101():
    """1068 cameras, one of them constant: 6 * 1067 + 4 = 6406 rows, 101 block columns, one past the
    dataflow solve's limit: the panel / update launch chain and the all-resident back substitution."""
    sc = H.Scene(1068, DENSE_CHAIN_POINTS, 6, vis_mode=1, outliers=0.2)
    sh = _schedule(sc)
    assert (sh["flow"], sh["nt"], sh["nF"]) == (0, 101, 6406), sh
    sh = _schedule(H.Scene(1067, DENSE_CHAIN_POINTS, 6, vis_mode=1, outliers=0.2))
    assert (sh["flow"], sh["nt"]) == (1, 100), sh
    return sc


def _shape(sc):
    sh = api.ba_describe(sc.problem())
    return {k: getattr(sh, k) for k, _ in sh._fields_}


class Case:
    def __init__(self, name, sc, n_iter=3, radius=None, jacobi=1, check=None):
        self.name, self.sc, self.n_iter = name, sc, n_iter
        o = abi.default_options()
        o.function_tolerance = o.parameter_tolerance = o.gradient_tolerance = 0.0
        o.jacobi_scaling = jacobi
        if radius is not None:
            o.initial_trust_region_radius = radius
        self.opts = o
        self.shape = _shape(sc)
        self.x0 = R.pack(sc.params())
        self.lay = R.layout(sc)
        assert self.lay.n <= R.DENSE_MAX or name in LARGE    # (past the cap: the reference's matrix-free path)
        if check:
            check(self.shape)

    def options(self, n):
        o = abi.BAOptions.from_buffer_copy(bytes(self.opts))
        o.max_num_iterations = n
        return o


def _expect(**want):
    def check(sh):
        for k, v in want.items():
            assert (v(sh[k]) if callable(v) else sh[k] == v), (k, sh[k], sh)
    return check


def _build(name):
    S = H.Scene
    pos = lambda v: v > 0   # noqa: E731
    if name == "one_block":       # chunk points, a single BCR super-block
        return Case(name, S(8, 60, 3, outliers=0.2),
                    check=_expect(dense=0, n_general_pts=0, n_chunk_pts=60, n_cam_active=7))
    if name == "band_c4":         # the headline band (10-view tracks: 9 blocks), several BCR levels, short last super-block
        return Case(name, S(64, 400, 10, outliers=0.2),
                    check=_expect(dense=0, n_general_pts=0, n_chunk_pts=400, band_blocks=9, n_cam_active=63))
    if name == "band_arrow4":     # four intrinsics blocks: the 32-rhs arrow, top + corner launch
        return Case(name, S(64, 400, 10, n_intr=4, outliers=0.2),
                    check=_expect(dense=0, n_general_pts=0, band_blocks=9, n_intr_active=4))
    if name == "dense_random":    # general points, dense RCS
        return Case(name, S(30, 300, 6, vis_mode=1, outliers=0.2),
                    check=_expect(dense=1, n_general_pts=300, n_chunk_pts=0))
    if name == "mixed":           # chunks, general points and the dense RCS in one plan
        return Case(name, _merge(S(40, 400, 6, outliers=0.2), S(40, 20, 16, outliers=0.2)),
                    check=_expect(dense=1, n_chunk_pts=400, n_general_pts=20))
    if name == "long_track":      # > 64 observations per point: the Z kernel's second round
        sc = _merge(S(70, 200, 5, outliers=0.2), S(70, 6, 70, outliers=0.2))
        assert int(np.diff(sc.pt_offsets).max()) == 70
        return Case(name, sc, check=_expect(dense=1, n_general_pts=6, n_chunk_pts=200))
    if name == "repeats":         # repeated (point, image), band storage
        return Case(name, _with_repeats(S(20, 200, 5, outliers=0.2)),
                    check=_expect(dense=0, n_general_pts=(200 + 6) // 7, n_chunk_pts=pos))
    if name == "two_chains":      # the dataflow dense solve split in two chains
        return Case(name, _two_chains(), check=_expect(dense=1))
    if name == "snavely":         # the unused 4th intrinsics slot in gradient, step and scaling
        sc = _flip_z(S(16, 200, 4, model=abi.SFM_CAM_SNAVELY, outliers=0.2))
        sc.intr[3] = 123.0        # garbage in the slot: never read, never moved
        return Case(name, sc, check=_expect(dense=0, n_intr_active=1))
    if name == "snavely_intr":    # l1 off, poses nearly right: the largest gradient entry at x_0 is an intrinsics column
        sc = _flip_z(S(16, 200, 4, model=abi.SFM_CAM_SNAVELY, outliers=0.2, perturb=POINT_HEAVY))
        sc.intr[1] += 0.01
        sc.intr[3] = 123.0
        return Case(name, sc, check=_expect(dense=0, n_intr_active=1))
    if name == "band_c4_pt":      # band_c4 with the largest gradient entry in a (chunk) point column
        return Case(name, _point_heavy(S(64, 400, 10, outliers=0.2, perturb=POINT_HEAVY)),
                    check=_expect(dense=0, n_general_pts=0, n_chunk_pts=400, band_blocks=9, n_cam_active=63))
    if name == "dense_random_pt":  # dense_random with the largest gradient entry in a (general) point column
        return Case(name, _point_heavy(S(30, 300, 6, vis_mode=1, outliers=0.2, perturb=POINT_HEAVY)),
                    check=_expect(dense=1, n_general_pts=300, n_chunk_pts=0))
    if name == "radial3":         # 6-wide intrinsics, one block per camera
        return Case(name, S(16, 200, 4, n_intr=16, model=abi.SFM_CAM_RADIAL3, outliers=0.2),
                    check=_expect(dense=1, n_intr_active=16))
    if name == "per_cam_pinhole":  # many intrinsics blocks
        return Case(name, S(20, 300, 6, n_intr=20, outliers=0.2), check=_expect(dense=1, n_intr_active=20))
    if name == "plain":           # no loss, no scaling
        return Case(name, S(15, 200, 4, huber=0.0, outliers=0.2), jacobi=0, radius=PLAIN_RADIUS,
                    check=_expect(dense=0))
    if name == "no_gauge":        # rank-deficient J'J, held up by the LM diagonal only
        return Case(name, S(18, 200, 5, const_img=-1, outliers=0.2), check=_expect(dense=0, n_cam_active=18))
    if name == "clamped":         # min_lm_diagonal clamp, unobserved blocks
        return Case(name, _clamped(), radius=CLAMPED_RADIUS,
                    check=_expect(dense=0, n_cam_active=6, n_intr_active=1))
    if name == "rejecting":       # rejected steps (radius / 2, / 4), an accept after a reject
        sc = S(12, 150, 4, seed=REJECTING_SEED, outliers=0.2)
        return Case(name, sc, n_iter=4, radius=REJECTING_RADIUS, check=_expect(dense=0))
    if name == "dense_flow_wrap":    # the dataflow dense solve, more tasks than workers
        return Case(name, _dense_flow_wrap(), check=_expect(dense=1, n_general_pts=3000, n_chunk_pts=0))
    if name == "percam_radial3_band":    # the banded-arrow tile order over two chains
        return Case(name, _percam_radial3_band(), check=_expect(dense=1, n_intr_active=47))
    if name == "dense_chain_101":    # past the dataflow limit: the launch chain, dense_back_all_kernel
        return Case(name, _dense_chain_101(),
                    check=_expect(dense=1, n_general_pts=DENSE_CHAIN_POINTS, n_chunk_pts=0, rcs_dim=6406))
    raise KeyError(name)


# radii chosen on the CPU for the cap (kappa ~ radius): the largest power of ten that meets it
PLAIN_RADIUS = 1e3         # no Jacobi scaling: kappa = 2.9e9 already at 1e4
CLAMPED_RADIUS = 1e1       # the far point's columns are ~1e-7 of the others
# seed 11 at radius 1e7: the oracle's relative decreases are -0.54, -0.20, 0.72, 1.4 (reject, reject, accept,
# accept) with both Huber branches populated at every point
REJECTING_SEED, REJECTING_RADIUS = 11, 1e7

DENSE_CHAIN_POINTS = 6000  # 6 views each: ~34 observations per camera
NAMES = ("one_block", "band_c4", "band_c4_pt", "band_arrow4", "dense_random", "dense_random_pt", "mixed",
         "long_track", "repeats", "two_chains", "snavely", "snavely_intr", "radial3", "per_cam_pinhole", "plain",
         "no_gauge", "clamped", "rejecting")
# The many-tile dense scenes: the oracle runs them with 8 threads only (the factor of 6406 rows takes seconds)
LARGE = ("dense_flow_wrap", "percam_radial3_band", "dense_chain_101")
ALL_NAMES = NAMES + LARGE
# The column class (camera, intrinsics, point) that holds the largest |g| entry at x_0, x_1, ..: the part of
# the gradient reduction that gradient_max_norm of that trace entry witnesses (the reference's g, checked at
# every iteration, so the coverage is pinned).  The plain scenes are camera-dominated nearly everywhere; the
# _pt / _intr variants and long_track put the maximum into the other two classes.
GRADIENT_CLASS = {
    "one_block": ("cam", "cam", "cam", "cam"),
    "band_c4": ("cam", "cam", "cam", "cam"),
    "band_c4_pt": ("cam", "pt", "pt", "pt"),
    "band_arrow4": ("cam", "cam", "cam", "cam"),
    "dense_random": ("cam", "cam", "cam", "cam"),
    "dense_random_pt": ("cam", "pt", "pt", "pt"),
    "mixed": ("cam", "cam", "cam", "cam"),
    "long_track": ("pt", "cam", "cam", "cam"),
    "repeats": ("cam", "cam", "cam", "cam"),
    "two_chains": ("cam", "cam", "cam", "cam"),
    "snavely": ("cam", "cam", "cam", "cam"),
    "snavely_intr": ("intr", "cam", "cam", None),     # (x_3: camera and point maxima within 3 %: not claimed)
    "radial3": ("cam", "cam", "cam", "cam"),
    "per_cam_pinhole": ("cam", "cam", "cam", "cam"),
    "plain": ("cam", "cam", "cam", "cam"),
    "no_gauge": ("cam", "cam", "cam", "cam"),
    "clamped": ("cam", "cam", "cam", "cam"),
    "rejecting": ("cam", "cam", "cam", "cam", "cam"),
    "dense_flow_wrap": ("cam", "cam", "cam", "cam"),
    "percam_radial3_band": ("cam", "cam", "cam", "cam"),
    "dense_chain_101": ("cam", "cam", "cam", "cam"),
}
CAP_EXEMPT = ("no_gauge",)
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = _build(name)
    return _cases[name]


# ---- the single-iteration check -------------------------------------------------------
def _norm(v):
    return float(np.sqrt((v * v).sum()))


def check_iteration(cs, n, x_prev, x_new, trace, c=None, record=None, classes=None):
    """Iteration n of an implementation (its parameters before and after, its
    trace of the n-iteration run) against the reference step from x_prev."""
    c = C_STEP if c is None else c
    sc, opts, lay = cs.sc, cs.opts, cs.lay
    assert len(trace) == n + 1
    prev, it = trace[n - 1], trace[n]
    k = 0                                   # rejected steps directly before iteration n
    while n - 1 - k >= 1 and not trace[n - 1 - k].step_is_successful:
        k += 1
    dfac = 2.0 ** (k + 1)
    ref = R.lm_step(sc, cs.x0, x_prev, prev.trust_region_radius, opts, dfac)
    if sc.huber > 0:
        assert ref["n_inner"] > 0 and ref["n_outer"] > 0, "both Huber branches must be populated"
    yn, gn = _norm(ref["y"]), _norm(ref["g_scaled"])
    B = c * ref["cond"] * R.U
    if cs.name not in CAP_EXEMPT:
        assert B <= STEP_BOUND_CAP, (B, ref["cond"])
    prop = gn * yn * B
    tol_cand = 1e-12 * abs(ref["candidate_cost"]) + prop
    tol_cc = 1e-12 * abs(ref["x_cost"]) + tol_cand
    tol_m = 1e-12 * abs(ref["model_cost_change"]) + prop
    assert tol_m < abs(ref["model_cost_change"])
    tol_q = (tol_cc + abs(ref["relative_decrease"]) * tol_m) / (abs(ref["model_cost_change"]) - tol_m)
    assert abs(ref["relative_decrease"] - opts.min_relative_decrease) > tol_q, "the decision must not be marginal"
    assert ref["model_cost_change"] > tol_m

    # the step, in the scaled space
    assert np.array_equal(x_new[lay.free], cs.x0[lay.free]), "a non-parameter moved"
    ulp = np.spacing(np.maximum(np.abs(x_new), np.abs(x_prev)))[lay.cols].astype(LD)
    if ref["step_is_successful"]:
        y = -(x_new - x_prev)[lay.cols].astype(LD) / ref["scale"]
        err = _norm(y - ref["y"])
        if record is not None:
            record.append(dict(scene=cs.name, n=n, ratio=err / (ref["cond"] * R.U * yn), cond=ref["cond"],
                               unknowns=lay.n, backward_error=ref["backward_error"]))
        assert err <= B * yn + _norm(ulp / ref["scale"]), (err / yn, B)
    else:
        assert np.array_equal(x_new, x_prev)
    # the trace
    assert (it.iteration, it.step_is_valid, it.step_is_successful) == \
        (n, int(ref["step_is_valid"]), int(ref["step_is_successful"]))
    assert abs(it.cost - ref["candidate_cost"]) <= tol_cand, (it.cost, ref["candidate_cost"], tol_cand)
    assert abs(it.cost_change - ref["cost_change"]) <= tol_cc, (it.cost_change, ref["cost_change"], tol_cc)
    assert abs(it.model_cost_change - ref["model_cost_change"]) <= tol_m, \
        (it.model_cost_change, ref["model_cost_change"], tol_m)
    assert abs(it.relative_decrease - ref["relative_decrease"]) <= tol_q, \
        (it.relative_decrease, ref["relative_decrease"], tol_q)
    tol_s = float(ref["scale"].max()) * B * yn + _norm(ulp)
    assert abs(it.step_norm - ref["step_norm"]) <= tol_s, (it.step_norm, ref["step_norm"], tol_s)
    want_r = R.next_radius(prev.trust_region_radius, it.relative_decrease, bool(it.step_is_successful), dfac, opts)
    assert abs(it.trust_region_radius - want_r) <= 1e-15 * want_r, (it.trust_region_radius, want_r)
    _check_gradient(cs, x_new, it, classes)
    return ref


def _check_gradient(cs, x, it, classes=None):
    cls, mx = R.gradient_classes(cs.sc, x)
    if classes is not None:
        classes.append(cls)
    else:
        want = GRADIENT_CLASS[cs.name][it.iteration]
        assert want is None or (cls == want and sorted(mx)[-1] > 1.05 * sorted(mx)[-2]), (cls, want, mx)
    gref, gmax, xmax = R.gradient_max_norm(cs.sc, x)
    tol = 1e-12 * gmax + float(np.spacing(xmax))
    assert abs(it.gradient_max_norm - gref) <= tol, (it.gradient_max_norm, gref, tol)


def check_start(cs, it, classes=None):
    """Iteration 0: the cost and gradient at x_0, the initial radius."""
    assert (it.iteration, it.step_is_valid, it.step_is_successful) == (0, 1, 1)
    c0 = R.cost(cs.sc, cs.x0)
    assert abs(it.cost - c0) <= 1e-12 * c0
    assert it.trust_region_radius == cs.opts.initial_trust_region_radius
    assert (it.cost_change, it.model_cost_change, it.relative_decrease, it.step_norm) == (0.0, 0.0, 0.0, 0.0)
    _check_gradient(cs, cs.x0, it, classes)


def check_run(cs, solve, c=None, record=None, classes=None):
    """solve(n) -> (x_n flat, trace) of a run limited to n iterations."""
    x_prev, last = cs.x0, None
    flags = []
    for n in range(1, cs.n_iter + 1):
        x_new, trace = solve(n)
        if n == 1:
            check_start(cs, trace[0], classes)
        else:   # a rerun repeats the shorter run bit for bit
            assert [bytes(t) for t in trace[:n]] == [bytes(t) for t in last]
        check_iteration(cs, n, x_prev, x_new, trace, c, record, classes)
        flags.append(trace[n].step_is_successful)
        x_prev, last = x_new, trace
    if cs.name == "rejecting":
        assert flags == [0, 0, 1, 1], flags    # radius / 2, / 4, then two accepts after the rejects
    return flags


def oracle_run(cs, threads):
    def solve(n):
        rc, s, tr, prm = H.oracle_solve(cs.sc, cs.options(n), threads=threads)
        assert rc == 0 and s.iterations == n and s.termination == abi.SFM_TERM_NO_CONVERGENCE
        return R.pack(prm), tr
    return solve


# ---- tests -------------------------------------------------------------------------------
def threads_of(name):
    return (8,) if name in LARGE else THREADS


@pytest.mark.parametrize("name,threads", [(name, t) for name in ALL_NAMES for t in threads_of(name)])
def test_oracle_lm_step(name, threads):
    cs = case(name)
    check_run(cs, oracle_run(cs, threads))


def test_c_step_is_eight_times_the_oracle_worst_ratio():
    """C_STEP regenerated: the oracle's |y - y_ref|_2 / (kappa u |y_ref|_2) over every scene, thread count
    and accepted iteration (the reference steps are the cached ones of test_oracle_lm_step); C_STEP is the
    smallest power of two >= 8 x the maximum.  Prints the docstring's table (pytest -s)."""
    rows = {}
    for name in ALL_NAMES:
        cs = case(name)
        for threads in threads_of(name):
            rec = []
            check_run(cs, oracle_run(cs, threads), record=rec)
            assert rec
            for r in rec:
                row = rows.setdefault(name, dict(unknowns=r["unknowns"], ratio=0.0, cond=0.0))
                row["ratio"], row["cond"] = max(row["ratio"], r["ratio"]), max(row["cond"], r["cond"])
    for name, row in rows.items():
        print("  %-16s %5d   %-9.2g   %-8.2g  %.2g" % (name, row["unknowns"], row["ratio"], row["cond"],
                                                      C_STEP * row["cond"] * R.U))
    worst = max(row["ratio"] for row in rows.values())
    print("  maximum ratio %.3f -> 8 x = %.2f" % (worst, 8 * worst))
    assert C_STEP / 2 < 8 * worst <= C_STEP
    assert C_STEP == 2.0 ** round(math.log2(C_STEP))


def test_reference_condition_number_is_cond2():
    """kappa is lambda_max / lambda_min of the symmetric fp64 H (eigvalsh); that
    is np.linalg.cond(H) (the 2-norm, by SVD), which costs 7 x as much."""
    cs = case("one_block")
    radius = cs.opts.initial_trust_region_radius
    ref = R.lm_step(cs.sc, cs.x0, cs.x0, radius, cs.opts)
    Hm = R.normal_equations(cs.sc, cs.x0, cs.x0, radius, cs.opts)[0]
    assert abs(np.linalg.cond(Hm.astype(np.float64)) / ref["cond"] - 1) < 1e-9


@pytest.mark.parametrize("name", NAMES)
def test_matrix_free_reference_agrees_with_the_dense_one(name):
    """The reference's two ways to y at x_0, on every scene small enough for both: each one's y has a
    backward error <= 2^-59 under the other's H (the dense longdouble H; the matrix-free operator), and the
    two condition numbers (eigvalsh of the dense fp64 H; Lanczos on the sparse one) agree to 1e-3."""
    cs = case(name)
    sc, opts, radius = cs.sc, cs.opts, cs.opts.initial_trust_region_radius
    Hm, g, Js, _, _, _ = R.normal_equations(sc, cs.x0, cs.x0, radius, opts)
    y_dense, _, H64 = R._solve(Hm, g)
    ev = np.linalg.eigvalsh(H64)
    Js2, _, _, _, diag, g2 = R.scaled_rows(sc, cs.x0, cs.x0, radius, opts)
    assert np.array_equal(g, g2) and np.array_equal(Js, Js2)
    op = R.Operator(cs.lay, Js2, diag)
    y_free, be, cond = R.solve_matrix_free(op, g2, 3 * sc.n_pt)
    assert be <= R.BACKWARD_ERROR_MAX
    assert op.backward_error(y_dense, g) <= 2.0 ** -59
    hn, gn = np.abs(Hm).sum(axis=1).max(), np.abs(g).max()
    assert float(np.abs(g - Hm @ y_free).max() / (hn * np.abs(y_free).max() + gn)) <= 2.0 ** -59
    assert abs(cond / float(ev[-1] / ev[0]) - 1) <= 1e-3, (cond, ev[-1] / ev[0])


def test_clamped_scene_clamps():
    cs = case("clamped")
    cn = R.normal_equations(cs.sc, cs.x0, cs.x0, cs.opts.initial_trust_region_radius, cs.opts)[5]
    g = R.linearize(cs.sc, cs.x0)["g"]
    low = cn < cs.opts.min_lm_diagonal
    assert (cn == 0).sum() == 3                   # the unobserved track
    assert (low & (cn > 0)).sum() == 3            # the far single-observation track
    assert np.abs(g[low & (cn > 0)]).min() > 0
