"""GPU: single Levenberg-Marquardt iterations of the HIP bundle adjuster
against the extended-precision dense reference (tests/_lm_reference.py), with
the scenes, the procedure and the tolerances of test_lm_step.py -- C_STEP
included, which was measured on the CPU oracle and never against the GPU.

BAPlan.run restarts from the plan's initial parameters and reruns are bit
identical (test_deterministic_and_plan_reuse), so runs limited to n = 1, 2, 3
iterations give x_1, x_2, x_3 and their traces; the reference is fed the
GPU's own x_{n-1} and radius.  Every scene runs on a default context; the two
starred scenes (the headline band and the dense random-visibility one) and
their point-heavy variants (gradient_max_norm carried by the point columns,
the device's kScGmaxE slot) also run under every engine shape (SFM_CTX_BA_* / SFM_CTX_DIAG_SPEC_ALWAYS), each
in a context of its own, with plan.info() checked so that a flag the planner
ignored fails the test.  On dense_random the reduced camera system is dense
by structure: SEQ_BAND and SPLIT_BCR must leave it so.  plan.info() has no
field for SPLIT_REDUCE, NO_SPEC_GRAM, STEP_LANES, REDUCE_WAVES or
SFM_CTX_DIAG_SPEC_ALWAYS (nor for SPLIT_BCR and DENSE_CHAIN beyond the
solver): those shapes are checked for their results only, a silently ignored
flag among them would pass.
"""
import numpy as np
import pytest

import _helpers as H
import _lm_reference as R
import test_lm_step as T

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not R.LONGDOUBLE_OK, reason=R.SKIP_REASON)]
abi, api = H.abi, H.api

BCR, DENSE, SEQ = abi.SFM_RCS_BCR, abi.SFM_RCS_DENSE, abi.SFM_RCS_SEQ_BAND
# id -> (flags, rcs_solver on a band scene, tile_rows forced or None)
ENGINES = {
    "default": (0, BCR, None),
    "seq_band": (abi.SFM_CTX_BA_SEQ_BAND, SEQ, None),
    "split_bcr": (abi.SFM_CTX_BA_SPLIT_BCR, BCR, None),
    "dense_rcs": (abi.SFM_CTX_BA_DENSE_RCS, DENSE, None),
    "dense_chain": (abi.SFM_CTX_BA_DENSE_RCS | abi.SFM_CTX_BA_DENSE_CHAIN, DENSE, None),
    "tile80": (abi.SFM_CTX_BA_TILE80, BCR, 80),
    "split_reduce": (abi.SFM_CTX_BA_SPLIT_REDUCE, BCR, None),
    "no_spec_gram": (abi.SFM_CTX_BA_NO_SPEC_GRAM, BCR, None),
    "step_lanes1": (abi.SFM_CTX_BA_STEP_LANES(1), BCR, None),
    "step_lanes8": (abi.SFM_CTX_BA_STEP_LANES(8), BCR, None),
    "reduce_waves1": (abi.SFM_CTX_BA_REDUCE_WAVES(1), BCR, None),
    "reduce_waves4": (abi.SFM_CTX_BA_REDUCE_WAVES(4), BCR, None),
    "spec_always": (abi.SFM_CTX_DIAG_SPEC_ALWAYS, BCR, None),
}


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def _check(ctx, cs, solver=None, tile_rows=None):
    plan = api.BAPlan(ctx, cs.sc.problem(), *cs.sc.params())
    try:
        info = plan.info()
        # the planner's shape for the scene (asserted label by label in test_lm_step.case)
        assert info.rcs_solver == (solver if solver is not None else DENSE if cs.shape["dense"] else BCR)
        assert info.tile_rows == (tile_rows if tile_rows is not None else cs.shape["tile_rows"])

        def solve(n):
            rc, s = plan.run(cs.options(n))
            assert rc == 0 and s.iterations == n and s.termination == abi.SFM_TERM_NO_CONVERGENCE, \
                (rc, s.iterations, s.termination, abi.load().sfm_last_error())
            return R.pack(plan.download()), plan.trace()
        return T.check_run(cs, solve)
    finally:
        plan.close()


@pytest.mark.parametrize("name", T.ALL_NAMES)
def test_gpu_lm_step(ctx, name):
    _check(ctx, T.case(name), DENSE if name in T.LARGE else None)


# dense_flow_wrap (21 block columns) under the launch chain: several kDenseW groups with their trailing
# updates and the dense_back_kernel loop; under the dense engines only, not under all thirteen
DENSE_ENGINES = ("default", "dense_rcs", "dense_chain")


@pytest.mark.parametrize("name,engine", [(name, e) for name in T.STARRED for e in ENGINES] +
                         [("dense_flow_wrap", e) for e in DENSE_ENGINES])
def test_gpu_lm_step_engine_shapes(name, engine):
    cs = T.case(name)
    flags, solver, tile_rows = ENGINES[engine]
    if cs.shape["dense"]:
        solver = DENSE
    with H.engine_ctx(flags) as c:
        _check(c, cs, solver, tile_rows)
