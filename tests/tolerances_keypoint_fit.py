"""Bounds of tests/test_keypoint_fit_gpu.py: every one is 4 x the largest value measured on the MI355X against the float64
restatement (tests/keypoint_fit_reference.py) over the cases of that test, the margin convention of tolerances_penetration.py; it
covers box-to-box variation in sincosf and in the order of the fixed reductions.  The measured value stands next to each bound.
A failure a little above a bound after a compiler or libm change means RE-MEASURE (the tests print every figure) and record the
new value here and in DESIGN.md; a failure far above it is a defect."""
MARGIN = 4.0

# ---- mp_kp_objective, one evaluation (test_objective_against_float64: 4 maps x N in {1, 3})
# terms: | kernel - float64 | / | float64 | per term
OBJ_TERMS_REL_MEASURED = 1.733e-07          # the 'vertices' map
OBJ_TERMS_REL = MARGIN * OBJ_TERMS_REL_MEASURED
# projections in px (coordinates of a few hundred px: an ulp is 3e-5 px)
OBJ_PROJ_PX_MEASURED = 3.782e-05            # the 'vertices' map
OBJ_PROJ_PX = MARGIN * OBJ_PROJ_PX_MEASURED
# the 85 gradient entries, each relative to the largest entry of its group
OBJ_GRAD_REL_MEASURED = {"transl": 3.814e-06, "thetas": 2.347e-06, "betas": 6.209e-06}     # all three: the coco25-shaped map, N = 3
OBJ_GRAD_REL = {k: MARGIN * v for k, v in OBJ_GRAD_REL_MEASURED.items()}

# ---- mp_kp_fit against the float64 loop after `iters` steps (test_fit_against_the_float64_loop, the 'mixed' map, lr = 1e-3)
# parameters: max | kernel - float64 | over the 85 entries (radians / metres / shape units); rounding compounds over the steps --
# Adam divides each entry's step by the root of its own second moment, so an entry whose gradient is small against its group's
# carries a large RELATIVE error into its step -- hence one bound per step count, not the one-step bound reused
FIT_PARAMS_ABS_MEASURED = {1: 7.219e-08, 2: 1.746e-07, 25: 3.206e-07, 150: 1.218e-06}
FIT_PARAMS_ABS = {k: MARGIN * v for k, v in FIT_PARAMS_ABS_MEASURED.items()}
# history: | kernel - float64 | / | float64 | per term, the maximum over all steps before `iters`
FIT_HISTORY_REL_MEASURED = {1: 1.471e-07, 2: 1.569e-07, 25: 7.971e-07, 150: 2.811e-06}
FIT_HISTORY_REL = {k: MARGIN * v for k, v in FIT_HISTORY_REL_MEASURED.items()}

# ---- one term alone, 25 steps (test_each_term_alone)
FIT_ONE_TERM_PARAMS_ABS_MEASURED = {"2d": 8.194e-07, "temporal": 2.720e-07}
FIT_ONE_TERM_PARAMS_ABS = {k: MARGIN * v for k, v in FIT_ONE_TERM_PARAMS_ABS_MEASURED.items()}
FIT_ONE_TERM_HISTORY_REL_MEASURED = {"2d": 1.295e-06, "temporal": 1.347e-06}
FIT_ONE_TERM_HISTORY_REL = {k: MARGIN * v for k, v in FIT_ONE_TERM_HISTORY_REL_MEASURED.items()}

# ---- refine_sequence on 3 frames x 2 persons, 150 steps: | kernel's - float64 loop's | mean reprojection error after the fit, px
RECOVERY_PX_MEASURED = 1.537e-06        # 3.0323 px on both sides, from 15.10 px; the parameters differ by at most 9.8e-7
RECOVERY_PX = MARGIN * RECOVERY_PX_MEASURED
