"""Bounds of tests/test_geometry_train_gpu.py: mp_tr_composite_geometry_bwd (float32, one wave per ray) against float64 autograd
of tests/geometry_train_reference.py.

d sdf: max |error| over the case's max |d sdf|; d beta: relative error.  Ceilings: 1e-4 for d sdf, 1e-3 for d beta (S <= 129
float32 terms per person, and d beta is an atomic float32 sum over the rays).  The values are at most 5x the maxima measured
on the MI355X over the cases of geometry_train_reference.CASES (the 5x allows for other boxes and compiler versions) and never
above the ceilings; a measurement above a ceiling is a defect to explain, not a number to raise."""

CEIL_DSDF, CEIL_DBETA = 1e-4, 1e-3

# measured maxima on the MI355X (profiles/geometry_train.txt), over the six cases with all five upstream gradients and, on
# (70,3,98) beta 0.1 and (9,2,34), with every upstream gradient alone (errors of one term over the whole case's scales):
#   d sdf 1.062e-6 of the case's max |d sdf| ((70,3,98), beta 0.02);  d beta 1.743e-4 relative ((5,1,65), beta 0.001: 64 saturated
#   samples whose terms cancel to 0.78 from O(1/beta^2) parts; 5.5e-5 and below on the other cases)
DSDF = 5e-6
DBETA = 8.5e-4

assert DSDF <= CEIL_DSDF and DBETA <= CEIL_DBETA
