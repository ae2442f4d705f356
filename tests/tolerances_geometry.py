"""Bounds of tests/test_geometry_outputs_gpu.py: mp_composite_geometry (float32, one wave per ray) against the float64
reference tests/geometry_reference.py.

Ceilings, from S <= 129 float32 terms per person and t <= 6: opacities 2e-5, depth sums 1e-4, level depths on non-exempt
rays 1e-4 + (te - ts) * 2e-5 / fe per ray (te - ts and fe of the reference's crossing sample: an error of 2e-5 in E moves the
interpolated depth by that much).  The values are at most 5x what was measured on the MI355X and never above the ceilings;
a measurement above a ceiling is a defect to explain, not a number to raise."""

CEIL_ACC, CEIL_DEPTH, CEIL_LEVEL = 2e-5, 1e-4, (1e-4, 2e-5)

# measured maxima on the MI355X (profiles/geometry_outputs.txt), over the C-ABI cases ((R, P, n_z) = (70,3,98), (5,1,65), (9,2,34),
# (13,8,130) at beta 0.1 / 0.02 / 0.001 and level 0.5 / 0.9, the constructed rows) and the end-to-end frame (400 rays, 2 persons):
#   opacities 6.09e-7, depth sums 1.85e-6, level depths 1.30e-7 absolute = 1.26e-3 of the per-ray ceiling
ACC = 3e-6
DEPTH = 9e-6
LEVEL = (6e-7, 1.2e-7)       # (a, b): |depth - reference| <= a + b * (te - ts) / fe; 6e-3 of the ceiling's (1e-4, 2e-5)

assert ACC <= CEIL_ACC and DEPTH <= CEIL_DEPTH and LEVEL[0] <= CEIL_LEVEL[0] and LEVEL[1] <= CEIL_LEVEL[1]
