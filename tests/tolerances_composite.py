"""Bounds of tests/test_composite_gpu.py: mp_composite and mp_tr_composite_bwd (float32, one wave per ray) against the float64
reference tests/composite_reference.py.

Ceilings, by the siblings' reasoning (tolerances_geometry.py, tolerances_geometry_train.py: S <= 129 float32 terms per person,
values of order 1): 2e-5 absolute for acc, acc_person, bg_T, rgb_values, fg_rgb_values, normal_values (unit normals), and for
d rgb and d bg_rgb over the case's max |d rgb_values|; 1e-4 of the case's max |d sdf|, and the same for the restricted measure of
the thin cases (the last sample of every person on every ray and all samples of the rays with bg_T >= 0.05, over the maximum of
that subset); 1e-3 relative for d beta.  d beta is taken relative to |d beta|: every committed case satisfies
|d beta| >= 0.1 sum_rays |the ray's own d beta| (tests/test_composite_reference_cpu.py asserts it), so none of them needs the
sum of absolute parts as its scale; the comparison falls back to that sum only for rows that do not satisfy it (none today).
The launch-shape cases have S = 257 and S = 513 terms per person: `scaled(bound, S)` multiplies every bound by S / 129 there, and
by 1 up to S = 129; their measurements below are divided by the same factor.

The values are at most 5x the maxima measured on the MI355X (profiles/composite_colour.txt; the 5x allows for other boxes and
compiler versions) and never above the ceilings; a measurement above a ceiling is a defect to explain, not a number to raise."""

CEIL_OUT, CEIL_DSDF, CEIL_DBETA = 2e-5, 1e-4, 1e-3

# measured maxima on the MI355X (profiles/composite_colour.txt) over composite_reference.CASES and LAUNCH_CASES, the constructed
# rows (tied depth rows, the last-sample tie, the zero-weight rows at beta 0.001), the NULL-pointer runs and n_rays < R:
#   forward, absolute:  acc 3.16e-6, rgb_values 1.64e-6, fg_rgb_values 1.66e-6 ((5,8,258) thin, over S/129; acc 3.01e-6 on
#     (13,8,130) thin), acc_person 1.36e-6, bg_T 1.73e-7, normal_values 7.37e-7 (the zero-weight rows; bg_T 5.5e-8 elsewhere)
#   d sdf 9.83e-6 of the case's max |d sdf| ((5,1,65) at beta 0.001: samples within a few beta of the surface, d sigma / d sdf up
#     to 5e5; 5.2e-6 on (6,3,3) opaque, 3.2e-6 and below elsewhere);  restricted thin measure 3.21e-6 ((3,8,514), over S/129;
#     2.76e-6 on (13,8,130) thin);  the last samples alone on the last-sample tie rows, over their own maximum: 1.17e-7
#   d rgb 8.36e-7 and d bg_rgb 1.35e-7 of max |d rgb_values| (both on the zero-weight rows; 5.3e-8 and below elsewhere)
#   d beta 6.94e-5 relative ((5,1,65) at beta 0.001; 5.98e-5 on (9,2,34) at beta 0.02, 3.1e-5 and below elsewhere)
OUT = dict(acc=1.5e-5, acc_person=6.5e-6, bg_T=8.5e-7, rgb_values=8e-6, fg_rgb_values=8e-6, normal_values=3.6e-6)
DRGB = 4e-6
DBG = 6.5e-7
DSDF = 4.9e-5
DSDF_THIN = 1.6e-5
DSDF_LAST = 5.8e-7             # the last samples of the last-sample tie rows over their own maximum
DBETA = 3.4e-4


def scaled(bound, S):
    """the bound for S samples per person: times S / 129 past the siblings' 129"""
    return bound * max(1.0, S / 129.0)


assert max(OUT.values()) <= CEIL_OUT and DRGB <= CEIL_OUT and DBG <= CEIL_OUT
assert DSDF <= CEIL_DSDF and DSDF_THIN <= CEIL_DSDF and DSDF_LAST <= CEIL_DSDF and DBETA <= CEIL_DBETA
