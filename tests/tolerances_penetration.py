"""Bounds of tests/test_penetration_gpu.py: 4 x the worst value measured on the MI355X against the float64 reference
(tests/penetration_reference.py) on the cases of that file; the measured values stand next to them (and in DESIGN.md §6e).  The
margin covers the spread between boxes and hosts this suite has seen on its fp32 comparisons.  For comparison, the sibling term's
bounds (tests/test_smpl_surface_pose_grad_gpu.py) are 2e-5 max(1, |L|) on the value and 2e-4 rel-to-max on the gradients."""

# mp_pen_probe: |x_c - float64| over the probed points, P = 2 and 3 and the constructed points (the kernel reads the fp32 blend
# table: I_nn inverted in fp32).  Measured 2.5e-7 (x_c is O(1)).
XC = 1.0e-6
# mp_pen_loss: |L_pq - float64| / max(1, L_pq) on random s, up to 300 entries (double accumulation, one rounding to fp32).  Measured 3.5e-8.
LOSS_KERNEL = 1.4e-7
# mp_pen_scatter_bwd: |d verts - float64| / max |d verts|, random I_nn and d x_c, a draw that repeats vertices.  Measured 1.5e-7.
SCATTER = 6.0e-7
# field_interpenetration per pair and in total, and out['interpenetration_loss']: |L - float64| / max(1, |L|); the SDF runs in
# split-bfloat16 with fp32 accumulation.  Measured 2.65e-6 (pair (1,0) of the P = 3 scene; the training step's total: 9.9e-8).
VALUE = 1.1e-5
# end to end: rel-to-max error of d (loss + 0.05 L) / d (pose, trans, shape) against the oracle under torch autograd.
# Measured 1.2e-6 (pose), 1.6e-6 (trans), 2.0e-6 (shape).
GRAD = 8.2e-6
