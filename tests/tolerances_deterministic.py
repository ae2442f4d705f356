"""Bounds of tests/test_deterministic_sums_gpu.py: d beta of the two compositing adjoints and d tfs of the canonical warp's adjoint,
deterministic forms, against a float64 sum of the same per-point terms:  |got - want| <= c 2^-24 sum |terms|.

c is TWICE what the existing ATOMIC kernel needs on the same inputs (the largest of eight launches: its result varies from launch
to launch), measured on an MI355X; the deterministic forms' own figures are beside them for the record and were not used.

                                      atomic kernel needs      deterministic form needs
    d beta, mp_tr_composite_bwd            29.16 .. 29.58           28.96
    d beta, mp_tr_composite_geometry_bwd   86.77 .. 87.44           87.44
    d tfs with djinv (worst entry)         0.944 .. 0.953           1.435
    d tfs without djinv (worst entry)      1.656                    1.435

(d beta: the 2240 terms are each a product of float32 exponentials and prefix sums, so c is the terms' own error, not the
summation's; eight atomic launches each.)
"""
C_D_BETA = {"composite": 2 * 29.58, "geometry": 2 * 87.44}
C_D_TFS = {True: 2 * 0.953, False: 2 * 1.656}
