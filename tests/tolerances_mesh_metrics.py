"""Bounds of tests/test_mesh_closest_gpu.py and tests/test_mesh_metrics_gpu.py.  None of them is a measurement: they are the
closest-face kernel's own slack (csrc/mesh_index.hip, k_index_closest's comment) and the precision of fp32.

M = the largest |coordinate| of the query points and the mesh.  tri_closest forms the closest point q and p - q in fp32 with
every operation rounded on its own: each component is off by at most 6 u M (u = 2^-24), < 11 u M in norm, and the index skips a
box only beyond delta = 16 FLT_EPSILON M = 32 u M -- the bound everything here is stated in."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)


def coordinate_scale(*arrays):
    """M: the largest finite |coordinate| of the arrays"""
    m = 0.0
    for a in arrays:
        a = np.asarray(a, np.float64)
        a = a[np.isfinite(a)]
        m = max(m, float(np.abs(a).max()) if a.size else 0.0)
    return m


def delta(M):
    """the kernel's slack: | sqrt(d2) - float64 distance |, the distance of q to its face, | |p - q| - sqrt(d2) |"""
    return 16.0 * FLT_EPSILON * M


def face_membership(M):
    """the reported face's float64 distance exceeds the float64 minimum by at most this: its fp32 value is within delta of its
    own float64 distance and was not above the fp32 value of the true closest face, itself within delta"""
    return 2.0 * delta(M)


def mean(M, value):
    """a mean of fp32 values whose terms are within delta of float64, summed in double: the terms' slack and the rounding of
    the fp32 terms themselves (sqrt, the normals' dot product: a few ulp of the value)"""
    return delta(M) + 4.0 * FLT_EPSILON * abs(value)


def normal(M, shortest_edge):
    """a component of an fp32 unit face normal against float64, and a dot product of two such normals per normal: the edges
    b - a, c - a are rounded at the magnitude of the coordinates (FLT_EPSILON M / 2 per component), which is FLT_EPSILON M /
    shortest_edge relative to the edge; two edges, three components and the sine of a face's angle (>= 1/2 on the test meshes)
    make 8 of those; cross product, length, divide and the dot product itself add a few ulp of 1"""
    return 8.0 * FLT_EPSILON * M / shortest_edge + 4.0 * FLT_EPSILON


# normal consistency of the end-to-end sphere test (the issue's bound)
NORMAL_CONSISTENCY_SPHERE = 0.99
