"""Shapes and transforms of the registration tests (test_registration_*.py): numpy float32 vertices (V,3), int64 faces (F,3)."""
import numpy as np

from tests import mesh_metrics_shapes as S


def bumpy(n=3):
    """the icosphere of 20 * 4^n faces (n = 3: 1 280, n = 2: 320) with every unit direction u scaled to the radius
    0.5 (1 + 0.25 sin(3 u_x + 0.5) cos(2 u_y) + 0.15 u_z u_x + 0.2 sin(5 u_z + 1)), stretched by (1, 1.4, 0.7) and shifted by
    (0.03, -0.02, 0.05): a closed shape with no symmetry"""
    v, f = S.icosphere(n, 0.5, base=20)
    u = v.astype(np.float64) / 0.5
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    r = 0.5 * (1 + 0.25 * np.sin(3 * u[:, 0] + 0.5) * np.cos(2 * u[:, 1]) + 0.15 * u[:, 2] * u[:, 0] + 0.2 * np.sin(5 * u[:, 2] + 1))
    w = u * r[:, None] * np.array([1.0, 1.4, 0.7]) + np.array([0.03, -0.02, 0.05])
    return w.astype(np.float32), f


def rotation(axis, degrees):
    """Rodrigues: the rotation by `degrees` about `axis`, float64 (3,3)"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def moved(v, R, t, s=1.0):
    """s R v + t in float64, rounded once to float32"""
    return (s * (np.asarray(v, np.float64) @ np.asarray(R).T) + np.asarray(t, np.float64)).astype(np.float32)


def rotation_angle_deg(Ra, Rb):
    """the angle of Ra Rb^T in degrees"""
    c = (np.trace(np.asarray(Ra) @ np.asarray(Rb).T) - 1.0) / 2.0
    return float(np.rad2deg(np.arccos(np.clip(c, -1.0, 1.0))))
