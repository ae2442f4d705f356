"""The float64 reference of the volume-rendered depth outputs (tests/geometry_reference.py) against the existing compositing
oracle and an analytic case, and the interface of the feature (header, binding, model flag).  No GPU."""
import math
import os
import re

import numpy as np
import torch

from oracle import multiply_oracle as O
from tests import geometry_reference as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(beta=0.02):
    inv, z, sdf = G.ragged_case(70, 3, 98, seed=4, hits=G.RAGGED_HITS)
    return inv, z, sdf, G.geometry_reference(70, inv, z, sdf, beta, 0.5)


def test_reference_sums_are_the_oracles_compositing_of_the_depths():
    """packed_composite with rgb := (tm, tm, tm) and normal := tm * onehot(person) accumulates exactly depth and depth_person;
    its weight sums are the reference's.  Three persons, rays hit by none, one, two and three of them."""
    beta = 0.02
    inv, z, sdf, ref = _case(beta)
    tm = [0.5 * (a[:, :-1] + a[:, 1:]) for a in z]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rgb = [t(m)[..., None].expand(-1, -1, 3).contiguous() for m in tm]
    nrm = [t(m)[..., None] * torch.eye(3)[n] for n, m in enumerate(tm)]
    acc_rgb, acc_nrm, acc, accp, _ = O.packed_composite(70, [t(h) for h in G.RAGGED_HITS], [t(a[:, :-1]) for a in z],
                                                        [t(a[:, -1]) for a in z], [t(s) for s in sdf], rgb, nrm,
                                                        torch.tensor(beta), [0, 1, 2])
    err = lambda a, b: float(np.abs(a.double().numpy() - b).max())
    e = dict(depth=err(acc_rgb[:, 0], ref["depth"]), depth_person=err(acc_nrm, ref["depth_person"]), acc=err(acc, ref["acc"]),
             acc_person=err(accp, ref["acc_person"]))
    print("[geometry] reference vs packed_composite, max abs:", {k: f"{v:.2e}" for k, v in e.items()})
    assert max(e.values()) < 1e-5, e
    assert float(ref["acc"].max()) > 0.9 and (ref["acc"][65:] == 0).all() and (ref["depth"][65:] == 0).all()
    assert np.abs(ref["depth_person"].sum(1) - ref["depth"]).max() < 1e-12


def test_level_depth_of_a_plane_met_head_on():
    """sdf = d0 - t, uniform dt = beta / 20: the free energy in front of depth d0 + x beta is, in units of 1,
    1/2 (the half line outside, integral of exp(-s/beta)/(2 beta)) + x - 1/2 (1 - exp(-x)) inside; it equals ln 2 at the x that
    solves x - 1/2 (1 - e^-x) = ln 2 - 1/2."""
    lo, hi = 0.0, 2.0
    g = lambda x: x - 0.5 * (1.0 - math.exp(-x)) - (math.log(2.0) - 0.5)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if g(mid) < 0 else (lo, mid)
    x = 0.5 * (lo + hi)
    assert 0.3 < x < 0.5
    beta, d0 = 0.05, 2.0
    dt = beta / 20
    zz = (1.0 + dt * np.arange(int(2.0 / dt) + 1))[None]
    tmid = 0.5 * (zz[:, :-1] + zz[:, 1:])
    ref = G.geometry_reference(1, [np.zeros(1, np.int32)], [zz], [d0 - tmid], beta, 0.5)
    got = float(ref["depth_level"][0])
    print(f"[geometry] plane: level depth {got:.6f}, analytic {d0 + x * beta:.6f}, dt {dt:.4f}")
    assert abs(got - (d0 + x * beta)) <= 2 * dt
    assert int(ref["front_person"][0]) == 0 and float(ref["depth_solo_level"][0, 0]) == got


def test_solo_outputs_are_the_merged_outputs_of_the_person_alone():
    inv, z, sdf, ref = _case()
    for n in range(3):
        one = G.geometry_reference(70, [inv[n]], [z[n]], [sdf[n]], 0.02, 0.5)
        assert np.array_equal(one["acc"], ref["acc_solo"][:, n]) and np.array_equal(one["depth"], ref["depth_solo"][:, n])
        assert np.array_equal(one["depth_level"], ref["depth_solo_level"][:, n])
        assert np.array_equal(one["acc_solo"][:, 0], one["acc"]) and np.array_equal(one["depth_person"][:, 0], one["depth"])
        assert ((one["front_person"] == 0) == (one["depth_level"] >= 0)).all()
        assert (ref["acc_solo"][inv[n] < 0, n] == 0).all() and (ref["depth_solo_level"][inv[n] < 0, n] == -1).all()
    # a person in front of nobody is as visible as alone; behind somebody, less
    assert (ref["acc_person"] <= ref["acc_solo"] + 1e-12).all()


def test_level_depth_is_minus_one_exactly_when_the_free_energy_stays_below_the_level():
    for beta, level in ((0.1, 0.5), (0.02, 0.9), (0.001, 0.5)):
        inv, z, sdf = G.ragged_case(70, 3, 98, seed=4, hits=G.RAGGED_HITS)
        ref = G.geometry_reference(70, inv, z, sdf, beta, level)
        L = -math.log(1.0 - float(np.float32(level)))
        assert abs(ref["L"] - L) < 1e-12
        assert ((ref["depth_level"] == -1) == (ref["total"] < L)).all()
        assert ((ref["front_person"] == -1) == (ref["total"] < L)).all()
        assert ((ref["depth_solo_level"] == -1) == (ref["total_solo"] < L)).all()
        hit = ref["depth_level"] >= 0
        assert hit.any() and (ref["depth_level"][hit] >= 1.0).all() and (ref["depth_level"][hit] <= 3.0).all()
        # the accumulated opacity in front of the level depth is the level: acc >= level on those rays
        assert (ref["acc"][hit] >= float(np.float32(level)) - 1e-12).all()


def test_ties_go_to_the_lower_column():
    """two persons with identical depth rows: every t_end ties, the lower column's sample comes first"""
    inv, z, sdf = G.ragged_case(6, 2, 34, seed=1)
    z[1] = z[0].copy()
    ref = G.geometry_reference(6, inv, z, sdf, 0.02, 0.5)
    swapped = G.geometry_reference(6, inv[::-1], z[::-1], sdf[::-1], 0.02, 0.5)
    assert not np.allclose(ref["depth_person"], swapped["depth_person"][:, ::-1])      # the order matters ...
    r = 0                                                                              # ... and is (te, column): by hand on ray 0
    fe = [G.laplace_density(sdf[n][r].astype(np.float64), float(np.float32(0.02))) * np.diff(z[n][r].astype(np.float64)) for n in range(2)]
    E, d0 = 0.0, 0.0
    for i in range(33):
        for n in range(2):
            w = (1 - math.exp(-fe[n][i])) * math.exp(-E)
            d0 += w * 0.5 * (float(z[n][r, i]) + float(z[n][r, i + 1])) if n == 0 else 0.0
            E += fe[n][i]
    assert abs(d0 - ref["depth_person"][r, 0]) < 1e-12


def test_the_interface_exists():
    """the C ABI entry point, its binding and the model flag (none of these exist without the feature)"""
    from multiply_amd import hip
    from multiply_amd.multiply import Multiply
    hdr = open(os.path.join(REPO, "include", "multiply_hip.h")).read()
    assert re.search(r"\bint\s+mp_composite_geometry\s*\(", hdr)
    protos = hip.header_prototypes()
    assert "mp_composite_geometry" in protos
    rt, at = protos["mp_composite_geometry"]
    import ctypes as C
    assert rt is C.c_int and len(at) == 16 and at[7] is C.c_float and at[:3] == [C.c_int] * 3
    assert all(a is hip.DevPtr for a in at[3:7] + at[8:])
    assert Multiply.render_geometry is False and Multiply.geometry_level == 0.5
    from multiply_amd import mesh_losses as ML
    import inspect
    sig = inspect.signature(ML.frame_instance_masks)
    assert sig.parameters["source"].default == "mesh" and callable(ML.volume_depth_maps)
