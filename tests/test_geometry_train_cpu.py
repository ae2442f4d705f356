"""Differentiable volume depths for training, the parts that need no GPU: the torch restatement of the five differentiable
outputs (tests/geometry_train_reference.py) against the float64 reference of the forward kernel and against the closed-form
adjoint of the header; mesh_losses.ray_depth_order_loss against depth_order_loss; the interface of the feature."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import geometry_reference as G
from tests import geometry_train_reference as GT

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_KEYS = dict(depth="depth", depth_person="depth_person", acc_solo="acc_solo", depth_solo="depth_solo",
                depth_solo_level="depth_solo_level")


@pytest.mark.parametrize("shape,beta,level", GT.CASES)
def test_restatement_forward_and_its_gradient_against_the_formulas(shape, beta, level):
    inv, z, sdf, ref, up = GT.case(shape, beta, level)
    R = shape[0]
    beta32 = float(np.float32(beta))
    zt = [torch.tensor(a, dtype=torch.float64) for a in z]
    st = [torch.tensor(a, dtype=torch.float64) for a in sdf]
    out = GT.geometry_outputs(R, inv, zt, st, torch.tensor(beta32, dtype=torch.float64), level)
    for k in GT.DIFF_KEYS:
        err = float(np.abs(out[k].numpy() - ref[REF_KEYS[k]]).max())
        assert err <= 1e-12, (k, err)
    a_sdf, a_beta = GT.autograd_gradients(R, inv, z, sdf, beta32, level, up)
    f_sdf, f_beta = GT.adjoint_formulas(R, inv, z, sdf, beta32, level, up)
    e_sdf = max(float(np.abs(a - f).max()) for a, f in zip(a_sdf, f_sdf))
    e_beta = abs(a_beta - f_beta) / abs(a_beta)
    print(f"[geometry train] {shape} beta {beta} level {level}: autograd vs formulas d sdf {e_sdf:.2e} abs (max |d sdf| "
          f"{max(float(np.abs(a).max()) for a in a_sdf):.2e}), d beta {e_beta:.2e} rel")
    assert e_sdf <= 1e-10 and e_beta <= 1e-10, (e_sdf, e_beta)
    assert max(float(np.abs(a).max()) for a in a_sdf) > 0 and a_beta != 0
    # every term alone: the formulas' terms are separately right, not only their sum (d beta of one term can cancel to nothing,
    # e.g. a saturated opacity's: its error is taken relative to the whole gradient's d beta, of which it is a part)
    full_beta = abs(a_beta)
    for k in GT.DIFF_KEYS:
        one = {k: up[k]}
        a_sdf, a_beta = GT.autograd_gradients(R, inv, z, sdf, beta32, level, one)
        f_sdf, f_beta = GT.adjoint_formulas(R, inv, z, sdf, beta32, level, one)
        assert max(float(np.abs(a - f).max()) for a, f in zip(a_sdf, f_sdf)) <= 1e-10, k
        assert abs(a_beta - f_beta) <= 1e-10 * full_beta, k


def _rays():
    """6 rays, 2 persons: depths along the ray and SAM logits (one person labelled per ray)"""
    D = torch.tensor([[2.0, 3.0], [3.0, 2.0], [2.5, -1.0], [-1.0, -1.0], [1.5, 1.2], [2.0, 2.6]], dtype=torch.float64)
    lab = torch.tensor([0, 0, 0, 1, 0, 1])
    logits = torch.full((6, 2), -12.0, dtype=torch.float64)
    logits[torch.arange(6), lab] = 12.0
    return D, lab, logits


def test_ray_depth_order_loss_is_depth_order_loss_on_the_rays():
    from multiply_amd import mesh_losses as ML
    D, lab, logits = _rays()
    Dg = D.clone().requires_grad_(True)
    got = ML.ray_depth_order_loss({"depth_person_solo_level_list": Dg, "sam_mask": logits}, epoch=100, depth_order_weight=0.01)
    want = ML.depth_order_loss([D[:, p].reshape(2, 3) for p in range(2)], logits.reshape(1, 2, 3, 2), 100, 0.01)
    assert float(got.detach()) > 0 and abs(float(got.detach()) - float(want)) <= 1e-15
    got.backward()
    # out of order: rays 1, 4 (label 0 behind person 1) and 5 (label 1 behind person 0); ray 2: the other is empty; ray 3: nothing
    g = Dg.grad
    labelled = g[torch.arange(6), lab]
    assert (labelled[[1, 4, 5]] > 0).all() and (labelled[[0, 2, 3]] == 0).all()
    assert (g[torch.arange(6), 1 - lab][[1, 4, 5]] < 0).all() and (g[[0, 2, 3]] == 0).all()
    # sam_mask= overrides the dict's labels; z_scale multiplies the valid depths only
    zs = torch.tensor([0.5, 0.5, 2.0, 2.0, 1.0, 3.0], dtype=torch.float64)
    got2 = ML.ray_depth_order_loss({"depth_person_solo_level_list": D, "sam_mask": -logits}, 100, 0.01, z_scale=zs, sam_mask=logits)
    Ds = torch.where(D >= 0, D * zs[:, None], D)
    want2 = ML.depth_order_loss([Ds[:, p] for p in range(2)], logits, 100, 0.01)
    assert float(got2) == float(want2) and float(got2) != float(got)
    # every labelled person in front: zero, with a zero gradient
    front = torch.tensor([[2.0, 3.0], [2.0, 3.0], [2.5, -1.0]], dtype=torch.float64, requires_grad=True)
    zero = ML.ray_depth_order_loss({"depth_person_solo_level_list": front, "sam_mask": logits[:3]}, 100)
    zero.backward()
    assert float(zero) == 0.0 and (front.grad == 0).all()


def test_the_interface_exists():
    import ctypes as C
    from multiply_amd import hip
    from multiply_amd import mesh_losses as ML
    from multiply_amd.multiply import Multiply
    hdr = open(os.path.join(REPO, "include", "multiply_hip.h")).read()
    assert re.search(r"\bint\s+mp_tr_composite_geometry_bwd\s*\(", hdr)
    assert hdr.index("mp_tr_composite_bwd(") < hdr.index("mp_tr_composite_geometry_bwd(") < hdr.index("mp_tr_bg_points(")
    protos = hip.header_prototypes()
    assert "mp_tr_composite_geometry_bwd" in protos
    rt, at = protos["mp_tr_composite_geometry_bwd"]
    assert rt is C.c_int and len(at) == 16 and at[:3] == [C.c_int] * 3 and at[7] is C.c_float
    assert all(a is hip.DevPtr for a in at[3:7] + at[8:])
    assert Multiply.train_geometry is False and Multiply.render_geometry is False
    assert inspect.signature(ML.opt_depth_frame).parameters["depth_source"].default == "mesh"
    sig = inspect.signature(ML.ray_depth_order_loss).parameters
    assert sig["depth_order_weight"].default == 0.005 and sig["z_scale"].default is None and sig["sam_mask"].default is None
