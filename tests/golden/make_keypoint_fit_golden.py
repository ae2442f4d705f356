#!/usr/bin/env python
"""Generates tests/golden/keypoint_fit_golden.npz by RUNNING the reference's preprocessing/rotation.py::axis_to_rot6D (it imports
only torch and numpy) on 24 axis-angle rows: a zero rotation, rotations near pi about an axis and about a diagonal, a tiny one, and
seeded random ones up to 1.5 rad per component.  The fixture holds the inputs and the recorded 24 x 6 output in float32, the
precision the reference computes in.
Needs a checkout of the reference:  python tests/golden/make_keypoint_fit_golden.py REFERENCE_CHECKOUT"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    raise SystemExit(__doc__)
REF = sys.argv[1]

spec = importlib.util.spec_from_file_location("ref_rotation", os.path.join(REF, "preprocessing", "rotation.py"))
rotation = importlib.util.module_from_spec(spec)
spec.loader.exec_module(rotation)

g = torch.Generator().manual_seed(20)
axis = torch.randn(24, 3, generator=g) * 0.8
axis[0] = 0.0
axis[1] = torch.tensor([np.pi - 1e-3, 0.0, 0.0])
axis[2] = torch.tensor([1.0, 1.0, 1.0]) / np.sqrt(3.0) * (np.pi - 1e-4)
axis[3] = torch.tensor([1e-5, -2e-5, 3e-5])
axis[4] = torch.tensor([0.0, 0.0, -np.pi / 2])
axis = axis.float()
rot6d = rotation.axis_to_rot6D(axis)
assert rot6d.numel() == 144
np.savez(os.path.join(HERE, "keypoint_fit_golden.npz"), axis=axis.numpy(), rot6d=rot6d.numpy())
print("wrote", os.path.join(HERE, "keypoint_fit_golden.npz"), rot6d.shape, rot6d.dtype)
