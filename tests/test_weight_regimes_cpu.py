"""The weight regimes of tests/weight_regimes.py keep their promises (CPU, float64): the trained regime has a clear fraction of its
softplus units in transition and colour nets with a spread output, the range regime sits at its fraction of the f16 limit, and
the float64 reference is the oracle's arithmetic (fp32 oracle vs float64 printed)."""
import math

import torch

from oracle import multiply_oracle as O
from tests import weight_regimes as W


def test_trained_regime_promises():
    R = W.Regime("trained", n_fg=300, n_bg=48)          # the assertions live in Regime: >= 10 % in transition, rgb std >= 0.1
    print(R.summary())
    assert min(R.frac_transition) >= W.MIN_TRANSITION_FRACTION and min(R.fg_rgb_std) >= W.MIN_RGB_STD
    assert bool(R.on_surface.any()) and float(R.fg["sdf"][R.on_surface].abs().max()) < 1e-9
    sd32 = {k: v.float() for k, v in R.sd.items()}
    n = 300
    ref = W.fg_reference(sd32, R.x[:n].float(), R.cond.float(), R.jinv[:n].float())
    print(f"fp32 oracle vs float64: sdf {float((ref['sdf'] - R.fg['sdf'][:n]).abs().max()):.3e}, "
          f"rgb {float((ref['rgb'] - R.fg['rgb'][:n]).abs().max()):.3e}")
    assert float((ref["rgb"] - R.fg["rgb"][:n]).abs().max()) < 1e-4
    out = O.implicit_forward(R.sd, W.FG_PREFIX, R.x, R.cond, multires=6)
    assert torch.equal(out, W.implicit_preacts(R.sd, W.FG_PREFIX, R.x, R.cond, 6)[0])


def test_near_range_regime():
    R = W.Regime("near_range", n_fg=120, n_bg=3, normals=False)
    print(R.summary())
    assert 0.63 <= R.max_pre / W.Z_LIMIT <= 0.77
    assert abs(W.Z_LIMIT - 65504.0 * math.log(2.0) / 100.0) < 1e-9
