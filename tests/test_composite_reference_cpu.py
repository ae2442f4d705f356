"""Colour compositing and its adjoint, the parts that need no GPU: the float64 reference (tests/composite_reference.py) against
geometry_reference's weight sums, its torch restatement under autograd against the closed-form adjoint of the comment above
k_composite_bwd, the conditions the committed cases must satisfy for the device tests to mean something (thin rays that show the
background, a d beta that does not cancel, a gradient scale at beta = 0.001, the margins of the two tie rules), and what four
plausible mistakes change in float64 on those cases, against the bounds of tests/tolerances_composite.py."""
import numpy as np
import pytest
import torch

from tests import composite_reference as CR
from tests import geometry_reference as G
from tests import tolerances_composite as TOL

ALL = [c[0] for c in CR.CASES + CR.LAUNCH_CASES]


def _max_err(a, b):
    return max(float(np.abs(x - y).max()) for x, y in zip(a, b))


def _compare(a, f, scale_beta):
    e_sdf, e_rgb = _max_err(a["d_sdf"], f["d_sdf"]), _max_err(a["d_rgb"], f["d_rgb"])
    e_bg = float(np.abs(a["d_bg_rgb"] - f["d_bg_rgb"]).max())
    e_beta = abs(a["d_beta"] - f["d_beta"]) / scale_beta
    e_rays = float(np.abs(a["d_beta_rays"] - f["d_beta_rays"]).max()) / scale_beta
    return e_sdf, e_rgb, e_bg, e_beta, e_rays


@pytest.mark.parametrize("name", ALL)
def test_autograd_against_the_formulas_and_the_forward_against_geometry_reference(name):
    c, fwd, a, up = CR.reference(name)
    R, P, NZ = c["shape"]
    args = (R, c["inv"], c["z"], c["sdf"], c["rgb"], c["beta"], c["bg"])
    # forward: the weight sums are geometry_reference's; the torch restatement gives the numpy reference's values
    ref = G.geometry_reference(R, c["inv"], c["z"], c["sdf"], c["beta"], 0.5)
    assert np.abs(fwd["acc"] - ref["acc"]).max() <= 1e-12 and np.abs(fwd["acc_person"] - ref["acc_person"]).max() <= 1e-12
    assert np.abs(fwd["total"] - ref["total"]).max() <= 1e-9 * max(1.0, ref["total"].max())
    t64 = lambda x: torch.tensor(np.asarray(x), dtype=torch.float64)
    out = CR.composite_outputs(R, c["inv"], [t64(x) for x in c["z"]], [t64(x) for x in c["sdf"]], [t64(x) for x in c["rgb"]],
                               torch.full((R,), float(np.float32(c["beta"])), dtype=torch.float64), t64(c["bg"]))
    for k in CR.UP_KEYS:
        assert float(np.abs(out[k].numpy() - fwd[k]).max()) <= 1e-12, k
    hit = np.stack([np.asarray(iv) >= 0 for iv in c["inv"]], 1)
    none = ~hit.any(1)
    assert (fwd["bg_T"][none] == 1).all() and (fwd["rgb_values"][none] == c["bg"][none].astype(np.float64)).all()
    assert np.abs(fwd["fg_rgb_values"] - fwd["rgb_values"] - fwd["bg_T"][:, None] * (1 - c["bg"].astype(np.float64))).max() <= 1e-14
    # adjoint: all terms together, then each upstream gradient alone (its d beta relative to the whole gradient's)
    f = CR.adjoint_formulas(*args, up)
    top = max(float(np.abs(x).max()) for x in a["d_sdf"])
    errs = _compare(a, f, abs(a["d_beta"]))
    print(f"[composite] {name}: autograd vs formulas d sdf {errs[0]:.2e} abs (max |d sdf| {top:.2e}), d rgb {errs[1]:.2e}, d bg "
          f"{errs[2]:.2e}, d beta {errs[3]:.2e} rel, per ray {errs[4]:.2e}")
    assert max(errs) <= 1e-10, errs
    assert top > 0 and a["d_beta"] != 0
    for k in CR.UP_KEYS:
        _, _, a1, up1 = CR.reference(name, only=k) if name in ("thin-70x3", "opaque-9x2") else (None, None, None, None)
        if a1 is None:
            up1 = {k: c["up"][k]}
            a1 = CR.autograd_gradients(*args, up1)
        errs = _compare(a1, CR.adjoint_formulas(*args, up1), abs(a["d_beta"]))
        assert max(errs) <= 1e-10, (k, errs)
    # a white background: bg_rgb is None in both statements
    if name in ("thin-70x3", "opaque-9x2", "tiny-6x2-thin"):
        _, fw, aw, _ = CR.reference(name, white=True)
        fwh = CR.adjoint_formulas(*args[:-1], None, up)
        assert aw["d_bg_rgb"] is None and fwh["d_bg_rgb"] is None
        assert _max_err(aw["d_sdf"], fwh["d_sdf"]) <= 1e-10 and abs(aw["d_beta"] - fwh["d_beta"]) <= 1e-10 * abs(aw["d_beta"])
        assert np.abs(fw["rgb_values"] - fw["fg_rgb_values"]).max() == 0


@pytest.mark.parametrize("name", ALL)
def test_the_cases_are_conditioned(name):
    """thin cases: on at least half of the hit rays bg_T lies in [0.05, 0.95]; every case: |d beta| >= 0.1 sum |the rays' own
    d beta|; the case at beta = 0.001: max |d sdf| >= 1"""
    c, fwd, a, _ = CR.reference(name)
    hit = np.stack([np.asarray(iv) >= 0 for iv in c["inv"]], 1).any(1)
    T = fwd["bg_T"][hit]
    share = float(((T >= 0.05) & (T <= 0.95)).mean())
    ratio = abs(a["d_beta"]) / float(np.abs(a["d_beta_rays"]).sum())
    top = max(float(np.abs(x).max()) for x in a["d_sdf"])
    print(f"[composite] {name}: bg_T on hit rays min {T.min():.2e} median {np.median(T):.2e} max {T.max():.2e}, share in "
          f"[0.05, 0.95] {share:.2f}; |d beta| / sum |per ray| {ratio:.3f}; max |d sdf| {top:.3e}")
    if c["regime"] == "thin":
        assert share >= 0.5, share
    assert ratio >= 0.1, ratio
    if c["beta"] < 0.01:
        assert top >= 1.0, top
    assert abs(a["d_beta"] - a["d_beta_rays"].sum()) <= 1e-12 * np.abs(a["d_beta_rays"]).sum()
    # the inputs are of order 1, which the absolute bounds assume: colours and background in [0,1], unit normals
    for x in c["rgb"] + [c["bg"]]:
        assert x.min() >= 0 and x.max() <= 1
    assert all(np.abs(np.linalg.norm(n.astype(np.float64), axis=-1) - 1).max() < 1e-6 for n in c["nrm"])


def test_the_tie_rules_have_a_margin():
    # (a) identical depth rows: 'higher column first' (the columns swapped) gives other per-person opacities
    c = CR.tied_rows()
    R = c["shape"][0]
    ref = CR.composite_reference(R, c["inv"], c["z"], c["sdf"], c["rgb"], c["nrm"], c["beta"], c["bg"])
    swapped = CR.composite_reference(R, c["inv"], c["z"], c["sdf"][::-1], c["rgb"][::-1], c["nrm"][::-1], c["beta"], c["bg"])
    other = CR.composite_reference(R, c["inv"], c["z"], c["sdf"], c["rgb"], c["nrm"], c["beta"], c["bg"], person_sign=-1)
    assert np.abs(swapped["acc_person"][:, ::-1] - ref["acc_person"]).max() > 1e-2
    assert np.abs(swapped["acc_person"][:, ::-1] - other["acc_person"]).max() <= 1e-12      # the same statement twice
    assert np.abs(other["rgb_values"] - ref["rgb_values"]).max() > 1e-2
    # (b) the last-sample tie: rays 0..5 tie, 6 and 7 do not
    c = CR.last_tie_rows()
    R = c["shape"][0]
    args = (R, c["inv"], c["z"], c["sdf"], c["rgb"])
    ref = CR.composite_reference(*args, c["nrm"], c["beta"], c["bg"])
    other = CR.composite_reference(*args, c["nrm"], c["beta"], c["bg"], person_sign=-1)
    mut = CR.composite_reference(*args, c["nrm"], c["beta"], c["bg"], mutate="last_gt")
    print("[composite] last-sample tie: bg_T, higher person last", np.round(ref["bg_T"], 3), "lower person last", np.round(other["bg_T"], 3))
    assert (np.abs(ref["bg_T"][:6] - other["bg_T"][:6]) > 1e-2).all() and (ref["bg_T"][6:] == other["bg_T"][6:]).all()
    assert np.abs(mut["bg_T"] - other["bg_T"]).max() <= 1e-12 and ((ref["bg_T"] >= 0.05) & (ref["bg_T"] <= 0.95)).all()
    assert (ref["bg_T"][:3] < other["bg_T"][:3]).all() and (ref["bg_T"][3:6] > other["bg_T"][3:6]).all()
    # the mutation changes the last-sample rule and nothing else
    assert np.abs(ref["acc_person"] - mut["acc_person"]).max() == 0 and np.abs(ref["normal_values"] - mut["normal_values"]).max() == 0
    a = CR.autograd_gradients(*args, c["beta"], c["bg"], c["up"])
    f = CR.adjoint_formulas(*args, c["beta"], c["bg"], c["up"])
    assert _max_err(a["d_sdf"], f["d_sdf"]) <= 1e-10
    b = CR.autograd_gradients(*args, c["beta"], c["bg"], c["up"], person_sign=-1)
    last = CR.last_samples(c["inv"], c["sdf"])
    e, top = CR.dsdf_error(b["d_sdf"], a["d_sdf"], last)
    print(f"[composite] last-sample tie: d sdf of the last samples under the other rule differs by {e:.3e} of max {top:.3e}")
    assert e > 1e-2


def _mutation_sizes(c, mutate):
    """what the mutated float64 reference changes, in the measures of tests/test_composite_gpu.py:
    -> (forward, absolute; d sdf over max |d sdf|; d sdf on the restricted subset over its max; d bg_rgb over max |dC|)"""
    R = c["shape"][0]
    args = (R, c["inv"], c["z"], c["sdf"], c["rgb"])
    ref = CR.composite_reference(*args, c["nrm"], c["beta"], c["bg"])
    mut = CR.composite_reference(*args, c["nrm"], c["beta"], c["bg"], mutate=mutate)
    fwd = max(float(np.abs(ref[k] - mut[k]).max()) for k in ("rgb_values", "fg_rgb_values", "bg_T"))
    a = CR.adjoint_formulas(*args, c["beta"], c["bg"], c["up"])
    m = CR.adjoint_formulas(*args, c["beta"], c["bg"], c["up"], mutate=mutate)
    full, _ = CR.dsdf_error(m["d_sdf"], a["d_sdf"])
    thin, _ = CR.dsdf_error(m["d_sdf"], a["d_sdf"], CR.thin_subset(c["inv"], c["sdf"], ref["bg_T"]))
    dbg = float(np.abs(m["d_bg_rgb"] - a["d_bg_rgb"]).max()) / float(np.abs(c["up"]["rgb_values"]).max())
    return fwd, full, thin, dbg


def test_four_mistakes_would_be_seen_on_the_thin_cases():
    """Each mutation of the float64 reference, on every committed thin case (the last-sample tie rows for the tie rule, which
    random depths never draw): the change in the measure that sees it is at least 10x the measure's ceiling, and no committed
    bound is above its ceiling.  An opaque case is printed next to them: there the same mistakes vanish below the bounds, which
    is why the thin cases exist."""
    sees = dict(last_gt=(0, 2), no_exception=(2,), inclusive_last=(0, 2), ignore_bg=(0, 1))
    ceil = (TOL.CEIL_OUT, TOL.CEIL_DSDF, TOL.CEIL_DSDF, TOL.CEIL_OUT)
    for mutate in CR.MUTATIONS:
        cases = [CR.last_tie_rows()] if mutate == "last_gt" else [CR.case(n[0]) for n in CR.THIN]
        for c in cases + [CR.case("opaque-70x3-sharp")]:
            size = _mutation_sizes(c, mutate)
            print(f"[composite] mutation {mutate} on {c['name']}: forward {size[0]:.3e}, d sdf {size[1]:.3e}, d sdf restricted "
                  f"{size[2]:.3e}, d bg {size[3]:.3e}")
            if c["name"] != "opaque-70x3-sharp":
                for k in sees[mutate]:
                    assert size[k] >= 10 * ceil[k], (mutate, c["name"], k, size)


def test_constructed_zero_weight_rows():
    """the rows of (c): NaN colours exactly where fe == 0, a finite float64 answer, the empty ray shows the background"""
    c = CR.zero_weight_rows()
    R = c["shape"][0]
    assert all(np.isnan(x).any() for x in c["rgb"]) and all(np.isnan(x).any() for x in c["nrm"])
    ref = CR.composite_reference(R, c["inv"], c["z"], c["sdf"], c["rgb"], c["nrm"], c["beta"], c["bg"])
    for k, v in ref.items():
        assert np.isfinite(v).all(), k
    assert ref["bg_T"][0] == 1 and ref["acc"][0] == 0 and (ref["rgb_values"][0] == c["bg"][0]).all()
    assert ref["bg_T"][1] < 1e-80 and abs(ref["acc"][1] - 1) < 1e-12 and ref["acc_person"][1, 1] < 1e-80
    assert 0.05 < ref["acc"][2] < 0.99
