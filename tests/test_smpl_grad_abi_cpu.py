"""Layout constants of the SMPL adjoint's C ABI (include/multiply_hip.h) as the Python binding states them."""
import os
import re

from multiply_amd import hip

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_smpl_adjoint_layout_constants_match_the_header():
    hdr = open(os.path.join(REPO, "include", "multiply_hip.h")).read()
    consts = {m.group(1): eval(m.group(2)) for m in re.finditer(r"#define (MP_SMPL_\w+) \(([\d *+]+)\)", hdr)}
    assert consts["MP_SMPL_VBWD_SCRATCH"] == hip.SMPL_VBWD_SCRATCH
    assert consts["MP_SMPL_DLBS"] == hip.SMPL_DLBS == 24 * 16 + 207 + 86
    protos = hip.header_prototypes()
    for name, n_args in (("mp_smpl_verts_bwd", 9), ("mp_smpl_pose_bwd_lbs", 12), ("mp_tr_gather_bwd", 7)):
        assert len(protos[name][1]) == n_args, name
