"""The mesh-free interpenetration term, host side: the reference restatement (tests/penetration_reference.py) on the seeded
11 x 11 training scene -- the pair table, the cancellation of the translation gradients, its gradient against float64 finite
differences, the cap on the points a float32 implementation may decide differently -- and the header / binding / docs."""
import functools
import os
import re

import numpy as np
import torch

from oracle import multiply_oracle as O
from tests import penetration_reference as PR
from tests.util import seeded_networks, t32

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY = ("smpl_pose", "smpl_trans", "smpl_shape")
ENTRY_POINTS = ("mp_pen_probe", "mp_pen_loss", "mp_pen_scatter_bwd")
# (probed, active) of the ordered pairs, every SMPL vertex a probe point
TABLE = {2: {(0, 1): (322, 148), (1, 0): (989, 112)},
         3: {(1, 2): (424, 310), (2, 1): (916, 0), (0, 2): (0, 0), (2, 0): (0, 0)}}


def scene(P):
    """make_scene(P, seed=0, H=11, W=11) with the seeded geometric-init networks: the scene of test_train_step_gpu._train_setup"""
    from multiply_amd.synthetic import make_scene, make_smpl_tables
    tables = make_smpl_tables(0)
    sc = make_scene(P, seed=0, H=11, W=11)
    m, _ = seeded_networks(P, 0)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    sp = t32(sc["smpl_params"])
    inp = dict(uv=t32(sc["uv"]), intrinsics=t32(sc["intrinsics"]), pose=t32(sc["pose"]), smpl_params=sp, smpl_pose=sp[:, :, 4:76],
               smpl_shape=sp[:, :, 76:], smpl_trans=sp[:, :, 1:4], idx=torch.tensor([3]))
    return O.MultiplyOracle(sd, tables, sc["smpl_params"][0, :, 76:]), inp


def all_vertices(oracle):
    V = oracle.servers[0].verts_c.shape[0]
    return {p: torch.arange(V) for p in range(len(oracle.servers))}


@functools.lru_cache(maxsize=None)
def reference(P):
    """the float64 restatement with the body inputs attached, and its gradient -> (oracle, inp, result, {body tensor: grad})"""
    oracle, inp = scene(P)
    inp = dict(inp)
    for k in BODY:
        inp[k] = inp[k].clone().requires_grad_(True)
    res = PR.interpenetration(oracle, inp, all_vertices(oracle), cond_zero=False)
    g = torch.autograd.grad(res["loss"].sum(), [inp[k] for k in BODY])
    return oracle, inp, res, dict(zip(BODY, g))


def test_pair_table_of_the_seeded_scene():
    for P in (2, 3):
        _, _, res, _ = reference(P)
        got = {k: (int(v["probed"].sum()), int(v["active"].sum())) for k, v in res["pairs"].items()}
        print(f"[penetration] P = {P}: (probed, active) per pair {got}; L = {float(res['loss']):.4f}")
        for pair, want in TABLE[P].items():
            assert got[pair] == want, (P, pair, got[pair], want)
        for pair, v in res["pairs"].items():
            n_act = int(v["active"].sum())
            if n_act:                                        # both signs occur in every pair with active points
                assert 0 < n_act < int(v["probed"].sum()), (P, pair)
            assert torch.equal(v["ids"], torch.sort(v["ids"]).values)
    assert abs(float(reference(2)[2]["loss"]) - 6.079) < 2e-3
    # the total is symmetric in the roles only as a sum: the matrix is not (what catches p and q swapped)
    pairs = reference(2)[2]["pairs"]
    assert abs(float(pairs[(0, 1)]["loss"]) - float(pairs[(1, 0)]["loss"])) > 0.1


def test_translation_gradients_cancel_and_the_pose_gradient_is_large():
    _, _, _, g = reference(2)
    gt = g["smpl_trans"][0]
    print(f"[penetration] d L / d trans {gt.tolist()}; sum over persons {gt.sum(0).tolist()}; |d pose| max {float(g['smpl_pose'].abs().max()):.3f}")
    assert float(gt.abs().max()) > 1.0                       # each person is pushed ...
    assert float(gt.sum(0).abs().max()) < 1e-4               # ... and a common shift moves nothing (measured 2e-6)
    assert 8.0 < float(g["smpl_pose"].abs().max()) < 32.0    # measured 16


def test_reference_gradient_against_float64_finite_differences():
    """body models in float64 too (penetration_reference.servers64): central differences along 6 random directions of (pose, trans, shape)"""
    oracle, inp = scene(2)
    idx = all_vertices(oracle)
    with PR.float64_default():
        servers = PR.servers64(oracle)
        base = {k: inp[k].double() for k in BODY + ("smpl_params",)}

        def loss_of(delta, t, grad=False):
            x = dict(base)
            for k in BODY:
                x[k] = (base[k] + t * delta[k]).requires_grad_(grad)
            return PR.interpenetration(oracle, x, idx, servers=servers)["loss"].sum(), x
        L0, x0 = loss_of({k: torch.zeros_like(base[k]) for k in BODY}, 0.0, grad=True)
        g = dict(zip(BODY, torch.autograd.grad(L0, [x0[k] for k in BODY])))
        rs = np.random.RandomState(3)
        h = 1e-6
        for d in range(6):
            delta = {k: torch.from_numpy(rs.randn(*base[k].shape)) for k in BODY}
            with torch.no_grad():
                fd = (float(loss_of(delta, h)[0]) - float(loss_of(delta, -h)[0])) / (2 * h)
            an = sum(float((g[k] * delta[k]).sum()) for k in BODY)
            print(f"[penetration] direction {d}: analytic {an:.8f}, central difference {fd:.8f}")
            # the term is C^1 in s at 0 and only the 0.1 rule is discontinuous: a step of 1e-6 crosses it nowhere on this scene
            assert abs(an - fd) < 1e-5 * max(1.0, abs(an)), (d, an, fd)


def test_exclusion_cap_holds_on_the_reference_alone():
    for P in (2, 3):
        _, _, res, _ = reference(P)
        for pair, v in res["pairs"].items():
            k = int(v["excluded"].sum())
            print(f"[penetration] P = {P} pair {pair}: {k} excluded of {int(v['probed'].sum())} probed")
            assert PR.excluded_ok(v), (P, pair, k)


def test_header_binding_and_docs_agree():
    from multiply_amd import hip
    protos = hip.header_prototypes()
    hdr = open(hip.HEADER_PATH).read()
    src = open(os.path.join(REPO, "multiply_amd", "csrc", "penetration.hip")).read()
    for name in ENTRY_POINTS:
        assert name in protos and name not in hip.VALUE_RETURNING, name
        assert re.search(r'extern "C" int %s\(' % name, src), name
        assert protos[name][1][-1] is hip.DevPtr                 # the stream
    assert len(protos["mp_pen_probe"][1]) == 12 and len(protos["mp_pen_loss"][1]) == 8 and len(protos["mp_pen_scatter_bwd"][1]) == 11
    n = len(set(re.findall(r"\b(mp_[a-z_0-9]+)\s*\(", hdr)))
    for doc in ("README.md", "DESIGN.md"):
        quoted = re.findall(r"(\d+) `extern \"C\"` entry points", open(os.path.join(REPO, doc)).read())
        assert quoted and all(int(q) == n for q in quoted), (doc, quoted, n)
    # the person limit of a call is the compositing kernels'
    limit = int(re.search(r"constexpr int MAX_P = (\d+);", open(os.path.join(REPO, "multiply_amd", "csrc", "ray_merge.hpp")).read()).group(1))
    assert limit == 8 and "2 .. 8" in hdr
    from multiply_amd.multiply import Multiply
    assert Multiply.train_interpenetration is False and Multiply.interpenetration_points == 5120
