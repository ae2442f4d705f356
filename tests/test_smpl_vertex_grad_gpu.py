"""SMPLServer.forward under autograd: smpl_verts / smpl_jnts / smpl_all_jnts / smpl_tfs carry gradients to scale, transl,
thetas and betas (lib/model/smpl.py:50-94 returns them as ordinary autograd tensors), through the posed vertices' adjoint
(csrc/smpl.hip mp_smpl_verts_bwd) and the chain adjoint (csrc/smpl.hip mp_smpl_pose_bwd_lbs).  Reference: torch autograd on
the oracle's plain-torch restatement (oracle.multiply_oracle.smpl_server_forward), evaluated in float64 on the fp32 tables and
on the device's own canonical inverse transforms, so that the comparison measures the device's error alone."""
import copy

import numpy as np
import pytest
import torch

from oracle import multiply_oracle as O

pytestmark = pytest.mark.gpu

BETAS = np.linspace(-0.5, 0.5, 10).astype(np.float32)
KEYS = ("smpl_verts", "smpl_jnts", "smpl_all_jnts", "smpl_tfs")
SLICES = (("scale", slice(0, 1)), ("transl", slice(1, 4)), ("thetas", slice(4, 76)), ("betas", slice(76, 86)))
# relative to the largest entry of each slice.  d scale = sum_i g_i . x_i / s inherits the fp32 rounding of every posed position
# x_i: under a random functional that error adds over the N terms while the sum grows like sqrt(N) (measured up to 8.7e-5, zero
# thetas, all four outputs); the other slices measured <= 1.4e-6
GRAD_RTOL = {"scale": 3e-4, "transl": 1e-5, "thetas": 1e-5, "betas": 1e-5}


class _Oracle64:
    """oracle.smpl_server_forward in float64 (tables upcast) with the device server's tfs_c_inv"""

    def __init__(self, so, tfs_c_inv):
        self.T = copy.copy(so.T)
        for k, v in vars(so.T).items():
            if torch.is_tensor(v) and v.is_floating_point():
                setattr(self.T, k, v.double())
        self.tfs_c_inv = tfs_c_inv.detach().double().cpu()

    def forward(self, scale, transl, thetas, betas):
        dt = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)          # (the restatement's constant tensors follow the default dtype)
        try:
            return O.smpl_server_forward(self.T, scale.double(), transl.double(), thetas.double(), betas.double(), self.tfs_c_inv)
        finally:
            torch.set_default_dtype(dt)


@pytest.fixture(scope="module")
def servers(smpl_tables):
    from multiply_amd.smpl import SMPLServer
    server = SMPLServer(betas=BETAS, smpl_tables=smpl_tables)
    return server, _Oracle64(O.SMPLServerOracle(smpl_tables, BETAS), server.tfs_c_inv)


def _poses():
    g = torch.Generator().manual_seed(11)
    out = {}
    p = torch.zeros(86)
    p[0], p[76:] = 1.0, torch.tensor(BETAS)
    out["zero thetas"] = p.clone()                                    # every joint in the |theta + 1e-8| branch
    axis = torch.randn(24, 3, generator=g)
    p[4:76] = (axis / axis.norm(dim=1, keepdim=True) * (np.pi - 1e-3)).reshape(72)
    p[1:4] = torch.randn(3, generator=g) * 0.2
    out["near pi"] = p.clone()
    p = torch.zeros(86)
    p[0], p[4:76], p[76:] = 1.0, O.canonical_thetas(), torch.tensor(BETAS)
    out["A-pose"] = p.clone()
    p = torch.zeros(86)
    p[0] = 1.3
    p[1:4] = torch.randn(3, generator=g) * 0.3
    p[4:76] = torch.randn(72, generator=g) * 0.4
    p[76:] = torch.tensor(BETAS) + 0.2 * torch.randn(10, generator=g)
    out["scale 1.3, betas"] = p
    return out


def _oracle_outputs(so, pg):
    o = so.forward(pg[0], pg[1:4], pg[4:76], pg[76:])
    from multiply_amd.smpl import FACE_KEYPOINT_VERTS
    allj = torch.cat([o["smpl_jnts"], o["smpl_verts"][list(FACE_KEYPOINT_VERTS)]], 0)
    return {"smpl_verts": o["smpl_verts"], "smpl_jnts": o["smpl_jnts"], "smpl_all_jnts": allj, "smpl_tfs": o["smpl_tfs"]}


def _device_grad(server, prm, weights, keys):
    pg = prm.cuda().requires_grad_(True)
    out = server(pg[0:1], pg[1:4], pg[4:76], pg[76:86])
    loss = sum((out[k][0] * weights[k].cuda()).sum() for k in keys)
    (g,) = torch.autograd.grad(loss, pg)
    return g.cpu().double(), out


def _rel(got, want):
    return {n: (got[sl] - want[sl]).abs().max().item() / (want[sl].abs().max().item() + 1e-30) for n, sl in SLICES}


@pytest.mark.parametrize("pose", list(_poses()))
def test_vertex_and_joint_gradients_match_autograd(servers, pose):
    server, so = servers
    prm = _poses()[pose]
    g = torch.Generator().manual_seed(3)
    pg = prm.clone().double().requires_grad_(True)
    want_out = _oracle_outputs(so, pg)
    weights = {k: torch.randn(want_out[k].shape, generator=g) for k in KEYS}
    weights["smpl_tfs"][:, 3, :] = 0                                    # (the constant last row)
    worst = 0.0
    for keys in [(k,) for k in KEYS] + [KEYS]:
        (want,) = torch.autograd.grad(sum((want_out[k] * weights[k].double()).sum() for k in keys), pg, retain_graph=True)
        got, out = _device_grad(server, prm, weights, keys)
        for k in KEYS:       # the values are the no-grad forward's
            assert out[k].requires_grad
            assert (out[k][0].detach().cpu().double() - want_out[k].detach()).abs().max() < 1e-4, k
        err = _rel(got, want)
        worst = max(worst, max(err.values()))
        print(f"[grad parity] smpl {pose} d({'+'.join(keys)}): " + ", ".join(f"{n} {e:.2e}" for n, e in err.items()))
        assert all(e < GRAD_RTOL[n] for n, e in err.items()), (pose, keys, err)
    print(f"[grad parity] smpl {pose}: worst {worst:.2e}")


def test_values_unchanged_by_grad_mode(servers):
    server, _ = servers
    prm = _poses()["scale 1.3, betas"].cuda()
    with torch.no_grad():
        ref = server(prm[0:1], prm[1:4], prm[4:76], prm[76:86])
    pg = prm.clone().requires_grad_(True)
    out = server(pg[0:1], pg[1:4], pg[4:76], pg[76:86])
    for k in KEYS:
        assert torch.equal(out[k].detach(), ref[k]), k
        assert not ref[k].requires_grad
    absolute = server(pg[0:1], pg[1:4], pg[4:76], pg[76:86], absolute=True)
    assert not any(absolute[k].requires_grad for k in KEYS)


def test_backward_is_deterministic(servers):
    server, so = servers
    prm = _poses()["near pi"]
    g = torch.Generator().manual_seed(5)
    w = {k: torch.randn(v.shape, generator=g) for k, v in _oracle_outputs(so, prm).items()}
    a, _ = _device_grad(server, prm, w, KEYS)
    b, _ = _device_grad(server, prm, w, KEYS)
    assert torch.equal(a, b)
    dv = torch.randn(6890, 3, generator=g).cuda()
    d1 = server.pose_backward(prm.cuda(), dverts=dv)
    d2 = server.pose_backward(prm.cuda(), dverts=dv)
    assert torch.equal(d1, d2) and d1.abs().max() > 0


def test_keypoint_loss_reaches_only_its_frame_of_body_model_params(servers):
    """A loss on smpl_all_jnts of frame k (keypoint reprojection is the usual case) gives gradients on row k of the per-frame
    embeddings and on the shared betas row only, equal to the oracle's."""
    from multiply_amd.body_model_params import BodyModelParams
    server, so = servers
    n_frames, k = 4, 2
    g = torch.Generator().manual_seed(9)
    bm = BodyModelParams(n_frames).cuda()
    init = {"betas": torch.tensor(BETAS)[None] + 0.1, "global_orient": torch.randn(n_frames, 3, generator=g) * 0.3,
            "transl": torch.randn(n_frames, 3, generator=g) * 0.2, "body_pose": torch.randn(n_frames, 69, generator=g) * 0.3}
    for name, v in init.items():
        bm.init_parameters(name, v.cuda(), requires_grad=True)
    w = torch.randn(29, 3, generator=g)
    rows = bm(torch.tensor([k]).cuda())
    scale = torch.tensor([1.1]).cuda()
    out = server(scale, rows["transl"], torch.cat([rows["global_orient"], rows["body_pose"]], 1), rows["betas"])
    (out["smpl_all_jnts"][0] * w.cuda()).sum().backward()
    # oracle
    params = {n: v.clone().double().requires_grad_(True) for n, v in init.items()}
    th = torch.cat([params["global_orient"][k], params["body_pose"][k]])
    want_all = _oracle_outputs(so, torch.cat([torch.tensor([1.1], dtype=torch.float64), params["transl"][k], th,
                                              params["betas"][0]]))["smpl_all_jnts"]
    (want_all * w.double()).sum().backward()
    for name in init:
        got = getattr(bm, name).weight.grad.cpu().double()
        want = params[name].grad
        row = 0 if name == "betas" else k
        others = [r for r in range(got.shape[0]) if r != row]
        assert got[others].abs().max() == 0 if others else True, name
        assert got[row].abs().max() > 0, name
        e = (got[row] - want[row]).abs().max().item() / want[row].abs().max().item()
        print(f"[grad parity] BodyModelParams.{name} row {row}: rel-to-max err {e:.2e}")
        assert e < GRAD_RTOL["thetas"], name
