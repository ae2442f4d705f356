"""Inputs shared by tests/test_keypoint_fit_cpu.py and tests/test_keypoint_fit_gpu.py: the maps, the rows and the recovery
sequence, all seeded; the float64 results are computed once per process and never modified.  Not a test."""
import functools

import numpy as np
import torch

from multiply_amd import keypoint_fit as KF
from tests import keypoint_fit_reference as R

FX = 500.0        # a body 3 m away: 1 cm is 1.7 px, so noise of a few px is well below rho = 100 and a swapped limb well above


def extra_regressor(seed=3):
    """9 random 8-sparse rows that sum to 1 (a stand-in for J_regressor_extra.npy, which is not distributed)"""
    rng = np.random.default_rng(seed)
    ex = np.zeros((9, 6890))
    for r in range(9):
        ids = rng.choice(6890, 8, replace=False)
        w = rng.random(8) + 0.1
        ex[r, ids] = w / w.sum()
    return ex


@functools.lru_cache(None)
def maps():
    rng = np.random.default_rng(5)
    shared = 4321
    ra = ("regressor", np.array([shared, 10, 2000]), np.array([0.5, 0.25, 0.25]))
    rb = ("regressor", np.array([6000, shared]), np.array([0.3, 0.7]))
    return {
        "joints": KF.KeypointMap.from_joints([0, 7, 21]),
        "vertices": KF.KeypointMap.from_vertices([332, 6787]),
        "mixed": KF.KeypointMap.from_rows([("joint", 15), ("vertex", 3216), ra, rb, ("joint", 4)]),
        # coco25-shaped: 15 joints, the nose vertex, and all 9 extra-regressor rows
        "coco25-shaped": KF.KeypointMap.from_smpl54(KF.COCO25_SMPL54[:16] + tuple(range(45, 54)), extra_regressor(),
                                                    joint_weights=np.where(np.isin(np.arange(25), KF.COCO25_IGNORED), 0.0, 1.0)),
    }


def camera_row(extrinsic):
    E = np.eye(4)[:3]
    if extrinsic:                       # a camera turned 0.2 rad about y and moved
        a = 0.2
        E = np.array([[np.cos(a), 0, np.sin(a), 0.1], [0, 1, 0, -0.05], [-np.sin(a), 0, np.cos(a), 0.4]])
    return torch.tensor(np.concatenate([[FX, FX * 1.1, 256.0, 250.0], E.reshape(-1)]), dtype=torch.float64)


def rows(seed=0):
    """three parameter rows (3, 85): zero pose; N(0, 0.3) with betas; N(0, 0.6) with betas (used with the extrinsic)"""
    g = torch.Generator().manual_seed(seed)
    p = torch.zeros(3, 85, dtype=torch.float64)
    p[:, 0:3] = torch.tensor([0.0, 0.2, 3.0]) + 0.1 * torch.randn(3, 3, generator=g).double()
    p[1, 3:75] = 0.3 * torch.randn(72, generator=g).double()
    p[2, 3:75] = 0.6 * torch.randn(72, generator=g).double()
    p[1, 75:] = torch.randn(10, generator=g).double()
    p[2, 75:] = 0.5 * torch.randn(10, generator=g).double()
    return p.float().double()           # (exactly representable in float32)


def cameras():
    return torch.stack([camera_row(False), camera_row(False), camera_row(True)])


def objective_case(T, name, seed=1):
    """inputs of the three rows for map `name`: targets with residuals of a few px and of several rho, confidences of which some
    fall below the threshold, a temporal target near the row.  Everything float32-representable doubles."""
    kmap = maps()[name]
    g = torch.Generator().manual_seed(seed)
    p, cam = rows(), cameras()
    K = kmap.K
    Tr, kr = R.reduced_tables(T, kmap)
    targets = torch.zeros(3, K, 2, dtype=torch.float64)
    for n in range(3):
        with R._Double():
            uv, _ = R.project(R.keypoints3d(Tr, kr, p[n]), cam[n])
        noise = 4.0 * torch.randn(K, 2, generator=g).double()
        noise[::2] += 350.0 * torch.randn((K + 1) // 2, 2, generator=g).double().sign()     # every other keypoint: far outside rho
        targets[n] = uv + noise
    conf = torch.rand(3, K, generator=g).double()
    conf[:, K // 2] = 0.1                                    # below the threshold: c = 0
    prev = (p[:, :75] + 0.05 * torch.randn(3, 75, generator=g).double())
    f = lambda x: x.float().double()
    return dict(kmap=kmap, params=p, cam=f(cam), targets=f(targets), c=f(KF.keypoint_weights(conf, kmap, 0.3)), prev=f(prev),
                reduced=(Tr, kr))


@functools.lru_cache(None)
def _tables():
    from multiply_amd.synthetic import make_smpl_tables
    return R.tables64(make_smpl_tables(0))


@functools.lru_cache(None)
def objective_reference(name):
    """per row: terms, grad, proj of the float64 restatement"""
    cs = objective_case(_tables(), name)
    Tr, kr = cs["reduced"]
    out = [R.objective_and_grad(Tr, kr, cs["params"][n], cs["targets"][n], cs["c"][n], cs["cam"][n], cs["prev"][n]) for n in range(3)]
    return cs, out


FIT_ITERS = (0, 1, 2, 25, 150)


@functools.lru_cache(None)
def fit_reference(name="mixed", iters=150, w_2d=R.REF["w_2d"], w_t=R.REF["w_t"]):
    """per row: the parameters after each count of FIT_ITERS (<= iters) and the history of all steps"""
    cs = objective_case(_tables(), name)
    Tr, kr = cs["reduced"]
    out = []
    for n in range(3):
        p = cs["params"][n].clone()
        m, v, lrs = torch.zeros_like(p), torch.zeros_like(p), R.lr_row(1e-3)
        hist, snap = torch.zeros(iters, 3, dtype=torch.float64), {0: p.clone()}
        for it in range(iters):
            terms, gr, _, _ = R.objective_and_grad(Tr, kr, p, cs["targets"][n], cs["c"][n], cs["cam"][n], cs["prev"][n], w_2d=w_2d, w_t=w_t)
            hist[it] = terms
            p, m, v = R.adam_step(p, gr, m, v, it + 1, lrs)
            if it + 1 in FIT_ITERS:
                snap[it + 1] = p.clone()
        out.append((snap, hist))
    return cs, out


# ---- recovery: 3 frames x 2 persons, person 1 tracked in frame 2, frame 1 copied
REC_F, REC_P, REC_ITERS = 3, 2, 150
REC_TRACKING, REC_INTERP = ((2, 1),), (1,)
REC_POSE_NOISE, REC_TRANS_NOISE = 0.12, 0.04      # chosen on the CPU: the float64 loop alone more than halves the error
                                                   # (test_keypoint_fit_cpu.py asserts it)


@functools.lru_cache(None)
def recovery_case():
    T = _tables()
    kmap = maps()["coco25-shaped"]
    Tr, kr = R.reduced_tables(T, kmap)
    g = torch.Generator().manual_seed(9)
    gt = torch.zeros(REC_F, REC_P, 85, dtype=torch.float64)
    base = torch.zeros(REC_P, 85, dtype=torch.float64)
    base[:, 0:3] = torch.tensor([[-0.4, 0.1, 3.0], [0.5, 0.15, 3.4]])
    base[:, 3:75] = 0.25 * torch.randn(REC_P, 72, generator=g).double()
    base[:, 75:] = 0.5 * torch.randn(REC_P, 10, generator=g).double()
    for f in range(REC_F):                                   # a slow motion
        gt[f] = base
        gt[f, :, 0] += 0.02 * f
        gt[f, :, 3:75] += 0.01 * f * torch.randn(REC_P, 72, generator=g).double()
    cam = camera_row(False)
    kps = torch.zeros(REC_F, REC_P, kmap.K, 3, dtype=torch.float64)
    for f in range(REC_F):
        for q in range(REC_P):
            with R._Double():
                kps[f, q, :, :2] = R.project(R.keypoints3d(Tr, kr, gt[f, q]), cam)[0]
    kps[..., 2] = 0.9
    kps[:, :, 3, 2] = 0.2                                    # one undetected keypoint
    init = gt.clone()
    init[:, :, 3:75] += REC_POSE_NOISE * torch.randn(REC_F, REC_P, 72, generator=g).double()
    init[:, :, 0:3] += REC_TRANS_NOISE * torch.randn(REC_F, REC_P, 3, generator=g).double()
    f32 = lambda x: x.float()
    return dict(kmap=kmap, reduced=(Tr, kr), gt=gt, cam=cam, keypoints=f32(kps), init=f32(init))


def reprojection_error(case, params):
    """mean distance in px between the detected keypoints with weight and the projections of params (F, P, 85), in float64"""
    Tr, kr = case["reduced"]
    kp = case["keypoints"].double()
    w = KF.keypoint_weights(kp[..., 2], case["kmap"], 0.6) > 0
    d = []
    for f in range(REC_F):
        for q in range(REC_P):
            with R._Double():
                uv = R.project(R.keypoints3d(Tr, kr, params[f, q].double()), case["cam"])[0]
            d.append((uv - kp[f, q, :, :2]).norm(dim=1)[w[f, q]])
    return float(torch.cat(d).mean())


@functools.lru_cache(None)
def recovery_reference():
    """the float64 loop through multiply_amd.keypoint_fit.sequence_loop: results (F, P, 85), temporal targets, errors before/after"""
    cs = recovery_case()
    Tr, kr = cs["reduced"]
    init = cs["init"].double()
    kp = cs["keypoints"].double()
    c = KF.keypoint_weights(kp[..., 2], cs["kmap"], 0.6)
    tracked = torch.zeros(REC_F, REC_P, dtype=torch.bool)
    for f, q in REC_TRACKING:
        tracked[f, q] = True

    def fit(f, start, prev):
        return torch.stack([R.fit(Tr, kr, start[q], kp[f, q, :, :2], c[f, q], cs["cam"], prev[q], REC_ITERS)[0] for q in range(REC_P)])

    res, prevs = KF.sequence_loop(init, tracked, REC_INTERP, fit)
    return dict(results=res, prev=prevs, before=reprojection_error(cs, init), after=reprojection_error(cs, res))
