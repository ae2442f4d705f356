"""Yardsticks of the trainer's tests: torch.optim.Adam's single-tensor step (no weight decay, no amsgrad) in float64, the same step
through torch's own CPU fp32 optimiser, the table of tensors both GPU and CPU tests use, and the conditions of the reference's
training step (multiply_model.py:137-160) written out."""
import numpy as np
import torch

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8

# ---- the table of test 1 / 2 / 3: sizes, groups, step counts and the float offsets (within 16 bytes) of each tensor's buffers
SIZES = [(1,), (3,), (10,), (63,), (64,), (65,), (257,), (256, 295)]
GROUPS = [0, 1, 0, 1, 0, 1, 0, 1]
LRS = [5e-4, 5e-5]
STEPS = [0, 999, 0, 999, 999, 0, 999, 0]
INACTIVE, ZERO_GRAD = 3, 4                  # record 3 has no gradient; record 4 an all-zero one on non-zero moments
G_PHASE = [0, 1, 2, 3, 0, 1, 2, 3]          # gradients: views at float offsets 0, 1, 2, 3 of one flat buffer
P_PHASE = [0, 1, 2, 3, 0, 2, 0, 3]
M_PHASE = [0, 1, 2, 3, 0, 2, 1, 3]          # = P_PHASE except record 6: its moments sit elsewhere within 16 bytes -> scalar path
MODES = [1, 1, 1, 1, 1, 2, 0, 1]            # trainer.ADAM_VEC / ADAM_VEC_G4 / ADAM_SCALAR expected from those offsets


def make_state(seed=0):
    """fp32 arrays per tensor: p, m, v, and the step count before the step (fresh tensors: zero moments)"""
    rs = np.random.RandomState(seed)
    ps, ms, vs = [], [], []
    for shape, t in zip(SIZES, STEPS):
        ps.append(rs.normal(0, 0.3, shape).astype(np.float32))
        if t:
            ms.append(rs.normal(0, 3e-3, shape).astype(np.float32))
            vs.append((rs.normal(0, 1e-2, shape) ** 2 * rs.uniform(0.1, 1.0, shape)).astype(np.float32))
        else:
            ms.append(np.zeros(shape, np.float32))
            vs.append(np.zeros(shape, np.float32))
    return ps, ms, vs, list(STEPS)


def make_grads(seed=1):
    """fp32 gradients per tensor; None for the inactive record, zeros for the zero-gradient one"""
    rs = np.random.RandomState(seed)
    gs = []
    for i, shape in enumerate(SIZES):
        g = (rs.normal(0, 1e-2, shape) * np.exp(rs.normal(0, 1.0, shape))).astype(np.float32)
        gs.append(None if i == INACTIVE else (np.zeros(shape, np.float32) if i == ZERO_GRAD else g))
    return gs


def layout(phases, sizes=SIZES):
    """float offsets of the tensors in one flat buffer: each starts `phase` floats past a 16-byte boundary -> (offsets, total)"""
    offs, cur = [], 0
    for shape, ph in zip(sizes, phases):
        cur = (cur + 3) // 4 * 4 + ph
        offs.append(cur)
        cur += int(np.prod(shape))
    return offs, cur + 4


def adam_step64(p, g, m, v, t, lr, beta1=BETA1, beta2=BETA2, eps=EPS):
    """one step in float64 from fp32 (or float64) state; t = the count BEFORE the step -> p', m', v' (float64)"""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    t1 = t + 1
    m2 = m + (g - m) * (1.0 - beta1)
    v2 = v * beta2 + (1.0 - beta2) * g * g
    denom = np.sqrt(v2) / np.sqrt(1.0 - beta2 ** t1) + eps
    return p - (lr / (1.0 - beta1 ** t1)) * (m2 / denom), m2, v2


def lr32(lr):
    """the rate as the device holds it (one fp32), as a python float"""
    return float(np.float32(lr))


def table_step64(ps, gs, ms, vs, steps, groups=GROUPS, lrs=LRS):
    """the float64 step of a whole table; an entry without a gradient is returned as it is (same objects), count unchanged"""
    out_p, out_m, out_v, out_t = [], [], [], []
    for p, g, m, v, t, gr in zip(ps, gs, ms, vs, steps, groups):
        if g is None:
            out_p.append(p); out_m.append(m); out_v.append(v); out_t.append(t)
            continue
        p2, m2, v2 = adam_step64(p, g, m, v, t, lr32(lrs[gr]))
        out_p.append(p2); out_m.append(m2); out_v.append(v2); out_t.append(t + 1)
    return out_p, out_m, out_v, out_t


def torch_state_dict(opt, ms, vs, steps):
    """a torch.optim.Adam state dict over opt's parameters carrying the given moments and counts (count 0: no state, as torch has
    none before a tensor's first step)"""
    sd = opt.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(t)), "exp_avg": torch.as_tensor(np.array(m, dtype=np.float32)),
                       "exp_avg_sq": torch.as_tensor(np.array(v, dtype=np.float32))}
                   for i, (m, v, t) in enumerate(zip(ms, vs, steps)) if t}
    return sd


def torch_cpu_optimizer(ps, groups=GROUPS, lrs=LRS):
    params = [torch.tensor(np.array(p, dtype=np.float32)) for p in ps]
    gl = [{"params": [q for q, g in zip(params, groups) if g == k], "lr": lr32(lr)} for k, lr in enumerate(lrs)]
    order = [i for k in range(len(lrs)) for i, g in enumerate(groups) if g == k]       # state-dict index -> table index
    return torch.optim.Adam(gl, lr=lr32(lrs[0]), betas=(BETA1, BETA2), eps=EPS, foreach=False), params, order


def table_step_torch32(ps, gs, ms, vs, steps, groups=GROUPS, lrs=LRS, n_steps=1, grads_per_step=None):
    """the same step(s) through torch.optim.Adam(foreach=False) on CPU fp32 tensors -> p, m, v (fp32 numpy), counts"""
    opt, params, order = torch_cpu_optimizer(ps, groups, lrs)
    opt.load_state_dict(torch_state_dict(opt, [ms[i] for i in order], [vs[i] for i in order], [steps[i] for i in order]))
    for s in range(n_steps):
        cur = gs if grads_per_step is None else grads_per_step[s]
        for q, g in zip(params, cur):
            q.grad = None if g is None else torch.tensor(np.array(g, dtype=np.float32))
        opt.step()
    sd = opt.state_dict()["state"]
    inv = {i: k for k, i in enumerate(order)}
    out_m, out_v, out_t = [], [], []
    for i in range(len(ps)):
        st = sd.get(inv[i])
        out_m.append(st["exp_avg"].numpy().copy() if st else np.array(ms[i], np.float32))
        out_v.append(st["exp_avg_sq"].numpy().copy() if st else np.array(vs[i], np.float32))
        out_t.append(float(st["step"]) if st else steps[i])
    return [q.detach().numpy().copy() for q in params], out_m, out_v, out_t


def half_ulp32(x):
    return 0.5 * np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def c_of_step(got_p, got_m, got_v, ps, want_p, want_m, want_v):
    """the constants of test 1's bounds that `got` needs against the float64 step `want`:
    c_p = max (|p - p64| - half ulp(p64)) / (2^-24 |p64 - p_before|),  c_mv = max relative error of m', v' / 2^-24"""
    c_p = c_mv = 0.0
    for gp, gm, gv, p0, wp, wm, wv in zip(got_p, got_m, got_v, ps, want_p, want_m, want_v):
        if wp is p0:
            continue
        dp = np.abs(wp - np.asarray(p0, np.float64))
        over = np.abs(np.asarray(gp, np.float64) - wp) - half_ulp32(wp)
        ok = dp > 0
        if ok.any():
            c_p = max(c_p, float((over[ok] / (2.0 ** -24 * dp[ok])).max()))
        assert (over[~ok] <= 0).all()
        for got, want in ((gm, wm), (gv, wv)):
            nz = want != 0
            if nz.any():
                c_mv = max(c_mv, float((np.abs(np.asarray(got, np.float64) - want)[nz] / np.abs(want[nz])).max() / 2.0 ** -24))
            assert (np.asarray(got)[~nz] == 0).all()
    return max(c_p, 0.0), c_mv


# ---- the conditions of multiply_model.py:137-160 (and :187, :195) written out, for the grid test of trainer.step_plan
def reference_step_conditions(epoch, has_sam_mask, is_certain, depth_end, using_sam, pose_start_epoch=200, pose_end_epoch=1000,
                              pose_opt_interval=10, pose_opt_epoch=1, pose_correction_epoch=500, all_edge=False):
    pose_epoch = epoch % pose_opt_interval                                                           # :137
    is_pose_depth_opt = (has_sam_mask and epoch >= pose_start_epoch and pose_epoch < pose_opt_epoch
                         and epoch < pose_end_epoch and not depth_end)                               # :138
    is_delayed_pose_opt, cur_opt, freeze = False, None, False                                        # :139-141
    if using_sam:                                                                                    # :142
        is_delayed_pose_opt = epoch < pose_correction_epoch and not is_certain                       # :144
        if is_pose_depth_opt:                                                                        # :146-149
            cur_opt = "pose"
        elif is_delayed_pose_opt:                                                                    # :151-155
            cur_opt, freeze = "joint", True
        else:                                                                                        # :157-160
            cur_opt = "joint"
    return dict(cur_opt=cur_opt, freeze=freeze, edge=bool(is_delayed_pose_opt or all_edge), mesh=bool(is_pose_depth_opt))
