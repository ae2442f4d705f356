"""The error-bound sampler (VolSDF Algorithm 1; reference code/lib/model/ray_sampler.py:14-220).

  * RaySampler / UniformSampler / ErrorBoundSampler: the configuration objects with the reference's names and constructor
    arguments; ErrorBoundSampler.get_z_vals keeps the reference's public entry point for callers outside forward().
  * SamplerRun: the host driver of ONE person's sampler over the kernels of csrc/sampler.hip -- workspaces, the per-iteration
    launches, the network queries.
  * sample_persons: the iteration loop over the runs of every person of a call, with the data-parallel convergence vote.
    Multiply._sample_persons / _sample_person / sample_rays delegate here.

What a sampler leaves on the call context `cx` (the dict of Multiply._setup), and nothing else:
  * cx[POOL_KEY]: the ZeroPool of the samplers' device counters, ONE per context whoever samples on it and however often
    (sampler_pool; the eval path samples person by person on the same cx: one fill launch, not one per person);
  * cx['per'][p][RUN_KEY]: person p's closed SamplerRun.  It owns the workspaces the kernels were handed as raw addresses
    (MpSamplerState), so they live as long as the person's record does.  A run refers to neither cx nor the record: no cycle."""
import ctypes as C

import torch

from . import hip

POOL_KEY = "sampler_pool"
RUN_KEY = "sampler_run"


class RaySampler:
    def __init__(self, near, far):
        self.near = near
        self.far = far


class UniformSampler(RaySampler):
    def __init__(self, scene_bounding_sphere, near, N_samples, take_sphere_intersection=False, far=-1):
        super().__init__(near, 2.0 * scene_bounding_sphere if far == -1 else far)
        self.N_samples = N_samples
        self.scene_bounding_sphere = scene_bounding_sphere
        self.take_sphere_intersection = take_sphere_intersection


class ErrorBoundSampler(RaySampler):
    def __init__(self, scene_bounding_sphere, near, N_samples, N_samples_eval, N_samples_extra, eps, beta_iters,
                 max_total_iters, inverse_sphere_bg=False, N_samples_inverse_sphere=0, add_tiny=0.0):
        super().__init__(near, 2.0 * scene_bounding_sphere)
        self.N_samples = int(N_samples)
        self.N_samples_eval = int(N_samples_eval)
        self.N_samples_extra = int(N_samples_extra)
        self.eps = float(eps)
        self.beta_iters = int(beta_iters)
        self.max_total_iters = int(max_total_iters)
        self.scene_bounding_sphere = float(scene_bounding_sphere)
        self.add_tiny = float(add_tiny)
        self.inverse_sphere_bg = inverse_sphere_bg
        self.uniform_sampler = UniformSampler(scene_bounding_sphere, near, N_samples_eval,
                                              take_sphere_intersection=inverse_sphere_bg)
        # the reference overrides the configured count with 32 (ray_sampler.py:62-64)
        self.N_samples_inverse_sphere = 32
        if inverse_sphere_bg:
            self.inverse_sphere_sampler = UniformSampler(1.0, 0.0, 32, False, far=1.0)
        if not inverse_sphere_bg:
            raise NotImplementedError("the shipped configs always render with the inverted-sphere background")

    def get_z_vals(self, ray_dirs, cam_loc, model, cond, smpl_tfs, eval_mode, smpl_verts, person_id):
        """ray_sampler.py:66-220 for explicit rays: -> ((z_vals (R, N + N_extra + 2), z_vals_inverse_sphere (R, 32)),
        z_samples_eik (R, 1)) like the reference.  The depths come from the same device kernels Multiply.forward drives
        (Multiply.sample_rays).  `model.training` selects the reference's random branches (ray_sampler.py:32-40 stratified
        jitter, :171 random u of the final inverse-CDF draw, :202 randperm of the extra samples, and the jittered
        inverted-sphere depths); the draws are taken here with torch's generator on the rays' device, in the reference's order
        (multiply_amd.train.make_draws draws the same quantities for a whole training forward)."""
        dev = ray_dirs.device
        R = ray_dirs.reshape(-1, 3).shape[0]
        draws = None
        if model.training:
            NE, NS, NX = self.N_samples_eval, self.N_samples, self.N_samples_extra
            draws = dict(t_rand=torch.rand(R, NE, device=dev), u_final=torch.rand(R, NS, device=dev),
                         extra_idx=torch.stack([torch.randperm(NE * k, device=dev)[:NX] for k in range(1, self.max_total_iters + 1)]
                                               ).to(torch.int32).contiguous())
        z_vals = model.sample_rays(ray_dirs, cam_loc, cond, smpl_tfs, smpl_verts, person_id, draws=draws)
        idx = torch.randint(z_vals.shape[-1], (z_vals.shape[0],), device=z_vals.device)          # ray_sampler.py:212-213
        z_eik = torch.gather(z_vals, 1, idx.unsqueeze(-1))
        n_bg = self.inverse_sphere_sampler.N_samples
        t = torch.linspace(0.0, 1.0, steps=n_bg, device=z_vals.device)                            # near 0, far 1
        z_bg = t[None].expand(z_vals.shape[0], -1)
        if model.training:                                                                         # ray_sampler.py:32-40
            mids = 0.5 * (z_bg[..., 1:] + z_bg[..., :-1])
            upper, lower = torch.cat([mids, z_bg[..., -1:]], -1), torch.cat([z_bg[..., :1], mids], -1)
            z_bg = lower + (upper - lower) * torch.rand(z_bg.shape, device=z_vals.device)
        return (z_vals, z_bg * (1.0 / self.scene_bounding_sphere)), z_eik


def sampler_pool(cx):
    """the ZeroPool of the samplers' device counters of call context `cx` (created on first use: one fill for ALL persons)"""
    if POOL_KEY not in cx:
        cx[POOL_KEY] = hip.ZeroPool(cx["dev"], 1 << 16)
    return cx[POOL_KEY]


class SamplerRun:
    """ErrorBoundSampler.get_z_vals (ray_sampler.py:66-220) for ONE person of a call, in steps -- query(it), resample(it) for
    it = 0 .. max_total_iters-1, then close() -- so that the persons of a call can advance iteration by iteration together
    (one convergence-vote collective per iteration for ALL persons, sample_persons)."""

    __slots__ = ("p", "Rp", "NE", "R", "group", "n_groups", "train", "mode", "ph", "imp", "lins", "cfg", "state", "draws",
                 "dirs", "pose", "far", "beta", "hit_index", "count", "vsorted", "cbound", "btab", "cond", "pk_sdf", "fs",
                 "zs", "sdfs", "nz", "znew", "sdfnew", "betar", "active", "gflag", "zfinal", "iters", "any_active",
                 "xc_new", "work", "wcount", "bin_work")

    def __init__(self, cx, n, p, sampler, imp, mode, ph, draws, pool, lins=None):
        """workspaces of person p (the n-th of cx) + mp_sampler_init.  sampler: the ErrorBoundSampler; imp: the person's
        ImplicitNet; mode: the resolved arithmetic of the network queries (sdf); ph: phase-bracket factory (Multiply._ph);
        draws = None: eval-mode determinism, else the training randomness {t_rand [R_p,NE], u_final [R_p,N], extra_idx
        [max_iters,N_extra] int32}; pool: the counters' ZeroPool (sampler_pool(cx)); lins: this iteration's resolved layers of
        `imp` inside a training forward (TrainGraph.run), None: the run resolves the weights itself."""
        L, st = hip.lib(), hip.stream()
        dev = cx["dev"]
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        rs = sampler
        self.cfg = hip.MpSamplerCfg(rs.N_samples, rs.N_samples_eval, rs.N_samples_extra, rs.beta_iters, rs.max_total_iters,
                                    rs.eps, rs.add_tiny, rs.near)
        NE = self.NE = rs.N_samples_eval
        NZ = rs.N_samples + rs.N_samples_extra + 2
        ZM = NE * rs.max_total_iters
        R, group = cx["R"], cx["group"]
        self.p, self.R, self.group, self.n_groups = p, R, group, (R + group - 1) // group
        self.mode, self.ph, self.imp, self.lins, self.draws = mode, ph, imp, lins, draws
        self.dirs, self.pose, self.far, self.beta = cx["dirs"], cx["pose"], cx["far"], cx["beta"]
        pp = cx["per"][p]
        self.hit_index, self.count, self.cond = pp["hit_index"], pp["count"], pp["cond"]
        self.vsorted, self.cbound, self.btab = pp["vsorted"], pp["cbound"], pp["btab"]
        Rp = self.Rp = max(int(cx["n_hit"][n]), 1)
        self.pk_sdf = hip.packed(imp, "sdf", 2)
        self.pk_sdf.refresh(self.cond, force=imp.training)      # (a sub-module of the model: the model's mode)
        self.fs = None                                          # mode 'bf16x3': the fused kernel's weights, at the first query
        self.zs = torch.empty(Rp, ZM, **f32); self.sdfs = torch.empty(Rp, ZM, **f32)
        self.nz = torch.empty(Rp, **i32); self.znew = torch.empty(Rp, NE, **f32); self.sdfnew = torch.empty(Rp, NE, **f32)
        self.betar = torch.empty(Rp, **f32); self.active = torch.empty(Rp, **i32)
        self.gflag = torch.empty((rs.max_total_iters + 1) * self.n_groups, **i32)
        self.zfinal = torch.empty(Rp, NZ, **f32); self.iters = pool.take(self.n_groups, dtype=torch.int32)
        self.any_active = pool.take(rs.max_total_iters + 1, dtype=torch.int32)
        self.state = hip.MpSamplerState(self.zs.data_ptr(), self.sdfs.data_ptr(), self.nz.data_ptr(), self.znew.data_ptr(),
                                        self.sdfnew.data_ptr(), self.betar.data_ptr(), self.active.data_ptr(),
                                        self.gflag.data_ptr(), self.zfinal.data_ptr(), self.iters.data_ptr(),
                                        self.any_active.data_ptr())
        self.train = draws is not None
        t_rand = draws["t_rand"] if self.train else None
        L.mp_sampler_init(C.byref(self.cfg), C.byref(self.state), self.far, self.hit_index, self.count, Rp, group, R, t_rand, st)
        self.xc_new = torch.empty(Rp * NE, 3, **f32)
        self.work = torch.empty(Rp * NE, **i32)
        self.wcount = pool.take(rs.max_total_iters + 1, dtype=torch.int32)
        # training: the rays are random pixels -- the warp first groups a call's samples by their nearest vertex cluster
        self.bin_work = torch.empty(int(L.mp_warp_bin_work_bytes(Rp * NE)), dtype=torch.uint8, device=dev) if self.train else None

    def query(self, it):
        """iteration `it`, first half: warp the new samples, query the SDF net, evaluate the error bound (sets the group flags)"""
        L, st = hip.lib(), hip.stream()
        with self.ph("sampler_warp"):
            L.mp_warp_inverse(None, self.dirs, self.pose, self.hit_index, self.count, self.znew, self.NE, self.NE, self.Rp,
                              self.vsorted, self.cbound, self.btab, 0 if self.train else 1, self.active,
                              self.any_active[it:it + 1], self.xc_new, None, self.sdfnew, self.work, self.wcount[it:it + 1],
                              self.bin_work, st)
        with self.ph("sampler_mlp_sdf"):
            self.sdf(it)
        with self.ph("sampler_bound"):
            L.mp_sampler_bound(C.byref(self.cfg), C.byref(self.state), self.beta, self.hit_index, self.count, self.Rp,
                               self.group, self.R, it, st)

    def sdf(self, it):
        """the sampler's network queries of iteration `it` (`model.sampler_sdf_mode`, MP_SAMPLER_SDF):
        'bf16x3' (what 'auto' resolves to for the shipped network shape): the value sweep of the training path's layer-fused
        kernel (mp_tf_sdf_val: split-bfloat16 products, fp32 activations, ~2^-16 per product) -- near-fp32 queries, 3x the time
        of the half-precision kernel; 'f16x2': split activations on the half-precision weights (mp_mlp_sdf_x2, 2x the time, a
        quarter of the mean depth error, any network shape); 'f16': the fused half-precision kernel (csrc/mlp.hip k_mlp_sdf);
        'bf16x3-layerwise': the bf16x3 arithmetic layer by layer (the independent implementation tools/sampler_precision.py
        first measured with; reads the worklist count on the host)."""
        L, st = hip.lib(), hip.stream()
        pk_sdf, wcount, mode, n_max = self.pk_sdf, self.wcount, self.mode, self.Rp * self.NE
        if mode == "bf16x3":
            # the value sweep of the training path's layer-fused kernel (csrc/tfuse.hip k_tf_sdf_val): same worklist, device-side count
            if self.fs is None:      # once per call and person: on the layers handed in, else the state resolves the weights itself
                from . import train as T
                if not T.fused_sdf_supported(self.imp):
                    raise NotImplementedError("sampler_sdf_mode 'bf16x3' needs the network shape csrc/tfuse.hip is specialised for")
                self.fs = T.fused_sdf_state(self.imp, self.lins).refresh(self.cond)
            L.mp_tf_sdf_val(self.fs.wpack, self.fs.bias_all, self.xc_new, self.work, wcount[it:it + 1], n_max, self.sdfnew, st)
            return
        if mode == "bf16x3-layerwise":          # the measurement path of tools/sampler_precision.py (host read per iteration)
            from . import train as T
            n = int(wcount[it])
            if n > 0:
                idx = self.work[:n].long()
                x = self.xc_new[idx].contiguous()
                lins = [T.LinW(l) for l in self.imp.layers()]
                parts = [T.ImplicitTrain(self.imp, x[c0:c0 + (1 << 18)], self.cond, fwd=False, lins=lins).out[:, 0].clone()
                         for c0 in range(0, n, 1 << 18)]
                self.sdfnew.view(-1)[idx] = torch.cat(parts)
            return
        if mode not in ("f16", "f16x2"):
            raise ValueError(f"sampler_sdf_mode {mode!r}: expected 'f16x2', 'f16', 'bf16x3' or 'bf16x3-layerwise'")
        # 'f16x2': split activations on the same packed half-precision weights (csrc/mlp.hip k_mlp_sdf_x2)
        fn = L.mp_mlp_sdf_x2 if mode == "f16x2" else L.mp_mlp_sdf
        fn(C.byref(pk_sdf.net), pk_sdf.wpack, pk_sdf.bias, self.xc_new, self.work, wcount[it:it + 1], n_max, self.sdfnew, st)

    def resample(self, it):
        """iteration `it`, second half: new samples where the bound is not met (or, converged, the final inverse-CDF draw)"""
        u_final = self.draws["u_final"] if self.train else None
        extra_idx = self.draws["extra_idx"] if self.train else None
        with self.ph("sampler_resample"):
            hip.lib().mp_sampler_resample(C.byref(self.cfg), C.byref(self.state), self.beta, self.far, self.hit_index,
                                          self.count, self.Rp, self.group, self.R, it, u_final, extra_idx, hip.stream())

    def close(self):
        """-> (zfinal [R_p][N+N_extra+2], the iteration counters, the per-iteration SDF worklist counts).  The run keeps every
        workspace a kernel in flight may still address; the warp's binning scratch is done with and released."""
        self.bin_work = None
        return self.zfinal, self.iters, self.wcount


def _vote_groups_check(n_groups, grp, dev):
    """Every rank of the vote's process group must contribute the same number of convergence-group flags (uneven ray shards
    with convergence_group set would mismatch the collective's sizes -- undefined behaviour on RCCL).  A FIXED-size collective,
    issued by every rank on every call in which the flag count is not 1 by construction (convergence_group set), whatever
    its own n_groups: a rank that skipped it would desynchronise the collective sequence it is meant to protect."""
    import torch.distributed as dist
    t = torch.tensor([n_groups, -n_groups], device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=grp)
    hi, lo = int(t[0]), int(-t[1])
    if hi != n_groups or lo != n_groups:
        raise RuntimeError(f"sampler vote: the ranks hold different numbers of convergence groups (this rank {n_groups}, "
                           f"range {lo}..{hi}); shard the rays at multiples of convergence_group, equally many per rank")


def sample_persons(model, cx, draws_by_person=None, persons=None, shared_lins=None):
    """The sampler of EVERY person of the call, advancing iteration by iteration together -> {p: (zfinal, iters, wcount)}.
    The persons' samplers are independent (same launches as one after the other, other order); what the interleaving buys
    is the data-parallel convergence vote: the reference's `not_converge = beta.max() > beta0` (ray_sampler.py:137) spans
    ALL rays of the call -- here the rays of every rank -- and with `model.sampler_vote_group` set ONE MAX all-reduce per
    sampler iteration carries the flags of all persons (P x n_groups ints; P x max_total_iters collectives before), between the
    bound and the resampling kernels: the N-rank step samples exactly like the single-process step.
    shared_lins = {p: resolved layers of p's ImplicitNet}: a training forward's weights of this iteration (TrainGraph.run)."""
    persons = list(cx["persons"]) if persons is None else list(persons)
    order = {p: n for n, p in enumerate(cx["persons"])}
    pool = sampler_pool(cx)
    runs = [SamplerRun(cx, order[p], p, model.ray_sampler, model.foreground_implicit_network_list[p],
                       model.resolved_sampler_sdf_mode(p), model._ph, None if draws_by_person is None else draws_by_person[p],
                       pool, None if shared_lins is None else shared_lins[p]) for p in persons]
    vote = model.sampler_vote_group is not None
    if vote and runs:
        import torch.distributed as dist
        grp = None if model.sampler_vote_group is True else model.sampler_vote_group
        ng = runs[0].n_groups
        if model.convergence_group is not None:      # (None: one flag per person and call on every rank, by construction)
            _vote_groups_check(ng, grp, cx["dev"])
    for it in range(model.ray_sampler.max_total_iters):
        for run in runs:
            run.query(it)
        if vote and runs:
            flags = [run.gflag[it * ng:(it + 1) * ng] for run in runs]
            if len(flags) == 1:
                dist.all_reduce(flags[0], op=dist.ReduceOp.MAX, group=grp)
            else:
                packed = torch.cat(flags)
                dist.all_reduce(packed, op=dist.ReduceOp.MAX, group=grp)
                torch._foreach_copy_(flags, list(packed.split(ng)))
            model.vote_collectives = getattr(model, "vote_collectives", 0) + 1
        for run in runs:
            run.resample(it)
    out = {}
    for run in runs:
        out[run.p] = run.close()
        cx["per"][run.p][RUN_KEY] = run      # keeps the workspaces alive with the person's record (see the module docstring)
    return out
