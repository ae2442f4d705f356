"""Multiply scene model: the reference's nn.Module API over the HIP hot path.

Drop-in for `lib.model.multiply.Multiply` (reference code/lib/model/multiply.py:23-598):
  * constructor Multiply(opt, betas_path) building the same sub-module tree, in the same order and with the same
    state-dict names (multiply.py:35-100) -- including the SMPL tables under smpl_server_list.N.smpl.* and
    deformer_list.N.smpl.smpl.* -- so the reference's checkpoints load with strict=True (tests/test_state_dict_gpu.py) and
    seeded initialisation is bit-identical;
  * forward(input, id=-1, cond_zero_shit=False, canonical_pose=False) -> the reference's output dict
    (multiply.py:566-597);
  * the attributes the Lightning module reaches into.
Everything between the input dict and the output dict runs in hand-written HIP kernels (multiply_amd/csrc) through
the C ABI of include/multiply_hip.h.  There is no PyTorch / CPU fallback: without the library or a gfx950 device the
forward raises.

Extensions that do not exist in the reference (all optional, defaults reproduce the reference):
  * input['hit_index'] : list of per-person ascending ray-id tensors replacing the box cull (parity tests; the
    reference's trimesh box, multiply.py:208-214, 256-266, is third-party code);
  * self.convergence_group : number of consecutive rays that share the sampler's convergence vote
    (ray_sampler.py:137).  None = the whole call, exactly like the reference; set it to pixel_per_batch to render a
    whole frame in one call with the results of the reference's chunked loop (multiply_model.py:1051-1055);
  * self.render_geometry / self.geometry_level : eval mode only, the output dict also carries the volume-rendered depth maps
    (depth_values, depth_person_list, depth_level_values, front_person, acc_person_solo_list, depth_person_solo_list,
    depth_person_solo_level_list: _composite_geometry).  Off by default: exactly the reference's keys;
  * self.train_geometry : training mode only, the same seven keys on the training forward's rays, differentiable except
    depth_level_values / front_person (train.TrainGraph, mp_tr_composite_geometry_bwd).  Off by default;
  * self.train_interpenetration / self.interpenetration_points : training mode only, the dict's 'interpenetration_loss' (a
    dead zeros(1) slot in the reference, multiply.py:237,581) carries the mesh-free interpenetration term on the persons' SDF
    fields (train.Interpenetration, csrc/penetration.hip).  Off by default.
"""
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from . import hip
from .density import AbsDensity, LaplaceDensity
from .networks import ImplicitNet, RenderingNet
from .ray_sampler import ErrorBoundSampler, sample_persons
from .smpl import NUM_JOINTS, NUM_VERTS, SMPLDeviceTables, SMPLServer, knn_cluster_perm, load_smpl_tables
from .deformer import SMPLDeformer
from .sampler import PointInSpace


class Multiply(nn.Module):
    # eval mode only: the output dict also carries the volume-rendered depth maps (_composite_geometry); geometry_level is the
    # opacity in (0,1) at which depth_level_values / front_person / depth_person_solo_level_list are read off the ray
    render_geometry = False
    geometry_level = 0.5
    # training mode only: forward_train's dict carries the same seven keys for the iteration's rays, on the training node: the sums
    # and the per-person solo level depth are differentiable (sdf weights, density.beta, and the body inputs through the pose path);
    # depth_level_values / front_person are not.  geometry_level is shared.  Not built for person-sharded training.
    train_geometry = False
    # training mode only: forward_train's 'interpenetration_loss' carries the mesh-free interpenetration term of the call's persons
    # (train.Interpenetration: posed SMPL vertices of p probed against q's SDF field), raw, differentiable w.r.t. the body inputs
    # only; interpenetration_points vertices per person are drawn (the reference's num_pixels).  Off: zeros(1), no launch, no draw.
    # Not built for person-sharded training.
    train_interpenetration = False
    interpenetration_points = 5120

    def __init__(self, opt, betas_path, smpl_tables=None, gender_list=None):
        super().__init__()
        hip.require_device()
        betas = np.load(betas_path) if isinstance(betas_path, str) else np.asarray(betas_path)
        self.using_nerfacc = True
        self.smpl_surface_weight = opt.loss.get("smpl_surface_weight", 0)
        self.zero_pose_weight = opt.loss.get("zero_pose_weight", 0)
        self.smpl_vertex_part = None
        # opt-in: the smpl_surface term back-propagates into smpl_pose / smpl_trans / smpl_shape when they are optimised (the
        # posed vertices' adjoint, train.TrainGraph._regularisers_*); off, that combination still raises
        self.smpl_surface_pose_grad = os.environ.get("MP_SMPL_SURFACE_POSE_GRAD", "0") == "1"
        if self.smpl_surface_weight > 0:      # multiply.py:112-113 (the reference's asset ./outputs/smpl_vert_segmentation.json)
            import json
            seg = os.path.abspath(opt.get("smpl_vert_segmentation_path", "./outputs/smpl_vert_segmentation.json"))
            if os.path.exists(seg):
                with open(seg) as f:
                    self.smpl_vertex_part = json.load(f)
            # (absent: train.surface_sampling_weights raises at the first training forward unless model.smpl_vertex_part is assigned)
        self.use_person_encoder = opt.get("use_person_encoder", False)
        if self.use_person_encoder:
            raise NotImplementedError("use_person_encoder (shared triplane networks) is outside the hot-path scope")
        betas2 = betas.reshape(-1, 10) if betas.ndim == 2 else betas.reshape(1, 10)
        self.num_person = betas2.shape[0]

        # same construction order as the reference (multiply.py:35-66): RNG consumption is identical
        self.foreground_implicit_network_list = nn.ModuleList()
        self.foreground_rendering_network_list = nn.ModuleList()
        for _ in range(self.num_person):
            self.foreground_implicit_network_list.append(ImplicitNet(opt.implicit_network))
            self.foreground_rendering_network_list.append(RenderingNet(opt.rendering_network))
        self.with_bkgd = opt.with_bkgd
        self.bg_implicit_network = ImplicitNet(opt.bg_implicit_network)
        self.bg_rendering_network = RenderingNet(opt.bg_rendering_network)
        self.frame_latent_encoder = nn.Embedding(opt.num_training_frames, opt.dim_frame_encoding)
        self.sampler = PointInSpace()
        self.use_smpl_deformer = opt.use_smpl_deformer
        if not self.use_smpl_deformer:
            raise NotImplementedError("only the SMPL deformer branch exists in the reference's shipped configs")

        if gender_list is None:
            # multiply.py:71: gender.npy next to mean_shape.npy.  Without it the reference fails; a silent default would
            # pick the wrong body model -- only the explicit synthetic-table route (tests, benchmarks) has no genders.
            gpath = betas_path[:-14] + "gender.npy" if isinstance(betas_path, str) else None
            if gpath and os.path.exists(gpath):
                gender_list = np.load(gpath)
            elif smpl_tables is not None:
                gender_list = ["male"] * self.num_person
            else:
                raise FileNotFoundError(f"gender.npy not found ({gpath}); pass gender_list=[...] explicitly")
        self.gender_list = gender_list
        device = torch.device("cuda")
        cache = {}

        def tables_for(gender):
            g = str(gender)
            if g not in cache:
                raw = smpl_tables if smpl_tables is not None else load_smpl_tables(g)
                cache[g] = raw if isinstance(raw, SMPLDeviceTables) else SMPLDeviceTables(raw, device)
            return cache[g]

        self.deformer_list = nn.ModuleList()
        self.smpl_server_list = nn.ModuleList()
        for i in range(self.num_person):
            server = SMPLServer(gender=self.gender_list[i], betas=betas2[i], smpl_tables=tables_for(self.gender_list[i]))
            self.smpl_server_list.append(server)
            self.deformer_list.append(SMPLDeformer(betas=betas2[i], gender=self.gender_list[i], server=server))

        self.sdf_bounding_sphere = 3.0
        self.threshold = 0.05
        self.shade_mode = hip.SHADE_MODE      # 'reverse' | 'forward' (csrc/mlp.hip: k_mlp_shade_rev | k_mlp_shade)
        # the SDF networks' feature rows folded into the colour networks' first layer (hip.FoldedColor): reverse-mode shading and the
        # background; False = the unfolded entry points (the cross-check; forward-mode shading is always unfolded)
        self.feature_fold = True
        # in / off-surface flags (training, epochs < 250): 'auto' | 'index' | 'brute' -- the face index (csrc/mesh_index.hip) or brute
        # force (csrc/mesh.hip), same values; 'auto' = the index for a closed surface of hip.MESH_INDEX_MIN_FACES faces or more, where it
        # was measured to win (hip.mesh_index_wanted); MP_MESH_INDEX=0: brute; fit_smpl_init(model, ...) follows it too
        self.mesh_index_mode = hip.MESH_INDEX_MODE
        self.mesh_index_cache = hip.MeshIndexCache()       # one index per person, rebuilt when mesh_face_vertices_list[p] changes
        self.density = LaplaceDensity(**opt.density)
        self.bg_density = AbsDensity()
        self.ray_sampler = ErrorBoundSampler(self.sdf_bounding_sphere, inverse_sphere_bg=True, **opt.ray_sampler)
        if opt.get("smpl_init", False):      # multiply.py:101-108
            path = os.path.abspath(opt.get("smpl_init_path", "./outputs/smpl_init_male_256.pth"))
            if not os.path.exists(path):
                raise FileNotFoundError(f"smpl_init is set but {path} (an asset of the reference, not shipped here) is missing; "
                                        f"set smpl_init: false to start from the geometric initialisation instead")
            state = torch.load(path, map_location=device)
            for net in self.foreground_implicit_network_list:
                net.load_state_dict(state["model_state_dict"], strict=False)
        self.mesh_v_cano_list = [s.verts_c for s in self.smpl_server_list]
        self.mesh_f_cano_list = [torch.tensor(s.smpl.faces.astype(np.int64), device=device) for s in self.smpl_server_list]
        self.mesh_face_vertices_list = [v[0][f] [None] for v, f in zip(self.mesh_v_cano_list, self.mesh_f_cano_list)]
        self.convergence_group = None
        self.obb_inflate = 1.2
        # cull box (multiply.py:208-214): "hull" = the minimum-volume box trimesh's bounding_box_oriented computes, by the published
        # algorithm (multiply_amd/obb.py: Qhull on the host, one extra device sync + ~3 ms per person and call; the candidate search
        # on the device, mp_obb_hull); "pca" = principal-axes box, device only (k_obb; conservative: identical eval pixels).
        # "auto" (default): the reference's box wherever the hit set changes the result -- TRAINING mode, where no outlier override
        # exists (multiply.py:142-143 is eval-only) and the rays a person is sampled on enter the loss -- and the device-only box
        # in eval mode, where both give the same pixels (test_forward_eval_box_cull_is_conservative).
        self.obb_mode = os.environ.get("MP_OBB_MODE", "auto")
        # eval-mode refinement of the box cull that provably leaves every pixel unchanged (mp_ray_cull_near); 0 = box only
        self.near_cull = os.environ.get("MP_NEAR_CULL", "1") != "0"
        # ray-sharded data-parallel training: a torch.distributed process group (or True = the default group) over which the
        # sampler's per-iteration convergence vote is all-reduced (MAX) -- see ray_sampler.sample_persons; None: the vote is per process
        self.sampler_vote_group = None
        # arithmetic of the sampler's network queries (ray_sampler.SamplerRun.sdf): 'auto' (default, round 6) = 'bf16x3' -- near-fp32: the depths
        # then agree with the fp32 reference to 1e-3 instead of 2e-2 and the grazing-ray tail of the render disappears -- for the
        # network shape csrc/tfuse.hip is specialised for (the shipped configs), 'f16x2' (split activations, any shape) otherwise;
        # 'f16': the fused half-precision kernel (the round 1-5 default), a third of the query time
        self.sampler_sdf_mode = os.environ.get("MP_SAMPLER_SDF", "auto")
        self.last_stats = {}
        self.profile = False
        self.phase_events = {}
        self.to(device)

    # ------------------------------------------------------------------ helpers
    class _Phase:
        """HIP-event bracket around a group of launches on the current stream (enabled by `model.profile = True`)."""

        def __init__(self, owner, name):
            self.o, self.name = owner, name

        def __enter__(self):
            if self.o.profile:
                self.e0 = torch.cuda.Event(enable_timing=True)
                self.e1 = torch.cuda.Event(enable_timing=True)
                self.e0.record()

        def __exit__(self, *a):
            if self.o.profile:
                self.e1.record()
                self.o.phase_events.setdefault(self.name, []).append((self.e0, self.e1))

    def _ph(self, name):
        return Multiply._Phase(self, name)

    def phase_times_ms(self):
        """{phase: (n_brackets, total ms)} of the events recorded since the last reset (synchronises)."""
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in self.phase_events.items()}

    @property
    def mesh_index_mode(self):
        return self._mesh_index_mode

    @mesh_index_mode.setter
    def mesh_index_mode(self, mode):
        self._mesh_index_mode = hip.mesh_index_mode(mode)

    def train(self, mode=True):
        """nn.Module.train, and every switch of mode drops the packed-weight caches (hip.invalidate_packed: an optimizer may have
        updated the parameters without bumping their version counters -- torch's fused Adam does)"""
        if bool(mode) != self.training:
            hip.invalidate_packed()
        return super().train(mode)

    def _obb_mode_now(self):
        if self.obb_mode not in ("auto", "hull", "pca"):
            raise ValueError(f"obb_mode {self.obb_mode!r}: expected 'auto', 'hull' or 'pca'")
        return ("hull" if self.training else "pca") if self.obb_mode == "auto" else self.obb_mode

    def forward(self, input, id=-1, cond_zero_shit=False, canonical_pose=False):
        if self.training:
            from . import train
            return train.forward_train(self, input, id, cond_zero_shit, canonical_pose)
        with torch.no_grad():
            return self._forward_eval(input, id, canonical_pose)

    def _beta_value(self):
        """the density's beta as the kernels read it (abs + beta_min, multiply.py's density call), on the current stream"""
        return (self.density.beta.detach().abs() + self.density.beta_min).reshape(1).float().contiguous()

    def _setup(self, input, id, canonical_pose, side_stream=False, host_hull=False):
        """Rays, SMPL posing, nearest-vertex structures and the box cull for every person of the call
        (multiply.py:177-266).  Ends with the one host sync of the call (hit counts size the workspaces).
        side_stream: run it on a stream of its own (_setup_side_stream); host_hull: the convex hulls on the host."""
        if side_stream:
            return self._setup_side_stream(input, id, canonical_pose, host_hull)
        return self._setup_body(input, id, canonical_pose, self._beta_value(), host_hull)

    def _setup_side_stream(self, input, id, canonical_pose, host_hull):
        """The setup kernels read only the call's inputs, so they run on a stream of their own and the host waits
        for THAT stream only: it does not wait for the previous iteration's backward pass (or the previous frame) still
        running on the caller's stream, and keeps enqueueing.  The inputs must be resident and complete (produced by work
        the host has already waited for, e.g. a data loader's copies); everything allocated here is handed to the caller's
        stream (record_stream + an event wait).  What is NOT an input of the call stays on the caller's stream:
          * `density.beta` is a trained parameter -- the previous iteration's optimizer step may still be updating it on
            the caller's stream.  Training: the setup kernels do not read it (the near cull is eval-only) and the call's
            `beta` is computed on the caller's stream behind the join.  Eval: the near cull does read it, so the value is
            computed on the caller's stream once per parameter version and the side stream waits for that event;
          * body-model inputs that are being optimised (requires_grad / produced by BodyModelParams in this iteration on
            the caller's stream): the side stream is refused, the setup runs in order."""
        if any(torch.is_tensor(input.get(k)) and (input[k].requires_grad or input[k].grad_fn is not None)
               for k in ("smpl_params", "smpl_pose", "smpl_shape", "smpl_trans")):
            return self._setup_body(input, id, canonical_pose, self._beta_value(), host_hull)
        main = torch.cuda.current_stream()
        side = self.__dict__.get("_setup_stream")
        if side is None:
            side = self.__dict__["_setup_stream"] = torch.cuda.Stream()
        beta = None               # training: no setup kernel reads it
        if not self.training:
            b = self.density.beta
            cache = self.__dict__.get("_eval_beta")
            # keyed on the parameter's storage and its version: writes through .data and a replaced Parameter with the
            # same version number must not leave a stale value behind (a load_state_dict bumps the version: copy_ in place)
            key = (b.data_ptr(), b._version, str(b.device), hip._GENERATION[0])
            if cache is None or cache[0] != key:
                val = self._beta_value()                                                                 # caller's stream
                ev = torch.cuda.Event()
                ev.record(main)
                side.wait_event(ev)          # once per parameter version: later side-stream work is ordered behind it
                val.record_stream(side)
                cache = self.__dict__["_eval_beta"] = (key, val)
            beta = cache[1]
        with torch.cuda.stream(side):
            cx = self._setup_body(input, id, canonical_pose, beta, host_hull)

        def hand_over(o):
            if torch.is_tensor(o):
                if o.is_cuda:
                    o.record_stream(main)
            elif isinstance(o, dict):
                for v in o.values():
                    hand_over(v)
            elif isinstance(o, (list, tuple)):
                for v in o:
                    hand_over(v)
        hand_over(cx)
        main.wait_stream(side)
        if beta is None:          # training: the parameter as the caller's stream sees it (behind the last optimizer step)
            cx["beta"] = self._beta_value()
        return cx

    def _setup_body(self, input, id, canonical_pose, beta, host_hull=False):
        """One run of the setup on the current stream -> cx.  beta: the density's beta [1], or None where the caller fills
        cx['beta'] in afterwards (side-stream training setup: no setup kernel reads it)."""
        assert beta is not None or self.training, "a deferred beta is only valid where the near cull (eval) does not run"
        L, st = hip.lib(), hip.stream()
        dev = self.density.beta.device
        f32 = dict(dtype=torch.float32, device=dev)
        uv = input["uv"].to(dev).float().reshape(-1, 2).contiguous()
        R = uv.shape[0]
        K = input["intrinsics"].to(dev).float().reshape(16).contiguous()
        pose = input["pose"].to(dev).float().reshape(16).contiguous()
        smpl = {k: input["smpl_" + k].detach().to(dev).float() for k in ("params", "pose", "shape", "trans")}
        P = smpl["trans"].shape[1]
        persons = list(id) if isinstance(id, (list, tuple)) else (list(range(P)) if id == -1 else [id])
        group = int(self.convergence_group or R)

        # rays (rend_util.get_camera_params)
        dirs = torch.empty(R, 3, **f32)
        far = torch.empty(R, **f32)
        L.mp_ray_setup(uv, K, pose, R, self.sdf_bounding_sphere, dirs, far, st)

        # SMPL posing, nearest-vertex structures, box cull  (multiply.py:196-214, 256-266)
        zp = hip.ZeroPool(dev, 1 << 16)             # the setup's device counters: one fill (on the setup's stream)
        counts = zp.take(len(persons), dtype=torch.int32)
        scan_tmp = torch.empty(R + (R + 1023) // 1024 + 8, dtype=torch.int32, device=dev)
        verts_all = torch.empty(len(persons), NUM_VERTS, 3, **f32)
        per = {p: self._setup_pose(p, smpl, canonical_pose, verts_all[n], counts[n:n + 1], R) for n, p in enumerate(persons)}
        given_hits = input.get("hit_index") is not None
        device_hull = not given_hits and self._obb_mode_now() == "hull" and not host_hull
        obb_all, hull_status = self._setup_device_hull(verts_all, zp) if device_hull else (None, None)
        for n, p in enumerate(persons):
            q = per[p]
            if given_hits:
                hi = input["hit_index"][p].to(dev).to(torch.int32).contiguous()
                if hi.numel() == 0:      # multiply.py:262-263: no ray meets the box -> ray 0
                    hi = torch.zeros(1, dtype=torch.int32, device=dev)
                q["hit_index"][:hi.numel()] = hi
                L.mp_ray_hits_from_index(q["hit_index"], hi.numel(), R, q["count"], q["inv_index"], st)
                continue
            obb = q["obb"] = obb_all[n] if device_hull else self._setup_box(q["verts"])
            if self.near_cull and not self.training:
                # eval: rays of the box that never come within the outlier radius of the body are background, bit for bit
                # (csrc/rays.hip k_ray_near_body); they are dropped before the sampler
                L.mp_ray_cull_near(dirs, pose, obb, q["cbound"], far, beta, self.ray_sampler.near, R, group, q["hit_index"],
                                   q["count"], q["inv_index"], scan_tmp, st)
            else:
                L.mp_ray_cull(dirs, pose, obb, R, group, q["hit_index"], q["count"], q["inv_index"], scan_tmp, st)

        # the one host sync of the call: sizes the per-person workspaces (+ the hulls' status)
        if hull_status is None:
            n_hit = counts.tolist()
        else:
            both = torch.cat([counts, hull_status[:, 3]]).tolist()
            n_hit = both[:len(persons)]
            if any(both[len(persons):]):
                import warnings
                # counted (advisor, round 5): a regression of the device wrap -- e.g. its grid barrier giving up under GPU sharing --
                # shows as a growing `hull_host_fallbacks` in `last_stats` / the bench line, not only as a warning
                self.hull_host_fallbacks = getattr(self, "hull_host_fallbacks", 0) + 1
                warnings.warn("device convex hull failed (degenerate vertex configuration): falling back to the host-side hull")
                return self._setup_body(input, id, canonical_pose, beta, host_hull=True)
        return dict(dev=dev, R=R, uv=uv, K=K, pose=pose, dirs=dirs, far=far, per=per, persons=persons, n_hit=n_hit,
                    group=group, beta=beta, counts=counts, hull_status=hull_status)

    def _setup_pose(self, p, smpl, canonical_pose, verts, count, R):
        """person p's record: the posed body (into `verts`), its nearest-vertex tables and the ray-index workspaces"""
        dev = verts.device
        server = self.smpl_server_list[p]
        prm = torch.cat([smpl["params"][0, p, 0:1], smpl["trans"][0, p], smpl["pose"][0, p], smpl["shape"][0, p]]).contiguous()
        if canonical_pose:   # multiply.py:197-202
            prm = prm.clone()
            prm[1:4] = 0
            prm[4:76] = 0
            prm[4 + 5] = np.pi / 6
            prm[4 + 8] = -np.pi / 6
        tfs = torch.empty(NUM_JOINTS, 4, 4, dtype=torch.float32, device=dev)
        jnts = torch.empty(NUM_JOINTS, 3, dtype=torch.float32, device=dev)
        server.pose_into(prm, verts, tfs, jnts)
        vsorted, cbound = hip.knn_tables(verts, self.deformer_list[p].knn_perm)
        btab = hip.blend_table(server.tables.lbs_weights, tfs)        # per-vertex inverse blended transform of this pose
        hit_index = torch.empty(R, dtype=torch.int32, device=dev)
        inv_index = torch.empty(R, dtype=torch.int32, device=dev)
        cond = (smpl["pose"][0, p, 3:] / np.pi).contiguous()          # multiply.py:270
        return dict(verts=verts, tfs=tfs, btab=btab, vsorted=vsorted, cbound=cbound, hit_index=hit_index, obb=None,
                    inv_index=inv_index, count=count, cond=cond, prm=prm,
                    rest_joints=server.rest_joints() if self.training else None)

    def _setup_device_hull(self, verts_all, zp):
        """the convex hulls (gift wrapping), the candidate searches and the boxes of ALL bodies in one batch on the device: no
        host round trip; the status words are read with the hit counts (a failure -- exactly coplanar vertices tying into a
        non-manifold patch -- repeats the setup with the host-side hull) -> (boxes [P][16], status [P][8])"""
        L, dev, n = hip.lib(), verts_all.device, verts_all.shape[0]
        hull_status = zp.take(n, 8, dtype=torch.int32)
        work = torch.empty(n, int(L.mp_obb_hull_device_work_bytes()), dtype=torch.uint8, device=dev)
        obb_all = torch.empty(n, 16, dtype=torch.float32, device=dev)
        L.mp_obb_hull_device(verts_all, NUM_VERTS, n, self.obb_inflate, work, obb_all, hull_status, hip.stream())
        return obb_all, hull_status

    def _setup_box(self, verts):
        """one body's cull box [16] without the batched device hull: the hull on the host, or the principal-axes box"""
        L, st, dev = hip.lib(), hip.stream(), verts.device
        obb = torch.empty(16, dtype=torch.float32, device=dev)
        if self._obb_mode_now() != "hull":
            L.mp_obb(verts, self.obb_inflate, obb, st)
            return obb
        # hull on the host (Qhull, ~3 ms; one extra device sync), search + box on the device
        from .obb import hull_search_inputs, obb_record
        vhost = verts.cpu().numpy()
        buf, nh, nn_, ne = hull_search_inputs(vhost)
        if nh > 4096:      # beyond the kernel's LDS tile (a body's hull has a few hundred vertices): the host statement
            return torch.from_numpy(obb_record(vhost, self.obb_inflate)).to(dev)
        hb = torch.from_numpy(buf).to(dev)
        o_n, o_e = 3 * nh, 3 * (nh + nn_)
        work = torch.empty(2 * nn_, dtype=torch.float64, device=dev)
        L.mp_obb_hull(hb, nh, hb[o_n:], nn_, hb[o_e:], hb[o_e + 3 * ne:], hb[o_e + 6 * ne:], ne, self.obb_inflate, work, obb, st)
        return obb

    # ---- the error-bound sampler: the driver lives in ray_sampler.py (SamplerRun, sample_persons); these delegate
    def resolved_sampler_sdf_mode(self, p=0):
        """`sampler_sdf_mode` with 'auto' resolved for person p's network (see __init__)"""
        mode = getattr(self, "sampler_sdf_mode", "auto")
        if mode != "auto":
            return mode
        from . import train as T
        return "bf16x3" if T.fused_sdf_supported(self.foreground_implicit_network_list[p]) else "f16x2"

    def _sample_persons(self, cx, draws_by_person=None, persons=None, shared_lins=None):
        """The sampler of every person of the call, advancing together -> {p: (zfinal, iters, wcount)} (ray_sampler.sample_persons)"""
        return sample_persons(self, cx, draws_by_person, persons, shared_lins)

    def _sample_person(self, cx, n, p, draws=None):
        """ErrorBoundSampler.get_z_vals for person p's rays (ray_sampler.py:66-220): returns zfinal [R_p][N+N_extra+2],
        the iteration counters and the per-iteration SDF worklist counts."""
        return self._sample_persons(cx, None if draws is None else {p: draws}, persons=[p])[p]

    def sample_rays(self, ray_dirs, cam_loc, cond, smpl_tfs, smpl_verts, person_id, draws=None):
        """The sampler on explicit rays, outside forward(): what ErrorBoundSampler.get_z_vals(ray_dirs, cam_loc, model, cond,
        smpl_tfs, eval_mode, smpl_verts, person_id) does in the reference (ray_sampler.py:66-220) for ONE person (draws = None: eval mode):
        every ray is sampled (no box cull), the convergence vote spans the call.  ray_dirs (R,3) unit vectors, cam_loc (3,)
        or (R,3) with equal rows, cond the pose conditioning (69,) / {'smpl': (1,69)}, smpl_tfs (1,24,4,4), smpl_verts
        (1,6890,3) posed vertices.  -> z_vals (R, N_samples + N_samples_extra + 2) sorted depths."""
        dev = self.density.beta.device
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        dirs = ray_dirs.detach().to(dev).float().reshape(-1, 3).contiguous()
        R = dirs.shape[0]
        cam = cam_loc.detach().to(dev).float().reshape(-1, 3)[0].contiguous()
        pose = torch.eye(4, **f32)
        pose[:3, 3] = cam
        # far end: the ray / bounding-sphere intersection (rend_util.get_sphere_intersections, rend_util.py:131-147)
        od = (dirs * cam).sum(-1)
        far = (-od + torch.sqrt((od * od - (cam @ cam - self.sdf_bounding_sphere ** 2)).clamp_min(0.0))).contiguous()
        verts = smpl_verts.detach().to(dev).float().reshape(-1, 3).contiguous()
        tfs = smpl_tfs.detach().to(dev).float().reshape(24, 16).contiguous()
        vsorted, cbound = hip.knn_tables(verts, self.deformer_list[person_id].knn_perm)
        btab = hip.blend_table(self.smpl_server_list[person_id].tables.lbs_weights, tfs)
        if isinstance(cond, dict):
            cond = cond["smpl"]
        cvec = cond.detach().to(dev).float().reshape(-1).contiguous()
        beta = self._beta_value()
        per = {person_id: dict(verts=verts, tfs=tfs, btab=btab, vsorted=vsorted, cbound=cbound,
                               hit_index=torch.arange(R, **i32), count=torch.full((1,), R, **i32), cond=cvec)}
        cx = dict(dev=dev, R=R, pose=pose.reshape(16).contiguous(), dirs=dirs, far=far, per=per, persons=[person_id], n_hit=[R],
                  group=R, beta=beta)
        with torch.no_grad():      # draws (training mode): {t_rand [R,NE], u_final [R,N], extra_idx [max_iters,N_extra] int32}
            zfinal, _, _ = self._sample_person(cx, 0, person_id, draws)
        return zfinal

    def _forward_eval(self, input, id, canonical_pose, composite=True):
        """composite=False: stop after the per-person sampling + shading and return the per-person sample arrays (in hit
        order) -- the person-sharded multi-GPU mode composites them elsewhere (parallel.render_person_sharded)."""
        # async_setup (inputs resident and complete, e.g. a render loop over preloaded frames): the setup's host sync waits
        # for the setup kernels only, not for the previous frame still in flight on this stream
        cx = self._setup(input, id, canonical_pose, side_stream=bool(getattr(self, "async_setup", False)))
        dirs, far, per, persons, n_hit = cx["dirs"], cx["far"], cx["per"], cx["persons"], cx["n_hit"]
        stats = {"n_hit": n_hit, "iters": [], "n_sdf_evals": [], "n_shaded": [], "hull_host_fallbacks": getattr(self, "hull_host_fallbacks", 0)}

        for n, p in enumerate(persons):
            zfinal, iters, wcount = self._sample_person(cx, n, p)
            shaded = self._shade_person(cx, n, p, zfinal, wcount)
            stats["iters"].append(iters); stats["n_sdf_evals"].append(wcount)
            per[p].update(zfinal=zfinal, **shaded)

        stats["n_shaded"] = [per[p]["wc2"] for p in persons]
        self.last_stats = stats
        if not composite:
            self._last = dict(per=per, dirs=dirs, far=far, persons=persons, cx=cx)
            return {p: dict(z=per[p]["zfinal"], sdf=per[p]["sdf"], rgb=per[p]["rgb"], nrm=per[p]["nrm"],
                            hit_index=per[p]["hit_index"][:max(int(n_hit[n]), 1)], n_hit=int(n_hit[n]))
                    for n, p in enumerate(persons)}
        bg_rgb = self._background(input, cx)
        out, bg_T, keep = self._composite(cx, persons, bg_rgb)
        self._last = dict(per=per, dirs=dirs, far=far, bg_T=bg_T, bg_rgb=bg_rgb, persons=persons, keep=keep)
        return out

    def _shade_person(self, cx, n, p, zfinal, wcount):
        """shading of person p's final samples (multiply.py:294-308, 403-405): warp to canonical space, Jacobian, weight
        packing, SDF + normals, colour -> the arrays the compositing reads, in hit order"""
        L, st = hip.lib(), hip.stream()
        dev, pp = cx["dev"], cx["per"][p]
        f32 = dict(dtype=torch.float32, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        rs = self.ray_sampler
        NZ = rs.N_samples + rs.N_samples_extra + 2
        S = NZ - 1
        Rp = max(int(cx["n_hit"][n]), 1)
        imp, ren, dfm = self.foreground_implicit_network_list[p], self.foreground_rendering_network_list[p], \
            self.deformer_list[p]
        npts = Rp * S
        xc = torch.empty(npts, 3, **f32)
        sdf = torch.empty(npts, **f32)
        nrm = torch.zeros(npts, 3, **f32)
        rgb = torch.zeros(npts, 3, **f32)
        work2 = torch.empty(npts, **i32)
        need = torch.empty(npts, dtype=torch.uint8, device=dev)
        nn_posed = torch.empty(npts, **i32)
        wc2 = wcount[rs.max_total_iters:]
        with self._ph("shade_warp"):
            L.mp_warp_inverse_shade(cx["dirs"], cx["pose"], pp["hit_index"], pp["count"], zfinal, NZ, S, Rp, pp["vsorted"],
                                    pp["cbound"], pp["btab"], 1, cx["beta"], xc, None, need, sdf, work2, wc2, nn_posed, None, st)
        jinv = torch.empty(npts, 9, **f32)
        with self._ph("shade_jacobian"):
            L.mp_warp_jacobian(xc, need, pp["count"], Rp, S, 0, dfm.vsorted_c, dfm.cbound_c, pp["btab"], jinv, None, nn_posed,
                               dfm.verts_c_flat, st)
        fold = self.feature_fold and self.shade_mode == "reverse"
        pk_full = hip.packed(imp, "sdf" if fold else "full", 2)      # fold: the sampler's pack, feat carries h7'
        pk_full.refresh(pp["cond"])
        if fold:
            pk_col = hip.folded_color(ren, imp, 2).refresh(hip.pose_embed(ren)(pp["cond"]))
        else:
            pk_col = hip.packed(ren, "color", 2)
            pk_col.refresh(hip.pose_embed(ren)(pp["cond"]))
        feat = torch.empty(hip.feat_frag_bytes(npts), dtype=torch.uint8, device=dev)
        with self._ph("mlp_shade"):
            if self.shade_mode == "reverse":     # value sweep (parks the sigmoids) + reverse sweep for the normals
                hip.shade_rev_launch(pk_full, hip.grad_net(imp), xc, jinv, work2, wc2, npts, sdf, nrm, feat, fold=fold)
            else:
                L.mp_mlp_shade(C.byref(pk_full.net), pk_full.wpack, pk_full.bias, xc, jinv, work2, wc2, npts, sdf, nrm, feat, st)
        with self._ph("mlp_color"):
            L.mp_mlp_color(C.byref(pk_col.net), pk_col.wpack, pk_col.bias, xc, nrm, feat, work2, wc2, npts, rgb, st)
        return dict(sdf=sdf, rgb=rgb, nrm=nrm, xc=xc, work2=work2, wc2=wc2)

    def _background(self, input, cx):
        """NeRF++ background colour of every ray of the call, or None without a frame index (multiply.py:482-484,
        514-539)."""
        if input.get("idx", None) is None:
            return None
        rs = self.ray_sampler
        dev = cx["dev"]
        key = "image_id" if "image_id" in input else "idx"      # multiply.py:407-410
        w_lat = self.frame_latent_encoder.weight.detach()        # (row looked up on the device: no device -> host wait)
        code = w_lat.index_select(0, torch.as_tensor(input[key]).reshape(-1)[:1].to(w_lat.device, torch.long))[0]
        t = torch.linspace(0.0, 1.0, rs.N_samples_inverse_sphere, device=dev)
        z_bg = torch.flip(t * (1.0 / rs.scene_bounding_sphere), dims=[0]).contiguous()
        with self._ph("background"):
            return hip.background(self.bg_implicit_network, self.bg_rendering_network, cx["dirs"],
                                  cx["pose"].reshape(4, 4)[:3, 3].contiguous(), z_bg, code,
                                  radius=self.sdf_bounding_sphere, fold=self.feature_fold)

    def _composite(self, cx, persons, bg_rgb):
        """Packed multi-person compositing of the per-person sample arrays in cx['per'] for the subset `persons`
        (multiply.py:425-480, 544-545) -> (output dict, background transmittance, tensors to keep alive)."""
        L = hip.lib()
        dev, R, per = cx["dev"], cx["R"], cx["per"]
        f32 = dict(dtype=torch.float32, device=dev)
        NZ = self.ray_sampler.N_samples + self.ray_sampler.N_samples_extra + 2

        def table(key):
            return hip.device_ints([per[p][key].data_ptr() for p in persons], dev)
        t_inv, t_z, t_sdf, t_rgb, t_nrm = table("inv_index"), table("zfinal"), table("sdf"), table("rgb"), table("nrm")
        rgb_values = torch.empty(R, 3, **f32); fg_rgb_values = torch.empty(R, 3, **f32)
        normal_values = torch.empty(R, 3, **f32); acc_map = torch.empty(R, **f32)
        acc_person = torch.empty(R, len(persons), **f32); bg_T = torch.empty(R, **f32)
        with self._ph("composite"):
            L.mp_composite(R, len(persons), NZ, t_inv, t_z, t_sdf, t_rgb, t_nrm, cx["beta"], bg_rgb, rgb_values, fg_rgb_values,
                           normal_values, acc_map, acc_person, bg_T, hip.stream())
        out = {"acc_map": acc_map, "acc_person_list": acc_person, "rgb_values": rgb_values,
               "fg_rgb_values": fg_rgb_values, "normal_values": normal_values}
        if self.render_geometry and not self.training:
            out.update(self._composite_geometry(cx, persons, (t_inv, t_z, t_sdf)))
        return out, bg_T, (t_inv, t_z, t_sdf, t_rgb, t_nrm)

    def _composite_geometry(self, cx, persons, tables=None, level=None, solo_only=False):
        """The depth outputs of the same merge (render_geometry; csrc/composite.hip k_composite_geometry), a second launch on
        the compositing's tables: the merged depth sum Σ w t (unnormalised like acc_map) and its per-person split, the depth at
        which the ray's opacity reaches `level` (geometry_level) with the column of the person that owns that point, and every
        person's unoccluded ("solo": rendered alone) opacity, depth sum and level depth.  Depths are distances along the ray
        in the units of the samples, -1 = the level is never reached; columns follow acc_person_list.  solo_only: the merged
        outputs are not computed (NULL pointers)."""
        dev, R, per, P = cx["dev"], cx["R"], cx["per"], len(persons)
        f32 = dict(dtype=torch.float32, device=dev)
        NZ = self.ray_sampler.N_samples + self.ray_sampler.N_samples_extra + 2
        if tables is None:
            tables = tuple(hip.device_ints([per[p][key].data_ptr() for p in persons], dev) for key in ("inv_index", "zfinal", "sdf"))
        t_inv, t_z, t_sdf = tables
        level = float(self.geometry_level if level is None else level)
        acc_solo = torch.empty(R, P, **f32); depth_solo = torch.empty(R, P, **f32); depth_solo_level = torch.empty(R, P, **f32)
        depth = depth_person = depth_level = front = None
        if not solo_only:
            depth = torch.empty(R, **f32); depth_person = torch.empty(R, P, **f32)
            depth_level = torch.empty(R, **f32); front = torch.empty(R, dtype=torch.int32, device=dev)
        with self._ph("composite_geometry"):
            hip.lib().mp_composite_geometry(R, P, NZ, t_inv, t_z, t_sdf, cx["beta"], level, depth, depth_person, depth_level,
                                            front, acc_solo, depth_solo, depth_solo_level, hip.stream())
        out = {"acc_person_solo_list": acc_solo, "depth_person_solo_list": depth_solo,
               "depth_person_solo_level_list": depth_solo_level}
        if not solo_only:
            out.update({"depth_values": depth, "depth_person_list": depth_person, "depth_level_values": depth_level,
                        "front_person": front})
        return out

    def render_views(self, input, ids=None, canonical_pose=False):
        """Every view the reference's caller renders of one frame -- all persons (id -1) and each person alone
        (multiply_model.py:982-989, 1183-1190: P + 1 full chunk loops of forward(s, id)) -- from ONE sampling + shading
        pass: a person's samples do not depend on who else is rendered (multiply.py:254-423 loops persons independently),
        so view `id` is a compositing pass over that person's arrays plus the shared background.
        Returns {id: the eval output dict of forward(input, id)}; bit-identical to the separate calls.  With render_geometry every
        view carries the depth keys too; view -1's solo columns are then what the single-person views composite."""
        assert not self.training, "render_views is an eval-mode entry point"
        with torch.no_grad():
            samples = self._forward_eval(input, -1, canonical_pose, composite=False)
            cx = self._last["cx"]
            persons = cx["persons"]
            if ids is None:
                ids = [-1] + (persons if len(persons) > 1 else [])
            bg_rgb = self._background(input, cx)
            views, keep = {}, []
            for i in ids:
                out, bg_T, k = self._composite(cx, persons if i == -1 else [int(i)], bg_rgb)
                views[i] = out
                keep.append((bg_T, k))
            self._last.update(bg_rgb=bg_rgb, keep=keep, samples=samples)
            return views
