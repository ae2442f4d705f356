"""ctypes binding of libmultiply_hip.so (include/multiply_hip.h) + weight packing helpers.

This is the only place the Python host side touches the C ABI.  There is NO fallback: if the shared library is
missing or the device is not a gfx950, importing/using this module raises.
PyTorch is used for device memory and streams only (tensor.data_ptr(), torch.cuda.current_stream()).
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MP_LIB_PATH", os.path.join(_HERE, "libmultiply_hip.so"))  # override: experiments only

MAX_LAYERS, MAX_CHUNKS, BIAS_STRIDE = 10, 9, 288
ACT_NONE, ACT_SOFTPLUS, ACT_RELU, ACT_SIGMUL = 0, 1, 2, 3
KNN_CLUSTER, KNN_NC = int(os.environ.get("MP_KNN_CLUSTER", 32)), int(os.environ.get("MP_KNN_NC", 216))   # = include/multiply_hip.h
SMPL_VBWD_SCRATCH, SMPL_DLBS = 216 * 512, 24 * 16 + 207 + 86     # = include/multiply_hip.h (mp_smpl_verts_bwd)
SMPL_BATCH_ROWS, SMPL_BATCH_ROW_WORK = 16, 672                   # = include/multiply_hip.h (mp_smpl_pose_batch)
KNN_CB_ROWS = KNN_NC + KNN_NC // 2      # mp_knn_build's sphere table: the clusters, then the pairs of clusters the training searches use


class MpLayer(C.Structure):
    _fields_ = [("n_chunk", C.c_int), ("use_reg", C.c_int), ("use_in", C.c_int), ("act", C.c_int),
                ("out_chunk", C.c_int), ("aux", C.c_int)]


class MpNet(C.Structure):
    _fields_ = [("n_layers", C.c_int), ("total_chunks", C.c_int), ("layer", MpLayer * MAX_LAYERS)]


class MpPackLayer(C.Structure):
    _fields_ = [("v", C.c_void_p), ("g", C.c_void_p), ("b", C.c_void_p), ("rowmap", C.c_void_p), ("colmap", C.c_void_p),
                ("colscale", C.c_void_p), ("hoist_vec", C.c_void_p), ("wpack_layer", C.c_void_p), ("bias_layer", C.c_void_p),
                ("out_dim", C.c_int), ("in_dim", C.c_int), ("n_rows", C.c_int), ("hoist_col0", C.c_int), ("hoist_n", C.c_int),
                ("bias_scale", C.c_float)]


class MpSamplerCfg(C.Structure):
    _fields_ = [("n_samples", C.c_int), ("n_samples_eval", C.c_int), ("n_samples_extra", C.c_int),
                ("beta_iters", C.c_int), ("max_total_iters", C.c_int), ("eps", C.c_float), ("add_tiny", C.c_float),
                ("near_", C.c_float)]


class MpSamplerState(C.Structure):
    _fields_ = [("zs", C.c_void_p), ("sdfs", C.c_void_p), ("nz", C.c_void_p), ("znew", C.c_void_p),
                ("sdfnew", C.c_void_p), ("beta", C.c_void_p), ("ray_active", C.c_void_p), ("group_flag", C.c_void_p),
                ("zfinal", C.c_void_p), ("iters", C.c_void_p), ("any_active", C.c_void_p)]


_lib = None


def lib():
    """Loads the HIP library; raises loudly when it is absent (no CPU / PyTorch fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
                               f"g.build()'` (hipcc --offload-arch=gfx950). The MultiPly hot path has no fallback.")
        if "MP_LIB_PATH" not in os.environ:
            # the library must be what THIS tree's sources produce (multiply_amd/build.py stamps it with a content hash)
            from . import build as B
            have, want = B.library_hash(), B.source_hash()
            if have is not None and have != want:
                raise RuntimeError(f"{LIB_PATH} was built from sources {have}, this tree is {want}: rebuild it with "
                                   f"`python -m multiply_amd.build` (a stale library is never loaded)")
        _lib = C.CDLL(LIB_PATH)
        _declare_prototypes(_lib)
    return _lib


def lib_source_sha16():
    """content hash of the sources the loaded library was built from (multiply_amd/build.py)"""
    from . import build as B
    return B.library_hash()


HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "multiply_hip.h")


class DevPtr(C.c_void_p):
    """argtype of every pointer parameter: the one place a tensor becomes a device pointer.  Anything else (None, a c_void_p
    from ptr() / an offset pointer, byref(struct), a ctypes array, an int) converts as for c_void_p.  A refused tensor surfaces
    from the call as ctypes.ArgumentError, which names the argument's position."""

    @classmethod
    def from_param(cls, t):
        if isinstance(t, torch.Tensor):
            assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
            return C.c_void_p(t.data_ptr())
        return C.c_void_p.from_param(t)


def header_prototypes(path=HEADER_PATH):
    """{name: (restype, [argtypes])} parsed from include/multiply_hip.h -- the header is the single source of truth
    for the C ABI; scalars map to their exact ctypes width (a `long long` or `float` passed as a default Python int /
    double would otherwise be widened or truncated by ctypes' default conversions), every pointer to DevPtr."""
    import re
    with open(path) as f:
        txt = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    scal = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "long long": C.c_longlong, "unsigned": C.c_uint, "void": None}
    protos = {}
    for ret, name, args in re.findall(r"\b(int|void|const char\s*\*)\s+(mp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", txt):
        at = []
        for a in [x.strip() for x in args.split(",")]:
            if a in ("void", ""):
                continue
            if "*" in a:
                at.append(DevPtr)
            else:
                ty = re.sub(r"\bconst\b", "", a).strip().rsplit(" ", 1)[0].strip()
                at.append(scal[ty])
        protos[name] = (C.c_char_p if "char" in ret else (None if ret == "void" else C.c_int), at)
    return protos


# Every entry point returns a status (0, or a hipError_t / negative argument-error code: the header's top comment) except these,
# which return a value
VALUE_RETURNING = ("mp_device_ok", "mp_sig_bytes_per_point", "mp_obb_hull_device_work_bytes", "mp_warp_bin_work_bytes",
                   "mp_debug_hull_abandon", "mp_arch", "mp_mesh_index_bytes", "mp_image_work_bytes")
_DEBUG_SYNC = bool(int(os.environ.get("MP_DEBUG_SYNC", "0")))


def _errcheck(code, fn, args):
    """ctypes errcheck of every status-returning entry point: no launch's status goes unread"""
    check(code, fn.__name__)
    if _DEBUG_SYNC:                      # debugging aid: attribute asynchronous faults to the launch that caused them
        torch.cuda.synchronize()
        print("[mp sync ok]", fn.__name__, flush=True)
    return code


def _declare_prototypes(l):
    for name, (rt, at) in header_prototypes().items():
        fn = getattr(l, name)
        fn.restype, fn.argtypes = rt, at
        if name not in VALUE_RETURNING:
            fn.errcheck = _errcheck


def require_device():
    if not torch.cuda.is_available():
        raise RuntimeError("multiply_amd needs a ROCm device (MI355X / gfx950); none is visible")
    if not lib().mp_device_ok():
        raise RuntimeError("multiply_amd kernels are built for gfx950 only; the current device is not a gfx950")


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "device-resident contiguous tensors only"
    return C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def check(code, what):
    if code != 0:
        raise RuntimeError(f"{what} failed with code {code}")


# ------------------------------------------------------------------------------------------------ packing
def reg_slot_feature(s):
    """K slot s (0..255) of a register-fed K step -> index of the previous layer's output row it multiplies
    (the permutation documented in csrc/mlp_core.hpp)."""
    ks, sl = divmod(s, 32)
    g, e = divmod(sl, 8)
    return 32 * ks + (4 * g + e if e < 4 else 16 + 4 * g + e - 4)


_REG_FEATURE = np.array([reg_slot_feature(s) for s in range(256)], dtype=np.int64)


class LayerPlan:
    """How one nn.Linear maps onto the packed layout."""

    def __init__(self, lin, rowmap, reg_cols=None, in_cols=None, scale=1.0, hoist=None, act=ACT_NONE, out_chunk=-1,
                 in_scale=None, bias_scale=1.0, transpose=False, row_scale=None, aux=0):
        """transpose: pack W^T (rows = the layer's INPUT features, K = its outputs; reverse sweep); row_scale: optional
        per-row factors of the transposed matrix (the input-side scales of the forward plan); aux: see MpLayer.aux."""
        self.lin, self.act, self.out_chunk = lin, act, out_chunk
        self.transpose, self.row_scale, self.aux = transpose, row_scale, aux
        self.in_scale = float(scale if in_scale is None else in_scale)   # factor on the input-fed K slots
        self.bias_scale = float(bias_scale)
        rowmap = list(rowmap)
        while len(rowmap) % 32:
            rowmap.append(-1)
        self.rowmap = np.array(rowmap, dtype=np.int32)
        self.reg_cols = None if reg_cols is None else np.asarray(reg_cols, dtype=np.int64)
        self.in_cols = None if in_cols is None else np.asarray(in_cols, dtype=np.int64)
        self.scale = float(scale)
        self.hoist = hoist  # (col0, n) or None

    def colmap(self, ks_in):
        n = (8 + ks_in) * 32
        cm = -np.ones(n, dtype=np.int32)
        if self.reg_cols is not None:
            f = _REG_FEATURE
            ok = f < len(self.reg_cols)
            cm[:256][ok] = self.reg_cols[f[ok]]
        if self.in_cols is not None:
            assert len(self.in_cols) <= ks_in * 32
            cm[256:256 + len(self.in_cols)] = self.in_cols
        return cm


class PackedNet:
    """half (f16) fragment-ordered weights + fp32 bias table of one network role on the device."""

    def __init__(self, plans, ks_in, device):
        assert len(plans) <= MAX_LAYERS
        self.plans, self.ks_in, self.device = plans, ks_in, device
        self.chunk_bytes = 2 * (8 + ks_in) * 1024
        self.net = MpNet()
        self.net.n_layers = len(plans)
        off, self.offsets = 0, []
        for i, p in enumerate(plans):
            nch = len(p.rowmap) // 32
            assert 1 <= nch <= MAX_CHUNKS
            L = self.net.layer[i]
            L.n_chunk, L.use_reg, L.use_in = nch, int(p.reg_cols is not None), int(p.in_cols is not None)
            L.act, L.out_chunk, L.aux = p.act, p.out_chunk, p.aux
            self.offsets.append(off)
            off += nch
        self.net.total_chunks = off
        acts = [p.act != ACT_NONE for p in plans]
        assert acts == sorted(acts, reverse=True), "the core runs hidden layers first, then the linear output layer(s)"
        self.wpack = torch.zeros(off * self.chunk_bytes, dtype=torch.uint8, device=device)
        self.bias = torch.zeros(MAX_LAYERS * BIAS_STRIDE, dtype=torch.float32, device=device)
        self.rowmaps = [torch.from_numpy(p.rowmap).to(device) for p in plans]
        self.colmaps = [torch.from_numpy(p.colmap(ks_in)).to(device) for p in plans]
        self.colscales = []
        for p in plans:
            cs = torch.full(((8 + ks_in) * 32,), p.scale, dtype=torch.float32, device=device)
            cs[256:] = p.in_scale
            self.colscales.append(cs)
        self.version = None

    def _params(self, lin):
        if hasattr(lin, "weight_g"):
            return lin.weight_v, lin.weight_g, lin.bias
        return lin.weight, None, lin.bias

    def _pack_layer(self, i, weights, hoist_vec):
        p = self.plans[i]
        v, g, b = self._params(p.lin)
        if p.transpose:      # reverse sweep: effective weight (weight norm resolved), transposed, input-side scales on the rows
            w = v.detach().float()
            if g is not None:
                w = w * (g.detach().reshape(-1, 1) / w.norm(dim=1, keepdim=True))
            w = w.t()
            if p.row_scale is not None:
                w = w * torch.as_tensor(p.row_scale, dtype=torch.float32, device=w.device).reshape(-1, 1)
            v, g, b = w.contiguous(), None, torch.zeros(w.shape[0], dtype=torch.float32, device=w.device)
        v, b = v.detach().contiguous(), b.detach().contiguous()
        g = None if g is None else g.detach().reshape(-1).contiguous()
        h0, hn = p.hoist if (p.hoist is not None and hoist_vec is not None) else (0, 0)
        wp = C.c_void_p(self.wpack.data_ptr() + self.offsets[i] * self.chunk_bytes) if weights else None
        bp = C.c_void_p(self.bias.data_ptr() + 4 * i * BIAS_STRIDE)
        lib().mp_pack_layer(v, g, b, v.shape[0], v.shape[1], self.rowmaps[i], len(p.rowmap), self.colmaps[i], self.colscales[i],
                            self.ks_in, h0, hn, hoist_vec if hn else None, p.bias_scale, wp, bp, stream())

    def param_version(self):
        vs = [_GENERATION[0]]
        for p in self.plans:
            for t in self._params(p.lin):
                if t is not None:
                    vs.append((t.data_ptr(), t._version))
        return tuple(vs)

    def _table(self, weights, hoisted):
        """device-resident MpPackLayer records of every layer (mp_pack_layers), cached per (parameter pointers, variant): the
        hoisted vector is read from a persistent buffer of this object, so the table survives from call to call"""
        ptrs = tuple(t.data_ptr() if t is not None else 0 for p in self.plans for t in self._params(p.lin))
        key = (weights, hoisted)
        cache = self.__dict__.setdefault("_tables", {})
        if key not in cache or cache[key][0] != ptrs:
            arr = (MpPackLayer * len(self.plans))()
            for i, p in enumerate(self.plans):
                v, g, b = self._params(p.lin)
                assert v.is_contiguous() and b.is_contiguous() and v.dtype == torch.float32
                h0, hn = p.hoist if (p.hoist is not None and hoisted) else (0, 0)
                skip = not weights and p.hoist is None            # bias-only refresh: only the hoisted layer changes
                arr[i] = MpPackLayer(v.data_ptr(), g.data_ptr() if g is not None else None, b.data_ptr(),
                                     self.rowmaps[i].data_ptr(), self.colmaps[i].data_ptr(), self.colscales[i].data_ptr(),
                                     self._hoist_buf.data_ptr() if hn else None,
                                     (self.wpack.data_ptr() + self.offsets[i] * self.chunk_bytes) if weights else None,
                                     None if skip else self.bias.data_ptr() + 4 * i * BIAS_STRIDE,
                                     v.shape[0], v.shape[1], 0 if skip else len(p.rowmap), h0, hn, p.bias_scale)
            cache[key] = (ptrs, torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.device))
        return cache[key][1]

    def refresh(self, hoist_vec=None, force=False):
        """(Re)packs the weights if a parameter changed (or `force`: training mode, see invalidate_packed), and the hoisted
        layer-0 bias for this call's conditioning."""
        ver = self.param_version()
        full = force or ver != self.version
        if not any(p.transpose for p in self.plans):
            # ONE launch for all layers (mp_pack_layers); the call's conditioning goes through a persistent buffer
            hoisted = hoist_vec is not None and any(p.hoist is not None for p in self.plans)
            if hoisted:
                hn = max(p.hoist[1] for p in self.plans if p.hoist is not None)
                if self.__dict__.get("_hoist_buf") is None or self._hoist_buf.numel() < hn:
                    self._hoist_buf = torch.empty(hn, dtype=torch.float32, device=self.device)
                    self.__dict__.pop("_tables", None)
                self._hoist_buf[:hn].copy_(hoist_vec.detach().reshape(-1)[:hn].float(), non_blocking=True)
            if full or hoisted:
                tab = self._table(bool(full), hoisted)
                lib().mp_pack_layers(tab, len(self.plans), self.ks_in, stream())
            self.version = ver
            return
        for i, p in enumerate(self.plans):
            if full:
                self._pack_layer(i, True, hoist_vec if p.hoist is not None else None)
            elif p.hoist is not None:
                self._pack_layer(i, False, hoist_vec)
        self.version = ver


SOFTPLUS_K = 100.0 * math.log2(math.e)   # scaled units of the softplus networks (csrc/mlp_core.hpp)


def implicit_plans(net, variant):
    """LayerPlans of an ImplicitNet (fg: d_in 3, L 6, cond 69; bg: d_in 4, L 10, cond 32).
    variant 'sdf': last layer = sdf row only; 'full': 256 feature rows then the sdf row as the extra out chunk.
    Hidden layers work in scaled units z' = K z, h' = K h: biases and input-fed weights x K, register-fed weights
    unchanged, last (linear) layer's weights x 1/K."""
    E, nl, K = net.embed_dim, net.num_layers - 1, SOFTPLUS_K
    plans = []
    for l, lin in enumerate(net.layers()):
        out_dim = (lin.weight_v if hasattr(lin, "weight_v") else lin.weight).shape[0]
        last = l == nl - 1
        act = ACT_NONE if last else ACT_SOFTPLUS
        if last:
            if variant == "sdf":
                plans.append(LayerPlan(lin, [0], reg_cols=np.arange(256), scale=1.0 / K, act=act, out_chunk=0))
            else:
                plans.append(LayerPlan(lin, list(range(1, out_dim)) + [0], reg_cols=np.arange(256), scale=1.0 / K,
                                       act=act, out_chunk=8))
        elif l == 0:
            hoist = (E, net.cond_dim) if net.cond_dim > 0 else None
            plans.append(LayerPlan(lin, range(out_dim), in_cols=np.arange(E), hoist=hoist, act=act, in_scale=K,
                                   bias_scale=K))
        elif l in net.skip_in:
            prev = net.dims[l] - E   # width of the previous layer's output
            r2 = 1.0 / math.sqrt(2.0)
            plans.append(LayerPlan(lin, range(out_dim), reg_cols=np.arange(prev), in_cols=prev + np.arange(E), scale=r2,
                                   in_scale=r2 * K, act=act, bias_scale=K))
        else:
            plans.append(LayerPlan(lin, range(out_dim), reg_cols=np.arange(net.dims[l]), act=act, bias_scale=K))
    return plans


def implicit_grad_plans(net):
    """Reverse sweep of the foreground ImplicitNet for d sdf / d x (csrc/mlp.hip k_mlp_shade_rev, sweep 2): layers 7..1 transposed
    (rows = that layer's inputs, K = its outputs in K-slot order, outputs multiplied by the stored sigmoid of the layer
    below), then the input-fed part of layer 0 transposed.  The skip layer's transpose also carries the 39 rows of the
    re-injected encoding (captured as gradient rows, capture id 2); layer 0's rows are captured with id 1."""
    if not (net.d_in == 3 and net.multires == 6 and list(net.skip_in) == [4] and net.num_layers - 1 == 9):
        # the shipped configs' foreground network (confs/model/*.yaml: dims 8 x 256, skip_in [4], multires 6); other depths /
        # skip positions still render through the forward-mode kernel
        raise NotImplementedError("reverse-mode shading is specialised for the 9-layer, skip-at-4, multires-6 ImplicitNet of the "
                                  "shipped configs; set model.shade_mode = 'forward' (MP_SHADE_MODE=forward) for other shapes")
    E, K = net.embed_dim, SOFTPLUS_K
    lins = list(net.layers())
    r2 = 1.0 / math.sqrt(2.0)
    plans = []
    for l in range(7, 0, -1):
        lin = lins[l]
        wv = lin.weight_v if hasattr(lin, "weight_v") else lin.weight
        out_dim, in_dim = wv.shape
        row_scale, aux = None, (l - 1) + 1           # outputs (= h_{l-1} adjoint) x sigma'_{l-1}
        if l in net.skip_in:
            prev = in_dim - E
            row_scale = np.concatenate([np.full(prev, r2), np.full(E, r2 * K)])
            aux |= 2 << 8
        plans.append(LayerPlan(lin, range(in_dim), reg_cols=np.arange(out_dim), act=ACT_SIGMUL, transpose=True,
                               row_scale=row_scale, aux=aux))
    lin0 = lins[0]
    plans.append(LayerPlan(lin0, range(E), reg_cols=np.arange(lin0.bias.shape[0]), act=ACT_NONE, transpose=True,
                           row_scale=np.concatenate([np.full(E, K), np.zeros(net.cond_dim)]), aux=1 << 8))
    return plans


def sdf_row_slots(net):
    """the sdf row of the last layer (effective weights) as 256 halves in K-slot order: V_8 of the reverse sweep"""
    lin = list(net.layers())[-1]
    w = (lin.weight_v if hasattr(lin, "weight_v") else lin.weight).detach().float()
    if hasattr(lin, "weight_g"):
        w = w * (lin.weight_g.detach().reshape(-1, 1) / w.norm(dim=1, keepdim=True))
    idx = torch.as_tensor(_REG_FEATURE, device=w.device)
    return w[0][idx].to(torch.float16).contiguous()


def feature_col0(net):
    """first of the 256 feature columns of a RenderingNet's first layer"""
    return 14 if net.mode == "pose_no_view" else 59


def rendering_plans(net, folded=None):
    """LayerPlans of a RenderingNet: 'pose_no_view' = [x_c3, n3 | pose8 hoisted | feat256]; 'nerf_frame_encoding' =
    [PE4(view) 27 | frame32 hoisted | feat256].
    folded: a FoldedLinear in place of layer 0 (FoldedColor): its feature columns multiply the SDF network's last hidden vector,
    which arrives in scaled units h' = K h, so the register-fed K slots carry 1/K; everything else as for the layer itself."""
    plans, nl = [], net.num_layers - 1
    for l, lin in enumerate(net.layers()):
        out_dim = (lin.weight_v if hasattr(lin, "weight_v") else lin.weight).shape[0]
        last = l == nl - 1
        act = ACT_NONE if last else ACT_RELU
        rows = range(out_dim)
        if l == 0:
            fold = {} if folded is None else dict(scale=1.0 / SOFTPLUS_K, in_scale=1.0)
            lin = lin if folded is None else folded
            if net.mode == "pose_no_view":
                plans.append(LayerPlan(lin, rows, reg_cols=14 + np.arange(256), in_cols=np.arange(6), hoist=(6, 8),
                                       act=act, out_chunk=0 if last else -1, **fold))
            else:
                plans.append(LayerPlan(lin, rows, reg_cols=59 + np.arange(256), in_cols=np.arange(27), hoist=(27, 32),
                                       act=act, out_chunk=0 if last else -1, **fold))
        else:
            plans.append(LayerPlan(lin, rows, reg_cols=np.arange(net.dims[l]), act=act, out_chunk=0 if last else -1))
    return plans


class _PinnedInts:
    """Small integer tables (device pointer lists, sizes) host -> device WITHOUT a host wait.  torch.tensor(list, device=dev)
    is a blocking copy from pageable memory: torch synchronises the current stream behind it, i.e. the host waits for every
    kernel enqueued so far -- seven such tables per training iteration kept the host from ever running ahead of the GPU.
    Here the values go into a ring of pinned memory and are copied with non_blocking=True (stream-ordered, no wait); a slot is
    reused after 64 k entries, long after its copy has run."""

    def __init__(self, n=1 << 16):
        self.buf = torch.empty(n, dtype=torch.int64).pin_memory()
        self.view = self.buf.numpy()
        self.pos = 0

    def put(self, values, dev):
        k = len(values)
        if self.pos + k > self.buf.numel():
            self.pos = 0
        sl = slice(self.pos, self.pos + k)
        self.view[sl] = values
        self.pos += k
        return self.buf[sl].to(dev, non_blocking=True)


_PINNED = {}


def device_ints(values, dev):
    """int64 device tensor of a short Python list (see _PinnedInts); CPU device: a plain tensor"""
    dev = torch.device(dev)
    if dev.type != "cuda":
        return torch.tensor(list(values), dtype=torch.int64, device=dev)
    ring = _PINNED.get("ring")
    if ring is None:
        ring = _PINNED["ring"] = _PinnedInts()
    return ring.put(list(values), dev)


class ZeroPool:
    """Zero-initialised scratch tensors of one call / one adjoint sweep as views of a few large zero-filled blocks: ONE fill per
    block instead of one per tensor (a training iteration asked for ~70 small zero tensors: gradient seeds, device counters,
    adjoint accumulators -- each a launch of its own).  A block lives as long as any of its views; a new pool per call, so a
    view handed to autograd as a gradient is never written again.  Requests above a quarter of a block get their own fill."""

    def __init__(self, device, block_bytes=8 << 20):
        self.device, self.block_bytes = torch.device(device), block_bytes
        self.buf, self.off = None, 0

    def take(self, *shape, dtype=torch.float32):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * torch.empty(0, dtype=dtype).element_size()
        if nbytes > self.block_bytes // 4 or self.device.type != "cuda":
            return torch.zeros(shape, dtype=dtype, device=self.device)
        if self.buf is None or self.off + nbytes > self.block_bytes:
            self.buf, self.off = torch.zeros(self.block_bytes, dtype=torch.uint8, device=self.device), 0
        v = self.buf[self.off:self.off + nbytes].view(dtype).view(shape)
        self.off += (nbytes + 255) // 256 * 256
        return v


# The packed weights are keyed on the parameters' (data_ptr, _version).  That is NOT enough for every optimizer: torch's fused
# Adam (torch._fused_adam_) updates the parameters WITHOUT bumping their version counters, so a cache keyed on them alone would
# keep rendering with the weights of the first step.  Two guards: a forward in training mode always repacks (force=True: the
# weights are expected to change between calls there), and every train() / eval() switch of the model bumps this generation,
# which is part of every cache key -- the first eval render after training packs afresh whatever the optimizer did.
_GENERATION = [0]


def invalidate_packed():
    """Forget every packed-weight cache (call after modifying parameters in a way that does not bump their _version)."""
    _GENERATION[0] += 1


def packed(module, role, ks_in):
    """Per-module cache of PackedNet objects."""
    cache = module.__dict__.setdefault("_mp_packed", {})
    dev = next(module.parameters()).device
    key = (role, ks_in, str(dev))
    if key not in cache:
        from .networks import ImplicitNet
        if isinstance(module, ImplicitNet):
            plans = implicit_grad_plans(module) if role == "grad" else implicit_plans(module, role)
        else:
            plans = rendering_plans(module)
        cache[key] = PackedNet(plans, ks_in, dev)
    return cache[key]


class FoldedLinear:
    """what mp_fold_features writes: the first layer of a rendering network as an effective fp32 weight (weight norm resolved)
    whose feature columns hold Wc[:, feat] . W8[1:], and its bias bc + Wc[:, feat] . b8[1:].  Packed like an nn.Linear."""

    def __init__(self, out_dim, in_dim, device):
        self.weight = torch.zeros(out_dim, in_dim, dtype=torch.float32, device=device)
        self.bias = torch.zeros(out_dim, dtype=torch.float32, device=device)


def _lin_params(lin):
    if hasattr(lin, "weight_g"):
        return lin.weight_v, lin.weight_g, lin.bias
    return lin.weight, None, lin.bias


class FoldedColor:
    """A rendering network PAIRED WITH its SDF network (eval path): the SDF network's last layer is linear and its 256 feature
    rows only feed the rendering network's first layer, which is linear in them -- so the product of the two (256 x 256; 128 x
    256 for the background) replaces both: the SDF side runs its 'sdf' plan (last layer = the sdf row alone), hands on its last
    hidden vector h7' (scaled units) where it handed on the features, and the colour side's first layer is packed from the
    product.  The product is formed on the device (mp_fold_features) when a parameter of EITHER of the two layers changed -- the
    (data_ptr, _version) key of PackedNet.param_version over both, with the cache generation (invalidate_packed) -- and the pack
    of the whole rendering network follows; per call only the hoisted pose / frame bias is refreshed, as for the plain pack."""

    def __init__(self, ren, imp, ks_in):
        self.lin_c, self.lin_8 = list(ren.layers())[0], list(imp.layers())[-1]
        vc, v8 = _lin_params(self.lin_c)[0], _lin_params(self.lin_8)[0]
        self.col0, self.n_feat = feature_col0(ren), v8.shape[0] - 1
        assert self.col0 + self.n_feat == vc.shape[1] and self.n_feat == 256 and v8.shape[1] <= 256, \
            "feature fold: the rendering network's first layer ends in the SDF network's 256 features"
        self.folded = FoldedLinear(vc.shape[0], vc.shape[1], vc.device)
        self.pk = PackedNet(rendering_plans(ren, self.folded), ks_in, vc.device)
        self.version = None

    def param_version(self):
        vs = [_GENERATION[0]]
        for lin in (self.lin_c, self.lin_8):
            vs += [(t.data_ptr(), t._version) for t in _lin_params(lin) if t is not None]
        return tuple(vs)

    def refresh(self, hoist_vec=None, force=False):
        """-> the PackedNet of the folded rendering network, current for the parameters of both modules and this call's
        conditioning"""
        ver = self.param_version()
        stale = force or ver != self.version
        if stale:
            (vc, gc, bc), (v8, g8, b8) = _lin_params(self.lin_c), _lin_params(self.lin_8)
            flat = lambda t: None if t is None else t.detach().reshape(-1).contiguous()
            lib().mp_fold_features(vc.detach().contiguous(), flat(gc), flat(bc), vc.shape[0], vc.shape[1], self.col0, self.n_feat,
                                   v8.detach().contiguous(), flat(g8), flat(b8), v8.shape[1], self.folded.weight,
                                   self.folded.bias, stream())
            self.version = ver
        self.pk.refresh(hoist_vec, force=stale)
        return self.pk


def folded_color(ren, imp, ks_in):
    """the FoldedColor of a rendering network and its SDF network (cached on the rendering module, per SDF module)"""
    cache = ren.__dict__.setdefault("_mp_folded", {})
    key = (id(imp), ks_in, str(next(ren.parameters()).device))
    fc = cache.get(key)
    if fc is None or fc.lin_8 is not list(imp.layers())[-1]:
        fc = cache[key] = FoldedColor(ren, imp, ks_in)
    return fc


class PoseEmbed:
    """lin_pose(cond) of RenderingNet 'pose_no_view' (networks.py:279-280) computed by the bias path of mp_pack_layer."""

    def __init__(self, net):
        self.net = net
        dev = net.lin_pose.weight.device
        self.rowmap = torch.tensor(list(range(8)) + [-1] * 24, dtype=torch.int32, device=dev)
        self.colmap = -torch.ones(10 * 32, dtype=torch.int32, device=dev)
        self.colscale = torch.ones(10 * 32, dtype=torch.float32, device=dev)
        self.out = torch.zeros(BIAS_STRIDE, dtype=torch.float32, device=dev)

    def __call__(self, cond_vec):
        lp = self.net.lin_pose
        w, b = lp.weight.detach().contiguous(), lp.bias.detach().contiguous()
        lib().mp_pack_layer(w, None, b, 8, 69, self.rowmap, 32, self.colmap, self.colscale, 2, 0, 69, cond_vec, 1.0, None,
                            self.out, stream())
        return self.out  # first 8 floats


def pose_embed(ren):
    """the PoseEmbed of a 'pose_no_view' RenderingNet (cached on the module)"""
    pe = ren.__dict__.get("_mp_pose_embed")
    if pe is None:
        pe = ren.__dict__["_mp_pose_embed"] = PoseEmbed(ren)
    return pe


# ------------------------------------------------------------------------------------------------ module-level ops
def knn_tables(verts, perm):
    """nearest-vertex structure of posed / canonical vertices (V,3) under the static cluster order `perm` (mp_knn_build):
    vsorted (KNN_NC * KNN_CLUSTER, 4) and the clusters' bounding spheres cbound (KNN_CB_ROWS, 4)"""
    f32 = dict(dtype=torch.float32, device=verts.device)
    vsorted = torch.empty(KNN_NC * KNN_CLUSTER, 4, **f32)
    cbound = torch.empty(KNN_CB_ROWS, 4, **f32)
    lib().mp_knn_build(verts, perm, vsorted, cbound, stream())
    return vsorted, cbound


def blend_table(lbs_weights, tfs):
    """(V,12) per-vertex inverse blended transform of the bone transforms tfs (24 x 16 floats) (mp_blend_table)"""
    n = lbs_weights.shape[0]
    tab = torch.empty(n, 12, dtype=torch.float32, device=lbs_weights.device)
    lib().mp_blend_table(lbs_weights, tfs, n, tab, stream())
    return tab


def implicit_forward(net, x, cond_vec):
    """ImplicitNet.forward for external callers: (N, d_in) -> (N, 257) fp32 (features are f16-rounded)."""
    require_device()
    x = x.detach().float().contiguous()
    ks_in = 2 if net.d_in == 3 else 3
    pk = packed(net, "full", ks_in)
    pk.refresh(None if cond_vec is None else cond_vec.detach().float().contiguous())
    out = torch.empty(x.shape[0], 257, dtype=torch.float32, device=x.device)
    lib().mp_mlp_full(C.byref(pk.net), pk.wpack, pk.bias, x, net.d_in, x.shape[0], out, stream())
    return out


def implicit_sdf(net, x_c, cond_vec, mode="f16"):
    """sdf column of the foreground ImplicitNet at canonical points (N,3) -> (N,).  mode 'f16' (mp_mlp_sdf) | 'f16x2' (split
    activations on the same packed weights, mp_mlp_sdf_x2)."""
    require_device()
    x_c = x_c.detach().float().contiguous()
    pk = packed(net, "sdf", 2)
    pk.refresh(cond_vec.detach().float().contiguous())
    out = torch.empty(x_c.shape[0], dtype=torch.float32, device=x_c.device)
    fn = {"f16": lib().mp_mlp_sdf, "f16x2": lib().mp_mlp_sdf_x2}[mode]
    fn(C.byref(pk.net), pk.wpack, pk.bias, x_c, None, None, x_c.shape[0], out, stream())
    return out


SHADE_MODE = os.environ.get("MP_SHADE_MODE", "reverse")   # "reverse" (2 sweeps, 2 network columns per point) | "forward"


class GradNet:
    """packed reverse-sweep network + the sdf row in K-slot order of one foreground ImplicitNet (cached on the module)"""

    def __init__(self, imp):
        self.imp = imp
        self.pk = packed(imp, "grad", 0)      # no input-fed K steps in the reverse sweep
        self.w8 = None
        self.version = None

    def refresh(self):
        self.pk.refresh(None)
        if self.version != self.pk.version:
            self.w8 = sdf_row_slots(self.imp)
            self.version = self.pk.version
        return self


def grad_net(imp):
    g = imp.__dict__.get("_mp_gradnet")
    if g is None:
        g = imp.__dict__["_mp_gradnet"] = GradNet(imp)
    return g.refresh()


SEG_POINTS = int(os.environ.get("MP_SEG_POINTS", 1 << 21))   # work items per segment of the reverse-mode shading (x 2 KiB of stored sigmoids)


def sig_scratch(device, n_points):
    """(buffer, segment size) for the stored sigmoids of the reverse-mode shading kernels: mp_sig_bytes_per_point() bytes (2 KiB:
    one byte per hidden unit; 4 KiB in a -DMP_EXP_SIG16 build) per work item of ONE segment, sized to the call (min(n rounded up to
    a tile, SEG_POINTS)) and grown on demand -- never a fixed multi-GiB block.  New parts are zero-initialised: the K steps a
    narrower layer never writes (layer 3 has 217 outputs) must read as finite numbers in the reverse sweep."""
    per = int(lib().mp_sig_bytes_per_point())
    seg = min(SEG_POINTS, max(256, (int(n_points) + 255) // 256 * 256))
    key = str(device)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < seg * per:
        grown = torch.empty(seg * per, dtype=torch.uint8, device=device)
        old = 0 if buf is None else buf.numel()
        if old:
            grown[:old] = buf
        grown[old:].zero_()
        buf = _SCRATCH[key] = grown
    return buf, seg


_SCRATCH = {}


def shade_rev_launch(pki, gn, x_c, jinv, worklist, count, n, sdf, nrm, feat, fold=False):
    """fold: pki is the 'sdf' pack and feat receives h7' for a FoldedColor pack (mp_mlp_shade_rev_fold)"""
    buf, seg = sig_scratch(x_c.device, n)
    fn = lib().mp_mlp_shade_rev_fold if fold else lib().mp_mlp_shade_rev
    fn(C.byref(pki.net), pki.wpack, pki.bias, C.byref(gn.pk.net), gn.pk.wpack, gn.w8, x_c, jinv, worklist, count, n, sdf, nrm,
       feat, buf, seg, stream())


def feat_frag_bytes(n):
    """size of the shade -> colour feature hand-off for n work items: f16 B-fragments, 8 K steps x 4 blocks x 1 KiB per tile of
    64 items, in whole launches of 4 tiles (csrc/mlp.hip feat_frag)"""
    return (int(n) + 255) // 256 * 4 * 8 * 4 * 1024


def shade_points(imp, ren, x_c, jinv, cond_vec, mode=None, fold=False):
    """sdf, normals, rgb at canonical points (ImplicitNet value + input gradient, RenderingNet 'pose_no_view').
    mode 'reverse': mp_mlp_shade_rev (two sweeps); 'forward': the forward-mode kernel mp_mlp_shade.
    fold (reverse mode only): the feature fold the renderer uses (FoldedColor, mp_mlp_shade_rev_fold)."""
    require_device()
    n = x_c.shape[0]
    x_c = x_c.detach().float().contiguous()
    jinv = jinv.detach().float().contiguous()
    cond_vec = cond_vec.detach().float().contiguous()
    if fold and (mode or SHADE_MODE) != "reverse":
        raise ValueError("the feature fold exists in reverse-mode shading only: the forward-mode kernel is its unfolded cross-check")
    pki = packed(imp, "sdf" if fold else "full", 2)
    pki.refresh(cond_vec)
    if fold:
        pkr = folded_color(ren, imp, 2).refresh(pose_embed(ren)(cond_vec))
    else:
        pkr = packed(ren, "color", 2)
        pkr.refresh(pose_embed(ren)(cond_vec))
    dev = x_c.device
    sdf = torch.empty(n, dtype=torch.float32, device=dev)
    nrm = torch.empty(n, 3, dtype=torch.float32, device=dev)
    rgb = torch.empty(n, 3, dtype=torch.float32, device=dev)
    feat = torch.empty(feat_frag_bytes(n), dtype=torch.uint8, device=dev)
    if (mode or SHADE_MODE) == "reverse":
        shade_rev_launch(pki, grad_net(imp), x_c, jinv, None, None, n, sdf, nrm, feat, fold=fold)
    else:
        lib().mp_mlp_shade(C.byref(pki.net), pki.wpack, pki.bias, x_c, jinv, None, None, n, sdf, nrm, feat, stream())
    lib().mp_mlp_color(C.byref(pkr.net), pkr.wpack, pkr.bias, x_c, nrm, feat, None, None, n, rgb, stream())
    return sdf, nrm, rgb


@functools.lru_cache(maxsize=None)
def _feat_frag_index():
    """feature index of [ks][g][e] in the colour kernel's operand-fragment order (csrc/mlp_core.hpp K permutation)"""
    idx = np.empty((8, 4, 8), dtype=np.int64)
    for ks in range(8):
        for g in range(4):
            for e in range(8):
                idx[ks, g, e] = 32 * ks + (4 * g + e if e < 4 else 16 + 4 * g + e - 4)
    return idx


def pack_feature_fragments(feat):
    """(N, 256) fp32 features -> the f16 fragment stream mp_mlp_color reads:
    [tile of 64 items][K step][16-column block][lane = column + 16 g][8 halves] (the layout k_mlp_fwdsave writes)."""
    n, dev = feat.shape[0], feat.device
    tiles = (n + 255) // 256 * 4
    f = torch.zeros(tiles * 64, 256, dtype=torch.float32, device=dev)
    f[:n] = feat
    idx = torch.from_numpy(_feat_frag_index()).to(dev)                     # (8, 4, 8)
    frag = f.reshape(tiles, 4, 16, 256)[:, :, :, idx]                      # (tile, block, j, ks, g, e)
    frag = frag.permute(0, 3, 1, 4, 2, 5).contiguous()                     # (tile, ks, block, g, j, e): lane = j + 16 g
    return frag.to(torch.float16).reshape(-1).view(torch.uint8)


def rendering_forward(net, points, normals, view_dirs, body_pose, feature_vectors, frame_latent_code):
    """RenderingNet.forward for external callers (networks.py:263-312), mode 'pose_no_view': rgb (N, 3) from canonical
    points, normals, the pose conditioning (69,) and (N, 256) feature vectors, through mp_mlp_color (features are rounded to
    f16 operands like everywhere on the inference path).  The background network ('nerf_frame_encoding') exists only fused
    into mp_background (its inputs never leave the kernel): a standalone call raises."""
    require_device()
    if net.mode != "pose_no_view":
        raise NotImplementedError("the background RenderingNet is evaluated inside mp_background only (hip.background)")
    x = points.detach().float().reshape(-1, 3).contiguous()
    nrm = normals.detach().float().reshape(-1, 3).contiguous()
    n = x.shape[0]
    cond_vec = body_pose.detach().float().reshape(-1).contiguous()
    pk = packed(net, "color", 2)
    pk.refresh(pose_embed(net)(cond_vec))
    frag = pack_feature_fragments(feature_vectors.detach().float().reshape(n, -1))
    rgb = torch.empty(n, 3, dtype=torch.float32, device=x.device)
    lib().mp_mlp_color(C.byref(pk.net), pk.wpack, pk.bias, x, nrm, frag, None, None, n, rgb, stream())
    return rgb


def background(bg_imp, bg_ren, dirs, cam, z_bg, frame_code, radius=3.0, fold=False):
    """bg_rgb (R,3) of the NeRF++ background branch. z_bg: (n_bg,) shared or (R,n_bg) per-ray inverse depths, descending.
    fold: the feature fold the renderer uses (FoldedColor, mp_background_fold)."""
    require_device()
    dirs = dirs.detach().float().contiguous()
    cam = cam.detach().float().contiguous()
    z_bg = z_bg.detach().float().contiguous()
    code = frame_code.detach().float().reshape(-1).contiguous()
    pki = packed(bg_imp, "sdf" if fold else "full", 3)
    pki.refresh(code)
    if fold:
        pkr = folded_color(bg_ren, bg_imp, 3).refresh(code)
    else:
        pkr = packed(bg_ren, "color", 3)
        pkr.refresh(code)
    R = dirs.shape[0]
    if z_bg.shape[-1] != 32:
        raise NotImplementedError("the fused background kernel is specialised for the 32 inverse-sphere samples of the shipped "
                                  f"configs (N_samples_inverse_sphere), got {z_bg.shape[-1]}")
    out = torch.empty(R, 3, dtype=torch.float32, device=dirs.device)
    fn = lib().mp_background_fold if fold else lib().mp_background
    fn(C.byref(pki.net), pki.wpack, pki.bias, C.byref(pkr.net), pkr.wpack, pkr.bias, dirs, cam, z_bg, int(z_bg.dim() == 2), R,
       radius, out, stream())
    return out


# ------------------------------------------------------------------------------------------------ mesh fit (csrc/fit.hip)
def fit_area_cdf(face_verts):
    """face_verts (F,3,3) -> area (F,), unit normal (F,3), inclusive area CDF (F,) normalised to 1 (mp_fit_area_cdf)"""
    require_device()
    fv = face_verts.detach().float().reshape(-1, 3, 3).contiguous()
    F, dev = fv.shape[0], fv.device
    area = torch.empty(F, dtype=torch.float32, device=dev)
    normal = torch.empty(F, 3, dtype=torch.float32, device=dev)
    cdf = torch.empty(F, dtype=torch.float32, device=dev)
    lib().mp_fit_area_cdf(fv, F, area, normal, cdf, stream())
    return area, normal, cdf


def fit_sample(face_verts, normal, cdf, u_surf, z_near, sigma_local, u_box, box, out=None):
    """One iteration's points of the mesh fit (mp_fit_sample).  u_surf (n_s,3) uniforms, z_near (n_near,3) standard normals,
    u_box (n_v - n_near,3) uniforms, box (2,3) = lo, hi.  Returns pts (n_s + n_v,3) -- surface points first, then the volume
    points, one tensor so that the network reads them in place --, the surface normals (n_s,3) and the face ids (n_s,) int32.
    out: (pts, normals, face_id) tensors of a previous call to write into."""
    n_s, n_near, n_box = u_surf.shape[0], z_near.shape[0], u_box.shape[0]
    n_v, dev = n_near + n_box, face_verts.device
    if out is None:
        out = (torch.empty(n_s + n_v, 3, dtype=torch.float32, device=dev), torch.empty(n_s, 3, dtype=torch.float32, device=dev),
               torch.empty(n_s, dtype=torch.int32, device=dev))
    pts, nrm, fid = out
    assert pts.shape[0] == n_s + n_v and nrm.shape[0] == n_s and fid.dtype == torch.int32
    lib().mp_fit_sample(face_verts, normal, cdf, cdf.shape[0], u_surf if n_s else None, n_s, z_near if n_near else None, n_near,
                        sigma_local, u_box if n_box else None, box, n_v, pts, nrm, fid, C.c_void_p(pts.data_ptr() + 12 * n_s),
                        stream())
    return pts, nrm, fid


def fit_loss(sdf, grad, normals, dist, weights, truncation=0.0, out=None):
    """The fit's objective and its adjoints in one launch (mp_fit_loss).  sdf (>= n,), grad (n,3): the network on the n_s surface
    points followed by the n_v volume points; normals (n_s,3); dist (n_v,); weights = (surface, normal, distance, eikonal).
    Returns terms (5,) = total, surface, normal, distance, eikonal; d_sdf (n,); d_grad (n,3)."""
    n_s, n_v, dev = normals.shape[0], dist.shape[0], grad.device
    n = n_s + n_v
    assert grad.shape[0] == n and sdf.numel() >= n
    if out is None:
        out = (torch.empty(5, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev),
               torch.empty(n, 3, dtype=torch.float32, device=dev))
    terms, d_sdf, d_grad = out
    w = [float(x) for x in weights]
    lib().mp_fit_loss(sdf, grad, normals if n_s else None, dist if n_v else None, n_s, n_v, w[0], w[1], w[2], w[3],
                      float(truncation), terms, d_sdf, d_grad, stream())
    return terms, d_sdf, d_grad


# ------------------------------------------------------------------------------------------------ mesh signed distance
# 'auto' | 'index' | 'brute': the face index (csrc/mesh_index.hip) or the brute-force kernel (csrc/mesh.hip); both return the same
# bits.  MP_MESH_INDEX=0 makes brute force the default.  'auto' picks the index only where it was MEASURED to win
# (profiles/mesh_index.txt): for a CLOSED SURFACE (every edge shared by exactly two faces) of at least MESH_INDEX_MIN_FACES
# faces.  Both conditions matter: below that count brute force is faster, and on a face list that is no surface (the synthetic
# SMPL tables' `f`: triangles between near neighbours of a sorted vertex list, overlapping at random) the boxes overlap
# everywhere and the index loses (0.7 x at 13 776 faces).  A caller that cannot say whether the faces are closed gets brute force.
# The count is the same for an index that is reused (training flags, the fit) and one built for a single query
# (interpenetration_loss): the build is 65-150 us and query + build was measured ahead from the same size on.
MESH_INDEX_MODES = ("auto", "index", "brute")
MESH_INDEX_MODE = "brute" if os.environ.get("MP_MESH_INDEX", "1") == "0" else "auto"
MESH_INDEX_MIN_FACES = 2048


def mesh_index_mode(mode):
    """validates a mesh_index_mode ('auto' | 'index' | 'brute'; None = the process default) and returns it"""
    mode = MESH_INDEX_MODE if mode is None else mode
    if mode not in MESH_INDEX_MODES:
        raise ValueError(f"mesh_index_mode must be one of {MESH_INDEX_MODES}, got {mode!r}")
    return mode


_CLOSED = {}


def faces_closed(faces):
    """is the face list (F,3) (any leading 1) a closed surface?  smpl_init.mesh_is_closed on the host (one copy + one sort of the
    edges), remembered per tensor (data_ptr, _version, shape; the entry keeps the tensor alive so that its address is not reused)"""
    from .smpl_init import mesh_is_closed
    if not torch.is_tensor(faces):
        return mesh_is_closed(faces)
    key = (faces.data_ptr(), faces._version, tuple(faces.shape), str(faces.device))
    e = _CLOSED.get(key)
    if e is None:
        if len(_CLOSED) >= 64:
            _CLOSED.clear()
        e = _CLOSED[key] = (mesh_is_closed(faces), faces)
    return e[0]


def mesh_index_wanted(mode, n_faces, faces=None):
    """does `mode` ask for the index on a mesh of n_faces faces?  faces: its (F,3) vertex ids, or True / False when the caller
    knows whether they form a closed surface; 'auto' without that knowledge (None) means brute force"""
    mode = mesh_index_mode(mode)
    if mode != "auto":
        return mode == "index"
    if n_faces < MESH_INDEX_MIN_FACES or faces is None:
        return False
    if isinstance(faces, bool):
        return faces
    return faces.numel() == 3 * n_faces and faces_closed(faces)


class MeshIndex:
    """Box tree over the faces of a triangle mesh (F,3,3) for mp_mesh_index_signed_distance; built on the device without a host
    synchronisation (torch sorts the curve keys, as plumbing).  The faces are copied into the index: the source tensor may change
    or go away afterwards -- the index then still describes the mesh it was built from (see MeshIndexCache)."""

    def __init__(self, face_verts):
        fv = face_verts.detach().reshape(-1, 9).float().contiguous()
        self.n_faces, dev = fv.shape[0], fv.device
        if self.n_faces < 1:
            raise ValueError("a mesh index needs at least one face")
        L = lib()
        self.buf = torch.empty(int(L.mp_mesh_index_bytes(self.n_faces)), dtype=torch.uint8, device=dev)
        keys = torch.empty(self.n_faces, dtype=torch.int32, device=dev)
        L.mp_mesh_index_keys(fv, self.n_faces, self.buf, keys, stream())
        self.order = torch.sort(keys, stable=True).indices       # sorted slot -> face: closest() reports faces by it
        L.mp_mesh_index_build(fv, self.n_faces, self.order, self.buf, stream())

    def signed_distance(self, pts, out=None, visits=None):
        """signed distance (n,) of pts (n,3), equal to mesh_signed_distance's; visits: optional (n,2) int32 = boxes tested, faces
        evaluated per point"""
        n = pts.shape[0]
        sd = torch.empty(n, dtype=torch.float32, device=pts.device) if out is None else out
        lib().mp_mesh_index_signed_distance(pts, n, self.buf, self.n_faces, sd, visits, stream())
        return sd

    def closest(self, pts, want_face=True, want_point=True, visits=None, sort_points=None):
        """(d2 (n,), face (n,) int32 or None, q (n,3) or None) of pts (n,3): squared distance to the closest face, its id in the
        mesh the index was built from, and the closest point on it (mp_mesh_index_closest) -- the bits of mesh_closest without an
        index.  Ties go to the lower face id; a non-finite point gets (+inf, -1, NaN).  visits: optional (n,2) int32 = boxes
        tested, faces evaluated per point.  sort_points (None = MESH_CLOSEST_SORT_POINTS): query the points in Hilbert-curve order
        of the mesh's box and put the answers back (two torch sorts' worth of plumbing; the answers do not depend on it)."""
        L, n, dev = lib(), pts.shape[0], pts.device
        pts = pts.detach().float().contiguous()
        sort_points = MESH_CLOSEST_SORT_POINTS if sort_points is None else sort_points
        perm = None
        if sort_points and n > 1:
            keys = torch.empty(n, dtype=torch.int32, device=dev)
            L.mp_mesh_index_point_keys(pts, n, self.buf, keys, stream())
            perm = torch.sort(keys).indices
            pts = pts[perm].contiguous()
        d2 = torch.empty(n, dtype=torch.float32, device=dev)
        face = torch.empty(n, dtype=torch.int32, device=dev) if want_face else None
        q = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_point else None
        vis = visits if perm is None or visits is None else torch.empty_like(visits)
        L.mp_mesh_index_closest(pts, n, self.buf, self.n_faces, self.order, d2, face, q, vis, stream())
        if perm is not None:
            back = lambda t: None if t is None else torch.empty_like(t).index_copy_(0, perm, t)
            d2, face, q = back(d2), back(face), back(q)
            if visits is not None:
                visits.index_copy_(0, perm, vis)
        return d2, face, q


class MeshIndexCache:
    """Per slot (a person): the MeshIndex of the slot's face tensor, or None where the mode asks for brute force; decided and
    built again when the tensor is another tensor or was written in place, when its face list changes, or when the mode does.  The
    key is the tensors' (data_ptr, _version, shape); the entry keeps them alive, so that the address of a replaced tensor cannot
    come back with a new mesh behind the same key.  Under 'auto' a new mesh costs one host-side closedness check (faces_closed)."""

    def __init__(self):
        self.slots = {}

    @staticmethod
    def _id(t):
        return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), str(t.device), t.dtype)

    def get(self, slot, face_verts, faces=None, mode="index"):
        key = (self._id(face_verts), self._id(faces), mesh_index_mode(mode))
        e = self.slots.get(slot)
        if e is None or e[0] != key:
            use = mesh_index_wanted(mode, face_verts.numel() // 9, faces)
            e = self.slots[slot] = (key, MeshIndex(face_verts) if use else None, face_verts, faces)
        return e[1]


def mesh_signed_distance(pts, face_verts, out=None, index=None):
    """exact signed distance (negative inside) of pts (n,3) to the closed mesh face_verts (F,3,3): mp_mesh_signed_distance, or
    through a MeshIndex of the same faces (same values)"""
    if index is not None:
        assert index.n_faces == face_verts.reshape(-1, 9).shape[0], "the index was built from another mesh"
        return index.signed_distance(pts, out)
    n = pts.shape[0]
    sd = torch.empty(n, dtype=torch.float32, device=pts.device) if out is None else out
    lib().mp_mesh_signed_distance(pts, n, face_verts, face_verts.shape[0], sd, stream())
    return sd


# ------------------------------------------------------------------------------------------------ closest face, mesh metrics
# Query points in Hilbert-curve order by default?  No: measured (profiles/mesh_closest.txt, tools/mesh_index_bench.py --closest)
# at 100 000 points the ordering cuts the faces a wave evaluates to a third but not the time (2 897 against 2 934 us against 24 660
# faces, inside the spread; 11 144 against 8 969 us against 394 184): the launch is one round of waves and ends with its slowest one.  DESIGN 6g.
MESH_CLOSEST_SORT_POINTS = False


def mesh_closest(pts, face_verts, index=None, want_face=True, want_point=True):
    """(d2 (n,), face (n,) int32, q (n,3)) of pts (n,3) against the mesh face_verts (F,3,3), closed or not: squared distance to
    the closest face, that face (ties: the lower id; -1 for a non-finite point or a mesh of zero-area faces only) and the closest
    point on it.  mp_mesh_closest, or through a MeshIndex of the same faces (same bits)."""
    fv = face_verts.detach().reshape(-1, 9).float().contiguous()
    if index is not None:
        assert index.n_faces == fv.shape[0], "the index was built from another mesh"
        return index.closest(pts, want_face, want_point)
    pts = pts.detach().float().contiguous()
    n, dev = pts.shape[0], pts.device
    d2 = torch.empty(n, dtype=torch.float32, device=dev)
    face = torch.empty(n, dtype=torch.int32, device=dev) if want_face else None
    q = torch.empty(n, 3, dtype=torch.float32, device=dev) if want_point else None
    lib().mp_mesh_closest(pts, n, fv, fv.shape[0], d2, face, q, stream())
    return d2, face, q


def mesh_metric_reduce(d2, face, normals, face_normals, thresholds=()):
    """One directed set of metrics (mp_mesh_metric_reduce) from a closest-face query: (7 + T,) float64 on the device = mean
    distance, mean squared distance, max distance, mean n.n', mean |n.n'|, samples counted, samples left out (face < 0), then
    per threshold the number of samples nearer than it."""
    n, dev = d2.shape[0], face_normals.device
    T = len(thresholds)
    tau = torch.tensor([float(t) for t in thresholds], dtype=torch.float32, device=dev) if T else None
    out = torch.empty(7 + T, dtype=torch.float64, device=dev)
    lib().mp_mesh_metric_reduce(d2 if n else None, face if n else None, normals if n else None, face_normals, n,
                                face_normals.shape[0], tau, T, out, stream())
    return out


# ------------------------------------------------------------------------------------------------ image metrics (csrc/image_metrics.hip)
SSIM_TILE, SSIM_WINDOW = 32, 11      # = include/multiply_hip.h MP_SSIM_TILE; the 11 x 11 window of mp_image_ssim


def _image_args(a, b, mask):
    """shape / dtype rules of the two image entry points: a, b (N,H,W,C) float32, mask (N,H,W) bool or None"""
    if a.dim() != 4 or a.shape != b.shape or a.shape[3] not in (1, 3):
        raise ValueError(f"images must be two (N, H, W, C) tensors of one shape with C = 1 or 3, got {tuple(a.shape)} and {tuple(b.shape)}")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise TypeError(f"images must be float32, got {a.dtype} and {b.dtype}")
    if mask is not None:
        if mask.dtype != torch.bool:
            raise TypeError(f"the mask must be bool, got {mask.dtype}")
        if tuple(mask.shape) != tuple(a.shape[:3]):
            raise ValueError(f"the mask must be (N, H, W) = {tuple(a.shape[:3])}, got {tuple(mask.shape)}")
        mask = mask.contiguous().view(torch.uint8)
    return a.detach().contiguous(), b.detach().contiguous(), mask


def _image_work(N, H, W, C, dev):
    nbytes = int(lib().mp_image_work_bytes(N, H, W, C))
    if nbytes < 0:
        raise ValueError(f"images of shape {(N, H, W, C)} are beyond what the image kernels take")
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=dev)


def image_ssim(a, b, mask=None, data_range=1.0, want_map=False):
    """Per-frame SSIM sums of a, b (N,H,W,C) float32 device tensors (mp_image_ssim; definitions: image_metrics.py): (N,5) float64
    on the device = sum of the SSIM map, windows counted, the same two over the windows whose centre lies in mask (N,H,W; None =
    everywhere), windows left out for a non-finite value; and the map (N,H-10,W-10,C) float32 (NaN where left out) or None."""
    a, b, mask = _image_args(a, b, mask)
    N, H, W, Cn = a.shape
    if H < SSIM_WINDOW or W < SSIM_WINDOW:
        raise ValueError(f"SSIM needs images of at least {SSIM_WINDOW} x {SSIM_WINDOW} pixels, got {H} x {W}")
    if not (float(data_range) > 0.0 and math.isfinite(float(data_range))):
        raise ValueError(f"data_range must be a positive finite number, got {data_range}")
    out = torch.empty(N, 5, dtype=torch.float64, device=a.device)
    smap = torch.empty(N, H - 10, W - 10, Cn, dtype=torch.float32, device=a.device) if want_map else None
    lib().mp_image_ssim(a, b, mask, N, H, W, Cn, float(data_range), _image_work(N, H, W, Cn, a.device), out, smap, stream())
    return out, smap


def image_sqerr(a, b, mask=None):
    """Per-frame squared-error sums of a, b (N,H,W,C) float32 device tensors (mp_image_sqerr): (N,5) float64 on the device = sum of
    (a - b)^2 over the finite values, their number, the same two inside mask (N,H,W; None = everywhere), values left out."""
    a, b, mask = _image_args(a, b, mask)
    N, H, W, Cn = a.shape
    out = torch.empty(N, 5, dtype=torch.float64, device=a.device)
    lib().mp_image_sqerr(a, b, mask, N, H, W, Cn, _image_work(N, H, W, Cn, a.device), out, stream())
    return out


# ------------------------------------------------------------------------------------------------ pose metrics (csrc/pose_metrics.hip)
def pose_errors(pred, gt, pred_root=None, gt_root=None):
    """Per item the three mean distances of pred against gt, both (M, n, 3) float32 device tensors, with optional roots (M, 3)
    (mp_pose_errors): (M, 4) float64 on the device = plain, root-aligned (NaN without roots), Procrustes-aligned, and 0 or why the
    item is left out (1: a non-finite coordinate, all three NaN; 2: the predicted points coincide, the Procrustes value NaN)."""
    if pred.dim() != 3 or pred.shape[2] != 3 or pred.shape != gt.shape or pred.shape[1] < 1:
        raise ValueError(f"points must be two (M, n, 3) tensors of one shape with n >= 1, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise TypeError(f"points must be float32, got {pred.dtype} and {gt.dtype}")
    M, n = pred.shape[0], pred.shape[1]
    if (pred_root is None) != (gt_root is None):
        raise ValueError("roots: give both or neither")
    if pred_root is not None:
        for r in (pred_root, gt_root):
            if tuple(r.shape) != (M, 3) or r.dtype != torch.float32:
                raise ValueError(f"roots must be (M, 3) = {(M, 3)} float32, got {tuple(r.shape)} {r.dtype}")
        pred_root, gt_root = pred_root.detach().contiguous(), gt_root.detach().contiguous()
    out = torch.empty(M, 4, dtype=torch.float64, device=pred.device)
    lib().mp_pose_errors(pred.detach().contiguous(), gt.detach().contiguous(), pred_root, gt_root, M, n, out, stream())
    return out


def contact_distance(verts, faces, corr, bary, frame_start):
    """Contact distances on the bodies verts (F, P, V, 3) float32 (mp_contact_distance): faces (Nf, 3) int32; corr (m, 5) int32 =
    frame, person a, vertex, person b, face of b, sorted by frame; bary (m, 3) float32; frame_start (F + 1,) int32.  Returns
    (2 + 2 F,) float64 on the device = overall mean, m, the per-frame means (NaN for a frame without one), the per-frame counts."""
    if verts.dim() != 4 or verts.shape[3] != 3 or min(verts.shape[:3]) < 1:
        raise ValueError(f"verts must be (F, P, V, 3) with F, P, V >= 1, got {tuple(verts.shape)}")
    F, P, V = verts.shape[0], verts.shape[1], verts.shape[2]
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError(f"faces must be (Nf, 3) with Nf >= 1, got {tuple(faces.shape)}")
    if corr.dim() != 2 or corr.shape[1] != 5:
        raise ValueError(f"corr must be (m, 5), got {tuple(corr.shape)}")
    m = corr.shape[0]
    if tuple(bary.shape) != (m, 3):
        raise ValueError(f"bary must be (m, 3) = {(m, 3)}, got {tuple(bary.shape)}")
    if tuple(frame_start.shape) != (F + 1,):
        raise ValueError(f"frame_start must be (F + 1,) = {(F + 1,)}, got {tuple(frame_start.shape)}")
    if verts.dtype != torch.float32 or bary.dtype != torch.float32:
        raise TypeError(f"verts and bary must be float32, got {verts.dtype} and {bary.dtype}")
    if faces.dtype != torch.int32 or corr.dtype != torch.int32 or frame_start.dtype != torch.int32:
        raise TypeError(f"faces, corr and frame_start must be int32, got {faces.dtype}, {corr.dtype} and {frame_start.dtype}")
    out = torch.empty(2 + 2 * F, dtype=torch.float64, device=verts.device)
    work = torch.empty(F, dtype=torch.float64, device=verts.device)
    lib().mp_contact_distance(verts.detach().contiguous(), F, P, V, faces.contiguous(), faces.shape[0], corr.contiguous() if m else None,
                              bary.contiguous() if m else None, frame_start.contiguous(), m, work, out, stream())
    return out


# ------------------------------------------------------------------------------------------------ registration (csrc/registration.hip)
REG_STATE, REG_SLOT, REG_MAX_BLOCKS = 32, 40, 256       # = include/multiply_hip.h MP_REG_STATE, MP_REG_SLOT, MP_REG_MAX_BLOCKS
# indices into a state block / a slot (= the header's MP_REG_* / MP_REG_SLOT_* enums)
REG_S, REG_R, REG_T, REG_TAU2, REG_RMS, REG_ACCEPTED, REG_REJECTED, REG_LEFT_OUT = 0, 1, 10, 13, 14, 15, 16, 17
REG_ITERS, REG_FLAG, REG_STEP, REG_C, REG_BOX_LO, REG_BOX_HI, REG_RMS_PLANE = 18, 19, 20, 21, 24, 27, 30
REG_SLOT_ATA, REG_SLOT_ATR, REG_SLOT_R2, REG_SLOT_D2, REG_SLOT_ACCEPTED, REG_SLOT_REJECTED, REG_SLOT_LEFT_OUT = 0, 28, 35, 36, 37, 38, 39
REG_CONVERGED, REG_DEGENERATE = 1, 2


def reg_state(scale, R, t, box_lo, box_hi, device, tau2=math.inf):
    """a fresh state block (REG_STATE,) float64 on the device: the transform x = scale R p + t, the acceptance threshold tau2, the
    target's bounding box and, as the fixed origin c, its centre; everything else zero"""
    st = np.zeros(REG_STATE, np.float64)
    st[REG_S] = float(scale)
    st[REG_R:REG_R + 9] = np.asarray(R, np.float64).reshape(9)
    st[REG_T:REG_T + 3] = np.asarray(t, np.float64).reshape(3)
    st[REG_TAU2] = float(tau2)
    lo, hi = np.asarray(box_lo, np.float64).reshape(3), np.asarray(box_hi, np.float64).reshape(3)
    st[REG_C:REG_C + 3] = 0.5 * (lo + hi)
    st[REG_BOX_LO:REG_BOX_LO + 3], st[REG_BOX_HI:REG_BOX_HI + 3] = lo, hi
    return torch.from_numpy(st).to(device)


def _reg_check_state(state):
    if state.dtype != torch.float64 or state.numel() != REG_STATE:
        raise ValueError(f"a registration state is {REG_STATE} float64 values, got {tuple(state.shape)} {state.dtype}")


def reg_apply(pts, state, inverse=False, out=None):
    """out = s R p + t, or R^T (p - t) / s with inverse=True, for pts (n,3) float32 and the transform of the state block
    (mp_reg_apply): computed in double, rounded once"""
    _reg_check_state(state)
    pts = pts.detach().float().contiguous()
    n = pts.shape[0]
    out = torch.empty(n, 3, dtype=torch.float32, device=pts.device) if out is None else out
    lib().mp_reg_apply(pts if n else None, n, state, int(bool(inverse)), out if n else None, stream())
    return out


def reg_work(device):
    """the scratch of reg_rows (the workgroups' partial sums)"""
    return torch.empty(REG_MAX_BLOCKS * REG_SLOT, dtype=torch.float64, device=device)


def reg_rows(p, q, normals, state, slot, face=None, normals_in_source=False, work=None, mask=None):
    """One direction's pairs into `slot` ((REG_SLOT,) float64, a row of the slots tensor) (mp_reg_rows): p (n,3) in the source
    frame, q (n,3) in the target frame; normals (n,3) per pair, or with face (n,) int32 the table (F,3) those ids point into;
    normals_in_source: the normals are rotated by the state's R.  mask: optional (n,) uint8 that receives 0 accepted / 1 rejected /
    2 left out."""
    _reg_check_state(state)
    n = p.shape[0]
    assert slot.dtype == torch.float64 and slot.numel() == REG_SLOT and q.shape[0] == n
    for x in (p, q, normals):
        assert x.dtype == torch.float32
    if face is not None:
        assert face.dtype == torch.int32 and face.shape[0] == n and normals.shape[0] >= 1
    else:
        assert normals.shape[0] == n
    assert mask is None or (mask.dtype == torch.uint8 and mask.shape[0] == n)
    work = reg_work(state.device) if work is None else work
    assert work.dtype == torch.float64 and work.numel() >= REG_MAX_BLOCKS * REG_SLOT
    lib().mp_reg_rows(p if n else None, q if n else None, normals if n else None, face if n else None,
                      normals.shape[0] if face is not None else 0, int(bool(normals_in_source)), n, state, work, slot,
                      mask if n else None, stream())
    return slot


def reg_step(slots, state, similarity=False, reject=3.0, tol=1e-6):
    """One Gauss-Newton step from the sums in slots (k, REG_SLOT) float64, in place on the state block (mp_reg_step)"""
    _reg_check_state(state)
    assert slots.dtype == torch.float64 and slots.dim() == 2 and slots.shape[1] == REG_SLOT and slots.shape[0] >= 1
    lib().mp_reg_step(slots, slots.shape[0], int(bool(similarity)), float(reject), float(tol), state, stream())
    return state


def reg_fit_pairs(p, q, weights=None, similarity=False):
    """The closed-form fit of x = s R p + t to the pairs p, q (n,3) float32 with optional weights (n,) (mp_reg_fit_pairs): (16,)
    float64 on the device = s, R (9, row-major), t (3), sum of weights, pairs left out, status (0; 1: no weight; 2: the p coincide)"""
    if p.dim() != 2 or p.shape[1] != 3 or p.shape != q.shape:
        raise ValueError(f"pairs must be two (n, 3) tensors of one shape, got {tuple(p.shape)} and {tuple(q.shape)}")
    n = p.shape[0]
    p, q = p.detach().float().contiguous(), q.detach().float().contiguous()
    if weights is not None:
        if tuple(weights.shape) != (n,):
            raise ValueError(f"weights must be (n,) = {(n,)}, got {tuple(weights.shape)}")
        weights = weights.detach().float().contiguous()
    out = torch.empty(16, dtype=torch.float64, device=p.device)
    lib().mp_reg_fit_pairs(p if n else None, q if n else None, weights if n else None, n, int(bool(similarity)), out, stream())
    return out


# ------------------------------------------------------------------------------------------------ mesh simplification
# (csrc/simplify.hip; the header documents every array; multiply_amd/simplify.py sorts between these calls)
SIMPLIFY_BITS, SIMPLIFY_LANES = 21, 16


def _simplify_mesh_args(verts, faces):
    assert verts.dtype == torch.float32 and verts.dim() == 2 and verts.shape[1] == 3
    assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3
    return verts.shape[0], faces.shape[0]


def simplify_keys(verts, lo, inv_h):
    """key (V,) int64 of every vertex's cell (mp_simplify_keys): lo = three floats, inv_h = the fp32 value of 1.0f / h"""
    assert verts.dtype == torch.float32 and verts.dim() == 2 and verts.shape[1] == 3
    n = verts.shape[0]
    key = torch.empty(n, dtype=torch.int64, device=verts.device)
    lib().mp_simplify_keys(verts if n else None, n, float(lo[0]), float(lo[1]), float(lo[2]), float(inv_h), key if n else None, stream())
    return key


def simplify_count(faces, key):
    """live (F,) uint8: the three corners of the face lie in three different cells (mp_simplify_count)"""
    assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and key.dtype == torch.int64
    F, V = faces.shape[0], key.shape[0]
    live = torch.empty(F, dtype=torch.uint8, device=faces.device)
    lib().mp_simplify_count(faces if F else None, F, key if V else None, V, live if F else None, stream())
    return live


def simplify_faces(faces, cell):
    """(tri (F,3) int32 cell ids, key_lo (F,) int64, key_hi (F,) int32, live (F,) uint8) (mp_simplify_faces)"""
    assert faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3 and cell.dtype == torch.int32
    F, V, dev = faces.shape[0], cell.shape[0], faces.device
    tri = torch.empty(F, 3, dtype=torch.int32, device=dev)
    key_lo = torch.empty(F, dtype=torch.int64, device=dev)
    key_hi = torch.empty(F, dtype=torch.int32, device=dev)
    live = torch.empty(F, dtype=torch.uint8, device=dev)
    lib().mp_simplify_faces(faces if F else None, F, cell if V else None, V, tri if F else None, key_lo if F else None,
                            key_hi if F else None, live if F else None, stream())
    return tri, key_lo, key_hi, live


def simplify_first(order, key_lo, key_hi, live):
    """keep (F,) uint8: the face is live and the first of its unordered triple in the sorted order (mp_simplify_first)"""
    F = order.shape[0]
    assert order.dtype == torch.int64 and key_lo.dtype == torch.int64 and key_hi.dtype == torch.int32 and live.dtype == torch.uint8
    assert key_lo.shape[0] == F and key_hi.shape[0] == F and live.shape[0] == F
    keep = torch.zeros(F, dtype=torch.uint8, device=order.device)
    lib().mp_simplify_first(order if F else None, F, key_lo if F else None, key_hi if F else None, live if F else None,
                            keep if F else None, stream())
    return keep


def simplify_quadrics(verts, faces, keys, pair_order, pair_start, vert_order, vert_start, lo, h, lam):
    """pos (C,3) float32: every cell's representative (mp_simplify_quadrics)"""
    V, F = _simplify_mesh_args(verts, faces)
    C = keys.shape[0]
    for t in (keys, pair_order, pair_start, vert_order, vert_start):
        assert t.dtype == torch.int64
    assert pair_order.shape[0] == 3 * F and vert_order.shape[0] == V and pair_start.shape[0] == C + 1 and vert_start.shape[0] == C + 1
    pos = torch.empty(C, 3, dtype=torch.float32, device=verts.device)
    lib().mp_simplify_quadrics(verts if V else None, V, faces if F else None, F, keys if C else None, C, pair_order if F else None,
                               pair_start, vert_order if V else None, vert_start, float(lo[0]), float(lo[1]), float(lo[2]), float(h),
                               float(lam), pos if C else None, stream())
    return pos


def simplify_attr_mean(attrs, vert_order, vert_start):
    """out (C,K) float32: per cell the mean of its vertices' rows of attrs (V,K) (mp_simplify_attr_mean)"""
    assert attrs.dtype == torch.float32 and attrs.dim() == 2 and vert_order.dtype == torch.int64 and vert_start.dtype == torch.int64
    V, K = attrs.shape
    C = vert_start.shape[0] - 1
    assert vert_order.shape[0] == V
    out = torch.empty(C, K, dtype=torch.float32, device=attrs.device)
    lib().mp_simplify_attr_mean(attrs if V * K else None, V, K, vert_order if V else None, vert_start, C, out if C * K else None,
                                stream())
    return out
