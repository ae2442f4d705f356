"""Training path: layer-wise fp32 forward with stash + hand-written backward (HIP), behind one torch.autograd.Function.

Replaces what torch autograd does for the reference's training iteration (multiply_model.py:192-217 around
Multiply.forward in training mode, multiply.py:254-545): the differentiable part of the forward (SDF net in forward
mode = value + spatial tangents, colour net, compositing, background) is evaluated layer by layer with the exact-fp32
MFMA GEMMs of csrc/gemm.hip, every pre-activation is kept, and the adjoint sweep -- including the mixed second
derivatives through the normals and the eikonal term -- is the reverse pass over that forward-mode graph.
Gradients are produced for every network parameter (weight-norm g/v, biases, lin_pose), density.beta and the frame
latent code, and -- when the caller's smpl_pose / smpl_trans / smpl_shape require grad (BodyModelParams in the reference's
trainer) -- for those too, through the canonical warp, the normals' Jacobian, the pose conditioning and SMPL's bone transforms.

The non-differentiable sampler (VolSDF Algorithm 1, ray_sampler.py:81-191, `torch.no_grad()` in the reference) runs on
the fused half-precision kernels exactly like in eval mode, with the training-mode randomness drawn by torch.rand on the device.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import torch
import torch.distributed as dist

from . import hip

F32 = torch.float32
_p, _chk = hip.ptr, hip.check      # the binding's helpers under their former names: tests/test_train_gpu.py and tools/ call them; no launch here does


# Arithmetic of the training GEMMs (csrc/gemm.hip):
#   "bf16x3" (default): every fp32 operand split into two bfloat16 halves on its way into LDS, three 16-bit MFMAs per product
#            (hi.hi + hi.lo + lo.hi), fp32 accumulation: ~2^-16 relative per product, the range of fp32 (no loss scaling),
#            5x less matrix-pipe time than the exact-fp32 instruction -- the GEMMs run at the rate HBM delivers their operands;
#   "f32":   v_mfma_f32_16x16x4_f32, bitwise an fmaf chain -- the cross-check (tests/test_train_step_gpu.py runs both).
TRAIN_PRECISION = os.environ.get("MP_TRAIN_PRECISION", "bf16x3")


def gemm_nt(A, lda, B, ldb, Cm, ldc, M, N, K, bias=None, bias_rows=0, accumulate=False, relu=False):
    if TRAIN_PRECISION == "f32":
        fn = hip.lib().mp_gemm_nt
    elif TRAIN_PRECISION == "bf16x3":
        fn = hip.lib().mp_gemm_nt_bf16x3
    else:
        raise ValueError(f"MP_TRAIN_PRECISION {TRAIN_PRECISION!r}: expected 'bf16x3' or 'f32'")
    fn(A, lda, B, ldb, Cm, ldc, M, N, K, bias, bias_rows, int(accumulate), int(relu), hip.stream())


# Deterministic training mode (opt-in): every gradient of a step is a function of its inputs alone.  The four places
# where the default step adds fp32 values with atomics -- the split weight-gradient contractions (csrc/gemm.hip), the last
# layer's sums of the fused SDF / background backward (csrc/tfuse.hip), d beta of the compositing adjoints (csrc/composite.hip)
# and the canonical warp's d tfs (csrc/train.hip) -- go through the `_det` entry points instead: partial results by plain
# stores, added by a finishing kernel in a fixed order.  Switches: MP_TRAIN_DETERMINISTIC=1 (this module's default),
# model.train_deterministic = True / False (overrides it for that model's training steps), the Trainer's config key
# `deterministic`.  Off by default: with it off nothing changes.
def _env_flag(value):
    return str(value).strip().lower() not in ("", "0", "false", "no", "off")


DETERMINISTIC = _env_flag(os.environ.get("MP_TRAIN_DETERMINISTIC", "0"))
_DET = [None]            # the mode of the TrainGraph whose forward / adjoint sweep is running; None outside one: the module default
DET_WS_BYTES = 68 << 20  # the contractions' workspace: one round of the wide form is at most 256 slices x 256 KiB (+ column sums)
_DET_WS = {}             # (device, stream) -> workspace; allocated once, grown only if a larger contraction ever arrives


def deterministic(model=None):
    """is the deterministic training mode on (for `model`'s steps: model.train_deterministic, when set, wins over the default)?"""
    v = getattr(model, "train_deterministic", None) if model is not None else None
    return DETERMINISTIC if v is None else bool(v)


def _det():
    return DETERMINISTIC if _DET[0] is None else _DET[0]


def det_workspace(n_bytes):
    """the deterministic contractions' workspace on the current device and stream (calls on one stream run in order, so they share it)"""
    key = (torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    ws = _DET_WS.get(key)
    if ws is None or 4 * ws.numel() < n_bytes:
        ws = _DET_WS[key] = torch.empty(max(int(n_bytes), DET_WS_BYTES) // 4 + 4, dtype=F32, device="cuda")
    return ws


def det_workspace_bytes():
    """bytes the deterministic mode holds in workspaces (all devices and streams)"""
    return sum(4 * ws.numel() for ws in _DET_WS.values())


def release_det_workspace():
    _DET_WS.clear()


def _in_graph_mode(fn):
    """TrainGraph method decorator: the graph's own mode holds while its forward / adjoint sweep runs"""
    def wrapped(self, *a, **k):
        prev, _DET[0] = _DET[0], self.det
        try:
            return fn(self, *a, **k)
        finally:
            _DET[0] = prev
    wrapped.__name__, wrapped.__doc__ = fn.__name__, fn.__doc__
    return wrapped


def _part(query, n):
    """scratch for the partial sums of a deterministic launch: `query(n, &floats)` floats"""
    need = C.c_longlong()
    query(n, C.byref(need))
    return torch.empty(max(int(need.value), 4), dtype=F32, device="cuda")


def tf_bwd(kind, wpack, w8, arena, P, dfeat, dsdf, dw8, db8):
    """mp_tf_sdf_bwd / mp_tf_bg_bwd (kind 'sdf' | 'bg'), or their deterministic forms"""
    L, st = hip.lib(), hip.stream()
    assert kind in ("sdf", "bg")
    if _det():
        part = _part(L.mp_tf_bwd_part_floats, P)
        if kind == "sdf":
            L.mp_tf_sdf_bwd_det(wpack, w8, arena, P, dfeat, dsdf, dw8, db8, part, st)
        else:
            L.mp_tf_bg_bwd_det(wpack, w8, arena, P, dfeat, dsdf, dw8, db8, part, st)
    elif kind == "sdf":
        L.mp_tf_sdf_bwd(wpack, w8, arena, P, dfeat, dsdf, dw8, db8, st)
    else:
        L.mp_tf_bg_bwd(wpack, w8, arena, P, dfeat, dsdf, dw8, db8, st)


def warp_bwd(xc, dxc, jinv, djinv, nn_posed, nn_cano, n, skin_w, tfs, dtfs):
    """mp_tr_warp_bwd, or its deterministic form"""
    L, st = hip.lib(), hip.stream()
    if _det():
        L.mp_tr_warp_bwd_det(xc, dxc, jinv, djinv, nn_posed, nn_cano, n, skin_w, tfs, dtfs, _part(L.mp_tr_warp_bwd_part_floats, n), st)
    else:
        L.mp_tr_warp_bwd(xc, dxc, jinv, djinv, nn_posed, nn_cano, n, skin_w, tfs, dtfs, st)


def gemm_tn(A, lda, B, ldb, Cm, ldc, M, N, K, colsum=None, colsum_rows=0):
    """Cm[M,N] += A[K,M]^T B[K,N];  colsum[M] += column sums of A's first colsum_rows rows (the bias gradient)"""
    if _det():
        return _gemm_tn_det(A, lda, B, ldb, Cm, ldc, M, N, K, colsum, colsum_rows)
    fn = hip.lib().mp_gemm_tn if TRAIN_PRECISION == "f32" else hip.lib().mp_gemm_tn_bf16x3
    fn(A, lda, B, ldb, Cm, ldc, M, N, K, colsum, colsum_rows, hip.stream())


def _gemm_tn_det(A, lda, B, ldb, Cm, ldc, M, N, K, colsum, colsum_rows):
    """gemm_tn in the deterministic mode: the workspace the size query asks for, then the `_det` entry point"""
    need = C.c_longlong()
    hip.lib().mp_gemm_tn_ws_bytes(M, N, K, int(TRAIN_PRECISION != "f32"), C.byref(need))
    ws = det_workspace(need.value)
    if TRAIN_PRECISION == "f32":
        hip.lib().mp_gemm_tn_det(A, lda, B, ldb, Cm, ldc, M, N, K, colsum, colsum_rows, ws, 4 * ws.numel(), hip.stream())
    else:
        hip.lib().mp_gemm_tn_bf16x3_det(A, lda, B, ldb, Cm, ldc, M, N, K, colsum, colsum_rows, ws, 4 * ws.numel(), hip.stream())


class MpTnGroup(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p), ("colsum", C.c_void_p), ("lda", C.c_int),
                ("ldb", C.c_int), ("ldc", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("colsum_rows", C.c_int),
                ("pad_", C.c_int)]


def tn_group(A, lda, B, ldb, Cm, ldc, M, N, K, colsum=None, colsum_rows=0):
    """one contraction of a grouped launch (mp_gemm_tn_bf16x3_grouped); pointers as returned by hip.ptr() / off()"""
    return MpTnGroup(A.value, B.value, Cm.value, colsum.value if colsum is not None else None, lda, ldb, ldc, M, N, K,
                     colsum_rows, 0)


def gemm_tn_grouped(groups):
    """all weight-gradient contractions of `groups` in ONE launch (aligned 128-multiples only); chunks of 24"""
    for i in range(0, len(groups), 24):
        chunk = groups[i:i + 24]
        arr = (MpTnGroup * len(chunk))(*chunk)
        if _det():
            need = C.c_longlong()
            hip.lib().mp_gemm_tn_grouped_ws_bytes(arr, len(chunk), C.byref(need))
            ws = det_workspace(need.value)
            hip.lib().mp_gemm_tn_bf16x3_grouped_det(arr, len(chunk), ws, 4 * ws.numel(), hip.stream())
            continue
        hip.lib().mp_gemm_tn_bf16x3_grouped(arr, len(chunk), hip.stream())


def _big_empty(n_floats, dev, grain=1 << 26, cap=None, cap_bytes=6 << 30):
    """fp32 scratch of at least n_floats, allocated in multiples of `grain` floats (256 MiB).  The per-iteration stashes are
    gigabytes whose exact size follows the number of rays that hit each body, i.e. changes every iteration: an exact-size
    request misses torch's caching allocator whenever it exceeds every cached block, and a fresh hipMalloc of 3 GB stalls the
    host for milliseconds (measured: 520 torch.empty calls = 12 ms of host time per iteration, nearly all of it in the two
    arena allocations).  A few coarse sizes are cached after the first iterations and always hit.  cap (floats): an upper bound of
    every request of this call site; when it is affordable (<= cap_bytes) it is what is allocated -- one size for good, so that no
    later iteration with a few more hit rays pays a fresh hipMalloc inside a timed region."""
    if cap is not None and n_floats <= cap and 4 * cap <= cap_bytes:
        n_floats = cap
    return torch.empty((n_floats + grain - 1) // grain * grain, dtype=F32, device=dev)


_ZP = [None]          # the running adjoint sweep's hip.ZeroPool (TrainGraph.backward); None outside a sweep


def _zeros(*shape, device):
    """zero-initialised fp32 tensor: a view of the sweep's zero-filled block when a sweep is running, else a fill of its own"""
    zp = _ZP[0]
    if zp is not None and zp.device == torch.device(device):
        return zp.take(*shape)
    return torch.zeros(*shape, dtype=F32, device=device)


def off(t, n_floats):
    """device pointer `n_floats` floats into tensor t"""
    return C.c_void_p(t.data_ptr() + 4 * n_floats)


class LinW:
    """effective fp32 weights of one nn.Linear (weight-norm resolved), its transpose, and gradient buffers"""

    def __init__(self, lin):
        self.lin = lin
        self.wn = hasattr(lin, "weight_g")
        self.v = (lin.weight_v if self.wn else lin.weight).detach().contiguous()
        self.g = lin.weight_g.detach().reshape(-1).contiguous() if self.wn else None
        self.b = lin.bias.detach().contiguous()
        self.out_dim, self.in_dim = self.v.shape
        dev = self.v.device
        self.W = torch.empty(self.out_dim, self.in_dim, dtype=F32, device=dev)
        self.WT = torch.empty(self.in_dim, self.out_dim, dtype=F32, device=dev)
        hip.lib().mp_tr_wn_fwd(self.v, self.g, self.out_dim, self.in_dim, self.W, self.WT, hip.stream())
        self.dW = torch.zeros(self.out_dim, self.in_dim, dtype=F32, device=dev)
        self.db = torch.zeros(self.out_dim, dtype=F32, device=dev)

    def param_grads(self):
        """gradients in the order of `params()`"""
        dv = torch.empty_like(self.v)
        dg = torch.empty(self.out_dim, 1, dtype=F32, device=self.v.device) if self.wn else None
        hip.lib().mp_tr_wn_bwd(self.v, self.g, self.out_dim, self.in_dim, self.dW, dv, dg if self.wn else None, hip.stream())
        return [dg, dv, self.db] if self.wn else [dv, self.db]

    def params(self):
        lin = self.lin
        return [lin.weight_g, lin.weight_v, lin.bias] if self.wn else [lin.weight, lin.bias]


class _NetParams:
    """parameters and their gradients of a network evaluated for training, in matching order: `extra_*` (the colour net's lin_pose)
    first, then every layer"""
    extra_params = extra_grads = ()

    def params(self):
        return list(self.extra_params) + [p for lw in self.lins for p in lw.params()]

    def param_grads(self):
        return list(self.extra_grads) + [g for lw in self.lins for g in lw.param_grads()]


def launch_tn_groups(groups):
    """the deferred aligned weight-gradient contractions of one network or person (tn_group records) in one grouped launch"""
    if TRAIN_PRECISION == "bf16x3":
        gemm_tn_grouped(groups)
    else:                                   # exact-fp32 cross-check: one launch per contraction
        for g in groups:
            gemm_tn(g.A, g.lda, g.B, g.ldb, g.C, g.ldc, g.M, g.N, g.K, g.colsum, g.colsum_rows)


def _layer0_adjoint(lw0, dZ0, X0, ldx, kx, rows, bias_rows, c0, n_h, hvec):
    """Layer 0 of a network whose conditioning is hoisted into the bias (b0 = b + W0[:, c0:c0+n_h] hvec): the weight gradient
    dW0[:, :kx] += dZ0^T X0 over `rows` rows, the bias gradient over the first `bias_rows`, dW0[:, c0:c0+n_h] += db0 (x) hvec;
    returns d hvec = W0[:, c0:c0+n_h]^T db0.  dZ0 [rows][out], X0 [rows][ldx]: tensors or device pointers."""
    out, dev = lw0.out_dim, lw0.W.device
    # layer 0's bias gradient of THIS evaluation on its own (db0), then added to the accumulator: the hoisted
    # conditioning's adjoint below must not see what other evaluations of the same network left in lw0.db
    # (the zero-pose regulariser evaluates a network under two conditionings in one sweep)
    db0 = _zeros(out, device=dev)
    gemm_tn(dZ0, out, X0, ldx, lw0.dW, lw0.in_dim, out, kx, rows, db0, bias_rows)
    lw0.db.add_(db0)
    hip.lib().mp_tr_hoist_bwd(db0, out, lw0.in_dim, c0, n_h, hvec, lw0.dW, hip.stream())
    dh = _zeros(n_h, device=dev)
    gemm_tn(db0, 1, off(lw0.W, c0), lw0.in_dim, dh, n_h, 1, n_h, out)
    return dh


# ----------------------------------------------------------------------------------------------------------------------
# An SDF-type network (foreground ImplicitNet, background ImplicitNet) evaluated for training.  Four evaluators, ONE surface:
#   .P                    points;  .lins  the layers (LinW / LinP)
#   .sdf [>= P]           column 0 of the reference's output, contiguous
#   .feat_ptr, .feat_ld   columns 1..256: device pointer to row 0 and the row stride (the colour net reads them in place)
#   .grad [P][3] | None   d sdf / d x, where the evaluator differentiates in space
#   new_dfeat(n)          the features' adjoint as THIS evaluator wants it delivered: a tensor in the evaluator's own layout, rows
#                         [0, n) to be filled by a colour net, the others zero;  dfeat_target(dfeat) -> (pointer, leading
#                         dimension, accumulate) for that colour net's backward (accumulate: it ADDS into a zeroed buffer;
#                         else it WRITES its rows).  Layer-wise evaluators: the reference's [rows][257] adjoint, features in
#                         columns 1..; fused ones: their own [P][256] matrix.
#   backward(dfeat, dsdf [P], dgrad [P][3] | None, want_dx=False, tn_groups=None) -> d cond
#                         accumulates dW / db of every layer.  want_dx: also self.dx [P][d_in], the adjoint of the points.
#                         tn_groups (a list): an evaluator with aligned weight-gradient contractions appends them instead of
#                         launching them (the caller: launch_tn_groups); the layer-wise ones launch their own.
#                         Layer-wise evaluators also take dsdf / dgrad = None: the caller has written column 0 of dfeat itself.
#   params(), param_grads()
# sdf_evaluator() / bg_evaluator() choose among them.
# ----------------------------------------------------------------------------------------------------------------------
class _SdfEvaluator(_NetParams):
    def dfeat_target(self, dfeat):
        """where a colour net's backward delivers the features' adjoint inside this evaluator's new_dfeat() tensor"""
        return off(dfeat, self.dfeat_col0), dfeat.shape[1], self.dfeat_accumulate


class _LayerwiseImplicit(_SdfEvaluator):
    """The ImplicitNet's value sweep layer by layer with every pre-activation kept, and its adjoint: shared by ImplicitTrain
    (4P rows in forward mode: the tangent rows ride through mp_tr_softplus_fwd / _bwd) and ImplicitTrainRev (P rows; sigma''
    enters the adjoint through dS, mp_tr_dz).  self.out [rows][257] is the reference's layout: column 0 = sdf."""
    feat_ld = 257
    dfeat_col0, dfeat_accumulate = 1, True

    def _value_sweep(self, net, x, cond_vec, fwd, lins):
        L, st = hip.lib(), hip.stream()
        self.net, self.fwd, self.x, self.cond = net, fwd, x, cond_vec
        dev = x.device
        self.P = P = x.shape[0]
        self.rows = rows = 4 * P if fwd else P
        self.E = E = net.embed_dim
        self.lins = lins if lins is not None else [LinW(l) for l in net.layers()]
        self.IN = torch.empty(rows, E, dtype=F32, device=dev)
        L.mp_tr_pe(x, net.d_in, P, net.multires, int(fwd), 1.0, self.IN, E, 0, st)
        self.Z, self.X = [], []          # pre-activations and layer inputs
        r2 = 1.0 / math.sqrt(2.0)
        Pm = P if fwd else 0
        for l, lw in enumerate(self.lins):
            out = lw.out_dim
            Z = torch.empty(rows, out, dtype=F32, device=dev)
            if l == 0:
                self.b0 = torch.empty(out, dtype=F32, device=dev)
                L.mp_tr_hoist_fwd(lw.W, out, lw.in_dim, lw.b, E, net.cond_dim, cond_vec, self.b0, st)
                Xl = self.IN
                gemm_nt(Xl, E, lw.W, lw.in_dim, Z, out, rows, out, E, self.b0, P)
            else:
                Zp, po = self.Z[l - 1], self.lins[l - 1].out_dim
                skip = l in net.skip_in
                Xl = torch.empty(rows, po + E if skip else po, dtype=F32, device=dev)
                L.mp_tr_softplus_fwd(Zp, po, rows, po, Pm, r2 if skip else 1.0, Xl, Xl.shape[1], 0, st)
                if skip:
                    L.mp_tr_copy_cols(self.IN, E, 0, Xl, po + E, po, rows, E, r2, 0, st)
                gemm_nt(Xl, Xl.shape[1], lw.W, lw.in_dim, Z, out, rows, out, lw.in_dim, lw.b, P)
            self.Z.append(Z)
            self.X.append(Xl)
        self.out = self.Z[-1]            # [rows][257]
        self.feat_ptr = off(self.out, 1)
        self.sdf = torch.empty(P, dtype=F32, device=dev)
        L.mp_tr_copy_cols(self.out, 257, 0, self.sdf, 1, 0, P, 1, 1.0, 0, st)

    def new_dfeat(self, n=0):
        return torch.zeros(self.rows, 257, dtype=F32, device=self.x.device)

    def _value_adjoint(self, dZ, dS=None, want_dx=False, grouped=False):
        """dZ [rows][257]: the last layer's adjoint -> dW / db of every layer; returns d cond (hoisted conditioning adjoint).
        dS[l] (reverse-over-reverse): the gradient sweep's adjoint w.r.t. sigma'(Z_l).  want_dx: adds the points' adjoint to
        self.dx [P][d_in] (created here unless the caller's own sweep already did).  grouped: the 256 x 256 weight gradients in
        one grouped launch."""
        L, st = hip.lib(), hip.stream()
        net, rows, P, E = self.net, self.rows, self.P, self.E
        dev = dZ.device
        Pm = P if self.fwd else 0
        r2 = 1.0 / math.sqrt(2.0)
        dIN = torch.zeros(rows, E, dtype=F32, device=dev) if want_dx else None
        # the 256 x 256 weight gradients wait for ONE grouped launch at the end (six small contractions launched one by one
        # cost 64 us each; their operands stay alive in `held`)
        groups, held = [], []
        for l in range(len(self.lins) - 1, 0, -1):
            lw, Xl = self.lins[l], self.X[l]
            out, po = lw.out_dim, self.lins[l - 1].out_dim
            if grouped and TRAIN_PRECISION == "bf16x3" and out == 256 and lw.in_dim == 256:
                groups.append(tn_group(hip.ptr(dZ), out, hip.ptr(Xl), 256, hip.ptr(lw.dW), lw.in_dim, out, 256, rows,
                                       hip.ptr(lw.db), P))
                held.append(dZ)
            else:
                gemm_tn(dZ, out, Xl, lw.in_dim, lw.dW, lw.in_dim, out, lw.in_dim, rows, lw.db, P)
            dX = torch.empty(rows, lw.in_dim, dtype=F32, device=dev)
            gemm_nt(dZ, out, lw.WT, out, dX, lw.in_dim, rows, lw.in_dim, out)
            skip = l in net.skip_in
            if want_dx and skip:      # the skip connection's copy of the encoded input
                L.mp_tr_copy_cols(dX, lw.in_dim, po, dIN, E, 0, rows, E, r2, 1, st)
            dZp = torch.empty(rows, po, dtype=F32, device=dev)
            scale = r2 if skip else 1.0
            if dS is None:
                L.mp_tr_softplus_bwd(self.Z[l - 1], po, rows, po, Pm, scale, dX, lw.in_dim, 0, dZp, po, st)
            else:
                L.mp_tr_dz(self.Z[l - 1], po, P, po, dX, lw.in_dim, scale, dS[l - 1], po, dZp, po, st)
            dZ = dZp
        lw0 = self.lins[0]
        dcond = _layer0_adjoint(lw0, dZ, self.IN, E, E, rows, P, E, net.cond_dim, self.cond)
        if want_dx:
            gemm_nt(dZ, lw0.out_dim, lw0.WT, lw0.out_dim, dIN, E, rows, E, lw0.out_dim, accumulate=True)
            if self.dx is None:
                self.dx = torch.zeros(P, net.d_in, dtype=F32, device=dev)
            L.mp_tr_pe_bwd(self.x, net.d_in, P, net.multires, int(self.fwd), dIN, E, self.dx, st)
        if groups:
            gemm_tn_grouped(groups)
        return dcond

    def _dsdf_into(self, dZ, dsdf):
        """d sdf -> column 0 of the value rows of dZ [rows][257]"""
        hip.lib().mp_tr_copy_cols(dsdf, 1, 0, dZ, 257, 0, self.P, 1, 1.0, 0, hip.stream())


class ImplicitTrain(_LayerwiseImplicit):
    """ImplicitNet (networks.py:126-208) evaluated layer by layer for P points; fwd=True: in FORWARD mode, three tangent row blocks
    below the P value rows carry d / d x_k through every layer (self.out [4P][257]), gathered into self.grad [P][3]."""

    def __init__(self, net, x, cond_vec, fwd, lins=None):
        self._value_sweep(net, x, cond_vec, fwd, lins)
        self.grad = None
        if fwd:
            L, P = hip.lib(), self.P
            self.grad = torch.empty(P, 3, dtype=F32, device=x.device)
            for k in range(3):           # column 0 of tangent block k
                L.mp_tr_copy_cols(off(self.out, (k + 1) * P * 257), 257, 0, self.grad, 3, k, P, 1, 1.0, 0, hip.stream())

    def backward(self, dfeat, dsdf=None, dgrad=None, want_dx=False, tn_groups=None):
        L, P, dZ = hip.lib(), self.P, dfeat
        assert dZ.shape == (self.rows, 257) and (dgrad is None or self.fwd)
        if dsdf is not None:
            self._dsdf_into(dZ, dsdf)
        if dgrad is not None:
            for k in range(3):
                L.mp_tr_copy_cols(dgrad, 3, k, off(dZ, (k + 1) * P * 257), 257, 0, P, 1, 1.0, 0, hip.stream())
        self.dx = None
        return self._value_adjoint(dZ, want_dx=want_dx, grouped=True)


class ImplicitTrainRev(_LayerwiseImplicit):
    """Foreground ImplicitNet for P points with d sdf / d x by REVERSE-over-reverse differentiation:

        forward   Z_l = X_l W_l^T + b_l,  X_{l+1} = softplus(Z_l)                       (value only, P rows)
        sweep     V_7 = s_7 (.) W_8[sdf row];  U_{l-1} = V_l W_l;  V_{l-1} = s_{l-1} (.) U_{l-1};  grad = J_PE^T (V_0 W_0in + ...)
        backward  the adjoint of BOTH sweeps (sigma'' enters through d s_l = U_l (.) dV_l)

    = what torch autograd does for the reference (multiply.py:643-659 with create_graph=True): 6 GEMMs per layer over P
    rows, where the forward-mode class above spends 3 GEMMs over 4P rows.  Same results, same parameter gradients.
    The value sweep and its adjoint are _LayerwiseImplicit's; this class adds the gradient sweep and that sweep's adjoint.
    Yields the adjoint of the input points (pose optimisation); the default evaluator for it (SDF_POSE_GRAD_MODE)."""

    def __init__(self, net, x, cond_vec, lins=None):
        L = hip.lib()
        st = hip.stream()
        assert net.d_in == 3 and len(net.skip_in) == 1
        self._value_sweep(net, x, cond_vec, False, lins)
        lins, P, E = self.lins, self.P, self.E
        self.nl = nl = len(lins)
        r2 = 1.0 / math.sqrt(2.0)
        f32 = dict(dtype=F32, device=x.device)
        # ---- reverse sweep for d sdf / d x
        nh = nl - 1                                   # hidden layers 0..nh-1
        self.w8 = lins[nh].W[0].contiguous()          # sdf row of the last layer
        self.V = [None] * nh
        self.T = [None] * nh                          # T[l] = V_l W_l  (U_{l-1} = scale_l * T[l][:, :out_{l-1}])
        self.V[nh - 1] = torch.empty(P, lins[nh - 1].out_dim, **f32)
        L.mp_tr_sigmul(self.Z[nh - 1], lins[nh - 1].out_dim, P, lins[nh - 1].out_dim, None, 0, self.w8, 1.0, self.V[nh - 1],
                       lins[nh - 1].out_dim, st)
        self.Gpe = torch.zeros(P, E, **f32)
        for l in range(nh - 1, 0, -1):
            lw, po = lins[l], lins[l - 1].out_dim
            T = torch.empty(P, lw.in_dim, **f32)
            gemm_nt(self.V[l], lw.out_dim, lw.WT, lw.out_dim, T, lw.in_dim, P, lw.in_dim, lw.out_dim)
            sc = r2 if l in net.skip_in else 1.0
            if l in net.skip_in:
                L.mp_tr_copy_cols(T, lw.in_dim, po, self.Gpe, E, 0, P, E, r2, 1, st)
            self.T[l] = T
            self.V[l - 1] = torch.empty(P, po, **f32)
            L.mp_tr_sigmul(self.Z[l - 1], po, P, po, T, lw.in_dim, None, sc, self.V[l - 1], po, st)
        lw0 = lins[0]
        gemm_nt(self.V[0], lw0.out_dim, lw0.WT, lw0.out_dim, self.Gpe, E, P, E, lw0.out_dim, accumulate=True)
        self.grad = torch.empty(P, 3, **f32)
        L.mp_tr_pe_grad_fwd(x, P, net.multires, self.Gpe, E, self.grad, st)

    def backward(self, dfeat, dsdf, dgrad, want_dx=False, tn_groups=None):
        L = hip.lib()
        st = hip.stream()
        net, P, E, lins = self.net, self.P, self.E, self.lins
        nh = self.nl - 1
        dZ = dfeat
        assert dZ.shape == (P, 257)
        f32 = dict(dtype=F32, device=dZ.device)
        r2 = 1.0 / math.sqrt(2.0)
        if dsdf is not None:
            self._dsdf_into(dZ, dsdf)
        # ---- adjoint of the reverse sweep (ascending l)
        dGpe = torch.empty(P, E, **f32)
        self.dx = torch.zeros(P, 3, **f32) if want_dx else None
        L.mp_tr_pe_grad_bwd(self.x, P, net.multires, dgrad, self.Gpe, E, dGpe, E, self.dx, st)
        lw0 = lins[0]
        dV = torch.empty(P, lw0.out_dim, **f32)
        gemm_nt(dGpe, E, lw0.W, lw0.in_dim, dV, lw0.out_dim, P, lw0.out_dim, E)
        gemm_tn(self.V[0], lw0.out_dim, dGpe, E, lw0.dW, lw0.in_dim, lw0.out_dim, E, P)
        dS = [None] * nh
        for l in range(0, nh - 1):
            lw1 = lins[l + 1]
            out_l = lins[l].out_dim
            sc = r2 if (l + 1) in net.skip_in else 1.0
            dU = torch.empty(P, out_l, **f32)
            dS[l] = torch.empty(P, out_l, **f32)
            L.mp_tr_rev_adj(self.Z[l], out_l, P, out_l, self.T[l + 1], lw1.in_dim, None, sc, dV, out_l, dU, out_l, dS[l], out_l,
                            st)
            if (l + 1) in net.skip_in:
                dT = torch.empty(P, lw1.in_dim, **f32)
                L.mp_tr_copy_cols(dU, out_l, 0, dT, lw1.in_dim, 0, P, out_l, r2, 0, st)
                L.mp_tr_copy_cols(dGpe, E, 0, dT, lw1.in_dim, out_l, P, E, r2, 0, st)
            else:
                dT = dU
            dV = torch.empty(P, lw1.out_dim, **f32)
            gemm_nt(dT, lw1.in_dim, lw1.W, lw1.in_dim, dV, lw1.out_dim, P, lw1.out_dim, lw1.in_dim)
            gemm_tn(self.V[l + 1], lw1.out_dim, dT, lw1.in_dim, lw1.dW, lw1.in_dim, lw1.out_dim, lw1.in_dim, P)
        # top of the sweep: V_7 = s_7 (.) W_8[sdf row]
        top = lins[nh - 1].out_dim
        dU = torch.empty(P, top, **f32)
        dS[nh - 1] = torch.empty(P, top, **f32)
        L.mp_tr_rev_adj(self.Z[nh - 1], top, P, top, None, 0, self.w8, 1.0, dV, top, dU, top, dS[nh - 1], top, st)
        dw8 = torch.empty(top, **f32)
        L.mp_tr_colsum(dU, top, P, top, dw8, st)
        lins[nh].dW[0] += dw8
        # ---- adjoint of the value sweep (descending l)
        return self._value_adjoint(dZ, dS, want_dx=want_dx)


class MpWnDesc(C.Structure):
    _fields_ = [("v", C.c_void_p), ("g", C.c_void_p), ("W", C.c_void_p), ("WT", C.c_void_p), ("dW_off", C.c_longlong),
                ("dv_off", C.c_longlong), ("dg_off", C.c_longlong), ("out_dim", C.c_int), ("in_dim", C.c_int), ("row0", C.c_int),
                ("pad_", C.c_int)]


class LinP(LinW):
    """LinW with PERSISTENT effective weights (W, optionally the transpose WT) and, under a TrainState, gradient accumulators /
    parameter gradients that are views of the iteration's two flat buffers (one fill, one batched weight-norm launch per group
    instead of two launches per layer).  Standalone (no TrainState): refresh() resolves the weight norm and zeroes its own
    accumulators, param_grads() runs the per-layer adjoint like LinW."""

    def __init__(self, lin, pad_rows=0, need_wt=False, standalone=True):
        """pad_rows: gradient accumulators of max(out_dim, pad_rows) rows (a 217-row layer contracted as 256 rows takes the
        aligned path of mp_gemm_tn; the extra rows receive exact zeros and are never read)"""
        self.lin = lin
        self.wn = hasattr(lin, "weight_g")
        v = lin.weight_v if self.wn else lin.weight
        self.out_dim, self.in_dim = v.shape
        dev = v.device
        self.W = torch.empty(self.out_dim, self.in_dim, dtype=F32, device=dev)
        self.WT = torch.empty(self.in_dim, self.out_dim, dtype=F32, device=dev) if need_wt else None
        self.rows = max(self.out_dim, pad_rows)
        self.standalone = standalone
        self._g = None
        self.read_params()
        if standalone:
            self.dW_full = torch.zeros(self.rows, self.in_dim, dtype=F32, device=dev)
            self.db_full = torch.zeros(self.rows, dtype=F32, device=dev)
            self.dW, self.db = self.dW_full[:self.out_dim], self.db_full[:self.out_dim]
            self.refresh()

    def read_params(self):
        lin = self.lin
        self.v = (lin.weight_v if self.wn else lin.weight).detach().contiguous()
        self.g = lin.weight_g.detach().reshape(-1).contiguous() if self.wn else None
        self.b = lin.bias.detach().contiguous()

    def refresh(self):
        self.read_params()
        hip.lib().mp_tr_wn_fwd(self.v, self.g, self.out_dim, self.in_dim, self.W, self.WT, hip.stream())
        self.dW_full.zero_()
        self.db_full.zero_()

    def bind(self, acc, o_dW, o_db, gbuf, o_dv, o_dg):
        """this iteration's accumulators / gradients: views of the flat buffers (TrainState.begin)"""
        n = self.rows * self.in_dim
        self.dW_full = acc[o_dW:o_dW + n].view(self.rows, self.in_dim)
        self.db_full = acc[o_db:o_db + self.rows]
        self.dW, self.db = self.dW_full[:self.out_dim], self.db_full[:self.out_dim]
        self._g = (gbuf, o_dv, o_dg)

    def param_grads(self):
        if self.standalone:
            gs = super().param_grads()
            gs[-1] = self.db.clone()          # the accumulator itself lives on: never hand it to autograd
            return gs
        # TrainState.finish_group ran the batched adjoint.  FRESH view objects on purpose: autograd's AccumulateGrad takes a
        # gradient over without a copy only if nothing else references the tensor object (a view kept here would make it
        # clone all ~110 gradients of an iteration)
        gbuf, o_dv, o_dg = self._g
        db = self.db_full[:self.out_dim]
        if not self.wn:
            return [self.dW_full[:self.out_dim], db]
        dv = gbuf[o_dv:o_dv + self.out_dim * self.in_dim].view(self.out_dim, self.in_dim)
        return [gbuf[o_dg:o_dg + self.out_dim].view(self.out_dim, 1), dv, db]


class TrainState:
    """Per-model state of the training path, shared by every network of an iteration: persistent effective weights, ONE batched
    weight-norm launch per group (a person's two networks; the background's two) in the forward and one in the backward, and two
    flat per-iteration buffers -- gradient accumulators (one fill) and parameter gradients -- of which every layer's tensors are
    views.  Replaces ~80 weight-norm launches, ~80 fills and ~40 allocations per iteration."""

    def __init__(self, model):
        m = self.model = model
        self.groups = []                      # (key, [nets])
        for p in range(len(m.foreground_implicit_network_list)):
            self.groups.append((p, [m.foreground_implicit_network_list[p], m.foreground_rendering_network_list[p]]))
        self.groups.append(("bg", [m.bg_implicit_network, m.bg_rendering_network]))
        self.lins = {}
        self.acc_size = self.grad_size = 0
        self.layout = {}                      # id(LinP) -> offsets
        self.tables = {}
        for key, nets in self.groups:
            for net in nets:
                fused = isinstance(net, _implicit_net_type()) and (fused_sdf_supported(net) or fused_bg_supported(net))
                ls = []
                for i, lin in enumerate(net.layers()):
                    lp = LinP(lin, pad_rows=256 if (fused and i == 3) else 0, need_wt=True, standalone=False)
                    o_dW = self.acc_size; self.acc_size += (lp.rows * lp.in_dim + 3) // 4 * 4
                    o_db = self.acc_size; self.acc_size += (lp.rows + 3) // 4 * 4
                    o_dv = self.grad_size; self.grad_size += (lp.out_dim * lp.in_dim + 3) // 4 * 4
                    o_dg = self.grad_size; self.grad_size += (lp.out_dim + 3) // 4 * 4 if lp.wn else 0
                    self.layout[id(lp)] = (o_dW, o_db, o_dv, o_dg)
                    ls.append(lp)
                self.lins[id(net)] = ls
        self.dev = next(iter(self.lins.values()))[0].W.device
        self._key = None

    def _build_tables(self):
        for key, nets in self.groups:
            lps = [lp for net in nets for lp in self.lins[id(net)]]
            arr = (MpWnDesc * len(lps))()
            row = 0
            for i, lp in enumerate(lps):
                o_dW, o_db, o_dv, o_dg = self.layout[id(lp)]
                arr[i] = MpWnDesc(lp.v.data_ptr(), lp.g.data_ptr() if lp.wn else None, lp.W.data_ptr(),
                                  lp.WT.data_ptr() if lp.WT is not None else None, o_dW, o_dv, o_dg, lp.out_dim, lp.in_dim, row, 0)
                row += lp.out_dim
            host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self.tables[key] = (host.to(self.dev), len(lps), row, lps)

    def begin(self, keys=None):
        """start of a training forward: effective weights of the groups in `keys` (default: all).  The gradient accumulators are
        NOT part of this: they belong to a backward pass (start_backward), so that several forwards may be alive before their
        backwards run (loss = f(A) + f(B), a forward between forward and backward, a retained graph swept twice) without one
        graph's sweep accumulating into another's buffers."""
        L, st = hip.lib(), hip.stream()
        ptrs = []
        for ls in self.lins.values():
            for lp in ls:
                lp.read_params()
                ptrs.append(lp.v.data_ptr())
                ptrs.append(lp.g.data_ptr() if lp.wn else 0)
        key = tuple(ptrs)
        if key != self._key:
            self._key = key
            self._build_tables()
        for k, _ in self.groups:
            if keys is None or k in keys:
                tab, n, rows, _ = self.tables[k]
                L.mp_tr_wn_fwd_multi(tab, n, rows, st)
        self.acc = self.gbuf = None
        return self

    def start_backward(self):
        """start of ONE adjoint sweep: fresh flat buffers -- accumulators (one fill) and parameter gradients -- and every shared
        layer's dW / db / gradient views re-bound to them.  Fresh per sweep on purpose: autograd takes the gradient views over as
        param.grad without a copy, so a buffer must never be written by a later sweep."""
        self.acc = torch.zeros(self.acc_size, dtype=F32, device=self.dev)
        self.gbuf = torch.empty(self.grad_size, dtype=F32, device=self.dev)
        for ls in self.lins.values():
            for lp in ls:
                lp.bind(self.acc, *self.layout[id(lp)][:2], self.gbuf, *self.layout[id(lp)][2:])
        self._finished = set()
        return self

    def finish_group(self, key):
        """the weight-norm adjoint of one group's layers: accumulators -> parameter gradients (views of the flat buffer)"""
        if key in self._finished:
            raise RuntimeError(f"TrainState.finish_group({key!r}) twice in one backward sweep")
        self._finished.add(key)
        tab, n, rows, lps = self.tables[key]
        hip.lib().mp_tr_wn_bwd_multi(tab, n, rows, self.acc, self.gbuf, hip.stream())


def _implicit_net_type():
    from .networks import ImplicitNet
    return ImplicitNet


def train_state(model):
    st = model.__dict__.get("_mp_train_state")
    if st is None:
        st = model.__dict__["_mp_train_state"] = TrainState(model)
    return st


def fused_sdf_supported(net):
    """the network shape csrc/tfuse.hip is specialised for: the shipped foreground ImplicitNet (confs/model/*.yaml)"""
    return (net.d_in == 3 and net.multires == 6 and list(net.skip_in) == [4] and net.num_layers - 1 == 9 and net.cond_dim == 69
            and list(net.dims[1:-1]) == [256] * 8 and net.dims[-1] == 257)


def fused_bg_supported(net):
    """the network shape the fused background kernels (csrc/tfuse.hip k_tf_bg_*) are specialised for: the shipped NeRF++ net"""
    return (net.d_in == 4 and net.multires == 10 and list(net.skip_in) == [4] and net.num_layers - 1 == 9 and net.cond_dim == 32
            and list(net.dims[1:-1]) == [256] * 8 and net.dims[-1] == 257 and not hasattr(net.lin0, "weight_g"))


def fused_col_supported(net):
    """the RenderingNet shape the fused colour kernels of csrc/tfuse.hip are specialised for (the shipped foreground net)"""
    return net.mode == "pose_no_view" and list(net.dims) == [270, 256, 256, 256, 256, 3]


# the three kernel families of csrc/tfuse.hip: (sizes entry point, pack entry point, layers, layer whose accumulators are padded to
# 256 rows -- its 217 / 172 rows are contracted as 256, see LinP)
_FUSED_KINDS = {"sdf": ("mp_tf_sdf_sizes", "mp_tf_sdf_pack", 9, 3), "bg": ("mp_tf_bg_sizes", "mp_tf_bg_pack", 9, 3),
                "col": ("mp_tf_col_sizes", "mp_tf_col_pack", 5, None)}


class FusedState:
    """Per-network device state of the layer-fused training kernels (csrc/tfuse.hip), kind 'sdf' | 'bg' | 'col': persistent
    effective weights, the split-bf16 chunk stream, the bias table and the pointer tables mp_tf_<kind>_pack reads."""

    def __init__(self, kind, net, lins=None):
        """lins: the network's LinP list of a TrainState (weights resolved and accumulators bound by TrainState.begin); None:
        standalone layers owned by this object (unit tests, tools)"""
        self.kind, self.net = kind, net
        sizes, self._pack, n_layers, pad = _FUSED_KINDS[kind]
        self.shared = lins is not None
        self.lins = lins if self.shared else [LinP(l, pad_rows=256 if i == pad else 0) for i, l in enumerate(net.layers())]
        dev = self.lins[0].W.device
        per_point, pack = C.c_longlong(0), C.c_longlong(0)
        getattr(hip.lib(), sizes)(1, C.byref(per_point), C.byref(pack))
        self.arena_per_point = int(per_point.value)
        self.wpack = torch.empty(int(pack.value), dtype=torch.uint8, device=dev)
        self.bias_all = torch.empty(n_layers * 288, dtype=F32, device=dev)
        self.b0 = torch.empty(256, dtype=F32, device=dev)
        self.pose8 = torch.empty(8, dtype=F32, device=dev) if kind == "col" else None
        self.wtab = _table([lw.W for lw in self.lins], dev)
        self._btab_key, self.btab = None, None

    def refresh(self, cond_vec):
        """this iteration's weights and conditioning -> chunk stream and bias table (layer 0's bias carries the hoisted conditioning)"""
        L, st = hip.lib(), hip.stream()
        net, lins = self.net, self.lins
        if not self.shared:
            for lw in lins:
                lw.refresh()
        if self.kind == "col":          # the colour net hoists lin_pose(cond) (8), columns 6..13 of its input
            lp = net.lin_pose
            self.lp_w, self.lp_b = lp.weight.detach().contiguous(), lp.bias.detach().contiguous()
            L.mp_tr_hoist_fwd(self.lp_w, 8, 69, self.lp_b, 0, 69, cond_vec, self.pose8, st)
            c0, n_h, hvec = 6, 8, self.pose8
        else:
            c0, n_h, hvec = net.embed_dim, net.cond_dim, cond_vec
        lw0 = lins[0]
        L.mp_tr_hoist_fwd(lw0.W, 256, lw0.in_dim, lw0.b, c0, n_h, hvec, self.b0, st)
        bs = [self.b0] + [lw.b for lw in lins[1:]]
        key = tuple(b.data_ptr() for b in bs)
        if key != self._btab_key:
            self._btab_key, self.btab = key, _table(bs, self.b0.device)
        getattr(L, self._pack)(self.wtab, self.btab, self.wpack, self.bias_all, st)
        return self


def fused_state(kind, net, lins=None):
    """the network's FusedState: one for its TrainState's shared layers, one standalone (created on first use)"""
    key = "_mp_tfuse_shared" if lins is not None else "_mp_tfuse"
    st = net.__dict__.get(key)
    if st is None or (lins is not None and st.lins is not lins):
        st = net.__dict__[key] = FusedState(kind, net, lins)
    return st


fused_sdf_state = functools.partial(fused_state, "sdf")      # (the eval sampler's near-fp32 mode, tests, tools)


class _FusedImplicit(_SdfEvaluator):
    """What the two layer-fused ImplicitNet evaluators share: the state, the stash arena and its layout, feat [P+1][256] and
    sdf [P+1] as their own tensors (one pad row, csrc/tfuse.hip), the value sweep's weight gradients."""
    feat_ld = 256
    dfeat_col0, dfeat_accumulate = 0, False

    def _begin(self, kind, net, x, cond_vec, lins, grain, p_cap=None, cap_bytes=6 << 30):
        L = hip.lib()
        self.net, self.x, self.cond = net, x, cond_vec
        self.P = P = x.shape[0]
        self.E = E = net.embed_dim
        self.fs = fs = fused_state(kind, net, lins).refresh(cond_vec)
        self.lins = fs.lins
        sizes = getattr(L, _FUSED_KINDS[kind][0])
        arena = C.c_longlong(0)
        sizes(P, C.byref(arena), None)
        cap = None
        if p_cap is not None and p_cap >= P:
            capv = C.c_longlong(0)
            sizes(int(p_cap), C.byref(capv), None)
            cap = int(capv.value)
        self.arena = _big_empty(int(arena.value), x.device, grain=grain, cap=cap, cap_bytes=cap_bytes)
        # the arena's layout (floats): [P+1][256] tensors dZ_l, (V_l,) X_l, (dT_l), then the [P][E] Fourier features (and the
        # gradient sweep's dG, G)
        self.R1 = R1 = 256 * (P + 1)
        self.t_dZ, self.t_V, self.t_X, self.t_dT, n_t = (0, 8, 15, 23, 46) if kind == "sdf" else (0, None, 7, None, 16)
        self.o_IN, self.o_dG, self.o_G = n_t * R1, n_t * R1 + E * P, n_t * R1 + 2 * E * P
        L.mp_tr_pe(x, net.d_in, P, net.multires, 0, 1.0, off(self.arena, self.o_IN), E, 0, hip.stream())
        self.feat = torch.empty(P + 1, 256, dtype=F32, device=x.device)  # columns 1.. of the reference's output (+ the pad row)
        self.sdf = torch.empty(P + 1, dtype=F32, device=x.device)        # column 0
        self.feat_ptr = hip.ptr(self.feat)

    def _at(self, t0, l):
        """device pointer to stash tensor l of the family starting at tensor t0 (t_dZ, t_V, t_X, t_dT)"""
        return off(self.arena, (t0 + l) * self.R1)

    def _skip_features(self):
        # the skip connection re-injects the Fourier features into layer 4's input (times 1/sqrt 2): the last E columns of X_4
        E = self.E
        hip.lib().mp_tr_copy_cols(off(self.arena, self.o_IN), E, 0, self._at(self.t_X, 4), 256, 256 - E, self.P, E,
                                  1.0 / math.sqrt(2.0), 0, hip.stream())

    @property
    def out(self):
        """the reference's [P][257] layout (column 0 = sdf), assembled on demand (tests; the trainer reads feat / sdf)"""
        return torch.cat([self.sdf[:self.P, None], self.feat[:self.P]], 1)

    def new_dfeat(self, n=0):
        d = torch.empty(self.P, 256, dtype=F32, device=self.x.device)    # its own aligned matrix, WRITTEN by the colour net
        if n < self.P:
            d[n:].zero_()
        return d

    def _weight_grads(self, dfeat, tn_groups, gradient_sweep):
        """dW_l += dZ_l^T X_l (value sweep; bias gradient = its column sums) [+ V_l^T dT_l (gradient sweep)]; returns d cond"""
        P, E, lins = self.P, self.E, self.lins
        lw0, lw8 = lins[0], lins[8]
        dcond = _layer0_adjoint(lw0, self._at(self.t_dZ, 0), off(self.arena, self.o_IN), E, E, P, P, E, self.net.cond_dim, self.cond)
        if gradient_sweep:
            gemm_tn(self._at(self.t_V, 0), 256, off(self.arena, self.o_dG), E, lw0.dW, lw0.in_dim, 256, E, P)
        groups = tn_groups if tn_groups is not None else []
        for l in range(1, 8):
            lw = lins[l]                                # (layer 3: its 217 / 172 rows contracted as 256, see LinP)
            rows = lw.dW_full.shape[0]
            groups.append(tn_group(self._at(self.t_dZ, l), 256, self._at(self.t_X, l), 256, hip.ptr(lw.dW_full), lw.in_dim, rows,
                                   lw.in_dim, P, hip.ptr(lw.db_full), P))
            if gradient_sweep:
                groups.append(tn_group(self._at(self.t_V, l), 256, self._at(self.t_dT, l), 256, hip.ptr(lw.dW_full), lw.in_dim,
                                       rows, lw.in_dim, P))
        groups.append(tn_group(hip.ptr(dfeat), 256, self._at(self.t_X, 8), 256, off(lw8.dW, 256), 256, 256, 256, P,
                               off(lw8.db, 1), P))
        if tn_groups is None:
            launch_tn_groups(groups)
        return dcond


class ImplicitTrainFused(_FusedImplicit):
    """ImplicitTrainRev's arithmetic (value sweep + gradient sweep, and the adjoint of both) on the LAYER-FUSED kernels of
    csrc/tfuse.hip: two launches instead of ~90 per person -- mp_tf_sdf_fwd (both forward sweeps) and mp_tf_sdf_bwd (the adjoint
    w.r.t. the activations) -- plus one weight-gradient contraction per layer over [dZ_l; V_l]^T [X_l; dT_l] (K = 2 P rows).
    backward(want_dx=True) also yields the adjoint of the input points (pose optimisation): one more launch, mp_tf_sdf_dx,
    which contracts the dZ_0 / dZ_4 stashes with the Fourier columns of W_0 / W_4; sdf_evaluator takes this class under
    pose_grad when SDF_POSE_GRAD_MODE is 'fused' (the default there is still ImplicitTrainRev)."""

    def __init__(self, net, x, cond_vec, lins=None, p_cap=None, cap_bytes=6 << 30):
        """p_cap: the largest P this caller can ever pass (all rays hit the body): the stash is then sized for it, i.e. the SAME
        allocation every iteration (_big_empty) -- when that is at most cap_bytes (the caller divides its arena budget by the
        number of persons whose stashes are alive together: a crowded scene must not hold n_persons x the all-rays-hit arena)"""
        L, st = hip.lib(), hip.stream()
        assert fused_sdf_supported(net)
        self._begin("sdf", net, x, cond_vec, lins, 1 << 26, p_cap, cap_bytes)
        fs, P, E = self.fs, self.P, self.E
        self.nl = len(fs.lins)
        self.w8 = fs.lins[8].W                          # row 0 = the sdf row of the last layer
        L.mp_tf_sdf_fwd(fs.wpack, fs.bias_all, self.w8, self.arena, P, self.feat, self.sdf, st)
        self._skip_features()
        self.grad = torch.empty(P, 3, dtype=F32, device=x.device)
        L.mp_tr_pe_grad_fwd(x, P, net.multires, off(self.arena, self.o_G), E, self.grad, st)

    def backward(self, dfeat, dsdf, dgrad, want_dx=False, tn_groups=None):
        assert dfeat.shape[1] == 256
        L, st = hip.lib(), hip.stream()
        net, P, E, fs, A = self.net, self.P, self.E, self.fs, self.arena
        dG = off(A, self.o_dG)
        # want_dx: the gradient sweep's second-order share of d x_c first, the value sweep's (mp_tf_sdf_dx) added below
        self.dx = torch.zeros(P, 3, dtype=F32, device=self.x.device) if want_dx else None
        L.mp_tr_pe_grad_bwd(self.x, P, net.multires, dgrad, off(A, self.o_G), E, dG, E, self.dx, st)
        lw8 = self.lins[8]                              # the sdf row's gradient goes straight into row 0 of dW_8 / db_8
        tf_bwd("sdf", fs.wpack, self.w8, A, P, dfeat, dsdf, lw8.dW, lw8.db)
        L.mp_tr_copy_cols(dG, E, 0, self._at(self.t_dT, 4), 256, 256 - E, P, E, 1.0 / math.sqrt(2.0), 0, st)
        if want_dx:                                     # d x_c += J_PE^T (dZ_0 W_0[:, :39] + dZ_4 W_4[:, 217:] / sqrt 2)
            lw0, lw4 = self.lins[0], self.lins[4]
            L.mp_tf_sdf_dx(A, P, lw0.W, lw0.in_dim, lw4.W, lw4.in_dim, self.x, self.dx, st)
        return self._weight_grads(dfeat, tn_groups, gradient_sweep=True)

    def points_adjoint(self, dsdf):
        """d x [P][3] of a term that reads the sdf column alone (dsdf [P] its adjoint) with the network held CONSTANT: the adjoint
        w.r.t. the activations on zero dfeat / dG (mp_tf_sdf_bwd; the sdf row's own gradient goes to scratch), then the points'
        adjoint from its stash (mp_tf_sdf_dx).  No weight-gradient contraction runs and no accumulator of the iteration is
        touched (the interpenetration term: the partner's net must not answer it by shrinking)."""
        L, st = hip.lib(), hip.stream()
        P, E, A = self.P, self.E, self.arena
        f32 = dict(dtype=F32, device=self.x.device)
        A[self.o_dG:self.o_dG + E * P].zero_()          # the gradient sweep has no upstream here
        scratch = torch.zeros(257, **f32)               # d w8 [256], d b8 [1]
        tf_bwd("sdf", self.fs.wpack, self.w8, A, P, torch.zeros(P, 256, **f32), dsdf, scratch, off(scratch, 256))
        dx = torch.zeros(P, 3, **f32)
        lw0, lw4 = self.lins[0], self.lins[4]
        L.mp_tf_sdf_dx(A, P, lw0.W, lw0.in_dim, lw4.W, lw4.in_dim, self.x, dx, st)
        return dx


class ImplicitTrainFusedBG(_FusedImplicit):
    """ImplicitTrain(fwd=False)'s arithmetic for the background ImplicitNet on the layer-fused kernels (csrc/tfuse.hip
    mp_tf_bg_fwd / mp_tf_bg_bwd): the nine layers in one launch each way, the weight gradients as one contraction per layer.
    x [P][4] (the inverted-sphere points), code (32,) the frame's latent row."""
    grad = None

    def __init__(self, net, x, code, lins=None):
        assert fused_bg_supported(net)
        self._begin("bg", net, x, code, lins, 1 << 22)
        fs = self.fs
        hip.lib().mp_tf_bg_fwd(fs.wpack, fs.bias_all, self.arena, self.P, self.feat, self.sdf, hip.stream())
        self._skip_features()

    def backward(self, dfeat, dsdf, dgrad=None, want_dx=False, tn_groups=None):
        assert dgrad is None and not want_dx and dfeat.shape[1] == 256
        lw8 = self.lins[8]
        tf_bwd("bg", self.fs.wpack, lw8.W, self.arena, self.P, dfeat, dsdf, lw8.dW, lw8.db)
        return self._weight_grads(dfeat, tn_groups, gradient_sweep=False)


# ----------------------------------------------------------------------------------------------------------------------
# A colour network evaluated for training.  Two evaluators, one surface:
#   (net, XA [n][na], feat_ptr, feat_ld, n, cond_vec, lins)      the features are read in place from the SDF evaluator
#   .rgb [n][3]
#   backward(drgb [n][3], dXA [n][na] (written), dfeat_ptr, dfeat_ld, feat_accumulate=True, tn_groups=None) -> d hoisted vector
#                         d feat: rows [0, n) at dfeat_ptr, added into (feat_accumulate) or written; an SDF evaluator's
#                         dfeat_target() says which
#   dcond()               the adjoint of the pose conditioning through lin_pose (after backward)
# colour_evaluator() chooses.
# ----------------------------------------------------------------------------------------------------------------------
class _ColourNet(_NetParams):
    def _lin_pose_adjoint(self, dh, lp_w):
        """lin_pose's own gradients from d pose8: dW = dh (x) cond, db = dh"""
        dlp_w = _zeros(8, 69, device=dh.device)
        hip.lib().mp_tr_hoist_bwd(dh, 8, 69, 0, 69, self.cond, dlp_w, hip.stream())
        self.extra_grads = [dlp_w, dh]
        self._dcond = (lp_w, dh)

    def dcond(self):
        lp_w, dh = self._dcond
        return torch.mv(lp_w.t(), dh)


class RenderTrain(_ColourNet):
    """RenderingNet (networks.py:263-312) layer by layer: mode 'pose_no_view' (inputs XA = [x_c, n] (6), feat) or
    'nerf_frame_encoding' (XA = PE_4(view) (27), feat)."""

    def __init__(self, net, XA, feat_ptr, feat_ld, n, cond_vec, lins=None):
        L = hip.lib()
        self.net, self.n = net, n
        dev = XA.device
        self.lins = lins if lins is not None else [LinW(l) for l in net.layers()]
        self.pose_mode = net.mode == "pose_no_view"
        self.na = XA.shape[1]                                # 6 or 27
        self.c_h0, self.n_h = (6, 8) if self.pose_mode else (27, 32)   # hoisted columns
        self.c_feat = self.c_h0 + self.n_h
        lw0 = self.lins[0]
        self.cond = cond_vec
        if self.pose_mode:
            lp = net.lin_pose
            self.extra_params = [lp.weight, lp.bias]
            self.lp_w, self.lp_b = lp.weight.detach().contiguous(), lp.bias.detach().contiguous()
            self.pose8 = torch.empty(8, dtype=F32, device=dev)
            L.mp_tr_hoist_fwd(self.lp_w, 8, 69, self.lp_b, 0, 69, cond_vec, self.pose8, hip.stream())
            self.hvec = self.pose8
        else:
            self.hvec = cond_vec
        self.b0 = torch.empty(lw0.out_dim, dtype=F32, device=dev)
        L.mp_tr_hoist_fwd(lw0.W, lw0.out_dim, lw0.in_dim, lw0.b, self.c_h0, self.n_h, self.hvec, self.b0, hip.stream())
        self.XA, self.feat_ptr, self.feat_ld = XA, feat_ptr, feat_ld
        self.H = []
        nl = len(self.lins)
        H0 = torch.empty(n, lw0.out_dim, dtype=F32, device=dev)
        last0 = nl == 1
        gemm_nt(XA, self.na, lw0.W, lw0.in_dim, H0, lw0.out_dim, n, lw0.out_dim, self.na, self.b0, n)
        gemm_nt(feat_ptr, feat_ld, off(lw0.W, self.c_feat), lw0.in_dim, H0, lw0.out_dim, n, lw0.out_dim, 256, None, 0,
                accumulate=True, relu=not last0)
        self.H.append(H0)
        for l in range(1, nl):
            lw = self.lins[l]
            Hl = torch.empty(n, lw.out_dim, dtype=F32, device=dev)
            gemm_nt(self.H[l - 1], self.lins[l - 1].out_dim, lw.W, lw.in_dim, Hl, lw.out_dim, n, lw.out_dim, lw.in_dim, lw.b, n,
                    relu=l < nl - 1)
            self.H.append(Hl)
        self.rgb = torch.empty(n, 3, dtype=F32, device=dev)
        L.mp_tr_sigmoid_fwd(self.H[-1], n * 3, self.rgb, hip.stream())

    def backward(self, drgb, dXA, dfeat_ptr, dfeat_ld, feat_accumulate=True, tn_groups=None):
        L = hip.lib()
        n, dev = self.n, drgb.device
        nl = len(self.lins)
        dZ = torch.empty(n, 3, dtype=F32, device=dev)
        L.mp_tr_sigmoid_bwd(self.rgb, drgb, n * 3, dZ, hip.stream())
        for l in range(nl - 1, 0, -1):
            lw, Hp = self.lins[l], self.H[l - 1]
            pout = self.lins[l - 1].out_dim
            gemm_tn(dZ, lw.out_dim, Hp, pout, lw.dW, lw.in_dim, lw.out_dim, lw.in_dim, n, lw.db, n)
            dH = torch.empty(n, pout, dtype=F32, device=dev)
            gemm_nt(dZ, lw.out_dim, lw.WT, lw.out_dim, dH, pout, n, pout, lw.out_dim)
            dZp = torch.empty(n, pout, dtype=F32, device=dev)
            L.mp_tr_relu_bwd(Hp, pout, n, pout, dH, pout, dZp, pout, hip.stream())
            dZ = dZp
        lw0 = self.lins[0]
        o0 = lw0.out_dim
        dh = _layer0_adjoint(lw0, dZ, self.XA, self.na, self.na, n, n, self.c_h0, self.n_h, self.hvec)
        gemm_tn(dZ, o0, self.feat_ptr, self.feat_ld, off(lw0.dW, self.c_feat), lw0.in_dim, o0, 256, n)
        # data gradients
        gemm_nt(dZ, o0, lw0.WT, o0, dXA, self.na, n, self.na, o0)
        gemm_nt(dZ, o0, off(lw0.WT, self.c_feat * o0), o0, dfeat_ptr, dfeat_ld, n, 256, o0, None, 0, accumulate=feat_accumulate)
        if self.pose_mode:
            self._lin_pose_adjoint(dh, self.lp_w)
        return dh


class RenderTrainFused(_ColourNet):
    """RenderTrain's arithmetic for the foreground colour net on the layer-fused kernels (csrc/tfuse.hip: mp_tf_col_fwd /
    mp_tf_col_bwd): the five layers in one launch each way, the weight gradients as one contraction per layer.  The features are
    a contiguous [>= n][256] matrix (the fused SDF net's feature rows), XA [n][6]."""

    def __init__(self, net, XA, feat_ptr, feat_ld, n, cond_vec, lins=None):
        L, st = hip.lib(), hip.stream()
        assert fused_col_supported(net) and feat_ld == 256
        self.net, self.n, self.XA, self.feat_ptr, self.cond = net, n, XA, feat_ptr, cond_vec
        self.cs = cs = fused_state("col", net, lins).refresh(cond_vec)
        self.lins = cs.lins
        self.extra_params = [net.lin_pose.weight, net.lin_pose.bias]
        stash = C.c_longlong(0)
        L.mp_tf_col_sizes(n, C.byref(stash), None)
        self.stash = _big_empty(int(stash.value), XA.device)
        self.rgb = torch.empty(n, 3, dtype=F32, device=XA.device)
        L.mp_tf_col_fwd(cs.wpack, cs.bias_all, self.stash, feat_ptr, XA, n, self.rgb, st)

    def backward(self, drgb, dXA, dfeat_ptr, dfeat_ld, feat_accumulate=False, tn_groups=None):
        assert not feat_accumulate and dfeat_ld == 256       # rows [0, n) of dfeat are written; see ImplicitTrainFused for tn_groups
        L, st = hip.lib(), hip.stream()
        n, lins, cs, S = self.n, self.lins, self.cs, self.stash
        NL = 256 * (n + 1)                               # one pad row per stash tensor
        dz4 = torch.empty(n, 3, dtype=F32, device=drgb.device)
        L.mp_tf_col_bwd(cs.wpack, S, lins[4].W, self.rgb, drgb, n, dfeat_ptr, dXA, dz4, st)
        H = lambda l: off(S, l * NL)
        dZ = lambda l: off(S, (4 + l) * NL)
        lw0 = lins[0]
        # the hoisted pose embedding: dW_0[:, 6:14] += db_0 (x) pose8 ; d pose8 = W_0[:, 6:14]^T db_0
        dh = _layer0_adjoint(lw0, dZ(0), self.XA, 6, 6, n, n, 6, 8, cs.pose8)
        groups = tn_groups if tn_groups is not None else []
        groups.append(tn_group(dZ(0), 256, self.feat_ptr, 256, off(lw0.dW, 14), lw0.in_dim, 256, 256, n))
        for l in range(1, 4):
            lw = lins[l]
            groups.append(tn_group(dZ(l), 256, H(l - 1), 256, hip.ptr(lw.dW), 256, 256, 256, n, hip.ptr(lw.db), n))
        if tn_groups is None:
            launch_tn_groups(groups)
        lw4 = lins[4]
        gemm_tn(dz4, 3, H(3), 256, lw4.dW, 256, 3, 256, n, lw4.db, n)
        self._lin_pose_adjoint(dh, cs.lp_w)
        return dh


# ======================================================================================================================
# Training-mode Multiply.forward (multiply.py:174-588, `self.training` branches) as ONE autograd node
# ======================================================================================================================
N_EIKONAL = 512          # multiply.py:324
ARENA_BUDGET_BYTES = int(os.environ.get("MP_TRAIN_ARENA_GB", "24")) << 30   # fixed-size SDF stashes of one iteration, all persons
# 'fused' (ImplicitTrainFused: layer-fused kernels, default) | 'reverse' (ImplicitTrainRev, layer by layer) | 'forward'
SDF_TRAIN_MODE = os.environ.get("MP_SDF_TRAIN_MODE", "fused")
# background ImplicitNet: 'fused' (ImplicitTrainFusedBG, default) | 'layerwise' (ImplicitTrain: the cross-check)
BG_TRAIN_MODE = os.environ.get("MP_BG_TRAIN_MODE", "fused")
# the SDF evaluator while the body-model inputs are optimised (pose_grad): 'layerwise' (ImplicitTrainRev, default) | 'fused'
# (ImplicitTrainFused + mp_tf_sdf_dx, where SDF_TRAIN_MODE, the precision and the network's shape allow the fused kernels)
SDF_POSE_GRAD_MODE = os.environ.get("MP_SDF_POSE_GRAD_MODE", "layerwise")


ZERO_POSE_SAMPLES = 2000          # multiply.py:363
SMPL_SURFACE_THRESHOLD = 0.02     # multiply.py:358
SURFACE_EXCLUDED_PARTS = ("head", "rightHand", "leftHand", "rightFoot", "leftFoot", "leftHandIndex1", "rightHandIndex1")   # multiply.py:340-343


def _table(ts, dev):
    return hip.device_ints([t.data_ptr() for t in ts], dev)      # (no host wait: hip._PinnedInts)


def surface_sampling_weights(model, n_verts, dev):
    """multiply.py:339-345: SMPL vertices the surface regulariser samples from -- all but head, hands and feet (cached)"""
    w = model.__dict__.get("_mp_surface_weights")
    if w is None or w.shape[0] != n_verts or w.device != torch.device(dev):
        part = getattr(model, "smpl_vertex_part", None)
        if part is None:
            raise FileNotFoundError("smpl_surface_weight > 0 needs the SMPL vertex segmentation (the reference reads "
                                    "./outputs/smpl_vert_segmentation.json, multiply.py:113, an asset it does not ship): set "
                                    "opt.smpl_vert_segmentation_path or assign model.smpl_vertex_part = {part name: [vertex ids]}")
        w = torch.ones(n_verts)
        w[[i for k in SURFACE_EXCLUDED_PARTS for i in part[k]]] = 0
        w = model.__dict__["_mp_surface_weights"] = w.to(dev)
    return w


def _random_prefixes(sizes, k, dev, gen):
    """row i = the first k entries of a uniform random permutation of range(sizes[i]) (what torch.randperm(n)[:k] draws), all
    rows in three launches: the k smallest of n independent uniform keys, in the order of their keys, ARE such a prefix.
    [One torch.randperm per row is ~7 launches each: 84 of an iteration's ~570.]"""
    n = max(sizes)
    assert k <= min(sizes), "a permutation prefix longer than the permutation"
    keys = torch.rand(len(sizes), n, device=dev, generator=gen)
    if min(sizes) < n:
        lim = hip.device_ints(sizes, dev).unsqueeze(1)
        keys = torch.where(torch.arange(n, device=dev).unsqueeze(0) < lim, keys, keys.new_full((), 2.0))
    return torch.topk(keys, k, dim=1, largest=False, sorted=True).indices


def make_draws(model, cx, gen=None):
    """The randomness one training forward consumes (ray_sampler.py:38,171,202; multiply.py:325; sampler.py:100):
    per person  t_rand [R_p,NE], u_final [R_p,N], extra_idx [max_iters,N_extra], eik_idx [512], eik_noise [512,3];
    shared      bg_rand [R,N_bg].  Drawn on the device with torch's generator; the permutation prefixes (the reference's
    torch.randperm(n)[:k]) come from _random_prefixes, all persons at once."""
    rs, dev = model.ray_sampler, cx["dev"]
    NE, NS, NX = rs.N_samples_eval, rs.N_samples, rs.N_samples_extra
    kw = dict(device=dev, generator=gen)
    draws = {"person": {}}
    persons = list(cx["persons"])
    T = rs.max_total_iters
    extra = _random_prefixes([NE * k for k in range(1, T + 1)] * len(persons), NX, dev, gen).to(torch.int32).reshape(len(persons), T, NX)
    nvs = [model.smpl_server_list[p].verts_c.reshape(-1, 3).shape[0] for p in persons]
    eik = _random_prefixes(nvs, N_EIKONAL, dev, gen)
    for n, p in enumerate(persons):
        Rp = max(int(cx["n_hit"][n]), 1)
        draws["person"][p] = dict(
            t_rand=torch.rand(Rp, NE, **kw), u_final=torch.rand(Rp, NS, **kw), extra_idx=extra[n].contiguous(),
            eik_idx=eik[n], eik_noise=torch.randn(N_EIKONAL, 3, **kw))
    draws["bg_rand"] = torch.rand(cx["R"], rs.N_samples_inverse_sphere, **kw)
    # the two regularisers of multiply.py:336-394 (weight 0 in the shipped configs): their vertex draws
    if model.smpl_surface_weight > 0:
        for n, p in enumerate(persons):                               # idx_weight.multinomial(num_pixels, replacement=True)
            draws["person"][p]["surf_idx"] = torch.multinomial(surface_sampling_weights(model, nvs[n], dev), cx["R"],
                                                               replacement=True, generator=gen)
    if model.zero_pose_weight > 0:
        nv_all = [v.shape[1] for v in model.mesh_v_cano_list]
        zp = _random_prefixes(nv_all * len(persons), min(ZERO_POSE_SAMPLES, min(nv_all)), dev, gen).reshape(len(persons), len(nv_all), -1)
        draws["zp_idx"] = {(q, p): zp[n, p] for n, q in enumerate(persons) for p in range(len(nv_all))}
    # the interpenetration term's probe vertices (Multiply.train_interpenetration): the LAST draw, and only with the flag on -- a
    # seeded run with the flag off consumes the generator exactly as before the term existed
    if model.training and getattr(model, "train_interpenetration", False) and len(persons) > 1:
        pen = _random_prefixes(nvs, min(int(model.interpenetration_points), min(nvs)), dev, gen)
        for n, p in enumerate(persons):
            draws["person"][p]["pen_idx"] = pen[n]
    return draws


def sdf_evaluator(net, x, cond_vec, lins, pose_grad, p_cap, cap_bytes):
    """THE choice of the foreground SDF evaluator (SDF_TRAIN_MODE, TRAIN_PRECISION, the network's shape; under pose_grad also
    SDF_POSE_GRAD_MODE: the fused kernels yield d x_c through mp_tf_sdf_dx only when it is 'fused')"""
    if SDF_POSE_GRAD_MODE not in ("layerwise", "fused"):
        raise ValueError(f"MP_SDF_POSE_GRAD_MODE = {SDF_POSE_GRAD_MODE!r}: 'layerwise' or 'fused'")
    mode = SDF_TRAIN_MODE
    if mode == "fused" and ((pose_grad and SDF_POSE_GRAD_MODE != "fused") or TRAIN_PRECISION != "bf16x3"
                            or not fused_sdf_supported(net)):
        mode = "reverse"      # the fused kernels: split-bf16 arithmetic, the shipped network shape
    if mode == "fused":
        return ImplicitTrainFused(net, x, cond_vec, lins=lins, p_cap=p_cap, cap_bytes=cap_bytes)
    if mode == "forward":
        return ImplicitTrain(net, x, cond_vec, fwd=True, lins=lins)
    return ImplicitTrainRev(net, x, cond_vec, lins=lins)


def bg_evaluator(net, x, code, lins):
    """THE choice of the background ImplicitNet's evaluator (BG_TRAIN_MODE, TRAIN_PRECISION, the network's shape)"""
    if BG_TRAIN_MODE == "fused" and TRAIN_PRECISION == "bf16x3" and fused_bg_supported(net):
        return ImplicitTrainFusedBG(net, x, code, lins=lins)       # the nine layers in one launch (csrc/tfuse.hip k_tf_bg_fwd)
    return ImplicitTrain(net, x, code, fwd=False, lins=lins)


def colour_evaluator(net, XA, it, n, cond_vec, lins):
    """THE choice of a colour net's evaluator on the first n points of SDF evaluator `it`: the fused kernels read a contiguous
    [.][256] feature matrix (which the fused SDF evaluators deliver) in split-bf16 arithmetic"""
    fused = TRAIN_PRECISION == "bf16x3" and it.feat_ld == 256 and fused_col_supported(net)
    return (RenderTrainFused if fused else RenderTrain)(net, XA, it.feat_ptr, it.feat_ld, n, cond_vec, lins=lins)


class Interpenetration:
    """The mesh-free interpenetration term of one call (the reference's mesh term: multiply_model.py:521-551).
    For every ORDERED pair (p, q), p != q, of the call's persons: person p's posed SMPL vertices pen_idx[p] are probe points; a
    point whose exact nearest posed vertex of q lies within the 0.1 outlier radius (mp_pen_probe: the rule and the capped search of
    mp_warp_inverse in eval mode) is warped into q's canonical space, x_c = I_nn (x - c_nn), and costs s^2 where q's signed
    distance s = sdf_q(x_c; cond_q) is negative.  .loss (1,) = the RAW sum over all pairs; .pair_loss / .active / .count [P*P]
    (device; count = the probed points per pair).
    The SDF runs on the fused training kernels (split-bf16, fp32 accumulation): ImplicitTrainFused on the compact entries of all
    p != q, one slot of n rows per p, concatenated per q and PADDED to capacity with points at the origin (their seed is zero, so
    is their adjoint): no host read of the counts, the same (P - 1) n rows in every iteration.  keep: the evaluators' stashes
    stay alive for backward(), which returns per person the term's share (d tfs [24][16], d posed vertices [V][3]) -- the warp
    path through q's transforms (mp_tr_warp_bwd) and the vertex path d x = I_nn^T d x_c on p's drawn vertices
    (mp_pen_scatter_bwd).  Networks and conditionings are constants of the term."""

    def __init__(self, model, cx, pen_idx, lins_of=None, keep=False):
        """pen_idx {person: vertex ids (n,)}; lins_of(net) -> the shared LinP list of a TrainState (None: standalone layers)"""
        L, st = hip.lib(), hip.stream()
        self.model, self.cx = model, cx
        self.persons = persons = list(cx["persons"])
        self.P = P = len(persons)
        dev = cx["dev"]
        f32, i32 = dict(dtype=F32, device=dev), dict(dtype=torch.int32, device=dev)
        nets = [model.foreground_implicit_network_list[q] for q in persons]
        if TRAIN_PRECISION != "bf16x3" or not all(fused_sdf_supported(net) for net in nets):
            raise NotImplementedError("the interpenetration term evaluates the SDF on the fused training kernels (csrc/tfuse.hip): "
                                      "split-bf16 arithmetic (MP_TRAIN_PRECISION=bf16x3) and the shipped ImplicitNet shape only")
        per = [cx["per"][p] for p in persons]
        idx64 = [pen_idx[p].to(dev).long().reshape(-1) for p in persons]
        self.n = n = int(idx64[0].numel())
        assert all(int(i.numel()) == n for i in idx64), "every person probes with the same number of vertices"
        self.idx = [i.to(torch.int32).contiguous() for i in idx64]
        PP = P * P
        self.count = torch.zeros(PP, **i32)                      # (the diagonal is never written)
        self.pair_loss, self.active = torch.zeros(PP, **f32), torch.zeros(PP, **i32)
        self.items = []
        if n == 0:
            self.loss = torch.zeros(1, **f32)
            return
        pts = [pp["verts"].index_select(0, i).contiguous() for pp, i in zip(per, idx64)]
        self.btabs = [pp["btab"] for pp in per]
        self.nn = torch.empty(PP, n, **i32)
        self.list = torch.zeros(PP, n, **i32)                    # zero-filled: a row's padding names point 0, masked below
        probed = torch.empty(PP, n, dtype=torch.uint8, device=dev)
        xc = torch.empty(PP, n, 3, **f32)
        L.mp_pen_probe(_table(pts, dev), _table([pp["vsorted"] for pp in per], dev), _table([pp["cbound"] for pp in per], dev),
                       _table(self.btabs, dev), P, n, probed, self.nn, xc, self.list, self.count, st)
        ar = torch.arange(n, device=dev)
        but = lambda t, b: torch.cat([t[:b, b], t[b + 1:, b]])   # column b of a [P][P][..] array without the diagonal: the slots of q
        sdf_at, seed_at = [0] * PP, [0] * PP
        for b, q in enumerate(persons):
            sel = but(self.list.view(P, P, n), b).long()                                         # (P - 1, n) point ids
            valid = ar[None, :] < but(self.count.view(P, P), b)[:, None]
            X = torch.gather(but(xc.view(P, P, n, 3), b), 1, sel[..., None].expand(-1, -1, 3))
            X = torch.where(valid[..., None], X, X.new_zeros(())).reshape(-1, 3).contiguous()    # (unwritten rows never get through)
            nnq = torch.where(valid, torch.gather(but(self.nn.view(P, P, n), b), 1, sel), 0).to(torch.int32).reshape(-1).contiguous()
            it = ImplicitTrainFused(nets[b], X, cx["per"][q]["cond"], lins=None if lins_of is None else lins_of(nets[b]))
            seed = torch.zeros(X.shape[0], **f32)
            for slot, a in enumerate(a for a in range(P) if a != b):
                sdf_at[a * P + b], seed_at[a * P + b] = it.sdf.data_ptr() + 4 * slot * n, seed.data_ptr() + 4 * slot * n
            self.items.append((q, b, it, X, nnq, seed))
        L.mp_pen_loss(hip.device_ints(sdf_at, dev), self.count, P, n, self.pair_loss, self.active, hip.device_ints(seed_at, dev), st)
        self.loss = self.pair_loss.sum().reshape(1)
        if not keep:                                             # value only: no stash outlives the forward
            self.items = []

    def backward(self, d_loss):
        """-> {person: (d tfs [24][16], d posed vertices [V][3])}: the adjoint with the seed 2 s [s < 0], scaled once by d_loss"""
        L, st = hip.lib(), hip.stream()
        m, cx, P, n = self.model, self.cx, self.P, self.n
        dev = cx["dev"]
        f32 = dict(dtype=F32, device=dev)
        scale = d_loss.reshape(()).to(dev, F32)
        V = m.smpl_server_list[self.persons[0]].verts_c.reshape(-1, 3).shape[0]
        shares = {p: [torch.zeros(24, 16, **f32), torch.zeros(V, 3, **f32)] for p in self.persons}
        if not self.items:
            return {p: tuple(s) for p, s in shares.items()}
        dxc_at, held = [0] * (P * P), []
        for q, b, it, X, nnq, seed in self.items:
            dxc = it.points_adjoint(seed)                        # (exact zeros on the padding and on the inactive entries)
            warp_bwd(X, dxc, None, None, nnq, None, X.shape[0], m.smpl_server_list[q].tables.lbs_weights, cx["per"][q]["tfs"],
                     shares[q][0])
            for slot, a in enumerate(a for a in range(P) if a != b):
                dxc_at[a * P + b] = dxc.data_ptr() + 12 * slot * n
            held.append(dxc)
        dverts = [shares[p][1] for p in self.persons]
        L.mp_pen_scatter_bwd(_table(self.idx, dev), self.list, self.count, self.nn, _table(self.btabs, dev), hip.device_ints(dxc_at, dev),
                             P, n, V, _table(dverts, dev), st)
        return {p: (s[0] * scale, s[1] * scale) for p, s in shares.items()}


class TrainGraph:
    """Everything one training forward keeps for its backward."""

    def __init__(self, model, cx, input, cond_zero, draws, surface_flags=False, pose_grad=False, shard=None, ts=None):
        """shard = (world, rank): person-sharded training: cx holds only this rank's persons
        {p : p % world == rank}; their per-sample rows are all-gathered once in the forward, every rank composites all rays
        (512 of them: cheaper than a second exchange in the backward), the background branch is ray-sliced."""
        self.model, self.cx, self.input, self.cond_zero, self.draws = model, cx, input, cond_zero, draws
        self.surface_flags, self.pose_grad, self.shard = surface_flags, pose_grad, shard
        self.det = deterministic(model)       # the deterministic training mode, fixed for this graph's forward and adjoint sweep
        self.ts = ts if ts is not None else train_state(model).begin()     # shared layers: weights resolved, accumulators zeroed
        self.reg_items, self.reg_losses = [], (None, None)
        self.reg_dcond = {}             # person -> adjoint of its pose conditioning from the regularisers (pose optimisation)
        self.reg_surf = {}              # person -> (d tfs [24][16], d posed vertices [V][3]) of the surface term (pose optimisation)
        # Multiply.train_geometry: the node also returns the volume-rendered depths of its rays (GEOMETRY_KEYS), with an adjoint
        self.geometry = bool(model.training and getattr(model, "train_geometry", False))
        # Multiply.train_interpenetration: the node also returns the mesh-free interpenetration term (Interpenetration), whose
        # adjoint reaches the body-model inputs and nothing else
        self.pen_on = bool(model.training and getattr(model, "train_interpenetration", False))
        self.pen, self.pen_loss = None, None

    # ---- forward ------------------------------------------------------------------------------------------------
    @_in_graph_mode
    def run(self):
        m, cx = self.model, self.cx
        rs = m.ray_sampler
        self.NZ = rs.N_samples + rs.N_samples_extra + 2
        persons = cx["persons"]
        if self.cond_zero:                                            # multiply.py:271-273
            for p in persons:
                cx["per"][p]["cond"] = torch.zeros_like(cx["per"][p]["cond"])
        # the samplers of all persons advance together (Multiply._sample_persons): in ray-sharded data-parallel training the
        # convergence vote is then ONE collective per sampler iteration for all persons
        todo = [p for p in persons if self.draws["person"][p].get("z_given") is None]
        # (the near-fp32 sampler mode queries on this iteration's resolved weights: the shared layers are handed in)
        sampled = m._sample_persons(cx, {p: self.draws["person"][p] for p in todo}, persons=todo,
                                    shared_lins={p: self.ts.lins[id(m.foreground_implicit_network_list[p])] for p in todo}) if todo else {}
        self.fg = {}
        local = [self._person_forward(n, p, sampled.get(p)) for n, p in enumerate(persons)]
        if m.smpl_surface_weight > 0 or m.zero_pose_weight > 0:
            self._regularisers_forward()
        if self.pen_on:
            self._interpenetration_forward()
        # the composited persons, in person order: one record each, the same fields whether this rank evaluated the person or not
        self.all_persons, self.composited, self.ray_slice = list(persons), local, (0, cx["R"])
        if self.shard is not None:
            self._exchange(local)
        self.bg_rgb = self._background_forward()
        return self._composite()

    def _person_forward(self, n, p, sampled):
        """person p (the n-th of this call): canonical points of its samples, SDF net, normals, colour net -> its compositing record"""
        m, cx, L, st = self.model, self.cx, hip.lib(), hip.stream()
        dev, R, NZ = cx["dev"], cx["R"], self.NZ
        f32 = dict(dtype=F32, device=dev)
        S = NZ - 1
        pp = cx["per"][p]
        dr = self.draws["person"][p]
        Rp = max(int(cx["n_hit"][n]), 1)
        imp, ren, dfm = m.foreground_implicit_network_list[p], m.foreground_rendering_network_list[p], m.deformer_list[p]
        server = m.smpl_server_list[p]
        if dr.get("z_given") is not None:
            # depths handed in by the caller instead of sampled here (the sampler runs without gradients in the reference,
            # ray_sampler.py:86-87): lets a test drive everything downstream from an INDEPENDENT sampler's depths
            zfinal, iters, wcount = dr["z_given"].to(dev).float().contiguous(), None, None
            assert zfinal.shape == (Rp, NZ), f"z_given of person {p}: {tuple(zfinal.shape)} != {(Rp, NZ)}"
        else:
            zfinal, iters, wcount = sampled
        npts = Rp * S
        E = N_EIKONAL
        Pt = npts + E
        X = torch.empty(Pt, 3, **f32)                             # canonical points: samples, then eikonal points
        # the nearest POSED vertex of every sample: the pose adjoint needs it, and it seeds the canonical nearest-vertex search
        # of the Jacobian (csrc/geom.hip k_warp_jacobian: its canonical distance is a tight, exact search radius -- the
        # unseeded search opens every cluster: 228 us instead of ~30 per person)
        nn_posed = torch.empty(npts, dtype=torch.int32, device=dev)
        nn_cano = torch.empty(npts, dtype=torch.int32, device=dev) if self.pose_grad else None
        # (a training batch's rays are random pixels: the warp first groups the samples by their nearest vertex cluster)
        bin_work = torch.empty(int(L.mp_warp_bin_work_bytes(npts)), dtype=torch.uint8, device=dev)
        L.mp_warp_inverse_shade(cx["dirs"], cx["pose"], pp["hit_index"], pp["count"], zfinal, NZ, S, Rp, pp["vsorted"],
                                pp["cbound"], pp["btab"], 0, cx["beta"], X, None, None, None, None, None, nn_posed, bin_work, st)
        jinv = torch.empty(npts, 9, **f32)
        L.mp_warp_jacobian(X, None, None, 0, 0, npts, dfm.vsorted_c, dfm.cbound_c, pp["btab"], jinv, nn_cano, nn_posed,
                           dfm.verts_c_flat, st)
        flags = None
        if self.surface_flags:        # multiply.py:311-315: in / off-surface rays w.r.t. the current canonical mesh
            src = m.mesh_face_vertices_list[p]
            sd = torch.empty(npts, **f32)
            index = None
            if src.device == X.device:       # 'auto': the index for a closed surface of hip.MESH_INDEX_MIN_FACES faces or more
                index = m.mesh_index_cache.get(p, src, m.mesh_f_cano_list[p], m.mesh_index_mode)
            if index is not None:
                index.signed_distance(X[:npts], out=sd)                               # same values as the brute-force kernel
            else:
                fv = src.detach().reshape(-1, 9).to(dev).float().contiguous()
                L.mp_mesh_signed_distance(X, npts, fv, fv.shape[0], sd, st)
            off_p = torch.empty(Rp, dtype=torch.uint8, device=dev); in_p = torch.empty(Rp, dtype=torch.uint8, device=dev)
            L.mp_mesh_ray_flags(sd, Rp, S, m.threshold, off_p, in_p, st)
            flags = (off_p.bool(), in_p.bool(), sd)
        # eikonal points near the canonical surface (multiply.py:322-327, sampler.py:84-108 with global_ratio 0)
        vc = server.verts_c.reshape(-1, 3)
        X[npts:] = vc[dr["eik_idx"]] + dr["eik_noise"] * m.sampler.local_sigma
        # all persons' stashes live from forward to backward: the fixed all-rays-hit size only while the sum stays in budget
        it = sdf_evaluator(imp, X, pp["cond"], self.ts.lins[id(imp)], self.pose_grad, p_cap=R * S + E,
                           cap_bytes=min(6 << 30, ARENA_BUDGET_BYTES // max(len(cx["persons"]), 1)))
        XA = torch.empty(npts, 6, **f32); nrm = torch.empty(npts, 3, **f32)
        sdf = it.sdf[:npts]
        # (sdf and d sdf / d x come from the evaluator as arrays of their own: the kernels' "no Z8" form)
        L.mp_tr_shade_in_fwd(None, Pt, npts, X, jinv, XA, nrm, None, it.grad, st)
        gth = torch.empty(E, 3, **f32)
        L.mp_tr_eik_fwd(None, Pt, npts, E, gth, it.grad, st)
        rt = colour_evaluator(ren, XA, it, npts, pp["cond"], self.ts.lins[id(ren)])
        self.fg[p] = dict(it=it, rt=rt, X=X, jinv=jinv, XA=XA, sdf=sdf, nrm=nrm, gth=gth, zfinal=zfinal, iters=iters,
                          wcount=wcount, npts=npts, Pt=Pt, Rp=Rp, flags=flags, nn_posed=nn_posed, nn_cano=nn_cano)
        # rows of z / sdf / rgb / nrm = the person's hit rays `rays`, found per ray through inv; hit (a mask over all rays) only
        # where the rows are all rays (_exchange); dsdf_rows: rows of the d sdf vector the backward hands to the SDF evaluator
        return dict(z=zfinal, sdf=sdf, rgb=rt.rgb, nrm=nrm, inv=pp["inv_index"], gth=gth, rays=pp["hit_index"][:Rp], hit=None,
                    off=flags[0] if flags else None, inn=flags[1] if flags else None, dsdf_rows=Pt)

    def _exchange(self, local):
        """person-sharded: THE exchange step of the forward.  Every rank's persons travel as dense per-ray rows; the persons of
        other ranks become records of R rows each (nothing of theirs is differentiated here: their owners compute the same
        compositing adjoint).  Also this rank's ray slice of the background branch."""
        cx = self.cx
        dev, R, NZ = cx["dev"], cx["R"], self.NZ
        f32 = dict(dtype=F32, device=dev)
        S, E = NZ - 1, N_EIKONAL
        world, rank = self.shard
        P_total = int(self.input["smpl_trans"].shape[1])
        n_slot = (P_total + world - 1) // world
        width = NZ + 7 * S + 3                                   # z, sdf, rgb3, nrm3 per sample; hit, off, in flags
        send = torch.zeros(n_slot, R * width + E * 3, **f32)
        for j, rec in enumerate(local):
            n_hit = int(cx["n_hit"][j])
            rows = rec["rays"][:n_hit].long()
            dense = torch.zeros(R, width, **f32)
            dense[rows, :NZ] = rec["z"][:n_hit]
            dense[rows, NZ:NZ + S] = rec["sdf"][:n_hit * S].reshape(n_hit, S)
            dense[rows, NZ + S:NZ + 4 * S] = rec["rgb"][:n_hit * S].reshape(n_hit, 3 * S)
            dense[rows, NZ + 4 * S:NZ + 7 * S] = rec["nrm"][:n_hit * S].reshape(n_hit, 3 * S)
            dense[rows, NZ + 7 * S] = 1.0
            if rec["off"] is not None:
                dense[rows, NZ + 7 * S + 1] = rec["off"][:n_hit].float()
                dense[rows, NZ + 7 * S + 2] = rec["inn"][:n_hit].float()
            send[j, :R * width] = dense.reshape(-1)
            send[j, R * width:] = rec["gth"].reshape(-1)
        bufs = [torch.empty_like(send) for _ in range(world)]
        dist.all_gather(bufs, send)
        ar = torch.arange(R, device=dev, dtype=torch.int32)
        mine = dict(zip(cx["persons"], local))
        self.all_persons, self.composited = list(range(P_total)), []
        for p in self.all_persons:
            rec = mine.get(p)
            if rec is None:
                blk = bufs[p % world][p // world]
                d = blk[:R * width].reshape(R, width)
                hit = d[:, NZ + 7 * S] > 0.5
                # (a ray the person misses is off its surface and not inside it: multiply.py:549-557)
                rec = dict(z=d[:, :NZ].contiguous(), sdf=d[:, NZ:NZ + S].contiguous(), rgb=d[:, NZ + S:NZ + 4 * S].contiguous(),
                           nrm=d[:, NZ + 4 * S:NZ + 7 * S].contiguous(), inv=torch.where(hit, ar, torch.full_like(ar, -1)).contiguous(),
                           gth=blk[R * width:].reshape(E, 3).contiguous(), rays=ar, hit=hit,
                           off=~hit | (d[:, NZ + 7 * S + 1] > 0.5), inn=hit & (d[:, NZ + 7 * S + 2] > 0.5), dsdf_rows=R * S)
            self.composited.append(rec)
        self.n_slice = n_slice = (R + world - 1) // world
        self.ray_slice = (min(R, rank * n_slice), min(R, (rank + 1) * n_slice))

    def _background_forward(self):
        """the background branch (multiply.py:482-484, 514-539) on this rank's ray slice; depths jittered per ray in training
        (ray_sampler.py:32-40).  -> bg_rgb [R][3] of all rays, or None without a frame index"""
        m, cx, L, st = self.model, self.cx, hip.lib(), hip.stream()
        dev, R, dirs = cx["dev"], cx["R"], cx["dirs"]
        f32 = dict(dtype=F32, device=dev)
        rs = m.ray_sampler
        s0, s1 = self.ray_slice
        self.bg = None
        if self.input.get("idx", None) is None:
            return None
        key = "image_id" if "image_id" in self.input else "idx"
        # the frame's row of the latent table, looked up ON THE DEVICE: int(<device tensor>) is a device -> host copy that
        # waits for everything enqueued so far (the whole previous iteration), i.e. the host could never run ahead
        w_lat = m.frame_latent_encoder.weight
        self.frame = torch.as_tensor(self.input[key]).reshape(-1)[:1].to(w_lat.device, torch.long, non_blocking=True)
        code = w_lat.detach().index_select(0, self.frame)[0].contiguous()
        NB = rs.N_samples_inverse_sphere
        Rb = s1 - s0                                              # this rank's rays of the background branch
        bdirs = dirs[s0:s1].contiguous()
        # stratified depths (ray_sampler.py:32-40): the bin edges are constants of (NB, bounding sphere) -- built once per model,
        # already flipped and scaled, so that the iteration pays one fused multiply-add instead of ten small launches
        strata = m.__dict__.get("_mp_bg_strata")
        if strata is None or strata[0] != (NB, float(rs.scene_bounding_sphere), str(dev)):
            t = torch.linspace(0.0, 1.0, NB, device=dev)[None]
            mids = 0.5 * (t[:, 1:] + t[:, :-1])
            upper = torch.cat([mids, t[:, -1:]], -1); lower = torch.cat([t[:, :1], mids], -1)
            c = 1.0 / rs.scene_bounding_sphere
            strata = m.__dict__["_mp_bg_strata"] = ((NB, float(rs.scene_bounding_sphere), str(dev)),
                                                    torch.flip(lower * c, dims=[-1]).contiguous(),
                                                    torch.flip((upper - lower) * c, dims=[-1]).contiguous())
        # zbg = flip((lower + (upper - lower) u) / r) = flip(lower / r) + flip((upper - lower) / r) flip(u)
        zbg = torch.addcmul(strata[1], strata[2], torch.flip(self.draws["bg_rand"][s0:s1], dims=[-1])).contiguous()
        bg_rgb = torch.zeros(R, 3, **f32) if Rb != R else None
        if Rb > 0:
            rows = Rb * NB
            pts = torch.empty(rows, 4, **f32)
            cam = cx["pose"].reshape(4, 4)[:3, 3].contiguous()
            L.mp_tr_bg_points(bdirs, cam, zbg, Rb, NB, m.sdf_bounding_sphere, pts, st)
            bit = bg_evaluator(m.bg_implicit_network, pts, code, self.ts.lins[id(m.bg_implicit_network)])
            drep = bdirs[:, None, :].expand(Rb, NB, 3).reshape(-1, 3).contiguous()
            XAb = torch.empty(rows, 27, **f32)
            L.mp_tr_pe(drep, 3, rows, 4, 0, 1.0, XAb, 27, 0, st)
            brt = colour_evaluator(m.bg_rendering_network, XAb, bit, rows, code, self.ts.lins[id(m.bg_rendering_network)])
            sdfb = bit.sdf[:rows]
            bg_slice = torch.empty(Rb, 3, **f32)
            L.mp_tr_bg_comp_fwd(sdfb, brt.rgb, zbg, Rb, NB, bg_slice, st)
            if bg_rgb is None:
                bg_rgb = bg_slice                                 # the whole call's rays: no scatter into a zero image
            else:
                bg_rgb[s0:s1] = bg_slice
            self.bg = dict(it=bit, rt=brt, zbg=zbg, sdfb=sdfb, XAb=XAb, NB=NB, code=code, pts=pts, Rb=Rb)
        if self.shard is not None:                                # every rank composites all rays
            pad = torch.zeros(self.n_slice, 3, **f32)
            pad[:Rb] = bg_rgb[s0:s1]
            parts = [torch.empty_like(pad) for _ in range(self.shard[0])]
            dist.all_gather(parts, pad)
            bg_rgb = torch.cat(parts, 0)[:R].contiguous()
        return bg_rgb

    def _composite(self):
        """compositing of all persons and the background (multiply.py:425-480, 544-545) -> the node's outputs"""
        cx, L, bg_rgb = self.cx, hip.lib(), self.bg_rgb
        dev, R = cx["dev"], cx["R"]
        f32 = dict(dtype=F32, device=dev)
        self.tabs = tuple(_table([rec[k] for rec in self.composited], dev) for k in ("inv", "z", "sdf", "rgb", "nrm"))
        t_inv, t_z, t_sdf, t_rgb, t_nrm = self.tabs
        P = len(self.composited)
        rgb_values = torch.empty(R, 3, **f32); fg_rgb_values = torch.empty(R, 3, **f32)
        normal_values = torch.empty(R, 3, **f32); acc_map = torch.empty(R, **f32)
        acc_person = torch.empty(R, P, **f32); bg_T = torch.empty(R, **f32)
        L.mp_composite(R, P, self.NZ, t_inv, t_z, t_sdf, t_rgb, t_nrm, cx["beta"], bg_rgb, rgb_values, fg_rgb_values,
                       normal_values, acc_map, acc_person, bg_T, hip.stream())
        grad_theta = torch.cat([rec["gth"] for rec in self.composited], 0)[None]               # multiply.py:565
        self.bg_T = bg_T
        outs = (rgb_values, normal_values, acc_map, acc_person, grad_theta)
        if self.reg_items:
            outs = outs + self.reg_losses
        if self.pen_on:
            outs, self.pen_loss = outs + (self.pen_loss,), None
        if self.geometry:
            outs = outs + self._composite_geometry()
        return outs

    def _composite_geometry(self):
        """train_geometry: mp_composite_geometry on the compositing's own tables -> the tensors of GEOMETRY_KEYS, in that order"""
        cx = self.cx
        dev, R, P = cx["dev"], cx["R"], len(self.composited)
        f32 = dict(dtype=F32, device=dev)
        self.level = float(self.model.geometry_level)
        depth = torch.empty(R, **f32); depth_person = torch.empty(R, P, **f32); acc_solo = torch.empty(R, P, **f32)
        depth_solo = torch.empty(R, P, **f32); depth_solo_level = torch.empty(R, P, **f32)
        depth_level = torch.empty(R, **f32); front = torch.empty(R, dtype=torch.int32, device=dev)
        t_inv, t_z, t_sdf = self.tabs[:3]
        hip.lib().mp_composite_geometry(R, P, self.NZ, t_inv, t_z, t_sdf, cx["beta"], self.level, depth, depth_person, depth_level,
                                        front, acc_solo, depth_solo, depth_solo_level, hip.stream())
        return depth, depth_person, acc_solo, depth_solo, depth_solo_level, depth_level, front

    # ---- the two optional regularisers (multiply.py:336-394) -----------------------------------------------------------------
    def _regularisers_forward(self):
        """smpl_surface: the SDF at `num_pixels` posed SMPL vertices (head / hands / feet left out), warped to canonical space, must not
        exceed 0.02 -- mean of (sdf - 0.02) over the offenders, per rendered person.  zero_pose: for every rendered person q and every
        network p, the network's outputs at 2 000 vertices of p's canonical mesh under q's pose conditioning vs under a zero
        conditioning -- L1 of the sdf + L1 of the features (the reference pairs q's conditioning with network p exactly like this).
        Value-only passes of the SDF net, layer by layer (ImplicitTrain) on the iteration's shared weights; their adjoints run at the
        head of the backward sweep, before any person's weight-norm adjoint retires its accumulators."""
        m, cx, L, st = self.model, self.cx, hip.lib(), hip.stream()
        dev = cx["dev"]
        if self.pose_grad and m.smpl_surface_weight > 0 and not getattr(m, "smpl_surface_pose_grad", False):
            # (the surface term reaches the pose through the sampled posed VERTICES, their warp and the conditioning; that adjoint is
            # built -- SMPLServer.pose_backward -- but opt-in: model.smpl_surface_pose_grad = True or MP_SMPL_SURFACE_POSE_GRAD=1)
            raise NotImplementedError("smpl_surface with body-model inputs under optimisation is opt-in: set model.smpl_surface_pose_grad "
                                      "= True (or MP_SMPL_SURFACE_POSE_GRAD=1)")
        ssl = torch.zeros(1, dtype=F32, device=dev)
        zpl = torch.zeros(1, dtype=F32, device=dev)
        for q in cx["persons"]:
            pp = cx["per"][q]
            cond = pp["cond"]
            if m.smpl_surface_weight > 0:
                imp = m.foreground_implicit_network_list[q]
                idx = self.draws["person"][q]["surf_idx"].to(dev).long()
                pts = pp["verts"].index_select(0, idx).contiguous()
                n = pts.shape[0]
                xc = torch.empty(n, 3, dtype=F32, device=dev)
                L.mp_warp_inverse(pts, None, None, None, None, None, 0, 1, n, pp["vsorted"], pp["cbound"], pp["btab"], 0, None,
                                  None, xc, None, None, None, None, None, st)
                warp = None
                if self.pose_grad:
                    # the backward needs the nearest posed vertex of every sample (ties: lowest id) and its inverse blended
                    # transform I_nn: the same exact search over the posed vertex structure (the weights are constants, deformer.py:47)
                    jv = torch.empty(n, 9, dtype=F32, device=dev)
                    nn = torch.empty(n, dtype=torch.int32, device=dev)
                    L.mp_warp_jacobian(pts, None, None, 0, 0, n, pp["vsorted"], pp["cbound"], pp["btab"], jv, nn, None, None, st)
                    warp = (xc, jv, nn, idx.to(torch.int32).contiguous())
                it = ImplicitTrain(imp, xc, cond, fwd=False, lins=self.ts.lins[id(imp)])
                sdf = it.out[:, 0]
                mask = sdf > SMPL_SURFACE_THRESHOLD
                cnt = mask.sum().clamp(min=1).to(F32)
                ssl = ssl + torch.where(mask, sdf - SMPL_SURFACE_THRESHOLD, torch.zeros_like(sdf)).sum() / cnt      # 0 when none offends
                self.reg_items.append(("surf", it, mask, cnt, q, warp))
            if m.zero_pose_weight > 0:
                for p, vcano in enumerate(m.mesh_v_cano_list):
                    net = m.foreground_implicit_network_list[p]
                    pts = vcano.reshape(-1, 3).to(dev).float().index_select(0, self.draws["zp_idx"][(q, p)].to(dev).long()).contiguous()
                    lins = self.ts.lins[id(net)]
                    it1 = ImplicitTrain(net, pts, cond, fwd=False, lins=lins)
                    it0 = ImplicitTrain(net, pts, torch.zeros_like(cond), fwd=False, lins=lins)
                    d = it1.out - it0.out
                    zpl = zpl + d[:, 0].abs().mean() + d[:, 1:].abs().mean()
                    self.reg_items.append(("zero", it1, it0, torch.sign(d), q))
        self.reg_losses = (ssl, zpl)

    def _regularisers_backward(self, d_ssl, d_zpl):
        dev = self.cx["dev"]
        self.reg_dcond, self.reg_surf = {}, {}
        L, st = hip.lib(), hip.stream()
        for item in self.reg_items:
            if item[0] == "surf":
                _, it, mask, cnt, q, warp = item
                if d_ssl is None:
                    continue
                dZ = torch.zeros(it.P, 257, dtype=F32, device=dev)
                dZ[:, 0] = d_ssl.reshape(()) * mask.to(F32) / cnt
                dcond = it.backward(dZ, want_dx=warp is not None)
                if warp is not None:
                    # x_c = I_nn (x - c_nn), x = verts[surf_idx]: d tfs through the blended transform (mp_tr_warp_bwd), d x = I_nn^T d x_c
                    # gathered onto the drawn vertices in sample order (mp_tr_gather_bwd; the draw repeats vertices)
                    xc, jv, nn, idx = warp
                    n = xc.shape[0]
                    pp, server = self.cx["per"][q], self.model.smpl_server_list[q]
                    dxc = it.dx.contiguous()
                    dtfs = torch.zeros(24, 16, dtype=F32, device=dev)
                    warp_bwd(xc, dxc, None, None, nn, None, n, server.tables.lbs_weights, pp["tfs"], dtfs)
                    dverts = torch.zeros(server.verts_c.reshape(-1, 3).shape[0], 3, dtype=F32, device=dev)
                    L.mp_tr_gather_bwd(idx, n, jv, dxc, dverts.shape[0], dverts, st)
                    prev = self.reg_surf.get(q)
                    self.reg_surf[q] = (dtfs, dverts) if prev is None else (prev[0] + dtfs, prev[1] + dverts)
                    if not self.cond_zero:
                        self.reg_dcond[q] = dcond if q not in self.reg_dcond else self.reg_dcond[q] + dcond
            else:
                _, it1, it0, sg, q = item
                if d_zpl is None:
                    continue
                n = sg.shape[0]
                dZ = torch.empty(n, 257, dtype=F32, device=dev)
                dZ[:, 0] = sg[:, 0] * (d_zpl.reshape(()) / n)
                dZ[:, 1:] = sg[:, 1:] * (d_zpl.reshape(()) / (n * 256))
                dcond = it1.backward(dZ)
                it0.backward(-dZ)
                if self.pose_grad and not self.cond_zero:
                    # person q's conditioning = smpl_pose[q, 3:] / pi (multiply.py:270): the term's only path to the body-model inputs
                    self.reg_dcond[q] = dcond if q not in self.reg_dcond else self.reg_dcond[q] + dcond

    # ---- the interpenetration term (Multiply.train_interpenetration) ---------------------------------------------------------
    def _interpenetration_forward(self):
        """the term of this call's persons on the iteration's shared weights; a single person has no pairs: zeros, no launch.
        With no body input under optimisation the term is value-only and keeps no stash."""
        cx = self.cx
        if len(cx["persons"]) < 2:
            self.pen_loss = torch.zeros(1, dtype=F32, device=cx["dev"])
            return
        missing = [p for p in cx["persons"] if "pen_idx" not in self.draws["person"][p]]
        if missing:
            raise KeyError(f"train_interpenetration: the draws of persons {missing} carry no 'pen_idx' (make_draws draws it with the flag on)")
        pen = Interpenetration(self.model, cx, {p: self.draws["person"][p]["pen_idx"] for p in cx["persons"]},
                               lins_of=lambda net: self.ts.lins[id(net)], keep=self.pose_grad)
        # the loss becomes an output of the autograd node, which holds this graph: neither the graph nor the term may keep it
        # (a reference cycle would keep the iteration's stashes alive until the garbage collector runs); _composite hands it over
        self.pen_loss, pen.loss = pen.loss, None
        self.pen = pen if self.pose_grad else None

    def _interpenetration_backward(self, d_pen):
        """the term's shares of d tfs / d posed vertices join the smpl_surface term's: ONE server.pose_backward per person"""
        for p, (dtfs, dverts) in self.pen.backward(d_pen).items():
            prev = self.reg_surf.get(p)
            self.reg_surf[p] = (dtfs, dverts) if prev is None else (prev[0] + dtfs, prev[1] + dverts)

    # ---- backward -----------------------------------------------------------------------------------------------
    @_in_graph_mode
    def backward(self, d_rgb_values, d_acc_map, d_acc_person, d_grad_theta, d_ssl=None, d_zpl=None, d_geometry=None, d_pen=None):
        """-> {id(parameter): gradient}.  d_geometry: the upstream gradients of GEOMETRY_KEYS[:5] (train_geometry), None = no term;
        d_pen: the upstream gradient of the interpenetration term (train_interpenetration), None = unused"""
        m, dev = self.model, self.cx["dev"]
        self.ts.start_backward()                  # this sweep's own accumulators / gradient buffer (TrainState.start_backward)
        self.reg_dcond, self.reg_surf = {}, {}
        if self.reg_items:                        # before any finish_group retires a network's accumulators
            self._regularisers_backward(d_ssl, d_zpl)
        if self.pen is not None and d_pen is not None:
            self._interpenetration_backward(d_pen)
        self.zp = _ZP[0] = hip.ZeroPool(dev)      # this sweep's zero-initialised tensors: views of one zero-filled block
        dsdf_l, drgb_l, d_bg_rgb, d_beta = self._composite_backward(d_rgb_values, d_acc_map, d_acc_person, d_geometry)
        self.grads, self.pose_grads = {}, {}
        # data-parallel training: buckets of retired gradients are all-reduced while the sweep goes on (parallel.BucketedGradientSync)
        sync = self.sync = getattr(m, "grad_bucket_sync", None)
        # the buckets retire in the order of THIS rank's persons: person-sharded ranks own different persons, so their bucket
        # sizes and counts differ and the collectives would mismatch -- that mode sums its shared gradients with PersonShardedGradSync
        assert sync is None or self.shard is None, "grad_bucket_sync (ray-/frame-sharded data parallelism) cannot be combined with shard="
        for p in self.cx["persons"]:
            n = self.all_persons.index(p)                             # position among the composited persons
            dgth = None
            if d_grad_theta is not None:
                dgth = d_grad_theta.reshape(-1, 3)[n * N_EIKONAL:(n + 1) * N_EIKONAL].contiguous().float()
            dcond, dXA, djinv = self._person_backward(p, dsdf_l[n], drgb_l[n], dgth)
            if self.pose_grad:
                self._pose_backward(p, dcond, dXA, djinv)
        if self.bg is not None:
            self._background_backward(d_bg_rgb)
        bp = m.density.beta
        # (handed over, not kept: autograd takes a gradient as param.grad without a copy only while nothing else references it)
        grads, self.grads = self.grads, None
        grads[id(bp)] = (d_beta.reshape(bp.shape) * torch.sign(bp.detach())).to(bp.dtype)     # density.py:31-33
        if sync is not None:
            b = self.bg
            tail = [bp] + ([m.frame_latent_encoder.weight] + b["it"].params() + b["rt"].params() if b is not None else [])
            sync.retire(tail, [grads[id(prm)] for prm in tail])
            grads = sync.finish(grads)
        _ZP[0] = None
        return grads

    def _collect(self, *objs, retire=True):
        """the evaluators' parameter gradients into self.grads; retire: in data-parallel training they leave as one bucket"""
        grads = self.grads
        for obj in objs:
            for prm, g in zip(obj.params(), obj.param_grads()):
                grads[id(prm)] = g if id(prm) not in grads else grads[id(prm)] + g
        if retire and self.sync is not None:
            prms = [prm for o in objs for prm in o.params()]
            self.sync.retire(prms, [grads[id(prm)] for prm in prms])

    def _composite_backward(self, d_rgb_values, d_acc_map, d_acc_person, d_geometry=None):
        """adjoint of mp_composite (and, train_geometry, of mp_composite_geometry: accumulated onto the same d sdf / d beta)
        -> per composited person d sdf and d rgb, d bg_rgb [R][3], d beta"""
        cx, zp = self.cx, self.zp
        dev, R = cx["dev"], cx["R"]
        P = len(self.composited)
        t_inv, t_z, t_sdf, t_rgb, _ = self.tabs
        zero = lambda t, shape: zp.take(shape) if t is None else t.contiguous().float()
        d_rgb_values = zero(d_rgb_values, (R, 3)); d_acc_map = zero(d_acc_map, (R,)); d_acc_person = zero(d_acc_person, (R, P))
        # persons of other ranks (person-sharded mode) get scratch rows: their owners compute the same compositing adjoint
        # (a local person's d sdf vector also covers its eikonal points, which no compositing term reaches: zeros)
        dsdf_l = [zp.take(rec["dsdf_rows"]) for rec in self.composited]
        drgb_l = [zp.take(rec["rgb"].numel() // 3, 3) for rec in self.composited]
        d_bg_rgb = zp.take(R, 3)
        d_beta = zp.take(1)
        t_dsdf, t_drgb = _table(dsdf_l, dev), _table(drgb_l, dev)
        det = _det()
        part = torch.empty(max(R, 1), dtype=F32, device=dev) if det else None      # the rays' own d beta sums (deterministic form)
        if det:
            hip.lib().mp_tr_composite_bwd_det(R, P, self.NZ, t_inv, t_z, t_sdf, t_rgb, cx["beta"], self.bg_rgb, d_rgb_values,
                                              d_acc_map, d_acc_person, t_dsdf, t_drgb, d_bg_rgb, d_beta, part, hip.stream())
        else:
            hip.lib().mp_tr_composite_bwd(R, P, self.NZ, t_inv, t_z, t_sdf, t_rgb, cx["beta"], self.bg_rgb, d_rgb_values, d_acc_map,
                                          d_acc_person, t_dsdf, t_drgb, d_bg_rgb, d_beta, hip.stream())
        if d_geometry is not None and any(g is not None for g in d_geometry):
            # after the store above, on the same stream: the kernel adds (a missing upstream gradient is a NULL pointer)
            d_depth, d_depth_person, d_acc_solo, d_depth_solo, d_depth_solo_level = (
                None if g is None else g.contiguous().float() for g in d_geometry)
            if det:
                hip.lib().mp_tr_composite_geometry_bwd_det(R, P, self.NZ, t_inv, t_z, t_sdf, cx["beta"], self.level, d_depth,
                                                           d_depth_person, d_acc_solo, d_depth_solo, d_depth_solo_level, t_dsdf,
                                                           d_beta, part, hip.stream())
            else:
                hip.lib().mp_tr_composite_geometry_bwd(R, P, self.NZ, t_inv, t_z, t_sdf, cx["beta"], self.level, d_depth,
                                                       d_depth_person, d_acc_solo, d_depth_solo, d_depth_solo_level, t_dsdf, d_beta,
                                                       hip.stream())
        return dsdf_l, drgb_l, d_bg_rgb, d_beta

    def _person_backward(self, p, dsdf, drgb, dgth):
        """colour net, normals / eikonal term, SDF net of person p; retires the person's two networks.
        -> d cond, dXA [npts][6], d Jinv [npts][9] (pose optimisation)"""
        L, st = hip.lib(), hip.stream()
        f = self.fg[p]
        it, rt, npts, Pt = f["it"], f["rt"], f["npts"], f["Pt"]
        f32 = dict(dtype=F32, device=self.cx["dev"])
        dgrad = self.zp.take(Pt, 3)
        dXA = torch.empty(npts, 6, **f32)
        dfeat = it.new_dfeat(npts)     # (the eikonal points have no colour path)
        tn_groups = []                 # the person's aligned weight-gradient contractions: ONE grouped launch below
        rt.backward(drgb, dXA, *it.dfeat_target(dfeat), tn_groups=tn_groups)
        djinv = torch.empty(npts, 9, **f32) if self.pose_grad else None
        L.mp_tr_shade_in_bwd(None, Pt, npts, f["jinv"], dXA, dsdf, None, None, djinv, it.grad, dgrad, st)
        if dgth is not None:
            L.mp_tr_eik_bwd(Pt, npts, N_EIKONAL, dgth, None, dgrad, st)
        dcond = it.backward(dfeat, dsdf, dgrad, want_dx=self.pose_grad, tn_groups=tn_groups)
        launch_tn_groups(tn_groups)
        self.ts.finish_group(p)                                   # one batched weight-norm adjoint for the person's two nets
        self._collect(it, rt)
        return dcond, dXA, djinv

    def _pose_backward(self, p, dcond, dXA, djinv):
        """pose optimisation: x_c enters the SDF net (value + gradient sweep) and the colour net (XA[:, :3]); the transforms also shape
        the normals through Jinv.  -> d tfs -> d (scale, transl, thetas, betas)   (multiply.py:196-206, 270)"""
        m, cx, L, st = self.model, self.cx, hip.lib(), hip.stream()
        f32 = dict(dtype=F32, device=cx["dev"])
        f, pp, server = self.fg[p], cx["per"][p], m.smpl_server_list[p]
        npts = f["npts"]
        dxc = (f["it"].dx[:npts] + dXA[:, :3]).contiguous()
        dtfs = torch.zeros(24, 16, **f32)
        warp_bwd(f["X"], dxc, f["jinv"], djinv, f["nn_posed"], f["nn_cano"], npts, server.tables.lbs_weights, pp["tfs"], dtfs)
        surf = self.reg_surf.get(p)
        if surf is None:
            dprm = torch.empty(86, **f32)
            L.mp_smpl_pose_bwd(server.tables.parents, pp["prm"], server.tfs_c_inv, pp["rest_joints"], server.tables.j_shapedirs,
                               dtfs, dprm, st)
        else:                                                    # + the surface term's posed vertices and transforms
            dprm = server.pose_backward(pp["prm"], dverts=surf[1], dtfs=dtfs + surf[0])
        if not self.cond_zero:                                   # cond = smpl_pose[3:] / pi  (multiply.py:270)
            dc = dcond + f["rt"].dcond()
            if p in self.reg_dcond:                              # + the regularisers' share (zero pose; surface, opt-in)
                dc = dc + self.reg_dcond[p]
            dprm[7:76] += dc / math.pi
        self.pose_grads[p] = dprm

    def _background_backward(self, d_bg_rgb):
        """inverse-sphere compositing, colour net, ImplicitNet of the background on this rank's ray slice; d frame code"""
        m, L, st = self.model, hip.lib(), hip.stream()
        f32 = dict(dtype=F32, device=self.cx["dev"])
        b = self.bg
        bit, brt, NB, Rb = b["it"], b["rt"], b["NB"], b["Rb"]
        rows = Rb * NB
        s0, s1 = self.ray_slice
        d_bg_slice = d_bg_rgb[s0:s1].contiguous()
        dsdfb = torch.empty(rows, **f32); drgbb = torch.empty(rows, 3, **f32)
        L.mp_tr_bg_comp_bwd(b["sdfb"], brt.rgb, b["zbg"], Rb, NB, d_bg_slice, dsdfb, drgbb, st)
        dXAb = torch.empty(rows, 27, **f32)
        dfeatb = bit.new_dfeat(rows)
        dcode = brt.backward(drgbb, dXAb, *bit.dfeat_target(dfeatb))
        dcode = dcode + bit.backward(dfeatb, dsdfb)
        self.ts.finish_group("bg")
        self._collect(bit, brt, retire=False)                     # (they leave with the sweep's tail bucket)
        w = m.frame_latent_encoder.weight
        gw = self.zp.take(tuple(w.shape), dtype=w.dtype)
        gw.index_copy_(0, self.frame, dcode.reshape(1, -1))
        self.grads[id(w)] = gw


class _TrainFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, graph, smpl_pose, smpl_trans, smpl_shape, *params):
        ctx.graph, ctx.params = graph, params
        ctx.body = (smpl_pose, smpl_trans, smpl_shape)
        outs = graph.run()
        if graph.geometry or graph.pen_on:
            # the unused ones of the geometry outputs must arrive as None (a NULL pointer skips the term), not as zero tensors;
            # an unused interpenetration term likewise (None: its adjoint sweep does not run)
            ctx.set_materialize_grads(False)
        if graph.geometry:
            ctx.mark_non_differentiable(outs[1], *outs[-2:])      # + depth_level_values, front_person: no adjoint
        else:
            ctx.mark_non_differentiable(outs[1])      # normal_values: no loss term reads it (loss.py:108-177)
        return outs

    @staticmethod
    def backward(ctx, d_rgb, d_nrm, d_acc, d_accp, d_gth, *rest):
        graph = ctx.graph
        d_geo = d_pen = None
        if graph.geometry:
            rest, d_geo = rest[:-len(GEOMETRY_KEYS)], rest[-len(GEOMETRY_KEYS):-2]
        if graph.pen_on:
            rest, d_pen = rest[:-1], rest[-1]
        d_ssl, d_zpl = rest if rest else (None, None)
        g = graph.backward(d_rgb, d_acc, d_accp, d_gth, d_ssl, d_zpl, d_geo, d_pen)
        body = [None, None, None]
        if graph.pose_grad:
            sl = ((4, 76), (1, 4), (76, 86))
            for k, t in enumerate(ctx.body):
                if t is not None and ctx.needs_input_grad[1 + k]:
                    gt = torch.zeros_like(t)
                    for p, dprm in graph.pose_grads.items():
                        gt[0, p] = dprm[sl[k][0]:sl[k][1]].to(t.device)
                    body[k] = gt
        return (None, *body) + tuple(g.get(id(p)) for p in ctx.params)


# Multiply.train_geometry: the keys of Multiply._composite_geometry in the order the training node returns them -- the five
# differentiable ones, then the merged crossing (no adjoint)
GEOMETRY_KEYS = ("depth_values", "depth_person_list", "acc_person_solo_list", "depth_person_solo_list",
                 "depth_person_solo_level_list", "depth_level_values", "front_person")


def forward_train(model, input, id=-1, cond_zero_shit=False, canonical_pose=False, draws=None, shard=None):
    """Multiply.forward with self.training == True.  Returns the reference's 19-key dict (multiply.py:566-588); the five
    tensors rgb_values / acc_map / acc_person_list / grad_theta (/ normal_values, not differentiable) hang off ONE autograd
    node whose backward is the hand-written adjoint sweep.  With model.train_geometry the dict also carries GEOMETRY_KEYS
    (Multiply._composite_geometry's names and shapes, columns = acc_person_list's) off the same node."""
    epoch = int(input["current_epoch"])
    if shard is not None and deterministic(model):
        raise NotImplementedError("person-sharded training (shard=) is not built for the deterministic training mode: the ranks' "
                                  "shared gradients are summed by collectives whose order this mode does not fix")
    if shard is not None and model.training and getattr(model, "train_geometry", False):
        raise NotImplementedError("train_geometry is not built for person-sharded training (shard=)")
    if shard is not None and model.training and getattr(model, "train_interpenetration", False):
        raise NotImplementedError("train_interpenetration is not built for person-sharded training (shard=): a rank holds only its own "
                                  "persons' fields")
    if (model.smpl_surface_weight > 0 or model.zero_pose_weight > 0) and shard is not None:
        raise NotImplementedError("the smpl_surface / zero_pose regularisers (multiply.py:336-394) are not built for person-sharded training")
    if model.zero_pose_weight > 0 and not (isinstance(id, int) and id == -1):
        # the zero-pose term evaluates EVERY person's network (multiply.py:377-394); the adjoint sweep retires only the rendered
        # persons' networks, so the other networks' weight gradients would be dropped while the loss value contains their terms
        raise NotImplementedError("zero_pose_weight > 0 with a subset of the persons rendered (id != -1): the regulariser's gradients to "
                                  "the networks that are not rendered are not collected")
    if shard is not None:                   # person-sharded: this rank evaluates persons {p : p % world == rank}
        assert id == -1, "person-sharded training renders all persons"
        id = [p for p in range(int(input["smpl_trans"].shape[1])) if p % shard[0] == shard[1]]
    # the setup's one host sync must not wait for the previous iteration's backward pass (Multiply._setup); opt in when the
    # inputs are resident (model.async_setup = True: bench.py, a prefetching data loader)
    cx = model._setup(input, id, canonical_pose, side_stream=bool(getattr(model, "async_setup", False)))
    dev = cx["dev"]
    cond_zero = epoch < 20 or epoch % 20 == 0 or bool(cond_zero_shit)              # multiply.py:271-273
    if draws is None:
        draws = make_draws(model, cx)
    body = [input["smpl_pose"], input["smpl_trans"], input["smpl_shape"]]
    pose_grad = (not canonical_pose) and any(torch.is_tensor(t) and t.requires_grad for t in body)
    graph = TrainGraph(model, cx, input, cond_zero, draws, surface_flags=epoch < 250, pose_grad=pose_grad, shard=shard)
    params = [p for p in model.parameters() if p.requires_grad]
    with torch.enable_grad():                                                       # multiply.py:176
        outs = _TrainFn.apply(graph, *body, *params)
        rgb_values, normal_values, acc_map, acc_person, grad_theta = outs[:5]
        geometry = ()
        if graph.geometry:
            outs, geometry = outs[:-len(GEOMETRY_KEYS)], outs[-len(GEOMETRY_KEYS):]
        interpenetration_loss = None
        if graph.pen_on:
            outs, interpenetration_loss = outs[:-1], outs[-1]
        smpl_surface_loss, zero_pose_loss = (outs[5], outs[6]) if len(outs) == 7 else (None, None)
        temporal_loss = torch.zeros(1, device=dev)
        if epoch > 250:                                                             # multiply.py:242-243
            temporal_loss = torch.mean(torch.square(input["smpl_pose_last"].to(dev) - input["smpl_pose"].to(dev)))
    cam = cx["pose"].reshape(4, 4)[:3, 3]
    last = graph.composited[-1]
    hit, z = last["rays"], last["z"]
    if last["hit"] is not None:             # person-sharded, the last person lives on another rank: its rows are all rays
        hit = torch.nonzero(last["hit"]).flatten()
        if hit.numel() == 0:
            hit = torch.zeros(1, dtype=torch.long, device=dev)      # the reference's empty-hit fallback, multiply.py:262-263
        z = z[hit]
    hit = hit.long()
    points = cam[None, None, :] + z[:, :-1, None] * cx["dirs"][hit][:, None, :]
    _z3 = torch.zeros(3, device=dev)            # the dict's constant zero entries: one fill
    _zi = iter(range(3))
    zeros1 = lambda: _z3[next(_zi):][:1]
    index_off_surface = index_in_surface = None
    if epoch < 250:                                                                 # multiply.py:549-557
        P = len(graph.composited)
        off_all = torch.ones(cx["R"], P, dtype=torch.bool, device=dev)
        in_all = torch.zeros(cx["R"], P, dtype=torch.bool, device=dev)
        for n, rec in enumerate(graph.composited):
            rays = rec["rays"].long()
            off_all[rays, n] = rec["off"]
            in_all[rays, n] = rec["inn"]
        index_off_surface, index_in_surface = off_all.all(dim=1), in_all.any(dim=1)
    out = {
        "zero_pose_loss": zero_pose_loss if zero_pose_loss is not None else zeros1(), "t_list": [], "fg_rgb_values_each_person_list": [],
        "cam_loc": cam[None].expand(cx["R"], 3), "hitted_mask_idx": [], "mean_hitted_vertex_list": [],
        "points": points, "rgb_values": rgb_values, "normal_values": normal_values,
        "index_outside": input.get("index_outside"), "index_off_surface": index_off_surface,
        "index_in_surface": index_in_surface,
        "acc_map": acc_map, "grad_theta": grad_theta,
        "interpenetration_loss": interpenetration_loss if interpenetration_loss is not None else zeros1(), "temporal_loss": temporal_loss,
        "acc_person_list": acc_person, "smpl_surface_loss": smpl_surface_loss if smpl_surface_loss is not None else zeros1(),
        "epoch": input["current_epoch"],
    }
    if "sam_mask" in input:
        out["sam_mask"] = input["sam_mask"].squeeze()
    out.update(zip(GEOMETRY_KEYS, geometry))
    model._last_train = graph
    model.last_stats = {"n_hit": cx["n_hit"], "iters": [graph.fg[p]["iters"] for p in cx["persons"]],
                        "n_sdf_evals": [graph.fg[p]["wcount"] for p in cx["persons"]],
                        "hull_host_fallbacks": getattr(model, "hull_host_fallbacks", 0)}
    return out
