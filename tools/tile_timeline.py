#!/usr/bin/env python
"""Ablation tool: shader-clock timeline of the last TWO tiles of workgroup 0 of k_mlp_sdf (library built with -DMP_EXP_STAMP):
tile-level phases (input staging, prologue, network, output) and the start time of every weight chunk per wave.
    MP_LIB_PATH=.../libmultiply_hip_stamp.so python tools/tile_timeline.py [sdf | fwdsave | grad | color] [--fold]
--fold: the shading kernels in feature-fold mode (mp_mlp_shade_rev_fold on the 'sdf' pack, hip.FoldedColor)"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multiply_amd import hip
from tests.util import seeded_networks
m, _ = seeded_networks(2, 0); m = m.cuda()
imp = m.foreground_implicit_network_list[0]
n = 256 * 256 * 30
x = (torch.rand(n, 3, device="cuda") - 0.5) * 1.6
cond = torch.randn(69, device="cuda") * 0.1
L = hip.lib()
L.mp_debug_stamps.argtypes = [C.c_void_p]; L.mp_debug_stamps.restype = C.c_int
buf = np.zeros(8 * 128 * 4, dtype=np.uint64)
FOLD = "--fold" in sys.argv
sys.argv = [a for a in sys.argv if a != "--fold"]
which = sys.argv[1] if len(sys.argv) > 1 else "sdf"       # sdf | fwdsave | grad | color (the last kernel launched is stamped)
ren = m.foreground_rendering_network_list[0]
jinv = torch.eye(3, device="cuda").reshape(1, 9).repeat(n, 1).contiguous()
for _ in range(2):
    if which == "sdf":
        hip.implicit_sdf(imp, x, cond)
    elif which == "color":
        hip.shade_points(imp, ren, x, jinv, cond, fold=FOLD)
    else:
        pki = hip.packed(imp, "sdf" if FOLD else "full", 2); pki.refresh(cond)
        sdf = torch.empty(n, device="cuda"); nrm = torch.empty(n, 3, device="cuda")
        feat = torch.empty((n + 255) // 256 * 4 * 8 * 4 * 1024, dtype=torch.uint8, device="cuda")
        if which == "grad":
            hip.shade_rev_launch(pki, hip.grad_net(imp), x, jinv, None, None, n, sdf, nrm, feat, fold=FOLD)
        else:   # fwdsave: launch the pair, then the forward sweep alone is not separable -> stamp build marks only fwdsave
            os.environ["MP_TIMELINE_FWD_ONLY"] = "1"
            hip.shade_rev_launch(pki, hip.grad_net(imp), x, jinv, None, None, n, sdf, nrm, feat, fold=FOLD)
torch.cuda.synchronize()
assert L.mp_debug_stamps(buf.ctypes.data) == 0
s = buf.reshape(8, 128, 4).astype(np.int64)
# the workgroup's tiles alternate between slots (120, 121) and (122, 123) (MP_TILE_SLOT): its last two tiles survive
first = lambda base: s[:, base, 0].min() if s[:, base, 0].min() > 0 else s[:, base, 2].min()   # kernels without the staging stamps
order = sorted((120, 122), key=first)
if first(order[0]) == 0:          # a workgroup that ran one tile only
    order = order[1:]
t0 = first(order[0])
PH = {"tile start": (0, 0), "inputs staged": (0, 1), "prologue done": (0, 2), "network done": (0, 3), "outputs written": (1, 0)}
for k, base in enumerate(order):
    print(f"tile {k + 1 - len(order)} (0 = the workgroup's last): phases in cycles from the earlier tile's start, per wave 0..7")
    for name, (ds, ev) in PH.items():
        print(f"  {name:16s}", (s[:, base + ds, ev] - t0).tolist())
if len(order) == 2:
    a, b = order
    med = lambda v: int(np.median(v))
    head = [med(s[:, x, 2] - s[:, x, 0]) for x in order]
    net = [med(s[:, x, 3] - s[:, x, 2]) for x in order]
    tail = [med(s[:, x + 1, 0] - s[:, x, 3]) for x in order]
    print("per tile, median over the waves:   head (tile start -> first M phase)  network  tail (last V phase -> outputs written)")
    for k in range(2):
        print(f"  tile {k - 1}: head {head[k]:6d}  network {net[k]:7d}  tail {tail[k]:6d}   outside run_net {head[k] + tail[k]:6d} = "
              f"{100.0 * (head[k] + tail[k]) / (head[k] + net[k] + tail[k]):.1f} %")
    print(f"  tile -1 outputs written -> tile 0 start (median): {med(s[:, b, 0] - s[:, a + 1, 0])}")
    print(f"  tile period (start to start, median): {med(s[:, b, 0] - s[:, a, 0])} cycles")
nch = int((s[0, :120, 0] > 0).sum())
print(f"{nch} chunks; per chunk and wave (0 = first wave of SIMD 0, 4 = second): start, then the spans between the stamps")
print("  phase-separated layers: waves 0..3: M | V | barrier wait;  waves 4..7: M | barrier wait + DMA issue | V;   old stream: compute | dma wait | barrier")
for c in range(nch):
    r = []
    for w in (0, 4):
        r.append((int(s[w, c, 0] - t0), int(s[w, c, 1] - s[w, c, 0]), int(s[w, c, 2] - s[w, c, 1]), int(s[w, c, 3] - s[w, c, 2])))
    print(f"  chunk {c:2d}: wave0 @{r[0][0]:7d} {r[0][1:]}   wave4 @{r[1][0]:7d} {r[1][1:]}")
print("(chunk stamps: the last tile's, cycles from the earlier tile's start)")
