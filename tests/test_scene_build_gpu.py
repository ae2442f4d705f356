"""The scene builder on the device (multiply_amd/scene_build.py; csrc/raster.hip mp_raster_mask_batch, csrc/scene.hip mp_mask_dilate,
mp_mask_stats, mp_verts_bounds): byte-for-byte against mp_raster_zbuf and numpy, and end to end against the float64 restatement
(tests/scene_build_reference.py) and through the dataset.  Every figure is printed before it is asserted; the bounds and what was
measured: tests/tolerances_scene_build.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from multiply_amd import hip
from multiply_amd import scene_build as SB
from tests import scene_build_reference as R
from tests import tolerances_scene_build as TOL

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _cam16(f, H, W):
    return [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0, f, f, W / 2.0, H / 2.0]


def _zbuf_mask(verts, faces, cam16, H, W):
    """mp_raster_zbuf's  zbuf >= 0  of one mesh as 0 / 255 bytes"""
    v, f = verts.contiguous(), faces.contiguous()
    keys = torch.empty(H * W, dtype=torch.int64, device=DEV)
    big = torch.empty(f.shape[0] + 1, dtype=torch.int32, device=DEV)
    zbuf = torch.empty(H, W, dtype=torch.float32, device=DEV)
    cam = (C.c_float * 16)(*cam16)
    hip.lib().mp_raster_zbuf(v, v.shape[0], f, f.shape[0], C.cast(cam, C.c_void_p), SB.Z_CLIP, H, W, keys, big, zbuf, None, None,
                             hip.stream())
    return (zbuf >= 0).to(torch.uint8) * 255


@pytest.fixture(scope="module")
def bodies(smpl_tables):
    v, f = R.raster_bodies(smpl_tables)
    return torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)


# ------------------------------------------------------------------------------------------------ mp_raster_mask_batch
@pytest.mark.parametrize("size", R.RASTER_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_batch_equals_the_zbuffer_coverage(bodies, size):
    verts, faces = bodies
    H, W, f = size
    cam = _cam16(f, H, W)
    want = torch.stack([_zbuf_mask(verts[i], faces, cam, H, W) for i in range(verts.shape[0])])
    got = SB.raster_mask_batch(verts, faces, cam, H, W)
    assert got.dtype == torch.uint8 and got.shape == (6, H, W)
    cov = (want > 0).float().mean(dim=(1, 2)).cpu().numpy()
    print(f"{H} x {W}: covered fractions {np.round(cov, 3).tolist()}")
    for i, tr in enumerate(R.RASTER_TRANS):
        assert (cov[i] == 0.0) if tr[2] < 0 else (0.05 <= cov[i] <= 0.95), (i, cov[i])       # not the equality of empty masks
        assert torch.equal(got[i], want[i]), i
    assert set(torch.unique(got).tolist()) == {0, 255} and not got[2].any()                   # behind the camera: empty, not garbage
    # a mesh has the same bytes alone, at another place of a batch, and under any rows_per_call
    for i in range(6):
        assert torch.equal(SB.raster_mask_batch(verts[i:i + 1], faces, cam, H, W)[0], want[i]), i
    order = [4, 3, 3, 0, 5, 2, 1]
    assert torch.equal(SB.raster_mask_batch(verts[order], faces, cam, H, W), want[order])
    for rows in (1, 4):
        assert torch.equal(SB.raster_mask_batch(verts, faces, cam, H, W, rows_per_call=rows), want), rows
    # the near body's faces went through the queue of large boxes
    big = torch.zeros(1 + faces.shape[0], dtype=torch.int32, device=DEV)
    one = torch.empty(1, H, W, dtype=torch.uint8, device=DEV)
    camc = (C.c_float * 16)(*cam)
    hip.lib().mp_raster_mask_batch(verts[3:4].contiguous(), 1, verts.shape[1], faces, faces.shape[0], C.cast(camc, C.c_void_p), SB.Z_CLIP,
                                   H, W, big, one, hip.stream())
    assert int(big[0]) > 100 and torch.equal(one[0], want[3])
    print(f"  near body: {int(big[0])} of {faces.shape[0]} faces queued as large")


def test_mask_batch_empty_call_and_argument_errors(bodies):
    verts, faces = bodies
    H, W, f = R.RASTER_SIZES[0]
    cam = (C.c_float * 16)(*_cam16(f, H, W))
    camp = C.cast(cam, C.c_void_p)
    L = hip.lib()
    out = torch.full((2, H, W), 7, dtype=torch.uint8, device=DEV)
    big = torch.empty(1 + 2 * faces.shape[0], dtype=torch.int32, device=DEV)
    v2 = verts[:2].contiguous()
    assert L.mp_raster_mask_batch(v2, 0, verts.shape[1], faces, faces.shape[0], camp, SB.Z_CLIP, H, W, big, out, hip.stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                                             # N == 0: nothing is touched
    assert SB.raster_mask_batch(verts[:0], faces, _cam16(f, H, W), H, W).shape == (0, H, W)
    for bad in (dict(N=-1), dict(mask=None), dict(big=None), dict(faces=None), dict(verts=None), dict(cam=None), dict(H=0), dict(nf=-1)):
        a = dict(verts=v2, N=2, faces=faces, nf=faces.shape[0], cam=camp, H=H, big=big, mask=out)
        a.update(bad)
        with pytest.raises(RuntimeError, match=r"^mp_raster_mask_batch failed with code -1$"):
            L.mp_raster_mask_batch(a["verts"], a["N"], verts.shape[1], a["faces"], a["nf"], a["cam"], SB.Z_CLIP, a["H"], W, a["big"],
                                   a["mask"], hip.stream())
    torch.cuda.synchronize()
    assert bool((out == 7).all())


def test_mask_batch_shared_edge_through_pixel_centres():
    """two triangles of a square whose diagonal passes exactly through pixel centres, and whose outer edges do too"""
    H, W = 9, 11
    cam = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 1.0, 0.0, 0.0]                     # pixel = (X / Z, Y / Z)
    sq = np.array([[1.5, 1.5, 1.0], [6.5, 1.5, 1.0], [6.5, 6.5, 1.0], [1.5, 6.5, 1.0]], np.float32)
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=DEV)
    verts = torch.from_numpy(np.stack([sq, sq * 2.0, sq + [0.25, 0.0, 0.0]]).astype(np.float32)).to(DEV)    # the same square twice, one shifted
    got = SB.raster_mask_batch(verts, faces, cam, H, W)
    for i in range(3):
        assert torch.equal(got[i], _zbuf_mask(verts[i], faces, cam, H, W)), i
    assert torch.equal(got[0], got[1])
    m = got[0].cpu().numpy()
    assert m[2:6, 2:6].sum() // 255 == 12 and not m[[2, 3, 4, 5], [2, 3, 4, 5]].any()          # strictly inside; the diagonal is on an edge
    assert m.sum() // 255 == 12                                                                 # centres ON the outline are outside
    assert got[2].cpu().numpy().sum() // 255 == 5 * 4                                           # shifted: columns 2 .. 6 minus nothing on the diagonal


# ------------------------------------------------------------------------------------------------ mp_mask_dilate, mp_mask_stats
IMAGES = ((1, 1), (7, 5), (37, 53), (64, 64), (130, 70))
KERNELS = ((1, 1, 0, 0), (3, 3, 1, 1), (20, 20, 10, 10), (5, 2, 0, 0), (5, 2, 4, 1), (64, 64, 32, 32))


def _inputs(H, W):
    rs = np.random.RandomState(H * 1000 + W)
    corners = np.zeros((H, W), np.uint8)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = 255
    sparse = (rs.rand(H, W) < 0.02).astype(np.uint8) * 255
    values = (rs.rand(H, W) < 0.02).astype(np.uint8) * rs.randint(1, 255, (H, W)).astype(np.uint8)      # values other than 255
    return np.stack([np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8), np.full((H, W), 1, np.uint8), corners, sparse, values])


@pytest.mark.parametrize("size", IMAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_dilate_against_the_numpy_loop(size):
    H, W = size
    x = _inputs(H, W)
    dev = torch.from_numpy(x).to(DEV)
    for kh, kw, ay, ax in KERNELS:
        got = SB.mask_dilate(dev, kh, kw, ay, ax).cpu().numpy()
        for n in range(x.shape[0]):
            want = R.dilate(x[n], kh, kw, ay, ax)
            if H * W <= 35:
                assert np.array_equal(want, R.dilate_gather(x[n], kh, kw, ay, ax))              # the definition, read literally
            assert np.array_equal(got[n], want), (size, (kh, kw, ay, ax), n)
    assert np.array_equal(SB.mask_dilate(dev, 20).cpu().numpy(), SB.mask_dilate(dev, 20, 20, 10, 10).cpu().numpy())   # cv2's default anchor


def test_dilate_caps_and_argument_errors():
    x = torch.zeros(2, 7, 5, dtype=torch.uint8, device=DEV)
    out = torch.full_like(x, 9)
    L = hip.lib()
    for kh, kw, ay, ax in ((65, 3, 1, 1), (3, 65, 1, 1), (0, 3, 0, 1), (3, 0, 1, 0), (3, 3, 3, 1), (3, 3, 1, 3), (3, 3, -1, 1), (3, 3, 1, -1)):
        with pytest.raises(RuntimeError, match=r"^mp_mask_dilate failed with code -2$"):
            L.mp_mask_dilate(x, 2, 7, 5, kh, kw, ay, ax, out, hip.stream())
    for a in ((x, -1, out), (None, 2, out), (x, 2, None), (x, 2, x)):
        with pytest.raises(RuntimeError, match=r"^mp_mask_dilate failed with code -1$"):
            L.mp_mask_dilate(a[0], a[1], 7, 5, 3, 3, 1, 1, a[2], hip.stream())
    assert L.mp_mask_dilate(x, 0, 7, 5, 3, 3, 1, 1, out, hip.stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 9).all())


@pytest.mark.parametrize("size", IMAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stats_against_numpy(size):
    H, W = size
    x = _inputs(H, W)
    got = SB.mask_stats(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert got.dtype == np.int64 and got.shape == (x.shape[0], 7)
    for n in range(x.shape[0]):
        assert np.array_equal(got[n], R.stats(x[n])), (size, n, got[n], R.stats(x[n]))
    assert got[0].tolist() == [0, H, -1, W, -1, 0, 0]                                          # the empty mask
    d = SB.stats_dict(torch.from_numpy(got), (x.shape[0],))
    assert np.isnan(d["centre"][0]).all() and np.array_equal(d["centre"][1], [(W - 1) / 2, (H - 1) / 2])
    assert hip.lib().mp_mask_stats(None, 0, H, W, None, hip.stream()) == 0
    with pytest.raises(RuntimeError, match=r"^mp_mask_stats failed with code -1$"):
        hip.lib().mp_mask_stats(None, 1, H, W, None, hip.stream())


# ------------------------------------------------------------------------------------------------ mp_verts_bounds
@pytest.mark.parametrize("n", [1, 63, 64, 65, 13780])
@pytest.mark.parametrize("F", [1, 3])
def test_verts_bounds(F, n):
    rs = np.random.RandomState(F * 100000 + n)
    v = rs.normal(0, 1.5, (F, n, 3)).astype(np.float32) - np.float32(0.5)
    v[0, 0] = [-9.0, 8.5, -8.0]                       # extremes (six sigma out) at the first ...
    v[-1, -1, 1], v[-1, -1, 2] = 8.75, -8.875         # ... and at the last element
    dev = torch.from_numpy(v).to(DEV)
    got = SB.verts_bounds(dev)
    assert torch.equal(got[:, :3], torch.amin(dev, dim=1)) and torch.equal(got[:, 3:], torch.amax(dev, dim=1))
    assert float(got[0, 0]) == -9.0 and float(got[-1, 2]) == -8.875 and float(got[-1, 4]) == 8.75
    shift = rs.normal(0, 1, (F, 3)).astype(np.float32)
    norm = SB.verts_bounds(dev, torch.from_numpy(shift)).cpu().numpy()
    want = np.linalg.norm(v.astype(np.float64) + shift.astype(np.float64)[:, None], axis=-1).max(1)
    err = np.abs(norm.astype(np.float64) - want).max()
    print(f"verts_bounds F = {F}, n = {n}: max-norm error {err:.3e} (values up to {want.max():.2f})")
    assert err <= TOL.bound(TOL.BOUNDS_NORM_ABS_MEASURED)


def test_verts_bounds_argument_errors():
    v = torch.zeros(1, 4, 3, device=DEV)
    out = torch.empty(6, device=DEV)
    L = hip.lib()
    assert L.mp_verts_bounds(None, 0, 4, None, None, hip.stream()) == 0
    for a in ((v, -1, 4, out), (v, 1, 0, out), (None, 1, 4, out), (v, 1, 4, None)):
        with pytest.raises(RuntimeError, match=r"^mp_verts_bounds failed with code -1$"):
            L.mp_verts_bounds(a[0], a[1], a[2], None, a[3], hip.stream())


# ------------------------------------------------------------------------------------------------ end to end
def _opt(root, **kw):
    from multiply_amd.config import to_config
    base = dict(data_root=os.path.dirname(root), data_dir=os.path.basename(root), start_frame=0, end_frame=3, num_sample=64,
                using_SAM=False, pixel_per_batch=512)
    base.update(kw)
    return to_config(base)


def test_build_scene_end_to_end(smpl_tables, tmp_path):
    from PIL import Image
    from multiply_amd.datasets import create_dataset
    from multiply_amd.smpl import SMPLServer
    server = SMPLServer(smpl_tables=smpl_tables)
    seq, ref = R.sequence(), R.sequence_reference(smpl_tables)
    H, W = R.SEQ_SIZE
    F, P = seq["pose"].shape[:2]
    assert 3.0 <= seq["trans"][..., 2].min() and seq["trans"][..., 2].max() <= 5.0 and np.abs(np.diff(seq["shape"], axis=0)).min() > 0
    raw, root = tmp_path / "raw", str(tmp_path / "scene")
    os.makedirs(raw / "frames")
    rs = np.random.RandomState(4)
    frames = rs.randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    paths = []
    for f in range(F):
        paths.append(str(raw / "frames" / ("%04d.png" % f)))
        Image.fromarray(frames[f]).save(paths[-1])
    sc = SB.build_scene(server, {k: torch.from_numpy(v) for k, v in seq.items()}, R.SEQ_K, (H, W), out_dir=root, frames=paths)

    # ---- the folder against the float64 restatement, array by array
    ld = lambda n: np.load(os.path.join(root, n))
    poses, ntrans, mshape = ld("poses.npy"), ld("normalize_trans.npy"), ld("mean_shape.npy")
    cams, cn = ld("cameras.npz"), ld("cameras_normalize.npz")
    assert poses.shape == (F, P, 72) and ntrans.shape == (F, P, 3) and mshape.shape == (P, 10)
    assert ld("gender.npy").tolist() == ["neutral"] * P
    assert sorted(cams.files) == sorted("cam_%d" % f for f in range(F))
    assert sorted(cn.files) == sorted(["scale_mat_%d" % f for f in range(F)] + ["world_mat_%d" % f for f in range(F)])
    rot = max(np.abs(R.rotvec_to_matrix(a[:3]) - R.rotvec_to_matrix(b[:3])).max() for a, b in zip(poses.reshape(-1, 72), ref["poses"].reshape(-1, 72)))
    fig = dict(root_rotation=rot, body_pose=np.abs(poses[..., 3:] - ref["poses"][..., 3:]).max(),
               mean_shape=np.abs(mshape - ref["mean_shape"]).max(),
               normalize_trans=np.abs(ntrans - ref["normalize_trans"]).max(),
               sphere=abs(float(ld("max_human_sphere.npy")) - ref["max_human_sphere"]),
               cam=max(np.abs(cams["cam_%d" % f] - ref["cams"][f]).max() / np.abs(ref["cams"][f]).max() for f in range(F)),
               radius=abs(sc["radius"] - ref["radius"]))
    # first_frame, no frames, rows_per_call: the same bodies under one shift
    sc2 = SB.build_scene([server, server], seq, R.SEQ_K, (H, W), normalize="first_frame", dilate=0, rows_per_call=4)
    ref2 = R.sequence_reference(smpl_tables, normalize="first_frame")
    fig["sphere_first_frame"] = abs(sc2["max_human_sphere"] - ref2["max_human_sphere"])
    fig["normalize_trans_first_frame"] = np.abs(sc2["normalize_trans"] - ref2["normalize_trans"]).max()
    print("build_scene against float64: " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    # ---- through the dataset
    loader = create_dataset(_opt(root, dataset="Hi4D", batch_size=1, drop_last=False, shuffle=False, worker=0, num_sample=0))
    ds = loader.dataset
    assert len(ds) == F and tuple(ds.img_size) == (H, W) and ds.num_person == P
    assert np.array_equal(ds.store.images.cpu().numpy(), frames)                                # image/ holds the input bytes
    worst_px, worst_r, outside = 0.0, 0.0, 0
    for f, (inputs, _) in enumerate(loader):
        prm, K, pose = inputs["smpl_params"][0], inputs["intrinsics"][0].double().numpy(), inputs["pose"][0].double().numpy()
        for p in range(P):
            out = server(prm[p, 0:1].to(DEV), prm[p, 1:4].to(DEV), prm[p, 4:76].to(DEV), prm[p, 76:].to(DEV), absolute=True)
            v = out["smpl_verts"][0].double().cpu().numpy()
            worst_r = max(worst_r, float(np.linalg.norm(v, axis=1).max()))
            xc = (v - pose[:3, 3]) @ pose[:3, :3]                                                  # R (x - C), R = pose[:3,:3]^T
            uv = xc[:, :2] / xc[:, 2:3] * [K[0, 0], K[1, 1]] + [K[0, 2], K[1, 2]]
            c = ref["cam_verts"][f, p]
            want = c[:, :2] / c[:, 2:3] * [R.SEQ_K[0, 0], R.SEQ_K[1, 1]] + [R.SEQ_K[0, 2], R.SEQ_K[1, 2]]
            worst_px = max(worst_px, float(np.abs(uv - want).max()))
            col, row = np.floor(want[:, 0]).astype(int), np.floor(want[:, 1]).astype(int)
            ok = (col >= 0) & (col < W) & (row >= 0) & (row < H)
            assert ok.sum() > 6000
            m = sc["masks"][f, p].cpu().numpy()
            outside += int((m[row[ok], col[ok]] == 0).sum())
            assert np.array_equal(np.asarray(Image.open(os.path.join(root, "mask", str(p), "%04d.png" % f))), m)
            assert Image.open(os.path.join(root, "mask", str(p), "%04d.png" % f)).mode == "L"
        assert np.array_equal(inputs["org_object_mask"][0].cpu().numpy(), (sc["masks"][f] > 0).sum(0).cpu().numpy())
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, "image", "%04d.png" % f))), frames[f])
    print(f"dataset items: reprojection {worst_px:.3e} px, largest |vertex| {worst_r:.4f} (sphere 3), vertex pixels outside the mask {outside}")
    # ---- masks: 0 / 255, the dilated box is the raw one grown by 9 towards the origin and 10 away from it, clipped
    raw_s, dil_s = sc["mask_stats"]["raw"], sc["mask_stats"]["dilated"]
    assert set(torch.unique(sc["masks"]).tolist()) == {0, 255} and set(torch.unique(sc["raw_masks"]).tolist()) == {0, 255}
    assert (raw_s["count"] > 0.02 * H * W).all() and (dil_s["count"] < 0.9 * H * W).all()
    grown = np.stack([np.maximum(raw_s["bbox"][..., 0] - 9, 0), np.minimum(raw_s["bbox"][..., 1] + 10, H - 1),
                      np.maximum(raw_s["bbox"][..., 2] - 9, 0), np.minimum(raw_s["bbox"][..., 3] + 10, W - 1)], -1)
    assert np.array_equal(dil_s["bbox"], grown)
    for f in range(F):
        for p in range(P):
            m = sc["raw_masks"][f, p].cpu().numpy()
            assert np.array_equal(sc["masks"][f, p].cpu().numpy(), R.dilate(m, 20, 20, 10, 10))
            rows, cols = np.nonzero(m)
            assert np.allclose(raw_s["centre"][f, p], [cols.mean(), rows.mean()], rtol=1e-12, atol=0)
    assert outside == 0 and worst_r < 3.0
    # ---- the float comparisons
    assert fig["body_pose"] == 0.0 and fig["root_rotation"] <= TOL.HOST_METRES and fig["mean_shape"] <= TOL.HOST_METRES
    assert fig["sphere"] <= TOL.bound(TOL.MAX_HUMAN_SPHERE_ABS_MEASURED)
    assert fig["normalize_trans"] <= TOL.bound(TOL.NORMALIZE_TRANS_ABS_MEASURED)
    assert fig["cam"] <= TOL.bound(TOL.CAM_REL_MEASURED)
    assert fig["radius"] <= 1.1 * max(TOL.bound(TOL.MAX_HUMAN_SPHERE_ABS_MEASURED), TOL.bound(TOL.NORMALIZE_TRANS_ABS_MEASURED))
    assert worst_px <= TOL.bound(TOL.REPROJECTION_PX_MEASURED)
    for f in range(F):
        assert np.array_equal(cn["world_mat_%d" % f], cams["cam_%d" % f]) and cn["scale_mat_%d" % f].dtype == np.float32
        assert np.array_equal(cn["scale_mat_%d" % f], np.diag([sc["radius"] / 3] * 3 + [1.0]).astype(np.float32))

    # ---- first_frame: one shift, the same poses and silhouettes
    assert np.array_equal(sc2["shift"], np.tile(sc["shift"][:1], (F, 1))) and np.array_equal(sc2["poses"], sc["poses"])
    assert torch.equal(sc2["raw_masks"], sc["raw_masks"]) and torch.equal(sc2["masks"], sc2["raw_masks"])
    assert fig["sphere_first_frame"] <= TOL.bound(TOL.MAX_HUMAN_SPHERE_ABS_MEASURED)
    assert fig["normalize_trans_first_frame"] <= TOL.bound(TOL.NORMALIZE_TRANS_ABS_MEASURED)

    # ---- scale_factor 2: half-size frames (PIL's box reduction) and masks, divided intrinsics, the same scene-space bodies
    root2 = str(tmp_path / "half")
    sc3 = SB.build_scene(server, seq, R.SEQ_K, (H, W), out_dir=root2, frames=paths, scale_factor=2)
    assert sc3["img_size"] == (H // 2, W // 2) and sc3["masks"].shape == (F, P, H // 2, W // 2)
    assert np.array_equal(sc3["normalize_trans"], sc["normalize_trans"]) and sc3["max_human_sphere"] == sc["max_human_sphere"]
    K2 = np.linalg.inv(np.block([[R.RT, (-R.RT @ sc3["shift"][0])[:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]))
    assert np.abs(sc3["cameras"]["cam_0"] @ K2 - SB.intrinsics4(R.SEQ_K, 2)).max() <= TOL.HOST_PIXELS
    half = np.asarray(Image.open(os.path.join(root2, "image", "0001.png")))
    assert half.shape == (H // 2, W // 2, 3) and np.array_equal(half, np.asarray(Image.fromarray(frames[1]).reduce(2)))
    assert (sc3["mask_stats"]["raw"]["count"] > 0).all() and (sc3["mask_stats"]["dilated"]["bbox"][..., 1] < H // 2).all()

    # ---- the tool on the same input prints the same numbers
    np.savez(raw / "refined_smpl.npz", **seq)
    np.save(raw / "intrinsics.npy", R.SEQ_K)
    env = dict(os.environ, MULTIPLY_SYNTHETIC_SMPL="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "build_scene.py"), str(raw), str(tmp_path / "tool_out")],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(r.stdout.strip().splitlines()[-1])
    assert (js["frames"], js["persons"], js["image_size"], js["empty_mask_person_frames"]) == (F, P, [H, W], 0)
    assert js["max_human_sphere"] == sc["max_human_sphere"] and js["scale"] == 1.0 / float(cn["scale_mat_0"][0, 0])
    frac = dil_s["count"] / float(H * W)
    assert js["covered_fraction_min"] == frac.min(0).tolist() and js["covered_fraction_mean"] == frac.mean(0).tolist()
    for n in ("poses.npy", "normalize_trans.npy", "mean_shape.npy", "max_human_sphere.npy"):
        assert np.array_equal(np.load(os.path.join(tmp_path / "tool_out", n)), ld(n)), n
