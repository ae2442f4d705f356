"""The overlay kernels (csrc/overlay.hip through multiply_amd/overlay.py) on the device: visibility against mp_raster_zbuf pixel
for pixel, colours against the float64 restatement (tests/overlay_reference.py) evaluated at mp_raster_zbuf's own barycentrics,
keypoint discs, normals and colour modes with bounds from the operand magnitudes, batch independence, argument statuses and
guard words."""
import ctypes as C

import numpy as np
import pytest
import torch

from multiply_amd import hip
from multiply_amd import overlay as OV
from multiply_amd.render import Z_CLIP
from tests import overlay_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, M = R.H, R.W, R.M
GUARD = 0x5A


def _dev(meshes):
    return [(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), torch.from_numpy(c).to(DEV)) for v, f, c in meshes]


def _zbuf(meshes, cam16=R.CAM):
    """mp_raster_zbuf on the meshes joined in order -> (record (H, W) or -1, local face, bary (H, W, 3), corner colours
    (H, W, 3, 3)) as numpy"""
    nv = np.cumsum([0] + [m[0].shape[0] for m in meshes])
    nf = np.cumsum([0] + [m[1].shape[0] for m in meshes])
    if not meshes:
        return -np.ones((H, W), int), -np.ones((H, W), int), -np.ones((H, W, 3), np.float32), np.zeros((H, W, 3, 3), np.float32)
    v = torch.from_numpy(np.concatenate([m[0] for m in meshes])).to(DEV)
    f = torch.from_numpy(np.concatenate([m[1] + o for m, o in zip(meshes, nv[:-1])]).astype(np.int32)).to(DEV)
    col = np.concatenate([m[2] for m in meshes])
    keys = torch.empty(H * W, dtype=torch.int64, device=DEV)
    big = torch.empty(f.shape[0] + 1, dtype=torch.int32, device=DEV)
    zbuf = torch.empty(H, W, dtype=torch.float32, device=DEV)
    p2f = torch.empty(H, W, dtype=torch.int32, device=DEV)
    bary = torch.empty(H, W, 3, dtype=torch.float32, device=DEV)
    cam = (C.c_float * 16)(*cam16)
    hip.lib().mp_raster_zbuf(v, v.shape[0], f, f.shape[0], C.cast(cam, C.c_void_p), Z_CLIP, H, W, keys, big, zbuf, p2f, bary, hip.stream())
    p2f, zb = p2f.cpu().numpy(), zbuf.cpu().numpy()
    assert ((p2f >= 0) == (zb >= 0)).all()
    rec = np.where(p2f >= 0, np.searchsorted(nf, np.maximum(p2f, 0), side="right") - 1, -1)       # face -> record via face_base
    local = np.where(p2f >= 0, p2f - nf[np.maximum(rec, 0)], -1)
    corner = col[f.cpu().numpy()[np.maximum(p2f, 0)]]
    return rec, local, bary.cpu().numpy(), corner


@pytest.fixture(scope="module")
def scene():
    s = R.base_scene()
    s["dev"] = _dev(s["meshes"])
    s["frames_dev"] = torch.from_numpy(s["frames"]).to(DEV)
    s["kp_dev"] = torch.from_numpy(s["keypoints"]).to(DEV)
    s["zbuf"] = [_zbuf([m for m, i in zip(s["meshes"], s["image_of"]) if i == im]) for im in range(M)]
    s["first"] = [0, 3, 5]                                       # first record of each image
    out, owner = OV.render_overlays(s["dev"], s["image_of"], R.CAM, H, W, frames=s["frames_dev"], opacity=0.6, keypoints=s["kp_dev"],
                                    kp_rgb=R.KP_RGB, kp_conf=R.KP_CONF, kp_radius=R.KP_RADIUS, want_owner=True)
    s["out"], s["owner"] = out, owner
    return s


def _render(s, **kw):
    a = dict(frames=s["frames_dev"], opacity=0.6, keypoints=s["kp_dev"], kp_rgb=R.KP_RGB, kp_conf=R.KP_CONF, kp_radius=R.KP_RADIUS)
    a.update(kw)
    return OV.render_overlays(s["dev"], s["image_of"], R.CAM, H, W, **a)


# ------------------------------------------------------------------------------------------------ 1. visibility
def test_visibility_equals_the_zbuffer(scene):
    owner = scene["owner"].cpu().numpy()
    assert owner.shape == (M, H, W) and owner.dtype == np.int32
    for im in range(M):
        rec = scene["zbuf"][im][0]
        want = np.where(rec >= 0, rec + scene["first"][im], -1)
        assert np.array_equal(owner[im], want), (im, int((owner[im] != want).sum()))
    # every path was reached
    assert set(np.unique(owner[0])) == {-1, 0, 1} and set(np.unique(owner[1])) == {3, 4} and (owner[2] == -1).all()
    assert (owner[1][:, -1] == 3).any()                                                          # the sphere cut by the border
    # the copied triangle ties with the first sphere's at every pixel it covers, and loses: the earlier record wins
    tri = scene["meshes"][2]
    alone = _zbuf([tri])[0] >= 0
    assert alone.sum() >= 3 and (owner[0][alone] == 0).all()
    # ... and wins when it comes first
    order = [2, 0, 1]
    o2 = OV.render_overlays([scene["dev"][i] for i in order], [0, 0, 0], R.CAM, H, W, want_owner=True)[1].cpu().numpy()[0]
    assert (o2[alone] == 0).all() and np.array_equal(o2 >= 0, owner[0] >= 0)
    assert np.array_equal(o2[~alone], np.where(owner[0] >= 0, owner[0] + 1, -1)[~alone])
    print(f"covered: {[(owner[i] >= 0).sum() for i in range(M)]} of {H * W}; tie pixels {alone.sum()}")


def test_single_record_coverage_equals_the_mask_batch(scene):
    from multiply_amd import scene_build as SB
    for i in (0, 3, 4):                                                     # a sphere, the one cut by the border, the queue mesh
        v, f, c = scene["dev"][i]
        owner = OV.render_overlays([(v, f, c)], [0], R.CAM, H, W, want_owner=True)[1]
        mask = SB.raster_mask_batch(v[None], f, R.CAM, H, W)[0]
        assert torch.equal(owner[0] >= 0, mask == 255) and int((mask == 255).sum()) > 50, i


# ------------------------------------------------------------------------------------------------ 2. colours
def _expected(s, im, opacity, frame):
    """the reference at mp_raster_zbuf's own face and barycentrics: (bytes (H, W, 3), near (H, W, 3) bool, covered (H, W))"""
    rec, _, bary, corner = s["zbuf"][im]
    v = R.mesh_value(bary, corner)
    hit = rec >= 0
    out = np.array(np.broadcast_to(frame, (H, W, 3)))
    out[hit] = R.blend(v[hit], out[hit], opacity)
    return out, (np.abs(v - np.round(v)) <= R.MARGIN) & hit[..., None], hit


def test_colours_against_float64(scene):
    """The margin.  The kernel forms c = fma(b2, c2, fma(b1, c1, b0 c0)) and v = 255 c in fp32 from the same fp32 barycentrics
    and colours the reference reads: three roundings of at most 2^-25 each on the sum (all partial sums are at most 1) make
    3 * 2^-25 on c, i.e. 255 * 3 * 2^-25 < 2^-15 on v, and the product 255 c rounds by at most half an ulp of a number below 256,
    2^-17.  Should the resolve pass's barycentrics differ from mp_raster_zbuf's in the last place (another contraction of the
    same expression), each moves c by at most 2^-24 and v by 3 * 255 * 2^-24 < 2^-14.  The sum is below 2^-13; the margin 2^-12
    is twice that.  Outside the margin floor(v) is the same in both arithmetics and, the blend being exact on bytes (below), so is
    the output byte; inside it the mesh byte may differ by one and the blend (opacity <= 1) passes on at most that."""
    out = scene["out"].cpu().numpy()
    covered = near_n = 0
    for im in range(M):
        want, near, hit = _expected(scene, im, 0.6, scene["frames"][im])
        want = R.paint_keypoints(want, scene["keypoints"][im], R.KP_RGB, R.KP_CONF, R.KP_RADIUS)
        kp = R.paint_keypoints(np.zeros((H, W, 3), np.uint8), scene["keypoints"][im], np.full((6, 3), 1, np.uint8), R.KP_CONF,
                               R.KP_RADIUS)[..., 0] > 0
        near &= ~kp[..., None]
        diff = np.abs(out[im].astype(int) - want.astype(int))
        assert (diff[~near] == 0).all(), (im, int((diff[~near] != 0).sum()))
        assert (diff[near] <= 1).all()
        assert np.array_equal(out[im][~hit & ~kp], scene["frames"][im][~hit & ~kp])              # uncovered: the frame's bytes
        covered += hit.sum()
        near_n += near.any(-1).sum()
    print(f"{covered} covered pixels, {near_n} with a channel within 2^-12 of an integer")
    assert covered > 2000 and near_n <= 0.01 * covered
    # over the background colour instead of frames
    bg = (10, 200, 77)
    got = _render(scene, frames=None, background=bg, keypoints=None, n_images=M).cpu().numpy()   # nothing else says M
    for im in range(M):
        want, near, hit = _expected(scene, im, 0.6, np.array(bg, np.uint8))
        diff = np.abs(got[im].astype(int) - want.astype(int))
        assert (diff[~near] == 0).all() and (diff[near] <= 1).all() and (got[im][~hit] == bg).all()


@pytest.mark.parametrize("opacity", [0.0, 1.0, 0.6])
def test_blend_is_exact_on_bytes(scene, opacity):
    """uniform colours (j + 0.5) / 255 per record: 255 c = (j + 0.5)(b0 + b1 + b2) is half a unit away from every integer whatever
    the rounding, so the mesh byte is j with no allowance, and so is the blended byte (in fp32 fmaf(opacity, m - f, f) + 0.5 is
    exact or far from an integer for these opacities: 0.6f (m - f) has a fraction of k / 5 + O(1e-5))"""
    js = [[12, 200, 99], [255, 0, 31],        # 255.5 / 255 > 1 clamps: still byte 255
          [7, 7, 250], [128, 64, 32], [1, 2, 3]]
    meshes = [(v, f, torch.tensor([(j + 0.5) / 255 for j in jj], dtype=torch.float32, device=DEV).expand(v.shape[0], 3).contiguous())
              for (v, f, _), jj in zip(scene["dev"], js)]
    got = OV.render_overlays(meshes, scene["image_of"], R.CAM, H, W, frames=scene["frames_dev"], opacity=opacity).cpu().numpy()
    owner = scene["owner"].cpu().numpy()
    for im in range(M):
        f = scene["frames"][im].astype(np.float64)
        want = scene["frames"][im].copy()
        for r in range(5):
            sel = owner[im] == r
            want[sel] = np.floor(float(np.float32(opacity)) * (np.array(js[r], np.float64) - f[sel]) + f[sel] + 0.5)
        assert np.array_equal(got[im], want), (im, opacity)
    if opacity == 0.0:
        assert np.array_equal(got, scene["frames"])


# ------------------------------------------------------------------------------------------------ 3. keypoints
def test_keypoints_are_exact_integer_discs(scene):
    none = []
    got = OV.render_overlays(none, [], R.CAM, H, W, frames=scene["frames_dev"], keypoints=scene["kp_dev"], kp_rgb=R.KP_RGB,
                             kp_conf=R.KP_CONF, kp_radius=R.KP_RADIUS).cpu().numpy()
    for im in range(M):
        want = R.paint_keypoints(scene["frames"][im], scene["keypoints"][im], R.KP_RGB, R.KP_CONF, R.KP_RADIUS)
        assert np.array_equal(got[im], want), im
    assert tuple(got[0, 0, 0]) == tuple(R.KP_RGB[0]) and tuple(got[0, 20, W - 1]) == tuple(R.KP_RGB[1])
    assert tuple(got[0, 21, W - 4]) == tuple(R.KP_RGB[5])                                     # in both discs: the higher index
    painted = (got[0] != scene["frames"][0]).any(-1)
    cols = {tuple(c) for c in got[0][painted].tolist()}
    assert cols <= {tuple(R.KP_RGB[k]) for k in (0, 1, 5)}                                    # outside, NaN, low confidence: nothing
    # radius 0 is the single pixel; K = 0 and keypoints=None agree
    one = OV.render_overlays(none, [], R.CAM, H, W, frames=scene["frames_dev"], keypoints=scene["kp_dev"], kp_rgb=R.KP_RGB,
                             kp_conf=R.KP_CONF, kp_radius=0).cpu().numpy()
    assert np.array_equal(one[0], R.paint_keypoints(scene["frames"][0], scene["keypoints"][0], R.KP_RGB, R.KP_CONF, 0))
    a = _render(scene, keypoints=None)
    b = _render(scene, keypoints=scene["kp_dev"][:, :0], kp_rgb=np.zeros((0, 3), np.uint8))
    assert torch.equal(a, b)
    # with meshes: the discs lie over them
    kp = R.paint_keypoints(np.zeros((H, W, 3), np.uint8), scene["keypoints"][0], np.full((6, 3), 1, np.uint8), R.KP_CONF, R.KP_RADIUS)[..., 0] > 0
    full = scene["out"].cpu().numpy()[0]
    assert np.array_equal(full[kp], got[0][kp]) and np.array_equal(full[~kp], a.cpu().numpy()[0][~kp])


# ------------------------------------------------------------------------------------------------ 4. normals and colour modes
def _batch7():
    rs = np.random.RandomState(5)
    v, f = R.icosphere()
    f = np.concatenate([f, f[:1]]).astype(np.int32)                                           # a repeated face
    vs = []
    for i in range(7):
        A = np.eye(3) + 0.3 * rs.normal(size=(3, 3))
        vs.append(np.concatenate([v @ A.T * (0.1 + i) + rs.normal(size=3), [[9.0, 9.0, 9.0]]]))       # vertex 42 in no face
    return np.stack(vs).astype(np.float32), f


def test_vertex_normals_against_float64():
    vs, f = _batch7()
    vt, ft = torch.from_numpy(vs).to(DEV), torch.from_numpy(f).to(DEV)
    adj = OV.vertex_adjacency(f, 43)
    got = OV.vertex_normals(vt, ft, adjacency=adj)
    assert got.shape == (7, 43, 3)
    g = got.cpu().numpy().astype(np.float64)
    worst = 0.0
    for i in range(7):
        want, bound = R.vertex_normals(vs[i], f)[0], R.normals_bound(vs[i], f)
        err = np.abs(g[i] - want)
        worst = max(worst, float((err / np.maximum(bound, 1e-300))[:42].max()))
        assert (err <= bound).all(), (i, float(err.max()), float(bound.max()))
        assert (g[i, 42] == 0).all()                                                          # the isolated vertex
        assert np.abs(np.linalg.norm(g[i, :42], axis=1) - 1).max() < 1e-6
        # alone, and without a prepared adjacency: the same bits
        assert torch.equal(OV.vertex_normals(vt[i], ft), got[i]) and torch.equal(OV.vertex_normals(vt[i:i + 1], ft, adj)[0], got[i])
    assert torch.equal(OV.vertex_normals(vt[[6, 2, 2, 0]], ft, adj), got[[6, 2, 2, 0]])
    print(f"normals: worst error / bound {worst:.3f}")
    # render_mesh_recon's definition
    v64 = torch.from_numpy(vs[1]).double()
    fl = torch.from_numpy(f).long()
    fn = torch.cross(v64[fl[:, 1]] - v64[fl[:, 0]], v64[fl[:, 2]] - v64[fl[:, 0]], dim=1)
    vn = torch.nn.functional.normalize(torch.zeros_like(v64).index_add_(0, fl.reshape(-1), fn.repeat_interleave(3, 0)), eps=1e-6, dim=1)
    assert np.abs(vn.numpy() - R.vertex_normals(vs[1], f)[0]).max() < 1e-12


def test_vertex_colour_modes_against_float64():
    vs, f = _batch7()
    nrm = OV.vertex_normals(torch.from_numpy(vs).to(DEV), torch.from_numpy(f).to(DEV))
    n64 = nrm.cpu().numpy().astype(np.float64)
    tint = np.random.RandomState(6).uniform(0, 1, (7, 3)).astype(np.float32)
    for mode, kw in (("normal", {}), ("shade", {}), ("shade", dict(light=(0.3, -0.5, 0.8))),
                     ("tint", dict(tint=tint)), ("tint", dict(tint=tint, light=(0.0, 0.6, -0.8), ambient=0.45))):
        got = OV.vertex_colors(nrm, mode, **{k: (torch.from_numpy(v).to(DEV) if k == "tint" else v) for k, v in kw.items()})
        want, bound = R.vertex_colors(n64, mode, **kw)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        assert (err <= bound + 1e-45).all(), (mode, float(err.max()), float(bound.max()))
        assert (got[:, 42] == (0.5 if mode == "normal" else 0.0)).all() or mode == "tint"
        assert torch.equal(OV.vertex_colors(nrm[3], mode, **{k: (v[3] if k == "tint" else v) for k, v in kw.items()}), got[3])
    assert torch.equal(OV.vertex_colors(nrm, "tint", tint=tint[0])[0], OV.vertex_colors(nrm, "tint", tint=tint)[0])
    with pytest.raises(ValueError):
        OV.vertex_colors(nrm, "phong")
    with pytest.raises(ValueError):
        OV.vertex_colors(nrm, "tint")
    L = hip.lib()
    out = torch.full((7, 43, 3), 7.0, device=DEV)
    with pytest.raises(RuntimeError, match=r"^mp_overlay_vertex_colors failed with code -2$"):
        L.mp_overlay_vertex_colors(nrm, 7, 43, 3, None, 0.0, 0.0, 1.0, 0.3, out, hip.stream())
    with pytest.raises(RuntimeError, match=r"^mp_overlay_vertex_colors failed with code -1$"):
        L.mp_overlay_vertex_colors(nrm, 7, 43, 2, None, 0.0, 0.0, 1.0, 0.3, out, hip.stream())
    with pytest.raises(RuntimeError, match=r"^mp_mesh_vertex_normals failed with code -1$"):
        L.mp_mesh_vertex_normals(nrm, 7, 43, None, 5, None, None, out, hip.stream())
    assert L.mp_overlay_vertex_colors(nrm, 0, 43, 0, None, 0.0, 0.0, 1.0, 0.3, out, hip.stream()) == 0
    assert L.mp_mesh_vertex_normals(nrm, 7, 0, None, 0, None, None, out, hip.stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------ 5. independence and limits
def test_an_image_does_not_depend_on_its_batch(scene):
    out, owner = scene["out"], scene["owner"]
    for per in (1, 2):
        o, w = _render(scene, images_per_call=per, want_owner=True)
        assert torch.equal(o, out) and torch.equal(w, owner), per
    cams = [R.CAM] * M
    o, w = _render(scene, want_owner=True)
    o3, w3 = OV.render_overlays(scene["dev"], scene["image_of"], cams, H, W, frames=scene["frames_dev"], opacity=0.6,
                                keypoints=scene["kp_dev"], kp_rgb=R.KP_RGB, kp_conf=R.KP_CONF, kp_radius=R.KP_RADIUS, want_owner=True)
    assert torch.equal(o, out) and torch.equal(o3, out) and torch.equal(w3, owner)
    for im in range(M):                                                     # alone
        idx = [i for i, k in enumerate(scene["image_of"]) if k == im]
        o1, w1 = OV.render_overlays([scene["dev"][i] for i in idx], [0] * len(idx), R.CAM, H, W, frames=scene["frames_dev"][im:im + 1],
                                    opacity=0.6, keypoints=scene["kp_dev"][im:im + 1], kp_rgb=R.KP_RGB, kp_conf=R.KP_CONF,
                                    kp_radius=R.KP_RADIUS, want_owner=True)
        assert torch.equal(o1[0], out[im]), im
        assert torch.equal(w1[0], torch.where(owner[im] >= 0, owner[im] - scene["first"][im], owner[im])), im
    # records interleaved over the images, and another camera per image really is used
    order = [3, 0, 4, 1, 2]
    o5 = OV.render_overlays([scene["dev"][i] for i in order], [scene["image_of"][i] for i in order], R.CAM, H, W,
                            frames=scene["frames_dev"], opacity=0.6, keypoints=scene["kp_dev"], kp_rgb=R.KP_RGB, kp_conf=R.KP_CONF,
                            kp_radius=R.KP_RADIUS)
    assert torch.equal(o5, out)
    moved = list(R.CAM)
    moved[14] += 7.0
    o6 = OV.render_overlays(scene["dev"], scene["image_of"], [R.CAM, moved, R.CAM], H, W, frames=scene["frames_dev"], opacity=0.6,
                            keypoints=scene["kp_dev"], kp_rgb=R.KP_RGB, kp_conf=R.KP_CONF, kp_radius=R.KP_RADIUS)
    assert torch.equal(o6[0], out[0]) and torch.equal(o6[2], out[2]) and not torch.equal(o6[1], out[1])
    # the batched form (one topology) is the list form
    va, f, ca = scene["dev"][0]
    vb, _, cb = scene["dev"][1]
    ob = OV.render_overlays((torch.stack([va, vb]), f, torch.stack([ca, cb])), [0, 0], R.CAM, H, W, n_images=1)
    assert torch.equal(ob, OV.render_overlays([scene["dev"][0], scene["dev"][1]], [0, 0], R.CAM, H, W))
    with pytest.raises(ValueError, match="faces index vertices"):
        OV.render_overlays([(va[:40], f, ca[:40])], [0], R.CAM, H, W)
    with pytest.raises(ValueError, match="outside"):
        OV.render_overlays([scene["dev"][0]], [1], R.CAM, H, W, n_images=1)
    assert OV.render_overlays([], [], R.CAM, H, W).shape == (0, H, W, 3)


def _direct(scene, guard=16):
    """the arguments of a direct mp_overlay_batch call on the whole scene, every output and scratch followed by guard bytes"""
    entries = [(v.data_ptr(), f.data_ptr(), c.data_ptr(), v.shape[0], f.shape[0], im) for (v, f, c), im in zip(scene["dev"], scene["image_of"])]
    table, blocks, faces = OV.record_table(entries, M)
    tab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(DEV)
    buf = lambda n: torch.full((n + guard,), GUARD, dtype=torch.uint8, device=DEV)
    cam = (C.c_float * 16)(*R.CAM)
    bg = (C.c_ubyte * 3)(1, 2, 3)
    a = dict(recs=tab, n_rec=5, blocks=blocks, faces=faces, M=M, H=H, W=W, cams=C.cast(cam, C.c_void_p), n_cam=1, frames=scene["frames_dev"],
             bg=C.cast(bg, C.c_void_p), opacity=0.6, kp=scene["kp_dev"], K=6, rgb=torch.from_numpy(R.KP_RGB).to(DEV), conf=R.KP_CONF,
             radius=R.KP_RADIUS, keys=buf(8 * M * H * W), big=buf(4 * (1 + faces)), cam_dev=buf(64), out=buf(3 * M * H * W),
             owner=buf(4 * M * H * W), _keep=(cam, bg))
    return a


def _call(a):
    return hip.lib().mp_overlay_batch(a["recs"], a["n_rec"], a["blocks"], a["faces"], a["M"], a["H"], a["W"], a["cams"], a["n_cam"], Z_CLIP,
                                      a["frames"], a["bg"], a["opacity"], a["kp"], a["K"], a["rgb"], a["conf"], a["radius"], a["keys"],
                                      a["big"], a["cam_dev"], a["out"], a["owner"], hip.stream())


def test_guard_words_statuses_and_empty_calls(scene):
    a = _direct(scene)
    assert _call(a) == 0
    torch.cuda.synchronize()
    n = M * H * W
    assert torch.equal(a["out"][:3 * n].view(M, H, W, 3), scene["out"])
    assert torch.equal(a["owner"][:4 * n].view(torch.int32).view(M, H, W), scene["owner"])
    for k, size in (("keys", 8 * n), ("big", 4 * (1 + a["faces"])), ("cam_dev", 64), ("out", 3 * n), ("owner", 4 * n)):
        assert bool((a[k][size:] == GUARD).all()), k
    queued = int(a["big"][:4].view(torch.int32)[0])
    assert 1 <= queued <= a["faces"]                                                         # the spanning triangle went through the queue
    # bad arguments: the status, and nothing is written
    bad1 = [dict(n_rec=-1), dict(blocks=-1), dict(faces=-1), dict(M=-1), dict(K=-1), dict(H=0), dict(W=0), dict(cams=None), dict(keys=None),
            dict(cam_dev=None), dict(out=None), dict(frames=None, bg=None), dict(recs=None), dict(big=None), dict(kp=None), dict(rgb=None),
            dict(H=1 << 15, W=1 << 15)]
    bad2 = [dict(n_cam=2), dict(n_cam=0), dict(faces=2 ** 32 - 1), dict(opacity=1.5), dict(opacity=-0.1), dict(opacity=float("nan")),
            dict(radius=-1), dict(radius=4097)]
    for code, cases in ((-1, bad1), (-2, bad2)):
        for bad in cases:
            b = _direct(scene)
            b.update(bad)
            with pytest.raises(RuntimeError, match=r"^mp_overlay_batch failed with code %d$" % code):
                _call(b)
            torch.cuda.synchronize()
            for k in ("keys", "big", "cam_dev", "out", "owner"):
                assert b[k] is None or bool((b[k] == GUARD).all()), (bad, k)
    # M == 0: status 0, nothing touched
    b = _direct(scene)
    b.update(M=0)
    assert _call(b) == 0
    torch.cuda.synchronize()
    assert all(bool((b[k] == GUARD).all()) for k in ("keys", "big", "cam_dev", "out", "owner"))
    # no record, M > 0: the frames plus the keypoints; no record table, no queue
    b = _direct(scene)
    b.update(recs=None, n_rec=0, blocks=0, faces=0, big=None)
    assert _call(b) == 0
    torch.cuda.synchronize()
    got = b["out"][:3 * n].view(M, H, W, 3).cpu().numpy()
    for im in range(M):
        assert np.array_equal(got[im], R.paint_keypoints(scene["frames"][im], scene["keypoints"][im], R.KP_RGB, R.KP_CONF, R.KP_RADIUS))
    assert bool((b["owner"][:4 * n].view(torch.int32) == -1).all()) and bool((b["out"][3 * n:] == GUARD).all())
