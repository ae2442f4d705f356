"""Host side of the mesh overlays (multiply_amd/overlay.py) and the float64 restatement the GPU tests compare against
(tests/overlay_reference.py): none of this needs a device."""
import ctypes as C
import re

import numpy as np
import pytest

from multiply_amd import hip
from multiply_amd import overlay as OV
from tests import overlay_reference as R


# ------------------------------------------------------------------------------------------------ vertex_adjacency
def test_adjacency_of_an_icosahedron():
    v, f = R.icosphere(subdivisions=0)
    assert v.shape == (12, 3) and f.shape == (20, 3)
    ptr, adj = OV.vertex_adjacency(f, 12)
    assert ptr.dtype == np.int32 and adj.dtype == np.int32
    assert ptr.tolist() == list(range(0, 61, 5)) and adj.shape == (60,)            # five faces around every vertex
    for i in range(12):
        mine = adj[ptr[i]:ptr[i + 1]].tolist()
        assert mine == sorted(mine) == [k for k in range(20) if i in f[k]]
    v1, f1 = R.icosphere()
    assert v1.shape == (42, 3) and f1.shape == (80, 3)
    ptr1, _ = OV.vertex_adjacency(f1, 42)
    assert sorted(np.diff(ptr1).tolist()) == [5] * 12 + [6] * 30


def test_adjacency_with_an_isolated_vertex_and_a_repeated_face():
    f = np.array([[0, 1, 2], [2, 1, 4], [0, 1, 2]])                                # vertex 3 in no face; face 0 twice
    ptr, adj = OV.vertex_adjacency(f, 6)
    assert ptr.tolist() == [0, 2, 5, 8, 8, 9, 9]
    assert adj.tolist() == [0, 2, 0, 1, 2, 0, 1, 2, 1]
    import torch
    ptr_t, adj_t = OV.vertex_adjacency(torch.tensor(f), 6)
    assert np.array_equal(ptr_t, ptr) and np.array_equal(adj_t, adj)
    e_ptr, e_adj = OV.vertex_adjacency(np.zeros((0, 3), int), 3)
    assert e_ptr.tolist() == [0, 0, 0, 0] and e_adj.size == 0
    with pytest.raises(ValueError, match="faces index vertices"):
        OV.vertex_adjacency(f, 4)
    with pytest.raises(ValueError, match="faces index vertices"):
        OV.vertex_adjacency(np.array([[0, -1, 2]]), 4)
    with pytest.raises(ValueError):
        OV.vertex_adjacency(f, -1)


# ------------------------------------------------------------------------------------------------ the record table
def test_record_table_prefix_sums_and_limits():
    entries = [(1000, 2000, 3000, 42, 80, 0), (1100, 2000, 3100, 42, 0, 0), (1200, 2200, 3200, 7, 256, 2), (1300, 2300, 3300, 9, 257, 1)]
    table, blocks, faces = OV.record_table(entries, 3)
    assert C.sizeof(OV.MpOverlayMesh) == 48 and len(table) == 4
    assert [r.face_base for r in table] == [0, 80, 80, 336] and faces == 593
    assert [r.block0 for r in table] == [0, 1, 1, 2] and blocks == 4               # a record without faces has no block
    assert [(r.verts, r.faces, r.colors, r.n_verts, r.n_faces, r.image) for r in table] == [tuple(e) for e in entries]
    empty, b0, f0 = OV.record_table([], 2)
    assert (b0, f0) == (0, 0) and len(empty) == 1
    with pytest.raises(ValueError, match=r"image 3 outside \[0, 3\)"):
        OV.record_table([(1, 2, 3, 4, 5, 3)], 3)
    with pytest.raises(ValueError, match=r"image -1 outside"):
        OV.record_table([(1, 2, 3, 4, 5, -1)], 3)
    with pytest.raises(ValueError, match="negative size"):
        OV.record_table([(1, 2, 3, 4, -5, 0)], 3)
    big = 2 ** 31 - 1
    assert OV.record_table([(1, 2, 3, 4, big, 0), (1, 2, 3, 4, big, 0)], 1)[2] == 2 ** 32 - 2 == OV.MAX_FACES
    with pytest.raises(ValueError, match="a face id is 32 bits"):                  # 2^32 - 1 is the empty key's low word
        OV.record_table([(1, 2, 3, 4, big, 0), (1, 2, 3, 4, big, 0), (1, 2, 3, 4, 1, 0)], 1)
    # the struct is the header's
    hdr = open(hip.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\} MpOverlayMesh;", hdr).group(1)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [n for n, _ in OV.MpOverlayMesh._fields_]
    assert [OV.MODES[k] for k in ("normal", "shade", "tint")] == [0, 1, 2]
    assert "enum { MP_OVERLAY_NORMAL = 0, MP_OVERLAY_SHADE = 1, MP_OVERLAY_TINT = 2 };" in hdr


def test_render_overlays_refuses_bad_arguments_before_touching_a_device():
    import torch
    v, f = R.icosphere()
    mesh = [(torch.from_numpy(v), torch.from_numpy(f), torch.zeros(42, 3))]
    for kw, msg in ((dict(opacity=1.5), "opacity"), (dict(opacity=float("nan")), "opacity"), (dict(kp_radius=-1), "kp_radius"),
                    (dict(kp_radius=5000), "kp_radius"), (dict(images_per_call=0), "images_per_call"),
                    (dict(frames=torch.zeros(1, 4, 5, 3)), "frames"), (dict(background=(0, 0, 256)), "background"),
                    (dict(keypoints=torch.zeros(1, 2, 3)), "kp_rgb"), (dict(keypoints=torch.zeros(2, 3)), "keypoints"),
                    (dict(frames=torch.zeros(2, 4, 5, 3, dtype=torch.uint8), keypoints=torch.zeros(1, 0, 3)), "keypoints")):
        with pytest.raises(ValueError, match=msg):
            OV.render_overlays(mesh, [0], R.CAM, 4, 5, **kw)
    with pytest.raises(ValueError, match="image size"):
        OV.render_overlays(mesh, [0], R.CAM, 0, 5)
    with pytest.raises(ValueError, match="cams"):
        OV.render_overlays(mesh, [0], R.CAM[:15], 4, 5)
    with pytest.raises(ValueError, match="2 cameras for 3 images"):
        OV.render_overlays(mesh, [0], [R.CAM, R.CAM], 4, 5, n_images=3)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_on_a_hand_computed_image():
    """4 x 5 pixels, camera f = 1 at the origin (pixel = X / Z).  Triangle 0 at z = 2 with the pixel-space corners (0, 0), (4, 0),
    (0, 4) and the corner colours red, green, blue: the pixel centres strictly inside are those with r + c <= 2 (r + c = 3 lies ON
    the hypotenuse: not covered), and at constant depth the barycentrics are the affine ones, b = (1 - (x + y) / 4, x / 4, y / 4).
    Triangle 1 at z = 1 with corners (0, 0), (1.2, 0), (0, 1.2), uniformly (0.5, 0.25, 0.75), covers the centre of pixel (0, 0)
    only and is nearer.  Frame = 100 everywhere, opacity 0.5: out = floor(0.5 (m - 100) + 100.5).  A keypoint at (3.7, 2.2) with
    radius 1 is the plus-shaped disc around column 3, row 2."""
    H, W = 4, 5
    cam = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 1.0, 0.0, 0.0]
    tri0 = (np.array([[0, 0, 2], [8, 0, 2], [0, 8, 2.0]]), np.array([[0, 1, 2]]), np.eye(3))
    tri1 = (np.array([[0, 0, 1], [1.2, 0, 1], [0, 1.2, 1.0]]), np.array([[0, 1, 2]]), np.tile([0.5, 0.25, 0.75], (3, 1)))
    kp, rgb = np.array([[3.7, 2.2, 1.0], [0.0, 0.0, 0.0]]), np.array([[9, 8, 7], [1, 1, 1]], dtype=np.uint8)
    out, owner, _ = R.render([tri0, tri1], cam, H, W, np.full((H, W, 3), 100, np.uint8), opacity=0.5, keypoints=kp, kp_rgb=rgb,
                             kp_conf=0.0, radius=1)
    want = np.full((H, W, 3), 100, np.uint8)
    want_owner = -np.ones((H, W), int)
    # m: (0,0) tri1 (127, 63, 191); tri0: 255 b floored
    for (r, c), m, who in (((0, 0), (127, 63, 191), 1), ((0, 1), (127, 95, 31), 0), ((0, 2), (63, 159, 31), 0),
                           ((1, 0), (127, 31, 95), 0), ((1, 1), (63, 95, 95), 0), ((2, 0), (63, 31, 159), 0)):
        want[r, c] = [int(np.floor(0.5 * (x - 100) + 100.5)) for x in m]
        want_owner[r, c] = who
    assert want[0, 0].tolist() == [114, 82, 146] and want[0, 2].tolist() == [82, 130, 66]      # the arithmetic by hand
    for r, c in ((2, 3), (1, 3), (3, 3), (2, 2), (2, 4)):
        want[r, c] = [9, 8, 7]
    assert np.array_equal(owner, want_owner)
    assert np.array_equal(out, want)
    # the other order: the nearer triangle still wins; at EQUAL depth the earlier record does
    assert R.render([tri1, tri0], cam, H, W, want * 0, opacity=1.0)[1][0, 0] == 0
    assert R.rasterize([tri0[:2], tri0[:2]], cam, H, W)[0].max() == 0
    # opacity 0 gives the frame back, 1 the mesh byte
    assert np.array_equal(R.blend(np.array([191.25]), 100, 0.0), [100]) and np.array_equal(R.blend(np.array([191.25]), 100, 1.0), [191])


def test_reference_normals_and_colour_modes():
    v, f = R.icosphere()
    n, mag, cnt = R.vertex_normals(v, f)
    assert np.abs(n - v / np.linalg.norm(v, axis=1, keepdims=True)).max() < 0.05             # a sphere's normals point outwards
    assert cnt.sum() == 240 and (mag > 0).all()
    v2 = np.concatenate([v, [[5, 5, 5]]]).astype(np.float32)
    assert (R.vertex_normals(v2, f)[0][42] == 0).all()                                        # an isolated vertex
    assert R.normals_bound(v, f).max() < 1e-5
    nn = n[None]
    c, b = R.vertex_colors(nn, "normal")
    assert np.allclose(c[0, :, 0], n[:, 2] * 0.5 + 0.5) and np.allclose(c[0, :, 2], n[:, 0] * 0.5 + 0.5) and b.max() <= 2 * R.U
    c, _ = R.vertex_colors(nn, "shade")
    assert np.array_equal(c[0, :, 0], np.maximum(n[:, 2], 0)) and np.array_equal(c[..., 0], c[..., 2])
    c, _ = R.vertex_colors(nn, "tint", tint=[[1.0, 0.5, 0.25]], light=(0, 0, -1), ambient=0.25)
    assert np.allclose(c[0, :, 1], 0.5 * (0.25 + 0.75 * np.maximum(-n[:, 2], 0)))


def test_base_scene_meets_the_conditions_the_gpu_test_relies_on():
    """in float64 alone: every path is reached, the tie exists, and at most 1 % of the covered pixels have a channel whose 255 c
    lies within the margin of an integer (the colours are seeded and kept away from the clamp for this)"""
    s = R.base_scene()
    assert [m[0].shape[0] for m in s["meshes"]] == [42, 42, 3, 42, 9] and s["image_of"] == [0, 0, 0, 1, 1]
    covered = near = 0
    for im in range(R.M):
        ms = [m for m, i in zip(s["meshes"], s["image_of"]) if i == im]
        out, owner, v = R.render(ms, R.CAM, R.H, R.W, s["frames"][im], opacity=0.6)
        hit = owner >= 0
        covered += hit.sum()
        near += (np.abs(v[hit] - np.round(v[hit])) <= R.MARGIN).any(-1).sum()
        if im == 0:
            assert set(np.unique(owner)) == {-1, 0, 1}                                        # the copy never wins its ties
            alone = R.rasterize([ms[2][:2]], R.CAM, R.H, R.W)[0] >= 0
            assert alone.sum() >= 3 and (owner[alone] == 0).all()                             # and they are visible ties
            assert (owner == 0).sum() > 100 and (owner == 1).sum() > 100
        if im == 1:
            assert hit.all() and (owner == 0).sum() > 50 and (owner[:, -1] == 0).any()        # the spanning triangle; sphere cut by the border
        if im == 2:
            assert not hit.any() and np.array_equal(out, s["frames"][2])
    assert covered > 2000 and near <= 0.01 * covered, (near, covered)
    kp = s["keypoints"][0]
    img = R.paint_keypoints(np.zeros((R.H, R.W, 3), np.uint8), kp, R.KP_RGB, R.KP_CONF, R.KP_RADIUS)
    seen = {tuple(c) for c in img.reshape(-1, 3).tolist()}
    assert seen == {(0, 0, 0), tuple(R.KP_RGB[0]), tuple(R.KP_RGB[1]), tuple(R.KP_RGB[5])}
    assert tuple(img[0, 0]) == tuple(R.KP_RGB[0]) and tuple(img[20, R.W - 1]) == tuple(R.KP_RGB[1])
    assert tuple(img[21, R.W - 4]) == tuple(R.KP_RGB[5])                                      # inside both discs: the higher index


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_the_entry_points():
    protos = hip.header_prototypes()
    src = open(hip.HEADER_PATH.replace("include/multiply_hip.h", "multiply_amd/csrc/overlay.hip")).read()
    for name, arity in (("mp_mesh_vertex_normals", 9), ("mp_overlay_vertex_colors", 11), ("mp_overlay_batch", 24)):
        assert name in protos and name not in hip.VALUE_RETURNING, name
        rt, at = protos[name]
        assert rt is C.c_int and len(at) == arity and at[-1] is hip.DevPtr, (name, len(at))
        assert re.search(r'extern "C" int %s\(' % name, src), name
    at = protos["mp_overlay_batch"][1]
    assert at[3] is C.c_longlong and at[12] is C.c_float and at[16] is C.c_float           # total_faces, opacity, kp_conf
    # the raster rule has one home
    raster = open(hip.HEADER_PATH.replace("include/multiply_hip.h", "multiply_amd/csrc/raster.hip")).read()
    assert '#include "raster_prims.hpp"' in raster and '#include "raster_prims.hpp"' in src
    assert "bool cover(" not in raster and "bool cover(" not in src
