"""Where the overlays are used: scene_build.build_scene(..., overlays=True) on the scene-builder tests' synthetic sequence, and
Trainer.test with the config key test_overlay on the trainer tests' written sequence, overlay.write_fit_overlays (tools/refine_smpl.py
--overlays) on the keypoint-fit tests' recovery sequence."""
import os

import numpy as np
import pytest
import torch

from multiply_amd import scene_build as SB
from tests import scene_build_reference as R

pytestmark = pytest.mark.gpu


def _files(root, skip=()):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            rel = os.path.relpath(os.path.join(d, n), root)
            if not rel.startswith(tuple(skip)):
                out[rel] = os.path.join(d, n)
    return out


def test_build_scene_writes_overlays_inside_the_masks(smpl_tables, tmp_path):
    from PIL import Image
    from multiply_amd.smpl import SMPLServer
    server = SMPLServer(smpl_tables=smpl_tables)
    seq = R.sequence()
    H, W = R.SEQ_SIZE
    F, P = seq["pose"].shape[:2]
    assert (F, P) == (3, 2)
    raw = tmp_path / "raw"
    os.makedirs(raw / "frames")
    frames = np.random.RandomState(4).randint(0, 256, (F, H, W, 3)).astype(np.uint8)
    paths = []
    for f in range(F):
        paths.append(str(raw / "frames" / ("%04d.png" % f)))
        Image.fromarray(frames[f]).save(paths[-1])
    refined = {k: torch.from_numpy(v) for k, v in seq.items()}
    plain, with_ov = str(tmp_path / "plain"), str(tmp_path / "overlays")
    SB.build_scene(server, refined, R.SEQ_K, (H, W), out_dir=plain, frames=paths)
    sc = SB.build_scene(server, refined, R.SEQ_K, (H, W), out_dir=with_ov, frames=paths, overlays=True)
    # without the flag: no overlay/ and the same bytes in every other file
    a, b = _files(plain), _files(with_ov, skip=("overlay",))
    assert sorted(a) == sorted(b) and not os.path.exists(os.path.join(plain, "overlay"))
    for rel in a:
        if rel.endswith(".npz"):                                                                # a zip archive carries time stamps
            x, y = np.load(a[rel]), np.load(b[rel])
            assert sorted(x.files) == sorted(y.files) and all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in x.files), rel
        else:
            assert open(a[rel], "rb").read() == open(b[rel], "rb").read(), rel
    want = sorted(os.path.join("overlay", d, "%04d.png" % f) for d in ("all", "0", "1") for f in range(F))
    assert sorted(_files(os.path.join(with_ov, "overlay")).keys()) == sorted(os.path.relpath(w, "overlay") for w in want)
    rawm = sc["raw_masks"].cpu().numpy() > 0                                                   # (F, P, H, W), undilated
    for f in range(F):
        img = np.asarray(Image.open(os.path.join(with_ov, "image", "%04d.png" % f)))
        assert np.array_equal(img, frames[f])
        pic = np.asarray(Image.open(os.path.join(with_ov, "overlay", "all", "%04d.png" % f)))
        assert pic.shape == (H, W, 3) and pic.dtype == np.uint8
        changed = (pic != img).any(-1)
        union = rawm[f].any(0)
        assert not changed[~union].any() and changed[union].mean() > 0.9, (f, changed[union].mean())
        for p in range(P):
            one = np.asarray(Image.open(os.path.join(with_ov, "overlay", str(p), "%04d.png" % f)))
            ch = (one != img).any(-1)
            assert not ch[~rawm[f, p]].any() and ch[rawm[f, p]].mean() > 0.9, (f, p)
        # the persons are tinted with COLOR_DICT: red and green dominate their own visible parts
        only0, only1 = rawm[f, 0] & ~rawm[f, 1], rawm[f, 1] & ~rawm[f, 0]
        assert (pic[only0][:, 1:] == 0).all() and (pic[only0][:, 0] > 0).all()
        assert (pic[only1][:, [0, 2]] == 0).all() and (pic[only1][:, 1] > 0).all()
    with pytest.raises(ValueError, match="overlays"):
        SB.build_scene(server, refined, R.SEQ_K, (H, W), overlays=True)


def test_trainer_test_writes_the_overlay(tmp_path):
    from PIL import Image
    from tests.test_trainer_gpu import _build
    tr = _build(tmp_path)
    tr.test(frames=[1])
    before = sorted(_files(tr.out_dir))
    assert not any(k.startswith("test_overlay") for k in before)
    tr.opt["test_overlay"] = True
    tr.test(frames=[1])
    after = _files(tr.out_dir)
    assert sorted(k for k in after if not k.startswith("test_overlay")) == before                # the other outputs: as without it
    assert sorted(k for k in after if k.startswith("test_overlay")) == [os.path.join("test_overlay", "0001.png")]
    pic = np.asarray(Image.open(after[os.path.join("test_overlay", "0001.png")]))
    _, targets, _, _, idx = tr._test_inputs(1)
    frame = (targets["rgb"].reshape(64, 64, 3).float() * 255).round().to(torch.uint8).cpu().numpy()
    assert idx == 1 and pic.shape == (64, 64, 3) and pic.dtype == np.uint8
    changed = (pic != frame).any(-1)
    assert 0.01 < changed.mean() < 0.9, changed.mean()                                           # the bodies, not the whole frame


def test_fit_overlays_show_the_body_and_both_keypoint_sets(smpl_tables, tmp_path):
    """overlay.write_fit_overlays (tools/refine_smpl.py --overlays) on the keypoint-fit tests' recovery sequence"""
    from PIL import Image
    from multiply_amd import keypoint_fit as KF
    from multiply_amd import overlay as OV
    from multiply_amd.smpl import SMPLServer
    from tests import keypoint_fit_cases as C
    server = SMPLServer(smpl_tables=smpl_tables)
    cs = C.recovery_case()
    H, W = 500, 512
    cam = dict(zip(("fx", "fy", "cx", "cy"), cs["cam"][:4].tolist()))
    frames = np.random.RandomState(2).randint(0, 256, (C.REC_F, H, W, 3)).astype(np.uint8)
    paths = []
    for f in range(C.REC_F):
        paths.append(str(tmp_path / ("%04d.png" % f)))
        Image.fromarray(frames[f]).save(paths[-1])
    fit = dict(zip(("pose", "trans", "shape"), KF.split_params(cs["init"])))
    dst = str(tmp_path / "init")
    OV.write_fit_overlays(dst, server, fit, cs["keypoints"], cs["kmap"], cam, paths, conf_threshold=0.6, kp_radius=2, frames_per_call=2)
    assert sorted(_files(dst)) == sorted(os.path.join(str(p), "%04d.png" % f) for p in range(C.REC_P) for f in range(C.REC_F))
    proj = KF.project_keypoints(server, cs["init"].reshape(-1, 85), cs["kmap"], cam)[0].reshape(C.REC_F, C.REC_P, -1, 2).cpu().numpy()
    kp = cs["keypoints"].numpy()
    for f in range(C.REC_F):
        for p in range(C.REC_P):
            pic = np.asarray(Image.open(os.path.join(dst, str(p), "%04d.png" % f)))
            assert pic.shape == (H, W, 3)
            changed = (pic != frames[f]).any(-1)
            assert 0.005 < changed.mean() < 0.5                                                  # a body, not the frame
            seen = 0
            for x, y in proj[f, p]:                                                              # green is painted last
                c, r = int(np.floor(x)), int(np.floor(y))
                if 0 <= c < W and 0 <= r < H:
                    assert tuple(pic[r, c]) == (0, 255, 0)
                    seen += 1
            for x, y, conf in kp[f, p]:                                                          # red unless a green disc covers it
                c, r = int(np.floor(x)), int(np.floor(y))
                if conf > np.float32(0.6) and 0 <= c < W and 0 <= r < H:
                    assert tuple(pic[r, c]) in ((255, 0, 0), (0, 255, 0))
            assert seen >= 10
    with pytest.raises(ValueError, match="frames"):
        OV.write_fit_overlays(dst, server, fit, cs["keypoints"], cs["kmap"], cam, paths[:1])
