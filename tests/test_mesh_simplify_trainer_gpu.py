"""Trainer.test with the config keys test_mesh_cell / test_mesh_faces (multiply_amd/trainer.py): the scene of
tests/test_trainer_gpu.py::test_test_run_on_one_frame (3 frames of 64 x 64, 2 persons), one frame tested."""
import os

import numpy as np
import pytest

from tests.test_trainer_gpu import _build, _load_ply_faces

pytestmark = pytest.mark.gpu


def _files(root):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            if n.endswith((".ply", ".png")):
                with open(os.path.join(d, n), "rb") as fh:
                    out[os.path.relpath(os.path.join(d, n), root)] = fh.read()
    return out


def test_test_run_writes_simplified_meshes_and_nothing_else_changes(tmp_path):
    tr = _build(tmp_path)
    assert tr.opt.get("test_mesh_cell", None) is None and tr.opt.get("test_mesh_faces", None) is None
    run = tr.out_dir

    def test_into(name, **keys):
        for k in ("test_mesh_cell", "test_mesh_faces"):
            tr.opt.pop(k, None)
        for k, v in keys.items():
            tr.opt[k] = v
        tr.out_dir = os.path.join(run, name)
        os.makedirs(tr.out_dir, exist_ok=True)
        tr.test(frames=[1])
        return _files(tr.out_dir)
    absent = test_into("absent")
    unset = test_into("unset", test_mesh_cell=None, test_mesh_faces=None)
    assert len(absent) == 4 * 3 + 2 + 4 and absent == unset               # every file, byte for byte
    # the renderings do not depend on the meshes: the third run skips them
    tr._render_frame = lambda *a, **k: {}
    fewer = test_into("fewer", test_mesh_faces=400)
    assert sorted(fewer) == sorted(k for k in absent if k.endswith(".ply"))
    for p in (0, 1):
        vc, fc = _load_ply_faces(os.path.join(run, "fewer", "test_mesh", str(p), "0001_canonical.ply"))
        vd, fd = _load_ply_faces(os.path.join(run, "fewer", "test_mesh", str(p), "0001_deformed.ply"))
        _, f0 = _load_ply_faces(os.path.join(run, "absent", "test_mesh", str(p), "0001_canonical.ply"))
        print(f"[trainer test_mesh_faces = 400] person {p}: {f0.shape[0]} -> {fc.shape[0]} faces")
        assert np.array_equal(fc, fd) and vc.shape == vd.shape and not np.array_equal(vc, vd)
        assert 0 < fc.shape[0] < f0.shape[0] and fc.max() == vc.shape[0] - 1
    cell = test_into("cell", test_mesh_cell=0.1)
    for p in (0, 1):
        _, fc = _load_ply_faces(os.path.join(run, "cell", "test_mesh", str(p), "0001_canonical.ply"))
        _, f0 = _load_ply_faces(os.path.join(run, "absent", "test_mesh", str(p), "0001_canonical.ply"))
        assert 0 < fc.shape[0] < f0.shape[0]
