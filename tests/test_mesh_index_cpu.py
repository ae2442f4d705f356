"""Face index of the mesh signed distance, host side: the header declares the entry points, hip.py binds them with the declared
arity, and the mode switch refuses values it does not know."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {"mp_mesh_index_bytes": 1, "mp_mesh_index_keys": 5, "mp_mesh_index_build": 5, "mp_mesh_index_signed_distance": 7}


def test_header_declares_and_hip_binds_the_index_entry_points():
    from multiply_amd import hip
    from multiply_amd.build import build
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "multiply_hip.h")).read(), flags=re.S)
    protos = hip.header_prototypes()
    lib = ctypes.CDLL(build(verbose=False))
    hip._declare_prototypes(lib)
    for name, arity in ENTRY_POINTS.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in the header"
        assert len([a for a in m.group(1).split(",") if a.strip() not in ("", "void")]) == arity
        assert name in protos and len(protos[name][1]) == arity
        fn = getattr(lib, name)
        assert len(fn.argtypes) == arity and fn.restype is ctypes.c_int
    # the size query returns a value, every other entry point a status that ctypes checks
    assert "mp_mesh_index_bytes" in hip.VALUE_RETURNING and lib.mp_mesh_index_bytes.errcheck is not hip._errcheck
    assert lib.mp_mesh_index_build.errcheck is hip._errcheck
    # header (16 floats) + 2 NLp nodes of 8 floats + 8 NL faces of 9 floats, NL = ceil(F / 8), NLp = NL rounded up to a power of two
    for F, NL, NLp in [(1, 1, 1), (8, 1, 1), (9, 2, 2), (1280, 160, 256), (20480, 2560, 4096)]:
        assert lib.mp_mesh_index_bytes(F) == 4 * (16 + 16 * NLp + 72 * NL)
    assert lib.mp_mesh_index_bytes(0) == 0


def test_unknown_mesh_index_mode_raises():
    from multiply_amd import hip
    from multiply_amd.multiply import Multiply
    for mode in hip.MESH_INDEX_MODES:
        assert hip.mesh_index_mode(mode) == mode
    assert hip.mesh_index_mode(None) == hip.MESH_INDEX_MODE
    with pytest.raises(ValueError, match="mesh_index_mode"):
        hip.mesh_index_mode("bvh")
    model = Multiply.__new__(Multiply)           # the setter alone: building a model needs a device
    model.mesh_index_mode = "brute"
    assert model.mesh_index_mode == "brute"
    with pytest.raises(ValueError, match="mesh_index_mode"):
        model.mesh_index_mode = "octree"
    assert model.mesh_index_mode == "brute"


def test_auto_asks_for_a_closed_surface_of_enough_faces():
    """'auto' = the index only where it was measured to win: a closed surface of MESH_INDEX_MIN_FACES faces or more; a face list
    that is no surface (as the synthetic SMPL tables' `f`), a small mesh, or faces the caller knows nothing about: brute force"""
    import torch
    from multiply_amd import hip
    from tests.test_mesh_index_gpu import icosphere
    assert hip.mesh_index_wanted("index", 1) and not hip.mesh_index_wanted("brute", 10 ** 6, True)
    N = hip.MESH_INDEX_MIN_FACES
    assert hip.mesh_index_wanted("auto", N, True) and not hip.mesh_index_wanted("auto", N - 1, True)
    assert not hip.mesh_index_wanted("auto", 10 ** 6) and not hip.mesh_index_wanted("auto", 10 ** 6, False)
    _, f = icosphere(4)                                             # 2 048 faces, closed
    assert f.shape[0] == 2048 >= N and hip.mesh_index_wanted("auto", 2048, f) and hip.mesh_index_wanted("auto", 2048, f[None])
    g = torch.Generator().manual_seed(0)
    soup = torch.randint(0, 1026, (2048, 3), generator=g)           # triangles between arbitrary vertices
    assert not hip.mesh_index_wanted("auto", 2048, soup)
    assert not hip.mesh_index_wanted("auto", 2048, f[:-1])          # one face missing: open, and not this mesh's face list
    _, f3 = icosphere(3)
    assert not hip.mesh_index_wanted("auto", 512, f3)
