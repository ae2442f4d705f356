"""Host side of the deterministic training mode (no GPU): the workspace size queries of include/multiply_hip.h against the slice
plans of tests/gemm_reference.py, the switch (environment variable, model attribute, Trainer config key), the checkpoint's record."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from tests import gemm_reference as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from multiply_amd.build import build
    build(verbose=False)
    from multiply_amd import hip
    return hip.lib()


def _single(lib, M, N, K, b3):
    need = C.c_longlong(-1)
    assert lib.mp_gemm_tn_ws_bytes(M, N, K, int(b3), C.byref(need)) == 0
    return need.value


def _up(x):
    return (x + 127) // 128 * 128


@pytest.mark.parametrize("shape", [(128, 128, 296), (100, 36, 296), (256, 256, 50000), (257, 39, 3000), (3, 128, 777)])
def test_single_launch_workspace_is_slices_times_padded_tile_plus_column_sums(lib, shape):
    M, N, K = shape
    rows, slices = G.tn_rows_per_block(M, N, K)
    for b3 in (False, True):
        assert _single(lib, M, N, K, b3) == 4 * slices * (_up(M) * _up(N) + _up(M)), (shape, b3)
    if shape[2] == 296:
        assert slices == 3                                   # the GPU test's three slices, the last ragged
    for empty in ((0, N, K), (M, 0, K), (M, N, 0)):
        assert _single(lib, *empty, True) == 0


def _groups(shapes, colsum):
    from multiply_amd.train import MpTnGroup
    recs = [MpTnGroup(4096, 8192, 12288 + 16 * i, 65536 + 16 * i if cs else None, M, N, N, M, N, K, K if cs else 0, 0)
            for i, ((M, N, K), cs) in enumerate(zip(shapes, colsum))]
    return (MpTnGroup * len(recs))(*recs), len(recs)


def _grouped(lib, shapes, colsum):
    need = C.c_longlong(-1)
    arr, n = _groups(shapes, colsum)
    assert lib.mp_gemm_tn_grouped_ws_bytes(arr, n, C.byref(need)) == 0
    return need.value


def test_grouped_workspace_follows_the_grouped_slice_plans(lib):
    # wide form: three 256 x 256 groups (the GPU test's), column sums on the first and the last
    Ks = (600, 256, 40)
    rows, per, _ = G.wide_rows_per_block(Ks)
    assert (rows, per) == (256, [3, 1, 1])
    want = 4 * sum(s * (256 * 256 + (256 if cs else 0)) for s, cs in zip(per, (True, False, True)))
    assert _grouped(lib, [(256, 256, k) for k in Ks], (True, False, True)) == want
    # the largest wide round: 24 groups of long contractions, at most 256 slices of 256 KiB (+ 1 KiB of column sums each)
    Ks = [60000 + 32 * i for i in range(24)]
    rows, per, _ = G.wide_rows_per_block(Ks)
    assert sum(per) <= G.TNW_WGS
    got = _grouped(lib, [(256, 256, k) for k in Ks], [True] * 24)
    assert got == 4 * sum(per) * (256 * 256 + 256) and got <= 256 * (256 * 1024 + 1024)
    from multiply_amd import train as T
    assert got <= T.DET_WS_BYTES                             # the host's workspace never has to grow for the shipped networks
    # tiled form: the GPU test's two groups of 128 x 256
    shapes = [(128, 256, 300), (128, 256, 257)]
    rows, per, mt, nt = G.tiled_rows_per_block([s[:2] for s in shapes], [s[2] for s in shapes])
    assert per == [2, 2]
    assert _grouped(lib, shapes, (True, True)) == 4 * sum(s * (128 * 256 + 128) for s in per)
    # the argument checks of the atomic entry point hold for the query too
    need = C.c_longlong(-1)
    arr, n = _groups([(192, 256, 64)], (False,))
    with pytest.raises(RuntimeError, match="mp_gemm_tn_grouped_ws_bytes failed with code -2"):
        lib.mp_gemm_tn_grouped_ws_bytes(arr, n, C.byref(need))


def test_small_partial_buffers(lib):
    n = C.c_longlong(-1)
    lib.mp_tf_bwd_part_floats(300, C.byref(n))
    assert n.value == (3 + 1) * 260                          # three tiles' rows and one run's
    lib.mp_tf_bwd_part_floats(66 * 128 - 127, C.byref(n))
    assert n.value == (66 + 2) * 260
    lib.mp_tr_warp_bwd_part_floats(700, C.byref(n))
    assert n.value == 3 * 288                                # runs of 256 points
    lib.mp_tr_warp_bwd_part_floats(256 * 512 + 1, C.byref(n))
    assert n.value == 257 * 288                              # more than 512 runs of 256: runs of 512 points
    lib.mp_tr_warp_bwd_part_floats(0, C.byref(n))
    assert n.value == 0


def test_flag_from_environment_model_and_config(monkeypatch):
    from multiply_amd import train as T
    from multiply_amd import trainer as TR
    from multiply_amd.config import to_config
    for v, want in (("1", True), ("true", True), ("on", True), ("0", False), ("", False), ("false", False), ("off", False)):
        assert T._env_flag(v) is want, v
    assert T.DETERMINISTIC == T._env_flag(os.environ.get("MP_TRAIN_DETERMINISTIC", "0"))

    class M:
        pass
    m = M()
    for default in (False, True):
        monkeypatch.setattr(T, "DETERMINISTIC", default)
        assert T.deterministic() is default and T.deterministic(m) is default
        m.train_deterministic = None
        assert T.deterministic(m) is default
        for v in (True, False):
            m.train_deterministic = v
            assert T.deterministic(m) is v               # the model's own setting wins over the process default
        del m.train_deterministic
    assert TR.deterministic_from_config(to_config({})) is None and TR.deterministic_from_config(to_config({}), default=False) is False
    assert TR.deterministic_from_config(to_config({"deterministic": True})) is True
    assert TR.deterministic_from_config(to_config({"deterministic": False})) is False
    assert TR.deterministic_from_config(to_config({"deterministic": "1"})) is True
    assert TR.deterministic_from_config(to_config({"deterministic": "off"})) is False


def test_environment_variable_is_read_at_import():
    code = "import multiply_amd.train as T; print(T.DETERMINISTIC, T.deterministic())"
    for value, want in (("1", "True True"), ("0", "False False")):
        r = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=dict(os.environ, MP_TRAIN_DETERMINISTIC=value),
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip().splitlines()[-1] == want


def test_checkpoint_records_the_mode():
    from multiply_amd import trainer as TR
    args = (4, 15, {}, [], [{}, {}], [])
    assert "deterministic" not in TR.checkpoint_dict(*args)
    assert TR.checkpoint_dict(*args, deterministic=True)["deterministic"] is True
    assert TR.checkpoint_dict(*args, deterministic=False)["deterministic"] is False
    ck = TR.checkpoint_dict(*args, deterministic=True)
    assert TR.split_checkpoint(ck) == ({}, [])              # the record does not disturb the readers of the state dict


def test_tools_take_the_switch():
    for tool in ("train.py", "train_bench.py", "determinism_check.py"):
        assert "--deterministic" in open(os.path.join(REPO, "tools", tool)).read(), tool
