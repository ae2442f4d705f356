"""bench.py's output dump on the host: float32 files, and above the size cap the same fixed seeded sample of the rays from every
output (two builds compared output for output see the same rays)."""
import numpy as np
import torch

import bench


def _outs(n):
    g = torch.Generator().manual_seed(0)
    return {"rgb_values": torch.rand(n, 3, generator=g), "acc_map": torch.rand(n, generator=g).double(),
            "acc_person_list": torch.rand(n, 2, generator=g).half(), "n_hit": torch.arange(n)}


def test_dump_writes_every_floating_output(tmp_path):
    outs = _outs(100)
    info = bench.dump_outputs(outs, str(tmp_path))
    assert sorted(info["arrays"]) == ["acc_map", "acc_person_list", "rgb_values"] and info["sampled_rays"] is None
    rgb, acc, accp = (np.load(tmp_path / f"{k}.npy") for k in ("rgb_values", "acc_map", "acc_person_list"))
    assert rgb.dtype == np.float32 and acc.dtype == np.float64 and accp.dtype == np.float32
    assert np.array_equal(rgb, outs["rgb_values"].numpy()) and np.array_equal(accp, outs["acc_person_list"].float().numpy())


def test_dump_above_the_cap_takes_the_same_seeded_rays_from_every_output(tmp_path):
    outs = _outs(1000)
    cap = 4000                                      # bytes: 1000 rays x (12 + 8 + 8) = 28 000 in all
    a = bench.dump_outputs(outs, str(tmp_path / "a"), limit_bytes=cap)
    b = bench.dump_outputs(outs, str(tmp_path / "b"), limit_bytes=cap)
    k = a["sampled_rays"]
    assert a == {**b, "dir": a["dir"]} and 0 < k <= 1000 * cap // 28000
    rgb = np.load(tmp_path / "a" / "rgb_values.npy")
    acc = np.load(tmp_path / "a" / "acc_map.npy")
    assert sum(np.load(tmp_path / "a" / f"{n}.npy").nbytes for n in a["arrays"]) <= cap
    assert np.array_equal(rgb, np.load(tmp_path / "b" / "rgb_values.npy"))
    # the rows of every output are the same rays, in their original order
    rows = [int(np.flatnonzero((outs["rgb_values"].numpy() == r).all(1))[0]) for r in rgb]
    assert rows == sorted(rows) and np.array_equal(acc, outs["acc_map"].numpy()[rows])


def test_dump_lists_rays_with_a_non_finite_output_instead_of_writing_them(tmp_path):
    outs = _outs(50)
    outs["rgb_values"][7, 1] = float("nan")
    outs["acc_map"][30] = float("inf")
    info = bench.dump_outputs(outs, str(tmp_path))
    assert info["nonfinite_rays"] == [7, 30] and info["nonfinite_ray_count"] == 2 and info["rays"] == 50
    keep = [i for i in range(50) if i not in (7, 30)]
    rgb, acc = np.load(tmp_path / "rgb_values.npy"), np.load(tmp_path / "acc_map.npy")
    assert rgb.shape == (48, 3) and np.isfinite(rgb).all() and np.isfinite(acc).all()
    assert np.array_equal(rgb, outs["rgb_values"].numpy()[keep]) and np.array_equal(acc, outs["acc_map"].numpy()[keep])
