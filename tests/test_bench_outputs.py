"""bench.py --dump-outputs (bench_outputs.py) on CPU tensors: file formats, the byte budget, the fixed sample."""
import types

import numpy as np
import torch

import bench_outputs as bo


def _dump(tmp_path, outputs, rank=0):
    bo.dump_outputs(types.SimpleNamespace(dump_outputs=str(tmp_path)), rank, outputs)
    return {p.stem: np.load(p) for p in sorted(tmp_path.glob("*.npy"))}


def test_small_arrays_are_stored_whole(tmp_path):
    z = torch.arange(12, dtype=torch.float32).view(3, 4)
    got = _dump(tmp_path, {"bytes": torch.arange(200, 256, dtype=torch.uint8).view(7, 8),
                           "iq": torch.complex(z, -z)[:, :3],  # a non-contiguous slice, as the sample buffers are
                           "counts": torch.tensor([-1, 7, 1 << 30], dtype=torch.int32),
                           "host": np.arange(6, dtype=np.float64).reshape(2, 3)})
    assert got["bytes"].dtype == np.float32 and got["bytes"].shape == (7, 8)
    assert np.array_equal(got["bytes"].ravel(), np.arange(200, 256))
    assert got["iq"].dtype == np.float32 and got["iq"].shape == (3, 3, 2)
    assert np.array_equal(got["iq"][..., 0], z[:, :3].numpy()) and np.array_equal(got["iq"][..., 1], -z[:, :3].numpy())
    assert got["counts"].dtype == np.float64 and got["counts"].tolist() == [-1.0, 7.0, float(1 << 30)]
    assert got["host"].dtype == np.float64 and got["host"].shape == (2, 3)


def test_large_array_is_a_fixed_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bo, "DUMP_BUDGET_BYTES", 4000)
    big = torch.arange(5000, dtype=torch.int16)
    a = _dump(tmp_path / "a", {"big": big, "small": torch.ones(10)})
    b = _dump(tmp_path / "b", {"big": big, "small": torch.ones(10)})
    assert sum(v.nbytes for v in a.values()) <= 4000
    assert a["big"].shape == (500,) and a["small"].shape == (10,)   # 2000 bytes each: 500 float32
    assert np.array_equal(a["big"], b["big"])                        # the same sample in every run
    assert np.all(np.diff(a["big"]) >= 0) and a["big"].max() > 4000  # sorted flat indices over the whole array


def test_only_rank_0_writes_and_no_directory_means_no_files(tmp_path):
    assert _dump(tmp_path, {"x": torch.ones(3)}, rank=1) == {}
    bo.dump_outputs(types.SimpleNamespace(dump_outputs=None), 0, {"x": torch.ones(3)})
    assert list(tmp_path.iterdir()) == []


def test_records_to_columns_flattens_nested_records():
    inner = np.dtype([("ok", "<i4"), ("its", "<u4")])
    dt = np.dtype([("data", inner), ("sinr", "<f4"), ("ack", "u1", (2,)), ("pad", "u1", (2,))])
    rec = np.zeros(3, dt)
    rec["data"]["ok"], rec["data"]["its"], rec["sinr"] = [1, 0, 1], [2, 6, 3], [30.5, -1.0, 12.25]
    rec["ack"] = [[1, 0], [0, 0], [1, 1]]
    raw = torch.from_numpy(rec.view(np.uint8).reshape(3, dt.itemsize))
    cols = bo.records_to_columns(raw, dt)
    assert cols.dtype == np.float64 and cols.shape == (3, 7)
    assert np.array_equal(cols[:, :5], [[1, 2, 30.5, 1, 0], [0, 6, -1.0, 0, 0], [1, 3, 12.25, 1, 1]])
