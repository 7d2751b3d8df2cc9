"""bench.py's command line and --dump-outputs writer, on CPU tensors (no GPU, no library)."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402  (tests/conftest.py puts the repository root on sys.path)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "somewhere"


@pytest.mark.parametrize("total", [100, 4096 * 3 + 17, 1208 * 5000, 4096 * 2100 + 5])
def test_dump_outputs_sums_cover_the_wire_and_sample_is_seeded(tmp_path, total):
    wire = (torch.arange(total, dtype=torch.int64) * 7919 % 251).to(torch.uint8)
    w = {"wire": wire, "out_off": torch.arange(3000, dtype=torch.int64) * 5, "out_len": torch.arange(3000, dtype=torch.int32)}
    bench.dump_outputs(w, str(tmp_path / "a"))
    bench.dump_outputs(w, str(tmp_path / "b"), "_rank1")
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["out_len_sample", "out_off_sample", "wire_block_sums", "wire_sample"]
    assert sorted(b) == [k + "_rank1" for k in sorted(a)]
    for k, x in a.items():
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, b[k + "_rank1"])
    host = wire.numpy()
    blk = min(bench.DUMP_BLOCK, total)
    want = np.add.reduceat(host.astype(np.int64), np.arange(0, total, blk))
    assert np.array_equal(a["wire_block_sums"], want.astype(np.float64))
    s = a["wire_sample"]
    assert s.shape == (min(total // blk, bench.DUMP_BLOCKS) + 1, blk)
    assert np.array_equal(s[-1], host[total - blk:].astype(np.float32))
    if total // blk <= bench.DUMP_BLOCKS:   # every block drawn, in ascending order
        assert np.array_equal(s[:-1].ravel(), host[:total // blk * blk].astype(np.float32))
    assert np.array_equal(a["out_off_sample"], np.arange(3000) * 5.0)
    assert np.array_equal(a["out_len_sample"], np.arange(3000, dtype=np.float32))


def test_dump_outputs_sum_blocks_double_past_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SUM_BLOCKS", 4)
    total = 4096 * 21 + 9   # 21 blocks of 4096 -> 5 of 16384 -> 2 of 32768, and a short tail
    wire = (torch.arange(total, dtype=torch.int64) * 31 % 253).to(torch.uint8)
    bench.dump_outputs({"wire": wire}, str(tmp_path))
    got = _load(tmp_path)
    assert sorted(got) == ["wire_block_sums", "wire_sample"]
    want = np.add.reduceat(wire.numpy().astype(np.int64), np.arange(0, total, 32768))
    assert np.array_equal(got["wire_block_sums"], want.astype(np.float64))


def test_dump_outputs_stays_under_64_mb_whatever_the_size():
    """The file sizes follow from the constants: block sums of at most DUMP_SUM_BLOCKS + 1
    blocks, the block sample, and for the ragged workload two entry samples."""
    total = 8 * (bench.DUMP_SUM_BLOCKS + 1) + 4 * (bench.DUMP_BLOCKS + 1) * bench.DUMP_BLOCK + (8 + 4) * bench.DUMP_ENTRIES
    assert total + 4 * 128 <= 64 * 10**6   # 128 B of .npy header per file
