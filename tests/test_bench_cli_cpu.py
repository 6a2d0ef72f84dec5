"""bench.py's options (CPU): --full and --dump-outputs exist, and dump_outputs writes what one step counted -- float64, at most
64 MB, the same seeded sample of bins every time -- here from a stand-in engine and a host vector."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _StandInEngine:
    """reset / submit_device / finish(copy=False) on a host vector: one submit adds (id % 7) to every bin."""

    def __init__(self, table):
        self.table = table

    def reset(self):
        self.table.zero_()

    def submit_device(self, bases_ptr, nbytes, offsets_ptr, nreads):
        import torch
        self.table += torch.arange(self.table.numel(), dtype=torch.int64) % 7

    def finish(self, copy=True):
        return None, int(self.table.sum()), int((self.table != 0).sum())


def test_bench_has_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "--steps" in p.stderr


@pytest.mark.parametrize("k", [8, 12])
def test_dump_outputs_one_step_float64_bounded_seeded(tmp_path, k):
    import torch
    b = _bench_module()
    dumps = []
    for run in range(2):
        table = torch.full((4 ** k,), 5, dtype=torch.int64)          # (what earlier steps left: cleared first)
        d = tmp_path / str(run)
        b.dump_outputs(torch, np, _StandInEngine(table), table, (table, table), 0, 0, k, str(d))
        files = sorted(os.listdir(d))
        assert files == ["counts_block_sums.npy", "counts_sample.npy", "counts_sample_ids.npy", "totals.npy"]
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        a = {f[:-4]: np.load(d / f) for f in files}
        assert all(v.dtype == np.float64 for v in a.values())
        dumps.append(a)
    a = dumps[0]
    ids = a["counts_sample_ids"].astype(np.int64)
    assert ids.size == min(4 ** k, b.DUMP_SAMPLE_BINS) and np.all(np.diff(ids) > 0) and ids[-1] < 4 ** k
    assert np.array_equal(a["counts_sample"], (ids % 7).astype(np.float64))
    want = np.arange(4 ** k, dtype=np.int64) % 7
    assert a["counts_block_sums"].size == min(4 ** k, b.DUMP_BLOCKS)
    assert np.array_equal(a["counts_block_sums"], want.reshape(a["counts_block_sums"].size, -1).sum(1).astype(np.float64))
    assert np.array_equal(a["totals"], [want.sum(), np.count_nonzero(want)])
    assert all(np.array_equal(dumps[0][n], dumps[1][n]) for n in a)
