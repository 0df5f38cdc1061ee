"""bench.py --dump-outputs on the CPU: u64 torus words become float64 values in [-0.5, 0.5), a larger output is cut to a
fixed, seeded sample of rows under the size cap, and the same call writes the same file."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("spf_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_torus_values_and_seeded_sample(tmp_path):
    bench = _bench()
    words = np.random.default_rng(3).integers(0, 1 << 64, size=(bench.DUMP_ROWS + 300, 64), dtype=np.uint64)
    t = torch.from_numpy(words.view(np.int64))
    bench._dump_outputs(str(tmp_path / "a"), {"glwe_out": t})
    bench._dump_outputs(str(tmp_path / "b"), {"glwe_out": t})
    a = np.load(tmp_path / "a" / "glwe_out.npy")
    assert a.dtype == np.float64 and a.shape == (bench.DUMP_ROWS, 64)
    assert np.array_equal(a, np.load(tmp_path / "b" / "glwe_out.npy"))
    assert np.all(a >= -0.5) and np.all(a < 0.5)
    # every sampled row is one of the input rows, in input order, converted word by word
    full = words.view(np.int64).astype(np.float64) * 2.0 ** -64
    idx = [int(np.flatnonzero((full == row).all(axis=1))[0]) for row in a]
    assert idx == sorted(set(idx))


def test_dump_outputs_small_output_whole_and_split_under_the_cap(tmp_path):
    bench = _bench()
    words = (np.arange(10 * 8, dtype=np.uint64).reshape(10, 8) << np.uint64(50))
    words[0, :4] = [0, 1 << 63, (1 << 64) - 1, 1 << 62]
    bench._dump_outputs(str(tmp_path), {"glwe_out": torch.from_numpy(words.view(np.int64))})
    got = np.load(tmp_path / "glwe_out.npy")
    assert np.array_equal(got, words.view(np.int64).astype(np.float64) * 2.0 ** -64)
    assert list(got[0, :4]) == [0.0, -0.5, -(2.0 ** -64), 0.25]
    big = torch.zeros((bench.DUMP_ROWS, 4), dtype=torch.int64)
    bench._dump_outputs(str(tmp_path / "m"), {"m0": big, "m1": big})
    assert [np.load(tmp_path / "m" / f"m{i}.npy").shape[0] for i in (0, 1)] == [bench.DUMP_ROWS // 2] * 2
