"""bench.py's own options without a GPU: what --dump-outputs writes, and --steps below 1 refused before anything starts."""
import os
import subprocess
import sys

import numpy as np

from helpers import ROOT


def test_dump_outputs_writes_exact_words_and_a_fixed_sample(tmp_path):
    import bench
    res = np.random.default_rng(5).integers(0, 2**32, (100, 7), dtype=np.uint64).astype(np.uint32)
    bench.dump_outputs(str(tmp_path / "all"), "nand", res)
    got = np.load(tmp_path / "all" / "nand.npy")
    assert got.dtype == np.float64 and np.array_equal(got, res.astype(np.float64))
    assert not (tmp_path / "all" / "nand_rows.npy").exists()
    # beyond the budget: the same rows on every run, their indices beside them, words and indices within the budget together
    budget = 20 * (7 * 8 + 8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "nand", res, budget=budget)
    words, rows = np.load(tmp_path / "a" / "nand.npy"), np.load(tmp_path / "a" / "nand_rows.npy")
    assert words.shape == (20, 7) and words.nbytes + rows.nbytes <= budget
    assert np.array_equal(rows, np.unique(rows)) and len(rows) == 20
    assert np.array_equal(words, res[rows.astype(np.int64)].astype(np.float64))
    assert np.array_equal(words, np.load(tmp_path / "b" / "nand.npy")) and np.array_equal(rows, np.load(tmp_path / "b" / "nand_rows.npy"))


def test_steps_below_one_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and '"metric"' not in r.stdout
