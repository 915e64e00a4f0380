"""bench.py's options without a GPU: a plain run is the default (--full off), and --dump-outputs writes float64 arrays whole,
or a fixed sample of them when they would pass the size cap."""
import os
import sys

import numpy as np

from helpers import ROOT

sys.path.insert(0, ROOT)
import bench                                             # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.steps == 5 and a.warmup == 2 and a.full is False and a.dump_outputs == ""
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_float64_exactly(tmp_path):
    hits = np.array([0, 1, 33688701, (1 << 53) - 1], dtype=np.int64)
    n = bench.dump_outputs(str(tmp_path / "o"), {"hits": hits})
    got = np.load(str(tmp_path / "o" / "hits.npy"))
    assert got.dtype == np.float64 and n == got.nbytes == 32
    assert np.array_equal(got.astype(np.int64), hits)


def test_dump_outputs_samples_past_the_cap_the_same_way_every_time(tmp_path):
    a = np.arange(1000, dtype=np.int64) * 3
    for d in ("x", "y"):
        n = bench.dump_outputs(str(tmp_path / d), {"hits": a}, cap=800)
        assert n == 800
    x, y = (np.load(str(tmp_path / d / "hits.npy")) for d in ("x", "y"))
    assert len(x) == 100 and np.array_equal(x, y)
    assert np.all(np.diff(x) > 0) and np.all(x % 3 == 0)          # ascending indices, values of the array
    assert bench.DUMP_CAP + 4096 < 64 * 10 ** 6
    assert os.listdir(str(tmp_path / "x")) == ["hits.npy"]
