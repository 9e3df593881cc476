"""bench.py's command line and its --dump-outputs writer, without a GPU: --full is off by default,
and the writer stores the whole float64 vector when it fits the budget and a fixed, seeded sample
with its positions when it does not."""
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _Ctx:
    def __init__(self, x):
        self.x = x

    def from_device(self, ptr, n):
        assert n == len(self.x)
        return self.x.copy()


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _args(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.dump_outputs, a.steps, a.warmup, a.config) == (False, None, 7, 2, "c2")
    a = _args(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(monkeypatch, tmp_path):
    x = np.random.default_rng(0).uniform(-1, 1, 1000)
    info = {"iterations": 100, "final_norm": 0.25, "initial_norm": 4.0}
    a = _args(monkeypatch, "--dump-outputs", str(tmp_path / "whole"))
    bench.dump_outputs(a, _Ctx(x), 0, len(x), info)
    got = np.load(tmp_path / "whole" / "x.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x)
    assert np.array_equal(np.load(tmp_path / "whole" / "solve_info.npy"), [100.0, 0.25, 4.0])
    assert sorted(os.listdir(tmp_path / "whole")) == ["solve_info.npy", "x.npy"]
    # over the budget: the same sorted positions on every call, values taken at them
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8 * 200)
    out = []
    for d in ("s1", "s2"):
        a = _args(monkeypatch, "--dump-outputs", str(tmp_path / d))
        bench.dump_outputs(a, _Ctx(x), 0, len(x), info)
        out.append((np.load(tmp_path / d / "x_index.npy"), np.load(tmp_path / d / "x.npy")))
    idx, xs = out[0]
    assert np.array_equal(idx, out[1][0]) and np.array_equal(xs, out[1][1])
    assert 0 < len(idx) <= 100 and (np.diff(idx) > 0).all() and idx.dtype == np.float64
    assert np.array_equal(xs, x[idx.astype(np.int64)])
    # two ranks share the budget and name their files by rank
    bench.dump_outputs(a, _Ctx(x), 0, len(x), info, rank=1, world=2)
    assert len(np.load(tmp_path / "s2" / "x_rank1.npy")) <= 50
