"""CPU: what `bench.py --dump-outputs DIR` writes (bench.dump_outputs): a
float32 .npy per array, whole up to DUMP_MAX_ELEMENTS elements, above that
the elements at positions drawn once from a fixed seed, so two runs (and two
builds) write the same positions; and the plain / --full split of the command
line."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_small_array_is_written_whole(bench, tmp_path):
    torch = pytest.importorskip("torch")
    x = torch.arange(1000, dtype=torch.float32) * 0.5
    x[3] = float("inf")
    path = bench.dump_outputs(torch, str(tmp_path / "new" / "dir"), "dst_last", x)
    assert path == str(tmp_path / "new" / "dir" / "dst_last.npy")
    got = np.load(path)
    assert got.dtype == np.float32 and got.shape == (1000,)
    assert got.view(np.uint32).tolist() == x.numpy().view(np.uint32).tolist()


def test_large_array_is_sampled_at_fixed_positions(bench, tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMENTS", 4096)
    n = 100_003
    x = torch.arange(n, dtype=torch.float32)   # value = position (exact in fp32)
    a = np.load(bench.dump_outputs(torch, str(tmp_path / "a"), "dst_last", x))
    b = np.load(bench.dump_outputs(torch, str(tmp_path / "b"), "dst_last", x))
    assert a.dtype == np.float32 and a.shape == (4096,)
    assert (a == b).all()
    want = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).integers(0, n, 4096))
    assert (a == want.astype(np.float32)).all()
    assert a.min() < n // 10 and a.max() > n - n // 10   # spread over the whole chunk


def test_finite_input_lanes_leave_out_exactly_the_inf_seeded_ones(bench):
    """Inputs laid out as bench.py lays them out (on the CPU): the lanes kept
    are those where dst and src are both finite, so dst + k * src is too."""
    torch = pytest.importorskip("torch")
    n = 100_003
    d, s = torch.rand(n) * 2 - 1, torch.rand(n) * 2 - 1
    specials = torch.tensor(bench.SPECIALS)
    for t, off in zip((d, s), bench.SPECIAL_OFFSETS):
        idx = torch.arange(off, n, bench.SPECIAL_EVERY)
        t[idx] = specials[torch.arange(idx.numel()) % specials.numel()]
    lanes = bench.finite_input_lanes(n)
    want = np.nonzero((torch.isfinite(d) & torch.isfinite(s)).numpy())[0]
    assert np.array_equal(lanes, want)
    assert 0 < n - len(lanes) < n // 100          # a fraction of the 1 % special lanes
    # zeros and denormals stay in
    assert bench.SPECIAL_EVERY * 2 in lanes and bench.SPECIAL_OFFSETS[1] in lanes
    assert np.isfinite((d + 5 * s).numpy()[lanes]).all()


def test_only_the_given_lanes_are_written(bench, tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    x = torch.arange(1000, dtype=torch.float32)
    lanes = np.array([i for i in range(1000) if i % 7])
    got = np.load(bench.dump_outputs(torch, str(tmp_path / "w"), "dst_last", x, lanes))
    assert np.array_equal(got, lanes.astype(np.float32))
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMENTS", 64)
    got = np.load(bench.dump_outputs(torch, str(tmp_path / "s"), "dst_last", x, lanes))
    assert got.shape == (64,) and (got % 7 != 0).all() and (np.diff(got) >= 0).all()


def test_dump_stays_within_64_mb(bench):
    # one array per run, float32, plus the .npy header
    assert bench.DUMP_MAX_ELEMENTS * 4 + 4096 <= 64 * 1000 * 1000


def test_full_and_dump_outputs_are_off_by_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
