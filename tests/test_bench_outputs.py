"""bench.py's plain run, --full and --dump-outputs.

The sample rule (bench.dump_sample) is checked on CPU; one small run of the
bench in this process on the GPU checks that a plain run carries the headline
fields and none of the --full legs, that --steps sets the number of timed
launches, and that the dumped files hold the parity the oracle computes for
the seeded stripes.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_sample_is_fixed_bounded_and_keeps_the_edges():
    # the headline shape: 256 stripes x 4 parity vectors of 1 MiB
    r, c = bench.dump_sample(1024, 1 << 20)
    r2, c2 = bench.dump_sample(1024, 1 << 20)
    assert np.array_equal(r, r2) and np.array_equal(c, c2)  # the same bytes every run
    assert np.array_equal(r, np.arange(1024))  # every vector of every stripe
    assert len(r) * len(c) <= bench.DUMP_ELEMS and len(r) * len(c) * 4 + 1024 * 8 <= 64e6  # sample + row sums
    assert len(c) > bench.DUMP_ELEMS // 1024 - 130  # the budget is used (edges may coincide with picks)
    assert np.all(np.diff(c) > 0) and c[0] == 0 and c[-1] == (1 << 20) - 1
    assert set(range(64)) <= set(c.tolist()) and set(range((1 << 20) - 64, 1 << 20)) <= set(c.tolist())
    # many small vectors (10+4 @ 8 KiB x 32768 stripes): vectors are sampled too
    r, c = bench.dump_sample(4 * 32768, 8192)
    assert len(r) <= bench.DUMP_ROWS and r[0] == 0 and r[-1] == 4 * 32768 - 1 and np.all(np.diff(r) > 0)
    assert len(r) * len(c) <= bench.DUMP_ELEMS and c[0] == 0 and c[-1] == 8191
    # an output that fits is written whole
    r, c = bench.dump_sample(12, 1000)
    assert np.array_equal(r, np.arange(12)) and np.array_equal(c, np.arange(1000))


def test_plain_run_is_the_default_and_steps_are_checked():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    a = bench.parse_args(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_parity(rslib, orc, tmp_path, capsys, monkeypatch):
    import torch

    S, steps, warmup = 3, 3, 2
    launches = []
    real = rslib.RS.encode_batch_split
    monkeypatch.setattr(rslib.RS, "encode_batch_split",
                        lambda self, *a, **kw: (launches.append(1), real(self, *a, **kw))[1])
    monkeypatch.setattr(bench, "time", _marking_clock(launches))  # bench's own view of the clock only
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "RSAMD_BENCH_DEVICE", "RSAMD_BENCH_LAYOUT"):
        monkeypatch.delenv(var, raising=False)
    out = tmp_path / "dump"
    line = bench.main(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--stripes", str(S),
                       "--prewarm-min", "1", "--prewarm-max", "8", "--dump-outputs", str(out)])
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(printed) == 1 and json.loads(printed[0]) == json.loads(json.dumps(line))

    # the headline fields, and none of the --full legs
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["metric"] == bench.metric_name(10, 4, 1 << 20)
    assert line["steps"] == steps and line["warmup"] == warmup and line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (ms_per_step is rounded to 1e-4 ms, and a
    # launch of this small batch costs the host well over 5e-3 ms: within 2 %)
    assert line["value"] == pytest.approx(S * 14 * (1 << 20) / (line["ms_per_step"] / 1e3) / 2 ** 30, rel=0.02)
    assert line["full"] is False
    assert all(line[key] is None for key in ("cold", "end_to_end", "cpu_baseline", "timed_spread"))
    # --steps is the number of launches between the clock's two readings; nothing runs behind them
    assert _marking_clock.marks[-1] - _marking_clock.marks[-2] == steps
    assert len(launches) == _marking_clock.marks[-1] == line["prewarm"]["launches"] + warmup + steps

    # the dumped files: the oracle's parity of the same seeded stripes
    sample = np.load(out / "parity_sample.npy")
    rowsum = np.load(out / "parity_rowsum.npy")
    assert sample.dtype == np.float32 and rowsum.dtype == np.float64
    assert sample.nbytes + rowsum.nbytes <= 64e6
    assert line["outputs"]["files"] == {"parity_sample": ["float32", list(sample.shape)],
                                        "parity_rowsum": ["float64", [S, 4]]}
    g = torch.Generator(device="cuda:0").manual_seed(0x5EED)
    data = torch.empty((S, 10, 1 << 20), dtype=torch.uint8, device="cuda:0")
    data.random_(0, 256, generator=g)  # S <= 32: one draw, as the bench fills its first 32 stripes
    exp = orc.encode_numpy(orc.gen_matrix(10, 4).reshape(4, 10), data.cpu().numpy())
    r, c = bench.dump_sample(S * 4, 1 << 20)
    assert np.array_equal(sample, exp.reshape(S * 4, -1)[r][:, c].astype(np.float32))
    assert np.array_equal(rowsum, exp.sum(axis=2, dtype=np.int64).astype(np.float64))


def _marking_clock(launches):
    """A stand-in for bench's `time` module whose perf_counter also notes how
    many launches had been made at each reading (the timed region reads it
    right before and right after its steps, and a plain run reads it nowhere
    later)."""
    import time
    import types

    _marking_clock.marks = marks = []

    def clock():
        marks.append(len(launches))
        return time.perf_counter()

    return types.SimpleNamespace(perf_counter=clock, sleep=time.sleep)
