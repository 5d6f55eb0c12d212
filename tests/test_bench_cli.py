"""bench.py's command line: what a plain run does (the headline's warm-up and timed steps, nothing else), what
``--dump-outputs`` writes, and -- on the GPU -- that the dumped counts are the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SMALL = ["--config", "C2", "--scale", "0.0005", "--tx-scale", "0.005"]     # 50 000 reads x 100 transcripts
LINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}


def test_dump_outputs_whole_and_sampled(tmp_path):
    """A vector within the budget is written whole; a larger one as a seeded sample of positions plus block sums that
    cover every element -- float64, within the budget, the same files for the same vector."""
    import bench
    rng = np.random.default_rng(3)
    small = rng.integers(0, 1000, 5000).astype(np.int64)
    bench.dump_outputs(str(tmp_path / "w"), small, budget=80000)
    assert os.listdir(str(tmp_path / "w")) == ["counts.npy"]
    got = np.load(str(tmp_path / "w" / "counts.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, small)

    big = rng.integers(0, 1 << 40, 300001).astype(np.int64)
    budget = 400000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big, budget=budget)
    names = sorted(os.listdir(str(tmp_path / "a")))
    assert names == ["counts_block_sums.npy", "counts_sample.npy"]
    data_bytes = 0
    for f in names:
        a, b = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert a.dtype == np.float64 and np.array_equal(a, b)
        data_bytes += a.nbytes
    assert data_bytes <= budget
    sums = np.load(str(tmp_path / "a" / "counts_block_sums.npy"))
    assert sums.sum() == float(big.sum())
    sample = np.load(str(tmp_path / "a" / "counts_sample.npy"))
    pos = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, big.size, size=budget * 3 // 4 // 8))
    assert np.array_equal(sample, big[pos].astype(np.float64))


def test_plain_run_times_the_steps_and_nothing_else(tmp_path, monkeypatch, capsys):
    """Without --full, bench.main() launches the headline plan warm-up + --steps times and nothing more, prints one line
    with the contract's keys (no oracle, CPU baseline, roofline or other configs), and --dump-outputs writes the counts of
    the last step; two runs with the same arguments dump the same counts.  Rehearsed with the oracle-backed stand-in
    engine of tests/oracle_engine.py through the one-job path (world of one, gloo)."""
    import bench
    from tests import oracle_engine

    launches = []

    class CountingPlan(oracle_engine.Plan):
        def launch(self, dtype):
            launches.append(dtype)
            super(CountingPlan, self).launch(dtype)

    class CountingEngine(oracle_engine.Engine):
        def plan(self, *a):
            return CountingPlan(self, *a)

    monkeypatch.setattr(bench, "ENGINE_OVERRIDE", CountingEngine)
    monkeypatch.setenv("PC_BENCH_BACKEND", "gloo")
    monkeypatch.setenv("PC_POOL_RESERVOIR_GB", "96")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    dumps = []
    for run in range(2):
        out_dir = str(tmp_path / ("run%d" % run))
        monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--one-job"] + SMALL +
                            ["--steps", "4", "--warmup", "2", "--dump-outputs", out_dir])
        del launches[:]
        bench.main()
        lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert LINE_KEYS <= set(d) and d["steps"] == 4 and d["warmup"] == 2
        assert d["metric"] == "mapped_reads_per_sec" and d["unit"] == "reads/s" and d["higher_is_better"] is True
        assert d["dtype"] == "int64" and d["ms_per_step"] > 0
        assert not {"cpu_baseline", "roofline", "configs", "scopes"} & set(d)
        assert len(launches) == 2 + 4
        assert os.listdir(out_dir) == ["counts.npy"]
        dumps.append(np.load(os.path.join(out_dir, "counts.npy")))
    assert dumps[0].dtype == np.float64 and dumps[0].sum() > 0 and np.array_equal(dumps[0], dumps[1])


@pytest.mark.gpu
def test_plain_bench_dumps_the_counts_of_the_timed_path(tmp_path):
    """``bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`` on the HIP engine: one line with the contract's keys,
    and DIR/counts.npy is bit for bit the oracle's count vector of the workload (every chain, every position)."""
    from oracle import oracle
    from plastid_amd import synth
    from plastid_amd.packing import concat_file_major
    import bench
    out_dir = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + SMALL + ["--steps", "3", "--warmup", "1",
                                                                                       "--dump-outputs", out_dir]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert proc.returncode == 0, proc.stderr.decode()[-3000:]
    lines = [ln for ln in proc.stdout.decode().splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert LINE_KEYS <= set(d) and d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "int64"
    got = np.load(os.path.join(out_dir, "counts.npy"))

    _g, tx, reads, mapping = synth.make_config("C2", scale=0.0005, tx_scale=0.005)
    p = tx.plan_arrays(rows=1)
    arrays, _ = oracle.count_segments(concat_file_major([reads]), bench.oracle_spec(oracle, mapping),
                                      p["tid"], p["start"], p["end"], p["strand"])
    idx, val = bench.sparse_expected(arrays, p, np.arange(len(p["tid"])), 1)
    want = np.zeros(int(p["out_elems"]), np.float64)
    want[idx] = val
    assert got.dtype == np.float64 and got.shape == want.shape and want.sum() > 0
    assert np.array_equal(got, want)
