"""bench.py's launcher and timing harness on the CPU (--stub: gloo, a trivial step instead of the encode).

`python bench.py --gpus N` without a torchrun environment must start N ranks itself (one process per GPU, before
the parent touches the GPU), each seeing RANK / LOCAL_RANK / WORLD_SIZE, and rank 0 must print one JSON line with
n_gpus = N (--gpus was parsed and ignored)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, env=None):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--steps", "3", "--warmup", "1",
           "--values", "4096", *extra]
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 3])
def test_bench_self_launches_n_ranks(n):
    d = _run("--gpus", str(n))
    assert d["n_gpus"] == n
    assert sorted(tuple(r[:3]) for r in d["ranks"]) == [(i, i, n) for i in range(n)]
    assert all(r[3] == "self" for r in d["ranks"])
    # one rendezvous on the loopback address, at the port torchrun's own store bound (not one picked beforehand)
    assert len({(r[4], r[5]) for r in d["ranks"]}) == 1 and d["ranks"][0][4] == "127.0.0.1"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0


def test_bench_single_rank():
    d = _run("--gpus", "1")
    assert d["n_gpus"] == 1 and d["ranks"][0][:4] == [0, 0, 1, "torchrun"]


def test_bench_programmatic_argv_reaches_ranks():
    """main(argv) launches its ranks with `argv`, not with the parent's sys.argv."""
    code = ("import sys; sys.argv = ['bench.py', '--steps', '999']; import bench; "
            "bench.main(['--stub', '--gpus', '2', '--steps', '2', '--warmup', '1', '--values', '4096'])")
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=240, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2


@pytest.mark.parametrize("n", [1, 2])
def test_bench_fails_loudly_on_oracle_mismatch(n):
    """a `*_matches_oracle` false in the line (a stitch or shard-offset bug on the driver's N-rank run) must
    end the run with rc != 0 after the line is printed, not only show up as a boolean in it."""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--stub", "--stub-mismatch", "--gpus", str(n), "--steps",
           "2", "--warmup", "1", "--values", "4096"]
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=e, cwd=ROOT)
    assert r.returncode != 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["stub_check"]["stream_matches_oracle"] is False
    assert "ORACLE CHECK FAILED" in r.stderr


def test_parity_failures_scan():
    sys.path.insert(0, ROOT)
    import bench
    line = {"a": {"gathered_stream_matches_oracle": True}, "c5_sharded": {"stitched_stream_matches_oracle": False},
            "legs": [{"x_matches_oracle": None}, {"y_matches_oracle": False}]}
    assert bench.parity_failures(line) == ["c5_sharded.stitched_stream_matches_oracle", "legs.1.y_matches_oracle"]


def test_launcher_lets_torchrun_pick_the_port():
    """the N > 1 launcher used to bind port 0, read the port, close it and pass it as --master-port, a
    window in which another job could take it. It now asks torchrun for a standalone rendezvous on 127.0.0.1."""
    sys.path.insert(0, ROOT)
    import bench
    cmd = bench.launcher_cmd(8, ["--gpus", "8"])
    assert "--standalone" in cmd and "--local-addr=127.0.0.1" in cmd and "--nproc-per-node=8" in cmd
    assert not any(a.startswith("--master-port") for a in cmd)
    assert cmd[-2:] == ["--gpus", "8"]


def test_dump_outputs_writes_last_step_as_float_npy(tmp_path):
    """--dump-outputs DIR: after the timed steps the last step's outputs are written as DIR/<name>.npy in float64, the
    same from run to run; --steps sets the number of timed steps (the stub counts its calls: warmup + steps)."""
    import numpy as np
    seen = []
    for run in ("a", "b"):
        out = tmp_path / run / "nested"
        d = _run("--gpus", "1", "--steps", "5", "--dump-outputs", str(out))
        assert d["steps"] == 5 and d["ms_per_step"] > 0
        assert sorted(os.listdir(out)) == ["stub_calls.npy", "stub_sum.npy"]
        arrs = {f: np.load(out / f) for f in sorted(os.listdir(out))}
        assert all(a.dtype == np.float64 for a in arrs.values())
        assert arrs["stub_sum.npy"].tolist() == [4096.0] and arrs["stub_calls.npy"].tolist() == [1.0 + 5.0]
        seen.append(arrs)
    assert all(np.array_equal(seen[0][f], seen[1][f]) for f in seen[0])


def test_dump_word_index_is_a_fixed_sample():
    """Streams up to DUMP_WORDS words are dumped whole; longer ones as one seeded word per stratum: ascending, in
    range, spread over the whole stream, the same on every call, and within the 64 MB budget as float64."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    assert np.array_equal(bench.dump_word_index(1000), np.arange(1000))
    assert np.array_equal(bench.dump_word_index(bench.DUMP_WORDS), np.arange(bench.DUMP_WORDS))
    for nwords in (bench.DUMP_WORDS + 1, 3 * bench.DUMP_WORDS + 17, 64 * bench.DUMP_WORDS):
        idx = bench.dump_word_index(nwords)
        assert idx.size == bench.DUMP_WORDS and idx.dtype == np.int64
        assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < nwords
        assert idx[-1] >= (nwords // bench.DUMP_WORDS) * (bench.DUMP_WORDS - 1)
        assert np.array_equal(idx, bench.dump_word_index(nwords))
    assert bench.DUMP_WORDS * 8 * 3 + 8 <= 64 * 1000 * 1000  # index + two 32-bit halves per word + bits


def test_multi_legs_needs_full():
    """The multi-GPU legs belong to --full: asking for them on a plain run is a usage error, not a silent no-op."""
    sys.path.insert(0, ROOT)
    import bench
    with pytest.raises(SystemExit):
        bench.parse(["--multi-legs"])
    assert bench.parse(["--multi-legs", "--full"]).full and not bench.parse([]).full
