"""bench.py's launch contract: `--gpus N` means N RCCL ranks, one per GPU -- never a silent
single rank. CPU part: the refusals. GPU part: one rank directly and under torch.distributed.run; both shard
schemes on two ranks when the box has two GPUs."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
SMALL = ["--steps", "2", "--warmup", "1", "--repeats", "2", "--cpu-baseline-seconds", "0", "--e2e-seconds", "0"]


def run(args, env_extra=None, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)


def json_line(stdout):
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout
    return json.loads(lines[0])


def gpu_count():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


@pytest.mark.skipif(gpu_count() >= 2, reason="needs a box with fewer than 2 GPUs")
def test_more_gpus_than_the_box_has_is_refused():
    r = run(["--gpus", "2"] + SMALL)
    assert r.returncode != 0
    assert "refusing" in r.stderr and "{" not in r.stdout


def test_world_size_must_match_gpus():
    # a launcher that started one rank for a two-GPU request: no line, non-zero exit
    r = run(["--gpus", "2"] + SMALL, {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1", "MASTER_ADDR": "127.0.0.1",
                                       "MASTER_PORT": "29999"})
    assert r.returncode != 0
    assert "WORLD_SIZE=1" in (r.stderr + r.stdout) and "\"n_gpus\"" not in r.stdout


def test_chunk_shard_needs_one_cloud():
    r = run(["--shard", "chunks", "--clouds", "2"] + SMALL)
    assert r.returncode != 0 and "--clouds 1" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_single_rank_line():
    r = run(["--gpus", "1", "--clouds", "2", "--points", "100000", "--full"] + SMALL)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json_line(r.stdout)
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["steps"] == 2 and d["warmup"] == 1
    assert d["repeats"]["blocks"] == 2 and d["value"] > 0
    assert d["roofline"]["frac"] > 0 and d["decode"]["value"] > 0
    assert d["bit_exact"] is True


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_dumps_the_last_step(tmp_path):
    """Without --full: the headline alone; --dump-outputs writes what the timed call handed back, here the whole streams
    (they are shorter than the sample), which must be the oracle's streams of the workload's seeded clouds."""
    import zlib

    import numpy as np
    from cloudini_amd import synth
    from oracle.binding import Oracle

    r = run(["--gpus", "1", "--clouds", "2", "--points", "100000", "--steps", "3", "--warmup", "1",
             "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    d = json_line(r.stdout)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["unit"] == "Mpoints/s" and d["metric"] and d["dtype"]
    assert not {"repeats", "roofline", "decode", "bit_exact", "cpu_baseline", "e2e", "transcode", "configs"} & set(d)
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == {"stream_offsets", "chunk_sizes", "modes", "stream_crc32", "stream_sample", "stream_sample_index"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64_000_000
    info, c0 = synth.lidar_xyzi(100000, seed=42)
    _info, c1 = synth.lidar_xyzi(100000, seed=43)
    streams = [Oracle().encode_stage1(info, c) for c in (c0, c1)]
    want = np.concatenate(streams)
    assert np.array_equal(got["stream_offsets"], [0, streams[0].size, want.size]) and want.size == d["job_stage1_bytes"]
    assert np.array_equal(got["stream_crc32"], [zlib.crc32(s) for s in streams])
    assert np.array_equal(got["stream_sample_index"], np.arange(want.size))
    assert np.array_equal(got["stream_sample"], want.astype(np.float32))


@pytest.mark.gpu
def test_single_rank_under_the_launcher_takes_the_rccl_path():
    env = dict(os.environ)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", "29517", BENCH, "--gpus", "1", "--clouds", "2", "--points", "100000"] + SMALL
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json_line(r.stdout)["n_gpus"] == 1


@pytest.mark.gpu
def test_single_rank_chunk_shard_runs_the_exchange_protocol():
    r = run(["--gpus", "1", "--workload", "c2", "--shard", "chunks", "--points", "200000"] + SMALL)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json_line(r.stdout)
    assert d["scaling"] == "strong" and d["config"]["shard"] == "chunks" and d["n_gpus"] == 1


@pytest.mark.gpu
@pytest.mark.skipif(gpu_count() < 2, reason="needs two GPUs")
@pytest.mark.parametrize("shard", ["clouds", "chunks"])
def test_two_ranks(shard):
    extra = ["--clouds", "4", "--points", "200000"] if shard == "clouds" else ["--workload", "c2", "--shard", "chunks",
                                                                               "--points", "400000"]
    r = run(["--gpus", "2"] + extra + SMALL, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json_line(r.stdout)
    assert d["n_gpus"] == 2
    one = json_line(run(["--gpus", "1"] + extra + SMALL).stdout)
    if shard == "clouds":  # weak scaling: twice the clouds, twice the bytes
        assert d["job_stage1_bytes"] == 2 * one["job_stage1_bytes"]
    else:                  # strong scaling: the same cloud, the same stream size whatever the cut
        assert d["job_stage1_bytes"] == one["job_stage1_bytes"]
