"""TranscodeOptions::device_zstd through the command-line tool: with --compression zstd the GPU stage writes the ZSTD frames
(literal-only blocks, cloudini_amd/csrc/zstd_kernels.hip) and stage 2 passes them on. The messages are not the plain run's
bytes; the compiled reference decodes each to what the plain run's message decodes to. Other compressions ignore the flag."""
import json
import os
import subprocess

import numpy as np
import pytest

from cloudini_amd import synth
from test_host_api import _cdr_pointcloud2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
SIZES = [70000, 20000, 1, 33000, 0, 5000]


def _messages():
    msgs = []
    for k, n in enumerate(SIZES):
        info, data = synth.velodyne_xyzir(n, seed=80 + k)
        msgs.append(_cdr_pointcloud2(info, data, stamp=(1700000000 + k, k)))
    return msgs


def _run(src, dst, *args):
    r = subprocess.run([EXE, src, dst, "--batch", "4", *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout, json.loads(r.stdout.strip().splitlines()[-1])


def _files(folder):
    return {nm: np.fromfile(os.path.join(folder, nm), dtype=np.uint8) for nm in sorted(os.listdir(folder))}


def _own_line(stdout):
    """the `estimate own` line as {label: number}"""
    ln = next(x for x in stdout.splitlines() if x.startswith("estimate own")).split()
    return {"own": float(ln[3]), **{ln[i]: float(ln[i + 1]) for i in range(4, len(ln) - 1, 2)}}


def test_device_zstd_messages_decode_to_what_the_plain_run_decodes_to(tmp_path, reflib):
    assert os.path.exists(EXE)
    src = str(tmp_path / "in")
    os.makedirs(src)
    for k, m in enumerate(_messages()):
        m.tofile(os.path.join(src, f"msg_{k:05d}.bin"))
    sweep = ["--sweep", "xyz:0.001,0.002", "--estimate"]
    out_plain, st_plain = _run(src, str(tmp_path / "plain"), "--compression", "zstd", *sweep)
    out_dev, st_dev = _run(src, str(tmp_path / "dev"), "--compression", "zstd", "--device-zstd", *sweep)
    plain, dev = _files(str(tmp_path / "plain")), _files(str(tmp_path / "dev"))
    assert list(plain) == list(dev) and len(plain) == len(SIZES)
    differ = 0
    for (nm, a), n in zip(plain.items(), SIZES):
        b = dev[nm]
        differ += not np.array_equal(a, b)
        cap = n * 22 + 4096
        want = reflib.ros_decompress(a, cap)
        assert np.array_equal(reflib.ros_decompress(b, cap), want), nm
    assert differ >= 4                                                         # (every message with points: other bytes)
    assert st_dev["messages"] == st_plain["messages"] == len(SIZES) and st_dev["points"] == st_plain["points"] == sum(SIZES)
    # velodyne streams are tokens: the frames without matches are within a percent of libzstd's
    assert 0.98 < st_dev["output_bytes"] / st_plain["output_bytes"] < 1.02
    # the estimate's figures do not move (they are taken from the stage-1 streams); actual_bytes adds up what was written
    own_plain, own_dev = _own_line(out_plain), _own_line(out_dev)
    assert own_plain["own"] == own_dev["own"] and own_plain["stage1_bytes"] == own_dev["stage1_bytes"]
    assert own_dev["actual_bytes"] - own_plain["actual_bytes"] == st_dev["output_bytes"] - st_plain["output_bytes"]
    assert [x for x in out_plain.splitlines() if x.startswith("estimate ") and " own " not in x] == \
           [x for x in out_dev.splitlines() if x.startswith("estimate ") and " own " not in x]


@pytest.mark.parametrize("compression", ["none", "lz4"])
def test_other_compressions_ignore_the_flag(tmp_path, compression):
    src = str(tmp_path / "in")
    os.makedirs(src)
    for k, m in enumerate(_messages()[1:4]):
        m.tofile(os.path.join(src, f"msg_{k:05d}.bin"))
    _run(src, str(tmp_path / "plain"), "--compression", compression)
    _run(src, str(tmp_path / "flag"), "--compression", compression, "--device-zstd")
    plain, flag = _files(str(tmp_path / "plain")), _files(str(tmp_path / "flag"))
    assert list(plain) == list(flag) and len(plain) == 3
    for nm in plain:
        assert np.array_equal(plain[nm], flag[nm]), nm


def test_device_zstd_is_refused_with_decode(tmp_path):
    os.makedirs(tmp_path / "in")
    r = subprocess.run([EXE, str(tmp_path / "in"), str(tmp_path / "out"), "--decode", "--device-zstd"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 2 and "--device-zstd is not available with --decode" in r.stderr
