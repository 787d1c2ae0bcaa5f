"""TranscodeOptions::device_zstd_matches through the command-line tool: with --compression zstd --device-zstd
--device-zstd-matches the GPU stage writes ZSTD frames whose blocks may hold sequences (cloudini_amd/csrc/zstd_seq_kernels.hip).
The compiled reference decodes each message to what the plain run's message decodes to; on the DDS layout (a ring field and
a lossless float64 stamp) the messages are smaller than the literal-only ones. The flag is refused where it has no meaning."""
import json
import os
import subprocess

import numpy as np
import pytest

import cases
from test_host_api import _cdr_pointcloud2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
SIZES = [40000, 9000, 1, 0, 33000]


def _messages():
    msgs = []
    for k, n in enumerate(SIZES):
        info, data = cases.ouster_like(n=max(n, 5000), seed=60 + k)                  # (its special stamps sit below point 4064)
        msgs.append(_cdr_pointcloud2(info.copy(width=n, height=1), data[:n * info.point_step], stamp=(1700000000 + k, k)))
    return msgs


def _run(src, dst, *args):
    r = subprocess.run([EXE, src, dst, "--batch", "4", *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _files(folder):
    return {nm: np.fromfile(os.path.join(folder, nm), dtype=np.uint8) for nm in sorted(os.listdir(folder))}


def test_messages_with_matches_decode_to_what_the_plain_run_decodes_to(tmp_path, reflib):
    assert os.path.exists(EXE)
    src = str(tmp_path / "in")
    os.makedirs(src)
    for k, m in enumerate(_messages()):
        m.tofile(os.path.join(src, f"msg_{k:05d}.bin"))
    st_plain = _run(src, str(tmp_path / "plain"), "--compression", "zstd")
    st_lit = _run(src, str(tmp_path / "lit"), "--compression", "zstd", "--device-zstd")
    st_seq = _run(src, str(tmp_path / "seq"), "--compression", "zstd", "--device-zstd", "--device-zstd-matches")
    plain, lit, seq = (_files(str(tmp_path / d)) for d in ("plain", "lit", "seq"))
    assert list(plain) == list(lit) == list(seq) and len(plain) == len(SIZES)
    for (nm, a), n in zip(plain.items(), SIZES):
        cap = n * 26 + 4096
        want = reflib.ros_decompress(a, cap)
        assert np.array_equal(reflib.ros_decompress(seq[nm], cap), want), nm
        assert np.array_equal(reflib.ros_decompress(lit[nm], cap), want), nm
        assert seq[nm].size <= lit[nm].size, nm
    assert st_seq["messages"] == st_plain["messages"] == len(SIZES) and st_seq["points"] == st_plain["points"] == sum(SIZES)
    print(f"output bytes: libzstd {st_plain['output_bytes']}, literal-only {st_lit['output_bytes']}, with matches {st_seq['output_bytes']}")
    # the flag reached the writer: the frames differ and are smaller (how much depends on the data: the synthetic stamps repeat
    # little; DESIGN.md 4j has the sample slice's figures)
    assert st_seq["output_bytes"] < st_lit["output_bytes"]


def test_other_compressions_ignore_the_flag(tmp_path):
    src = str(tmp_path / "in")
    os.makedirs(src)
    for k, m in enumerate(_messages()[:2]):
        m.tofile(os.path.join(src, f"msg_{k:05d}.bin"))
    _run(src, str(tmp_path / "plain"), "--compression", "lz4")
    _run(src, str(tmp_path / "flag"), "--compression", "lz4", "--device-zstd", "--device-zstd-matches")
    plain, flag = _files(str(tmp_path / "plain")), _files(str(tmp_path / "flag"))
    assert list(plain) == list(flag) and len(plain) == 2
    for nm in plain:
        assert np.array_equal(plain[nm], flag[nm]), nm


def test_the_flag_is_refused_without_device_zstd_and_with_decode(tmp_path):
    os.makedirs(tmp_path / "in")
    r = subprocess.run([EXE, str(tmp_path / "in"), str(tmp_path / "out"), "--compression", "zstd", "--device-zstd-matches"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--device-zstd-matches needs --device-zstd" in r.stderr
    r = subprocess.run([EXE, str(tmp_path / "in"), str(tmp_path / "out"), "--decode", "--device-zstd-matches"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "--device-zstd-matches is not available with --decode" in r.stderr
