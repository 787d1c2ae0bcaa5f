"""`cloudini_batch_transcode in.mcap out.mcap --mcap-device-zstd`: the container's ZSTD chunks stitched from the GPU's blocks
(TranscodeOptions::mcap_device_zstd).

One bag -- six clouds of 5000 points in two schemas, an empty cloud, three messages of another topic between them -- goes
through the tool without the option, with it, and with --device-zstd-matches on top. Read back with libzstd
(tests/test_mcap_stitched.py's reader, which checks every non-zero chunk CRC) the three outputs hold the same messages, one by
one in file order; the option changes chunk boundaries and nothing else. Decoded again they give the same PointCloud2 bytes."""
import json
import os
import subprocess

import numpy as np
import pytest

import mcap_py
from cloudini_amd import synth
from test_host_api import _cdr_pointcloud2
from test_mcap_stitched import read_checked

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")


def _bag(path):
    clouds = []
    for k in range(3):
        info, data = synth.lidar_xyzi(5000, seed=20 + k)
        clouds.append((1, _cdr_pointcloud2(info, data, stamp=(1700000000 + k, 1000 * k))))
        info, data = synth.depthcam_xyzrgba(100, 50, seed=30 + k)
        clouds.append((3, _cdr_pointcloud2(info, data, frame_id="camera")))
    info, data = synth.lidar_xyzi(0, seed=9)
    clouds.insert(4, (1, _cdr_pointcloud2(info, data)))
    pc2 = "sensor_msgs/msg/PointCloud2"
    schemas = [(1, pc2, "ros2msg", b"as recorded"), (2, "std_msgs/msg/String", "ros2msg", b"string data")]
    channels = [(1, 1, "/lidar", "cdr", []), (2, 2, "/chatter", "cdr", []), (3, 1, "/camera", "cdr", [])]
    msgs, t = [], 1000
    for k, (ch, c) in enumerate(clouds):
        if k in (1, 3, 6):
            msgs.append((2, 100 + k, t, t, b"between %d" % k))
            t += 5
        msgs.append((ch, k, t, t - 1, c.tobytes()))
        t += 5
    mcap_py.write(path, "ros2", schemas, channels, msgs, chunk_messages=3)
    return msgs


def _run(args):
    r = subprocess.run([TOOL] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_option_changes_chunk_boundaries_and_nothing_else(tmp_path):
    src = str(tmp_path / "in.mcap")
    msgs = _bag(src)
    assert len(msgs) == 10 and sum(1 for m in msgs if m[0] == 2) == 3
    plain, flagged, matched = (str(tmp_path / n) for n in ("plain.mcap", "flagged.mcap", "matched.mcap"))
    s0 = _run([src, plain, "--batch", "4"])
    s1 = _run([src, flagged, "--batch", "4", "--mcap-device-zstd"])
    s2 = _run([src, matched, "--batch", "4", "--mcap-device-zstd", "--device-zstd-matches"])
    m0, c0, _ = read_checked(plain)
    assert [(m[0], m[1], m[2], m[3]) for m in m0] == [(m[0], m[1], m[2], m[3]) for m in msgs]
    assert all(crc == 0 and comp == "zstd" for crc, comp, _r in c0)
    assert (s0["mcap_device_chunks"], s0["mcap_device_messages"], s0["mcap_host_fallback_messages"]) == (0, 0, 0)
    for out, st in ((flagged, s1), (matched, s2)):
        m, chunks, index = read_checked(out)                       # (asserts every non-zero CRC against the decompressed records)
        assert len(m) == len(m0)
        for a, b in zip(m, m0):
            assert a[:4] == b[:4] and a[4] == b[4], (out, a[:4])
        # the split: six clouds through stitched chunks, the empty one on the ordinary path; the other topic is not counted
        assert (st["mcap_device_messages"], st["mcap_host_fallback_messages"]) == (6, 1), st
        assert st["mcap_device_chunks"] == sum(1 for crc, _c, _r in chunks if crc) > 0
        assert (st["messages"], st["converted"]) == (10, 7)
        assert all(comp == "zstd" for _crc, comp, _r in chunks)
        # every cloud with points lies in a chunk with a CRC, everything else in chunks without
        for crc, _comp, recs in chunks:
            i, sizes = 0, []
            while i < len(recs):
                op, n = recs[i], int.from_bytes(recs[i + 1:i + 9], "little")
                if op == mcap_py.MESSAGE:
                    sizes.append((int.from_bytes(recs[i + 9:i + 11], "little"), n))
                i += 9 + n
            if crc:
                assert sizes and all(ch in (1, 3) and n > 2000 for ch, n in sizes), sizes
            else:
                assert all(ch == 2 or n < 2000 for ch, n in sizes), sizes
        for k, ch, entries in index:
            for lt, o in entries:
                assert chunks[k][2][o] == mcap_py.MESSAGE
    # and back: the decoder reads the flagged bags like the plain one
    outs = []
    for k, enc in enumerate((plain, flagged, matched)):
        dec = str(tmp_path / f"dec{k}.mcap")
        _run([enc, dec, "--decode", "--mcap-compression", "none"])
        outs.append(mcap_py.read(dec)["messages"])
    assert outs[0] == outs[1] == outs[2] and len(outs[0]) == 10
    # the C++ readers take the flagged bags too (McapFile and McapStream check the CRCs)
    for enc in (flagged, matched):
        again = str(tmp_path / "again.mcap")
        _run([enc, again, "--decode", "--mcap-compression", "zstd"])


def test_a_message_with_a_refused_frame_takes_the_ordinary_path(tmp_path):
    """The device writer makes no frame that zstd_stitch.hpp refuses, so TranscodeOptions::test_refuse_stitch names them
    (tests/cpp/mcap_refuse_stitch.cpp): the first and only chunk of one cloud, the second of three chunks of another (the
    chunks collected so far are given up), the last chunk of a third. Those messages are expanded on the host and written as
    the default path writes them; the file holds the same messages as a run without the option."""
    from test_mcap_stitched import _build
    exe = _build(tmp_path, "mcap_refuse_stitch")
    msgs, t = [], 1000
    for k, n in enumerate([5000, 70000, 3000, 40000, 0, 2000]):
        info, data = synth.lidar_xyzi(n, seed=50 + k)
        msgs.append((1, k, t, t, _cdr_pointcloud2(info, data).tobytes()))
        t += 5
    src, plain, out = (str(tmp_path / n) for n in ("in.mcap", "plain.mcap", "refused.mcap"))
    mcap_py.write(src, "ros2", [(1, "sensor_msgs/msg/PointCloud2", "ros2msg", b"")], [(1, 1, "/lidar", "cdr", [])], msgs, chunk_messages=2)
    _run([src, plain, "--batch", "4"])
    r = subprocess.run([exe, src, out, "0:0", "1:1", "3:1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    chunks_n, device, fallback = map(int, r.stdout.split())
    assert (device, fallback) == (2, 4) and chunks_n > 0                  # clouds 2 and 5 stitched; 0, 1, 3 refused, 4 empty
    m0, _c0, _ = read_checked(plain)
    m1, c1, _ = read_checked(out)
    assert len(m1) == len(m0) == 6
    for a, b in zip(m1, m0):
        assert a[:4] == b[:4] and a[4] == b[4], a[:4]
    assert chunks_n == sum(1 for crc, _c, _r in c1 if crc)
    r = subprocess.run([exe, src, out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and list(map(int, r.stdout.split()))[1:] == [5, 1], r.stdout
