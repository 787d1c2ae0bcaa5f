"""The stage-2 estimate through the host layers: TranscodeOptions::estimate behind the C facade, the Python API and the
command-line tool's --estimate. Expected figures are tests/hist_model.py over the oracle's streams of the message points: per
field name and rung the order-0 entropy of stream - own + candidate, summed over the messages. The tool prints three decimals,
the facade 17 digits; sums of a few hundred doubles in another order agree to far better than the 1e-9 asked for here."""
import json
import os
import subprocess

import numpy as np
import pytest

import hist_model as H
import sweep_model as S
from cloudini_amd import api, synth
from cloudini_amd.schema import CompressionOption
from test_host_api import _cdr_pointcloud2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")

SWEEP_TEXT = "xyz:0.0005,0.001,0.005; intensity:0.05,1"
SWEEP = {"xyz": [0.0005, 0.001, 0.005], "intensity": [0.05, 1.0]}
SIZES = [40000, 20000, 1, 33000, 5000]


def test_libraries_export_the_estimate_entry_point():
    assert hasattr(api.lib(), "cldn_amd_transcode_directory_estimate")
    with pytest.raises(ValueError):
        api.transcode_directory("nowhere", "nowhere_either", estimate=True)


def _messages():
    clouds, msgs = [], []
    for k, n in enumerate(SIZES):
        info, data = synth.velodyne_xyzir(n, seed=80 + k)
        clouds.append((info, data.copy()))
        msgs.append(_cdr_pointcloud2(info, data, stamp=(1700000000 + k, k)))
    return clouds, msgs


def _write(folder, msgs):
    os.makedirs(folder, exist_ok=True)
    for k, m in enumerate(msgs):
        m.tofile(os.path.join(folder, f"msg_{k:05d}.bin"))


def _same_files(one, two):
    names = sorted(os.listdir(one))
    assert names == sorted(os.listdir(two)) and names
    for nm in names:
        assert open(os.path.join(one, nm), "rb").read() == open(os.path.join(two, nm), "rb").read(), nm


def _model(oracle, clouds):
    """({(field name, float32 resolution): bytes}, own bytes, stage-1 bytes)"""
    fields, own, stage1 = {}, 0.0, 0
    for info, data in clouds:
        n = data.size // info.point_step
        stream = oracle.encode_stage1(info, data)
        whole = H.bytes_hist(stream)
        own += H.entropy_bytes(whole)
        stage1 += stream.size
        kinds = S.field_kinds(info)
        ladders = np.zeros((len(info.fields), 4), dtype=np.float32)
        for f, field in enumerate(info.fields):
            rungs = SWEEP.get(field.name, SWEEP["xyz"] if field.name in "xyz" else [])
            ladders[f, :len(rungs)] = rungs
            ladders[f, 3] = 0.0 if kinds[f] == S.NONE or field.name not in ("x", "y", "z", "intensity") else field.resolution
        rep = H.sweep_hist(info, data, [n], ladders)[0]
        for f, field in enumerate(info.fields):
            for c, r in enumerate(ladders[f, :3]):
                if r == 0 or kinds[f] == S.NONE:
                    continue
                key = (field.name, float(r))
                fields[key] = fields.get(key, 0.0) + H.entropy_bytes(H.moved(whole, rep[f, 3], rep[f, c]))
    return fields, own, stage1


def _lines(stdout, tag):
    return [ln for ln in stdout.splitlines() if ln.startswith(tag + " ")]


def _close(got, want, printed):
    return abs(got - want) <= 1e-9 * abs(want) + (0.0006 if printed else 0.0)


@pytest.mark.gpu
def test_estimate_lines_of_the_tool_and_the_api_match_the_model(tmp_path, oracle):
    assert os.path.exists(EXE)
    clouds, msgs = _messages()
    src = str(tmp_path / "in")
    _write(src, msgs)
    want, own, stage1 = _model(oracle, clouds)
    assert len(want) == 3 * 3 + 2
    runs = {}
    for name, extra in (("plain", []), ("swept", ["--sweep", SWEEP_TEXT]), ("estimated", ["--sweep", SWEEP_TEXT, "--estimate"]),
                        ("none", ["--sweep", SWEEP_TEXT, "--estimate", "--compression", "none"])):
        r = subprocess.run([EXE, src, str(tmp_path / name), "--batch", "2"] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        runs[name] = r.stdout
    assert not _lines(runs["plain"], "estimate") and not _lines(runs["swept"], "estimate")
    # the sweep lines stay byte for byte, the messages too
    assert _lines(runs["swept"], "sweep") == _lines(runs["estimated"], "sweep") and len(_lines(runs["swept"], "sweep")) == 1 + len(want)
    _same_files(str(tmp_path / "plain"), str(tmp_path / "swept"))
    _same_files(str(tmp_path / "plain"), str(tmp_path / "estimated"))
    for name in ("estimated", "none"):
        rows = [ln.split() for ln in _lines(runs[name], "estimate")]
        assert rows[0][1:] == ["field", "resolution", "stage2_bytes"] and rows[-1][1:3] == ["own", "-"]
        got = {(r[1], float(np.float32(r[2]))): float(r[3]) for r in rows[1:-1]}
        assert set(got) == set(want)
        for key, w in want.items():
            assert _close(got[key], w, True), (name, key, got[key], w)
        last = rows[-1]
        assert _close(float(last[3]), own, True) and last[4] == "stage1_bytes" and int(last[5]) == stage1
        # a coarser rung is a smaller file, and moving one field alone to its own resolution changes nothing
        assert got[("x", float(np.float32(0.005)))] < got[("x", float(np.float32(0.001)))] < got[("x", float(np.float32(0.0005)))]
        assert _close(got[("x", float(np.float32(0.001)))], own, True)
        if name == "none":
            assert len(last) == 6                                     # no actual size without ZSTD
            continue
        assert last[6] == "actual_bytes" and last[8] == "estimate/actual"
        actual = int(last[7])
        assert abs(float(last[9]) - own / actual) < 1e-4
        # the actual size is the ZSTD output: both outputs carry the same wrapping but for up to 3 bytes of CDR padding each
        out_z, out_n = json.loads(runs["estimated"].splitlines()[-1])["output_bytes"], json.loads(runs["none"].splitlines()[-1])["output_bytes"]
        assert abs((out_n - stage1) - (out_z - actual)) <= 3 * len(msgs) and 0 < actual < stage1
    # the facade and the Python API
    st = api.transcode_directory(src, str(tmp_path / "api"), compression_opt=int(CompressionOption.ZSTD), batch_messages=2, sweep=SWEEP,
                                 estimate=True)
    _same_files(str(tmp_path / "plain"), str(tmp_path / "api"))
    est = st["estimate"]
    got = {(c["name"], float(np.float32(c["resolution"]))): c["bytes"] for c in est["fields"]}
    assert set(got) == set(want) and all(_close(got[k], w, False) for k, w in want.items())
    assert _close(est["own_bytes"], own, False) and est["stage1_bytes"] == stage1 and est["actual_bytes"] == actual
    plain = api.transcode_directory(src, str(tmp_path / "api2"), batch_messages=2, sweep=SWEEP)
    assert "estimate" not in plain and plain["sweep"] == st["sweep"]


def test_estimate_without_sweep_or_with_decode_exits_with_status_2(tmp_path):
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(src)
    for args in (["--estimate"], ["--estimate", "--decode"], ["--sweep", "x:0.1", "--estimate", "--decode"],
                 ["--estimate", "--audit"]):
        r = subprocess.run([EXE, src, dst] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.stdout, r.stderr)
        assert not os.path.exists(dst) or not os.listdir(dst)
    r = subprocess.run([EXE, src, dst, "--sweep", "x:0.1", "--estimate"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 2, r.stdout + r.stderr                        # well-formed: past the parser
