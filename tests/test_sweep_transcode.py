"""The resolution sweep through the host layers: TranscodeOptions::sweep behind the C facade, the Python API and the
command-line tool, and the tool's --profile. Expected summaries are tests/sweep_model.py on the message points (with --viz: on
the oracle's survivors), summed over the messages."""
import json
import os
import subprocess

import numpy as np
import pytest

import cases
import sweep_model as S
from cloudini_amd import api, synth
from cloudini_amd.schema import CompressionOption
from test_host_api import _cdr_pointcloud2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")

SWEEP_TEXT = "xyz:0.0005,0.001,0.002,0.005; intensity:0.05,0.1,1"
SWEEP = {"xyz": [0.0005, 0.001, 0.002, 0.005], "intensity": [0.05, 0.1, 1.0]}
SIZES = [130048, 20000, 40000, 1, 33000, 5000]


def test_libraries_export_the_sweep_entry_points():
    from cloudini_amd import native
    for name in ("cldn_hip_sweep_clouds", "cldn_hip_sweep_last_encode", "cldn_hip_sweep_last_encode_clouds"):
        assert hasattr(native.lib(), name), name
    assert hasattr(api.lib(), "cldn_amd_transcode_directory_sweep")
    for name in ("sweep_clouds_host", "sweep_clouds_device", "sweep_last_encode"):
        assert hasattr(native.Codec, name), name
    assert native.SWEEP_DTYPE == S.DTYPE and native.SWEEP_MAX_CANDIDATES == S.MAX_CANDIDATES


def _velodyne_messages(resolution=0.001):
    """Velodyne-like messages (x y z intensity float32, ring u16) of different sizes."""
    clouds, msgs = [], []
    for k, n in enumerate(SIZES):
        info, data = synth.velodyne_xyzir(n, seed=60 + k, res=resolution)
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


def _model_summary(clouds):
    """{(field name, float32 resolution): [bytes, points, n_class_diff, n_over_limit, max_abs_err]} over (info, points) pairs."""
    total = {}
    for info, data in clouds:
        n = data.size // info.point_step
        ladders = np.zeros((len(info.fields), 4), dtype=np.float32)
        for f, field in enumerate(info.fields):
            rungs = SWEEP.get(field.name, SWEEP["xyz"] if field.name in "xyz" else [])
            ladders[f, :len(rungs)] = rungs
        rep = S.sweep(info, data, [n], ladders)[0]
        for f, field in enumerate(info.fields):
            for c, r in enumerate(ladders[f]):
                if r == 0 or S.field_kinds(info)[f] == S.NONE:
                    continue
                t = total.setdefault((field.name, float(r)), [0, 0, 0, 0, 0.0])
                cell = rep[f, c]
                t[0] += int(cell["bytes"])
                t[1] += n
                t[2] += int(cell["n_class_diff"])
                t[3] += int(cell["n_over_limit"])
                t[4] = max(t[4], float(cell["max_abs_err"]))
    return total


def _table(stdout):
    """The tool's `sweep` lines as {(name, float32 resolution): [bytes, bytes per point, class_diff, over_limit, max_abs_err]}."""
    rows = [ln.split() for ln in stdout.splitlines() if ln.startswith("sweep ")]
    assert rows[0][1:] == ["field", "resolution", "bytes", "bytes/point", "class_diff", "over_limit", "max_abs_err"]
    return {(r[1], float(np.float32(r[2]))): [int(r[3]), float(r[4]), int(r[5]), int(r[6]), float(r[7])] for r in rows[1:]}


def _check_table(table, want):
    assert set(table) == set(want)
    for key, w in want.items():
        got = table[key]
        assert (got[0], got[2], got[3], got[4]) == (w[0], w[2], w[3], w[4]), (key, got, w)
        assert abs(got[1] - w[0] / w[1]) < 1e-4, (key, got, w)


@pytest.mark.gpu
def test_sweep_summary_of_the_tool_and_the_api_matches_the_model(tmp_path):
    assert os.path.exists(EXE)
    clouds, msgs = _velodyne_messages()
    src = str(tmp_path / "in")
    _write(src, msgs)
    want = _model_summary(clouds)
    assert len(want) == 3 * 4 + 3 and all(v[1] == sum(SIZES) for v in want.values())
    r0 = subprocess.run([EXE, src, str(tmp_path / "plain"), "--batch", "4"], capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0 and "sweep" not in r0.stdout, r0.stdout + r0.stderr
    r = subprocess.run([EXE, src, str(tmp_path / "swept"), "--batch", "4", "--sweep", SWEEP_TEXT], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert json.loads(lines[-1])["messages"] == len(msgs) and all(ln.startswith("sweep ") for ln in lines[:-1])
    _check_table(_table(r.stdout), want)
    _same_files(str(tmp_path / "plain"), str(tmp_path / "swept"))
    # the facade and the Python API: the same numbers as JSON, the same files
    st = api.transcode_directory(src, str(tmp_path / "api"), compression_opt=int(CompressionOption.ZSTD), batch_messages=4, sweep=SWEEP)
    _same_files(str(tmp_path / "plain"), str(tmp_path / "api"))
    got = {(c["name"], float(np.float32(c["resolution"]))): [c["bytes"], c["points"], c["n_class_diff"], c["n_over_limit"], c["max_abs_err"]]
           for c in st["sweep"]}
    assert got == want
    assert "sweep" not in api.transcode_directory(src, str(tmp_path / "api2"), batch_messages=4)
    # a rung given twice counts once; an own entry for x wins over "xyz"; a name no message has is ignored
    st = api.transcode_directory(src, str(tmp_path / "api3"), batch_messages=4,
                                 sweep={"xyz": [0.002, 0.002], "x": [0.005], "nothing": [1.0], "ring": [1.0]})
    got = {(c["name"], float(np.float32(c["resolution"]))): [c["bytes"], c["points"], c["n_class_diff"], c["n_over_limit"], c["max_abs_err"]]
           for c in st["sweep"]}
    assert len(st["sweep"]) == 3 and got == {k: want[k] for k in (("x", float(np.float32(0.005))), ("y", float(np.float32(0.002))),
                                                                  ("z", float(np.float32(0.002))))}
    # the audit and the sweep behind the same encode calls
    both = subprocess.run([EXE, src, str(tmp_path / "both"), "--batch", "4", "--audit", "--sweep", SWEEP_TEXT], capture_output=True,
                          text=True, timeout=600)
    assert both.returncode == 0, both.stdout + both.stderr
    _check_table(_table(both.stdout), want)
    assert len([ln for ln in both.stdout.splitlines() if ln.startswith("audit ")]) == 1 + 5
    _same_files(str(tmp_path / "plain"), str(tmp_path / "both"))


@pytest.mark.gpu
def test_with_viz_the_summary_is_the_model_over_the_oracle_survivors(tmp_path, oracle):
    clouds, msgs = _velodyne_messages(resolution=0.05)
    src = str(tmp_path / "in")
    _write(src, msgs)
    survivors = [(info, oracle.viz_preprocess(data, info.point_step, 0, 0.05)) for info, data in clouds]
    kept = sum(d.size // i.point_step for i, d in survivors)
    assert 0 < kept < sum(SIZES)
    want = _model_summary(survivors)
    r0 = subprocess.run([EXE, src, str(tmp_path / "plain"), "--batch", "4", "--viz", "--resolution", "0.05"], capture_output=True,
                        text=True, timeout=600)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r = subprocess.run([EXE, src, str(tmp_path / "swept"), "--batch", "4", "--viz", "--resolution", "0.05", "--sweep", SWEEP_TEXT],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    _check_table(_table(r.stdout), want)
    assert all(v[1] == kept for v in want.values())
    _same_files(str(tmp_path / "plain"), str(tmp_path / "swept"))


@pytest.mark.gpu
def test_profile_strings_reach_the_transcoder(tmp_path):
    info, data = cases.xyzi_struct_4133()                                  # x y z intensity, all FLOAT32
    src = str(tmp_path / "floats")
    _write(src, [_cdr_pointcloud2(info, data, stamp=(1700000000, 1)), _cdr_pointcloud2(info.copy(width=100), data[:16 * 100], stamp=(1700000001, 2))])
    a = subprocess.run([EXE, src, str(tmp_path / "res"), "--resolution", "0.002"], capture_output=True, text=True, timeout=600)
    b = subprocess.run([EXE, src, str(tmp_path / "prof"), "--profile", "x:0.002; y:0.002; z:0.002; intensity:0.002"],
                       capture_output=True, text=True, timeout=600)
    c = subprocess.run([EXE, src, str(tmp_path / "prof_xyz"), "--profile", " xyz : 0.002 ;intensity:0.002;"], capture_output=True,
                       text=True, timeout=600)
    d = subprocess.run([EXE, src, str(tmp_path / "default")], capture_output=True, text=True, timeout=600)
    assert a.returncode == b.returncode == c.returncode == d.returncode == 0, a.stderr + b.stderr + c.stderr + d.stderr
    _same_files(str(tmp_path / "res"), str(tmp_path / "prof"))
    _same_files(str(tmp_path / "res"), str(tmp_path / "prof_xyz"))
    name = sorted(os.listdir(src))[0]
    assert open(tmp_path / "res" / name, "rb").read() != open(tmp_path / "default" / name, "rb").read()
    # ring:remove drops the field from the written message
    clouds, msgs = _velodyne_messages()
    src2 = str(tmp_path / "velodyne")
    _write(src2, msgs[1:2])
    keep = subprocess.run([EXE, src2, str(tmp_path / "keep"), "--compression", "none"], capture_output=True, text=True, timeout=600)
    drop = subprocess.run([EXE, src2, str(tmp_path / "drop"), "--compression", "none", "--profile", "ring:remove"],
                          capture_output=True, text=True, timeout=600)
    assert keep.returncode == drop.returncode == 0, keep.stderr + drop.stderr
    kept_msg = open(tmp_path / "keep" / "msg_00000.bin", "rb").read()
    dropped_msg = open(tmp_path / "drop" / "msg_00000.bin", "rb").read()
    assert b"ring" in kept_msg and b"ring" not in dropped_msg and b"intensity" in dropped_msg
    assert len(dropped_msg) < len(kept_msg)


def test_malformed_option_strings_exit_with_status_2(tmp_path):
    """The tool refuses them before it touches a file or a device."""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(src)
    for flag, text in (("--profile", "x"), ("--profile", "x:"), ("--profile", ":0.1"), ("--profile", "x:0.1:2"),
                       ("--profile", "x:abc"), ("--profile", "x:-0.1"), ("--profile", "x:nan"), ("--profile", "x:0.1;;y:0.1"),
                       ("--profile", ""), ("--sweep", "x"), ("--sweep", "x:0.1,"), ("--sweep", "x:0.1,,0.2"), ("--sweep", "x:0"),
                       ("--sweep", "x:-1"), ("--sweep", "x:inf"), ("--sweep", "x:remove"), ("--sweep", ""),
                       ("--sweep", "x:" + ",".join(["0.1"] * 17))):
        r = subprocess.run([EXE, src, dst, flag, text], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (flag, text, r.stdout, r.stderr)
        assert not os.path.exists(dst) or not os.listdir(dst)
    r = subprocess.run([EXE, src, dst, "--decode", "--sweep", "x:0.1"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2, r.stdout + r.stderr
    r = subprocess.run([EXE, src, dst, "--sweep", "x:" + ",".join(["0.1"] * 16), "--profile", "x:0.5; y:remove"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 2, r.stdout + r.stderr                        # well-formed: past the parser
