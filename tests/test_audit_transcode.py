"""The audit through the host layers: TranscodeOptions::audit behind the C facade, the Python API and the command-line tool.
Expected summaries are tests/audit_model.py on (message points, oracle round trip), summed over the messages."""
import json
import os
import subprocess

import numpy as np
import pytest

import audit_model as M
from cloudini_amd import api, synth
from cloudini_amd.schema import CompressionOption
from test_host_api import _cdr_pointcloud2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")


def test_libraries_export_the_audit_entry_points():
    from cloudini_amd import native
    for name in ("cldn_hip_audit_clouds", "cldn_hip_audit_streams", "cldn_hip_audit_last_encode"):
        assert hasattr(native.lib(), name), name
    assert hasattr(api.lib(), "cldn_amd_transcode_directory_audit")
    for name in ("audit_clouds_host", "audit_clouds_device", "audit_streams_host", "audit_streams_device", "audit_last_encode"):
        assert hasattr(native.Codec, name), name
    assert native.AUDIT_DTYPE == M.DTYPE


def _velodyne_messages(n_msgs=6, bad=None):
    """Velodyne-like messages (x y z intensity float32 at 1 mm, ring u16, 130 k points); `bad`: the message that carries one
    point 3.0e6 m out (3e9 ticks at 1 mm: beyond int32)."""
    clouds, msgs = [], []
    for k in range(n_msgs):
        info, data = synth.velodyne_xyzir(130048 if k % 2 == 0 else 20000, seed=40 + k)
        data = data.copy()
        if k == bad:
            data[77 * info.point_step + 4:77 * info.point_step + 8] = np.frombuffer(np.float32(3.0e6).tobytes(), np.uint8)
        clouds.append((info, data))
        msgs.append(_cdr_pointcloud2(info, data, stamp=(1700000000 + k, k)))
    return clouds, msgs


def _write(folder, msgs):
    os.makedirs(folder, exist_ok=True)
    for k, m in enumerate(msgs):
        m.tofile(os.path.join(folder, f"msg_{k:05d}.bin"))


def _model_summary(oracle, clouds):
    info0 = clouds[0][0]
    total = {f.name: dict(n_bitwise_diff=0, n_class_diff=0, n_over_limit=0, max_abs_err=0.0, first=None) for f in info0.fields}
    for k, (info, data) in enumerate(clouds):
        n = data.size // info.point_step
        dec = oracle.decode_stage1(info, oracle.encode_stage1(info, data), n)
        rep = M.audit(info, data, dec, [n])
        for j, f in enumerate(info.fields):
            t = total[f.name]
            for key in ("n_bitwise_diff", "n_class_diff", "n_over_limit"):
                t[key] += int(rep[0, j][key])
            t["max_abs_err"] = max(t["max_abs_err"], float(rep[0, j]["max_abs_err"]))
            is_float = int(f.type) in (7, 8)
            if t["first"] is None and (rep[0, j]["n_class_diff"] or rep[0, j]["n_over_limit"] or
                                       (not is_float and rep[0, j]["n_bitwise_diff"])):
                t["first"] = f"msg_{k:05d}.bin"
    return total


def _same_files(one, two):
    names = sorted(os.listdir(one))
    assert names == sorted(os.listdir(two)) and names
    for nm in names:
        assert open(os.path.join(one, nm), "rb").read() == open(os.path.join(two, nm), "rb").read(), nm


@pytest.mark.gpu
def test_api_audit_summary_matches_the_model_summed_over_the_messages(tmp_path, oracle):
    clouds, msgs = _velodyne_messages(bad=3)
    src = str(tmp_path / "in")
    _write(src, msgs)
    plain = api.transcode_directory(src, str(tmp_path / "plain"), compression_opt=int(CompressionOption.ZSTD), batch_messages=4)
    assert "audit" not in plain
    st = api.transcode_directory(src, str(tmp_path / "audited"), compression_opt=int(CompressionOption.ZSTD), batch_messages=4,
                                 audit=True)
    _same_files(str(tmp_path / "plain"), str(tmp_path / "audited"))
    want = _model_summary(oracle, clouds)
    assert [f["name"] for f in st["audit"]] == [f.name for f in clouds[0][0].fields]
    for f in st["audit"]:
        w = want[f["name"]]
        assert (f["n_bitwise_diff"], f["n_class_diff"], f["n_over_limit"]) == (w["n_bitwise_diff"], w["n_class_diff"], w["n_over_limit"]), f
        assert f["max_abs_err"] == w["max_abs_err"], f
        assert f["first_bad_message"] == w["first"], f
    assert want["y"]["n_over_limit"] == 1 and want["y"]["first"] == "msg_00003.bin" and want["x"]["first"] is None
    # a limit that covers the garbage: nothing is over it any more
    st = api.transcode_directory(src, str(tmp_path / "wide"), batch_messages=4, audit=True, audit_limits={"y": 1.0e10})
    y = [f for f in st["audit"] if f["name"] == "y"][0]
    assert y["n_over_limit"] == 0 and y["first_bad_message"] is None and y["max_abs_err"] == want["y"]["max_abs_err"]


@pytest.mark.gpu
def test_command_line_audit_exit_status_and_table(tmp_path, oracle):
    assert os.path.exists(EXE)
    clouds, msgs = _velodyne_messages()
    src = str(tmp_path / "in")
    _write(src, msgs)
    base = [EXE, src]
    r0 = subprocess.run(base + [str(tmp_path / "plain"), "--batch", "4"], capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0 and "audit" not in r0.stdout, r0.stdout + r0.stderr
    r = subprocess.run(base + [str(tmp_path / "audited"), "--batch", "4", "--audit"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert json.loads(lines[-1])["messages"] == len(msgs)
    rows = [ln.split() for ln in lines if ln.startswith("audit ")][1:]
    assert [row[1] for row in rows] == [f.name for f in clouds[0][0].fields]
    want = _model_summary(oracle, clouds)
    for row in rows:
        assert (int(row[3]), int(row[4]), row[6]) == (0, 0, "-"), row          # the zeros
        assert int(row[2]) == want[row[1]]["n_bitwise_diff"] and float(row[5]) == want[row[1]]["max_abs_err"], row
    assert [row[2] for row in rows if row[1] == "ring"] == ["0"]
    _same_files(str(tmp_path / "plain"), str(tmp_path / "audited"))

    # one message carries the int32-overflow point: status 3, the message and the field are named, the files are the same
    clouds, msgs = _velodyne_messages(bad=4)
    src2 = str(tmp_path / "in2")
    _write(src2, msgs)
    r0 = subprocess.run([EXE, src2, str(tmp_path / "plain2"), "--batch", "4"], capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0
    r = subprocess.run([EXE, src2, str(tmp_path / "audited2"), "--batch", "4", "--audit"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 3, r.stdout + r.stderr
    rows = {ln.split()[1]: ln.split() for ln in r.stdout.splitlines() if ln.startswith("audit ")}
    assert rows["y"][4] == "1" and rows["y"][6] == "msg_00004.bin"
    assert all(rows[nm][6] == "-" for nm in ("x", "z", "intensity", "ring"))
    assert json.loads(r.stdout.strip().splitlines()[-1])["messages"] == len(msgs)
    _same_files(str(tmp_path / "plain2"), str(tmp_path / "audited2"))
    # --audit-limit lifts the field's limit: clean again
    r = subprocess.run([EXE, src2, str(tmp_path / "audited3"), "--batch", "4", "--audit-limit", "y:1e10"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([EXE, src2, str(tmp_path / "x"), "--audit-limit", "y"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
