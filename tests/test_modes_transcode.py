"""The adaptive integer mode sweep through the host layers: TranscodeOptions::modes behind the C facade, the Python API and the
command-line tool. Expected summaries are tests/mode_model.py on the message points, summed over the messages; the message of
a `best` run is checked against the model's saving and decoded by the compiled reference."""
import json
import os
import subprocess

import numpy as np
import pytest

import mode_model as M
from cloudini_amd import api, synth
from cloudini_amd.schema import CompressionOption

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
SIZES = [20000, 40000, 1, 33000, 5000]
FOOLED = 1  # the message whose ring column fools the probe


def test_libraries_export_the_mode_entry_points_and_the_option():
    from cloudini_amd import native
    for name in ("cldn_hip_sweep_modes_clouds", "cldn_hip_sweep_modes_last_encode", "cldn_hip_codec_force_modes_per_cloud"):
        assert hasattr(native.lib(), name), name
    assert hasattr(api.lib(), "cldn_amd_transcode_directory_modes")
    for name in ("sweep_modes_host", "sweep_modes_device", "sweep_modes_last_encode", "force_modes_per_cloud"):
        assert hasattr(native.Codec, name), name
    assert native.MODE_DTYPE == M.DTYPE and native.MODE_DTYPE.itemsize == 40
    assert callable(api.sweep_modes) and callable(api.encode_stage1_with_modes)
    with pytest.raises(ValueError):
        api.transcode_directory("a", "b", modes="always")
    with pytest.raises(ValueError):
        api.transcode_directory("a", "b", modes="report", audit=True)


def test_tool_exit_codes(tmp_path):
    """The tool refuses a bad --modes before it touches a file or a device."""
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    os.makedirs(src)
    for args in (["--modes", "always"], ["--modes", ""], ["--modes"], ["--decode", "--modes", "report"], ["--modes", "best", "--decode"]):
        r = subprocess.run([EXE, src, dst] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.stdout, r.stderr)
        assert not os.path.exists(dst) or not os.listdir(dst)


def _messages():
    """Velodyne-like messages (x y z intensity float32, ring u16); in one of them the ring is constant over the first 4096
    points and noise behind them."""
    clouds, msgs = [], []
    for k, n in enumerate(SIZES):
        info, data = synth.velodyne_xyzir(n, seed=80 + k)
        data = data.copy()
        if k == FOOLED:
            ring = data.reshape(n, info.point_step)[:, 16:18].view("<u2").reshape(-1)
            ring[:4096] = 9
            ring[4096:] = np.random.RandomState(3).randint(0, 1 << 15, n - 4096)
        clouds.append((info, data))
        msgs.append(synth.cdr_pointcloud2(info, data, stamp=(1700000000 + k, k)))
    return clouds, msgs


def _write(folder, msgs):
    os.makedirs(folder, exist_ok=True)
    for k, m in enumerate(msgs):
        m.tofile(os.path.join(folder, f"msg_{k:05d}.bin"))


def _read(folder):
    return {nm: open(os.path.join(folder, nm), "rb").read() for nm in sorted(os.listdir(folder))}


def _model(clouds):
    """(summary as the JSON has it, stage-1 bytes `best` saves per message)."""
    fields, saved = {}, []
    for info, data in clouds:
        rep = M.sweep(info, data, [data.size // info.point_step])[0]
        gain = 0
        for a, f in enumerate(M.adaptive_fields(info)):
            t = fields.setdefault(f.name, {"name": f.name, "clouds": 0, "bytes": [0] * 4, "probed": [0] * 4, "best": [0] * 4, "saved_bytes": 0})
            p, b = int(rep["probe_mode"][a]), int(rep["best_mode"][a])
            t["clouds"] += 1
            t["bytes"] = [x + int(y) for x, y in zip(t["bytes"], rep["bytes"][a])]
            t["probed"][p] += 1
            t["best"][b] += 1
            t["saved_bytes"] += int(rep["bytes"][a, p]) - int(rep["bytes"][a, b])
            gain += int(rep["bytes"][a, p]) - int(rep["bytes"][a, b])
        saved.append(gain)
    return list(fields.values()), saved


def _table(stdout):
    rows = [ln.split() for ln in stdout.splitlines() if ln.startswith("modes ")]
    assert rows[0][1:] == ["field", "clouds", "DeltaVarint", "Palette", "Rle", "DeltaRle", "probed", "best", "saved_bytes"]
    assert rows[-1][1] == "reencoded_runs"
    fields = [{"name": r[1], "clouds": int(r[2]), "bytes": [int(x) for x in r[3:7]], "probed": [int(x) for x in r[7].split("/")],
               "best": [int(x) for x in r[8].split("/")], "saved_bytes": int(r[9])} for r in rows[1:-1]]
    return fields, int(rows[-1][2])


@pytest.mark.gpu
def test_report_leaves_the_files_alone_and_best_saves_what_the_model_says(tmp_path, reflib):
    assert os.path.exists(EXE)
    clouds, msgs = _messages()
    src = str(tmp_path / "in")
    _write(src, msgs)
    want, saved = _model(clouds)
    assert len(want) == 1 and want[0]["name"] == "ring" and want[0]["clouds"] == len(SIZES)
    assert saved[FOOLED] > 10000 and sum(saved) == saved[FOOLED]              # the other messages are probed right
    run = lambda dst, *more: subprocess.run([EXE, src, str(tmp_path / dst), "--batch", "2", "--compression", "none", *more],
                                            capture_output=True, text=True, timeout=600)
    r0 = run("plain")
    assert r0.returncode == 0 and "modes" not in r0.stdout, r0.stdout + r0.stderr
    plain = _read(tmp_path / "plain")
    # report: the model's numbers, the plain run's files
    r = run("report", "--modes", "report")
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert json.loads(lines[-1])["messages"] == len(msgs) and all(ln.startswith("modes ") for ln in lines[:-1])
    assert _table(r.stdout) == (want, 0)
    assert _read(tmp_path / "report") == plain
    st = api.transcode_directory(src, str(tmp_path / "api"), compression_opt=int(CompressionOption.NONE), batch_messages=2, modes="report")
    assert st["modes"] == {"reencoded_runs": 0, "fields": want} and _read(tmp_path / "api") == plain
    assert "modes" not in api.transcode_directory(src, str(tmp_path / "api2"), batch_messages=2)
    # best: one run of two messages is encoded again; the fooled message shrinks by the model's saving, the others stay
    r = run("best", "--modes", "best")
    assert r.returncode == 0, r.stdout + r.stderr
    assert _table(r.stdout) == (want, 1)
    best = _read(tmp_path / "best")
    for k, nm in enumerate(sorted(plain)):
        body = lambda msg: reflib.ros_describe(np.frombuffer(msg, np.uint8))[2]    # the compressed payload (the message pads behind it)
        assert body(plain[nm]) - body(best[nm]) == saved[k], nm
        if k != FOOLED:
            assert best[nm] == plain[nm], nm
        capacity = len(msgs[k]) + 4096
        a = reflib.ros_decompress(np.frombuffer(best[nm], np.uint8), capacity)
        assert a.tobytes() == reflib.ros_decompress(np.frombuffer(plain[nm], np.uint8), capacity).tobytes(), nm
    st = api.transcode_directory(src, str(tmp_path / "api3"), compression_opt=int(CompressionOption.NONE), batch_messages=2, modes="best")
    assert st["modes"] == {"reencoded_runs": 1, "fields": want} and _read(tmp_path / "api3") == best
    # with stage 2 behind it the messages still decode to the same points, and the audit behind a best run is clean
    r = subprocess.run([EXE, src, str(tmp_path / "zstd"), "--batch", "2", "--modes", "best", "--audit"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    nm = sorted(plain)[FOOLED]
    z = open(tmp_path / "zstd" / nm, "rb").read()
    capacity = len(msgs[FOOLED]) + 4096
    assert reflib.ros_decompress(np.frombuffer(z, np.uint8), capacity).tobytes() == \
        reflib.ros_decompress(np.frombuffer(plain[nm], np.uint8), capacity).tobytes()
