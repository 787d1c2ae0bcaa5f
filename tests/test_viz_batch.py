"""The viz profile at batch rates: cldn_hip_viz_preprocess_batch (a ragged batch filtered cloud by cloud in one pass),
cldn_hip_encode_stage1_viz / _gather (filter + encode without the survivors leaving the device) and the `--viz` route of the
batch transcoder on top of them. Everything byte-exact: the filter against the C oracle (itself pinned to the compiled
reference on the same batches, on the CPU), the fused call against the plain encode of the oracle-filtered clouds, the
transcoder against the reference's converter fed with the survivors."""
import json
import os
import subprocess

import numpy as np
import pytest

import cases
import viz_batch_cases as vb
from cloudini_amd import synth
from cloudini_amd.schema import CompressionOption, FieldType as F, PointField

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- no GPU
@pytest.mark.parametrize("seed", vb.SEEDS)
def test_batch_generator_expectations_are_the_references(oracle, reflib, seed):
    info, clouds, off, res, _twin, want = vb.expected(oracle, seed)
    for k, (c, w) in enumerate(zip(clouds, want)):
        ref = reflib.viz_preprocess(info.copy(width=c.size // info.point_step), c)[0]
        assert np.array_equal(w, ref), (seed, k)


def test_concatenation_is_not_a_batch(oracle):
    """Two copies of a cloud filtered as ONE cloud keep what one copy keeps; as two clouds of a batch they keep twice that
    (the cloud of tests/test_batch_transcoder.py::test_viz_prefilter_in_the_batch)."""
    _info, data = synth.lidar_xyzi(60000, seed=5)
    pts = data.reshape(-1, 16).copy()
    pts[::7, 0:4] = np.frombuffer(np.float32(np.nan).tobytes(), dtype=np.uint8)
    one = oracle.viz_preprocess(pts.reshape(-1), 16, 0, 0.01).size // 16
    both = oracle.viz_preprocess(np.concatenate([pts, pts]).reshape(-1), 16, 0, 0.01).size // 16
    assert (one, both) == (51428, 51428)


# ---------------------------------------------------------------------------------------------------- GPU: the filter
def _codec():
    from cloudini_amd import native
    return native.Codec(native.Plan(synth.lidar_xyz(1)[0]))   # the codec only lends device, stream, workspace


def _check_host(codec, clouds, step, off, res, want, tag):
    got, kept, tail = codec.viz_preprocess_batch_host(clouds, step, off, res, guard=64)
    assert [int(k) for k in kept] == [w.size // step for w in want], tag
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.size == w.size and np.array_equal(g, w), (tag, k)
    assert np.all(tail == 0xA5), (tag, "behind the last survivor: the rest of the capacity and the guard")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", vb.SEEDS)
def test_batch_filter_matches_the_oracle_per_cloud(oracle, seed):
    """Host buffers, and device-resident ones at odd input / output addresses, guard spans behind the output."""
    import torch
    info, clouds, off, res, twin, want = vb.expected(oracle, seed)
    step = info.point_step
    codec = _codec()
    _check_host(codec, clouds, step, off, res, want, seed)
    data = np.concatenate(clouds)
    npts = np.array([c.size // step for c in clouds], dtype=np.uint64)
    dev = torch.device("cuda", 0)
    mi, mo = seed % 4, seed // 4 % 4
    d_in = torch.zeros(data.size + 8, dtype=torch.uint8, device=dev)
    d_in[mi:mi + data.size] = torch.from_numpy(data).to(dev)
    d_out = torch.full((data.size + 8 + 256,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    kept = codec.viz_preprocess_batch_device(d_in.data_ptr() + mi, npts, step, off, res, d_out.data_ptr() + mo, data.size)
    codec.synchronize()
    assert [int(k) for k in kept] == [w.size // step for w in want], (seed, "device resident")
    out = d_out.cpu().numpy()
    flat = np.concatenate(want)
    assert np.array_equal(out[mo:mo + flat.size], flat), (seed, "device resident")
    assert np.all(out[:mo] == 0xA5) and np.all(out[mo + flat.size:] == 0xA5), (seed, "nothing behind the last survivor")
    codec.close()


@pytest.mark.gpu
def test_every_single_cloud_case_as_a_batch_of_one_and_tiled():
    """The clouds of tests/test_viz_preprocess.py: as an n_clouds == 1 call each equals cldn_hip_viz_preprocess, tiled three
    times as one batch each gives three times its own survivors."""
    from test_viz_preprocess import VIZ
    codec = _codec()
    for name, info, data, off, res in VIZ:
        step = info.point_step
        single = codec.viz_preprocess_host(data, step, off, res)
        got, kept, _ = codec.viz_preprocess_batch_host([data], step, off, res)
        assert int(kept[0]) * step == single.size and np.array_equal(got[0], single), name
        got3, kept3, _ = codec.viz_preprocess_batch_host([data] * 3, step, off, res)
        assert [int(k) * step for k in kept3] == [single.size] * 3, name
        for g in got3:
            assert np.array_equal(g, single), name
    codec.close()


@pytest.mark.gpu
def test_cloud_groups_do_not_change_a_byte(oracle):
    """The table memory of a batch is bounded by filtering consecutive cloud groups. With the limit at one slot every
    non-empty cloud is a group of its own: at least three groups, a boundary between the two identical clouds."""
    seed = vb.SEEDS[0]
    info, clouds, off, res, twin, want = vb.expected(oracle, seed)
    assert sum(1 for c in clouds if c.size) >= 3 and clouds[twin].size and clouds[twin + 1].size
    codec = _codec()
    codec.viz_group_slots(1)
    _check_host(codec, clouds, info.point_step, off, res, want, "one cloud per group")
    # two clouds per group where they fit: the tables of a group lie behind each other
    slots = 2 * max(1024, 1 << int(np.ceil(np.log2(2 * max(c.size // info.point_step for c in clouds)))))
    codec.viz_group_slots(slots)
    _check_host(codec, clouds, info.point_step, off, res, want, "pairs")
    codec.viz_group_slots(0)
    _check_host(codec, clouds, info.point_step, off, res, want, "default")
    codec.close()


@pytest.mark.gpu
def test_more_blocks_than_one_round_of_the_scan(oracle):
    """1100 clouds of 1 to 3 points are 1100 blocks: the one-workgroup scan of k_viz_offsets takes a second round of 1024, and
    the survivors per cloud are differences of block positions on both sides of that boundary."""
    rs = np.random.RandomState(77)
    step, off, res = 16, 0, 0.5
    clouds = []
    for k in range(1100):
        n = 1 + k % 3
        pts = np.zeros((n, 4), np.float32)
        pts[:, :3] = rs.randint(0, 2, (n, 3)) * (2 * res)    # two voxels per axis: points of a cloud often share one
        if k % 7 == 0:
            pts[0, 1] = np.nan
        clouds.append(pts.view(np.uint8).reshape(-1))
    want = [oracle.viz_preprocess(c, step, off, res) for c in clouds]
    kept = [w.size // step for w in want]
    assert len(clouds) == 1100 > 1024 and set(kept) == {0, 1, 2, 3}
    assert any(k < c.size // step for k, c in zip(kept[1024:], clouds[1024:]))
    codec = _codec()
    _check_host(codec, clouds, step, off, res, want, "1100 clouds")
    codec.close()


@pytest.mark.gpu
def test_batch_argument_checks():
    from cloudini_amd import native
    codec = _codec()
    data = synth.lidar_xyzi(100, seed=1)[1]
    for bad in ((16, 8, 0.001), (16, 0, 0.0), (16, 0, float("nan")), (16, 0, -1.0)):
        with pytest.raises(native.CloudiniHipError):
            codec.viz_preprocess_batch_host([data, data], *bad)
    got, kept, _ = codec.viz_preprocess_batch_host([], 16, 0, 0.01)
    assert got == [] and kept.size == 0
    got, kept, _ = codec.viz_preprocess_batch_host([data[:0], data[:0]], 16, 0, 0.01)
    assert [int(k) for k in kept] == [0, 0]
    # the limits: 2^32 - 2 points per cloud, and per batch (block offsets and ranks are 32-bit); refused before anything
    # is allocated or read
    for counts, text in (([2 ** 32 - 1], "more than 2^32 - 2 points"), ([5, 2 ** 32 - 1], "more than 2^32 - 2 points"),
                         ([2 ** 31, 2 ** 31], "more than 2^32 - 2 points in one batch")):
        with pytest.raises(native.CloudiniHipError) as e:
            codec.viz_preprocess_batch_device(0, np.array(counts, dtype=np.uint64), 16, 0, 0.01, 0, 0)
        assert e.value.code == -3 and e.value.message == "viz_preprocess: " + text, counts
    with pytest.raises(native.CloudiniHipError) as e:
        codec.viz_preprocess_device(0, 2 ** 32 - 1, 16, 0, 0.01, 0, 0)
    assert e.value.code == -3 and e.value.message == "viz_preprocess: more than 2^32 - 2 points"
    codec.close()


# ---------------------------------------------------------------------------------------------------- GPU: filter + encode
def _with_res(info, res):
    return info.copy(fields=[PointField(f.name, f.offset, f.type, res if f.type == F.FLOAT32 else f.resolution) for f in info.fields])


def _all_nan_like(data, step, n, off=0):
    pts = data[: n * step].reshape(-1, step).copy()
    pts[:, off:off + 4] = np.frombuffer(np.float32(np.nan).tobytes(), dtype=np.uint8)
    return pts.reshape(-1)


def _stamp_layout(n, res, seed):
    """x, y, z float32 + uint16 + a FLOAT64 stamp that carries the 1 us resolution the viz profile gives it."""
    rs = np.random.RandomState(seed)
    fields = [("x", 0, F.FLOAT32, res), ("y", 4, F.FLOAT32, res), ("z", 8, F.FLOAT32, res), ("i", 12, F.UINT16, None),
              ("t", 16, F.FLOAT64, 1e-6)]
    info = cases.make_info(fields, 24, n)
    xyz = vb._xyz(rs, n, 1, res)
    xyz[::50, 1] = np.nan
    cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "i": rs.randint(0, 300, n).astype(np.uint16),
            "t": 1.7e9 + np.arange(n) * 1e-5}
    return info, cases.pack(info, cols, n)


def _fused_batches():
    """(name, info, clouds, resolution): the resolutions at which the filter does real work (survivor table of the oracle:
    lidar_xyzi(60000, seed=5) keeps 44 584 at 0.25, velodyne_xyzir(130048, seed=42) 80 582, depthcam(320, 240) 11 589 at 0.01
    and 72 924 at 0.001 -- NaN drop only). Every batch has a cloud that loses every point and a zero-point cloud."""
    out = []
    info, a = synth.lidar_xyzi(60000, seed=5, res=0.25)
    b, c = synth.lidar_xyzi(70001, seed=6, res=0.25)[1], synth.lidar_xyzi(1025, seed=7, res=0.25)[1]
    out.append(("xyzi", info, [a, _all_nan_like(a, 16, 5000), b, a[:0], c, a], 0.25))
    info, a = synth.velodyne_xyzir(130048, seed=42, res=0.25)
    b = synth.velodyne_xyzir(40000, seed=43, res=0.25)[1]
    out.append(("velodyne_xyzir", info, [a, b, _all_nan_like(b, 18, 33000), a[:0], b], 0.25))
    info, a = synth.depthcam_xyzrgba(320, 240, res=0.01)
    b = synth.depthcam_xyzrgba(320, 240, seed=43, res=0.01)[1]
    out.append(("depthcam_xyzrgba", info, [a, _all_nan_like(a, 32, 1024), b, a[:0]], 0.01))
    info, a = synth.depthcam_xyzrgba(320, 240, res=0.001)
    out.append(("depthcam_nan_drop_only", info, [a, a[:0], _all_nan_like(a, 32, 63), a], 0.001))
    info, a = _stamp_layout(50000, 0.1, 3)
    b = _stamp_layout(33000, 0.1, 4)[1]
    out.append(("float64_stamp", info, [a, b, _all_nan_like(b, 24, 2000), a[:0]], 0.1))
    return out


FUSED = _fused_batches()


def _assert_same(got, want, tag):
    (gs, gc, gm, gk), (ws, wc, wm, wk) = got, want
    assert [int(k) for k in gk] == [int(k) for k in wk], (tag, "kept_points")
    assert len(gs) == len(ws)
    for k, (a, b) in enumerate(zip(gs, ws)):
        assert a.size == b.size and np.array_equal(a, b), (tag, "stream", k)
    assert np.array_equal(gc, wc), (tag, "chunk_sizes")
    assert np.array_equal(gm, wm), (tag, "modes")


@pytest.mark.gpu
@pytest.mark.parametrize("name,info,clouds,res", FUSED, ids=[f[0] for f in FUSED])
def test_fused_call_equals_the_encode_of_the_filtered_clouds(oracle, name, info, clouds, res):
    """encode_viz against encode of the oracle-filtered clouds: streams (hence stream_offsets), chunk_sizes, modes,
    kept_points -- contiguous and gather, host and device outputs, the two-step host output, device LZ4 on. A cloud that
    loses every point is a zero-point cloud of the batch: no bytes, no chunk, mode 0 (what the plain encode does with a
    zero-point cloud inside a batch; the oracle's stream of a zero-point cloud is 0 bytes)."""
    import torch
    from cloudini_amd import native
    step = info.point_step
    off = info.fields[0].offset
    filtered = [oracle.viz_preprocess(c, step, off, res) for c in clouds]
    kept = [f.size // step for f in filtered]
    lost_all = [k for k, (c, f) in enumerate(zip(clouds, filtered)) if c.size and not f.size]
    assert lost_all and any(0 < k < c.size // step for k, c in zip(kept, clouds))
    assert oracle.encode_stage1(info, filtered[lost_all[0]]).size == 0
    plan = native.Plan(info)
    ref_codec = native.Codec(plan)
    want = ref_codec.encode_host(filtered) + (np.array(kept, dtype=np.uint64),)
    for k in lost_all + [k for k, c in enumerate(clouds) if not c.size]:
        assert want[0][k].size == 0 and np.all(want[2][k] == 0), (name, k)
    for k, f in enumerate(filtered):                        # the plain encode itself is the oracle's, cloud by cloud
        assert np.array_equal(want[0][k], oracle.encode_stage1(info, f)), (name, k)
    codec = native.Codec(plan)
    _assert_same(codec.encode_viz(clouds, off, res), want, (name, "contiguous"))
    _assert_same(codec.encode_viz(clouds, off, res, gather=True), want, (name, "gather"))
    _assert_same(codec.encode_viz(clouds, off, res, two_step=True), want, (name, "two-step"))
    _assert_same(codec.encode_viz(clouds, off, res, gather=True, two_step=True), want, (name, "gather, two-step"))
    # device resident, device outputs, sized by the input counts
    dev = torch.device("cuda", 0)
    data = np.concatenate(clouds)
    npts = np.array([c.size // step for c in clouds], dtype=np.uint64)
    cap = int(sum(plan.stage1_bound(int(n)) for n in npts))
    n_chunks_in = int(sum((int(n) + 32767) // 32768 for n in npts))
    na = plan.adaptive_fields
    d_in = torch.from_numpy(data).to(dev)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_offs = torch.zeros(len(clouds) + 1, dtype=torch.int64, device=dev)
    d_sizes = torch.zeros(max(1, n_chunks_in), dtype=torch.int32, device=dev)
    d_modes = torch.full((max(1, len(clouds) * max(1, na)),), 0xEE, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    got_kept = codec.encode_viz_device(d_in.data_ptr(), npts, off, res, d_out.data_ptr(), cap, d_offs.data_ptr(),
                                       d_sizes.data_ptr(), d_modes.data_ptr())
    codec.synchronize()
    codec.status()
    offs = d_offs.cpu().numpy().astype(np.uint64)
    out = d_out.cpu().numpy()
    n_chunks = int(sum((k + 32767) // 32768 for k in kept))
    got = ([out[int(offs[k]):int(offs[k + 1])] for k in range(len(clouds))], d_sizes.cpu().numpy().view(np.uint32)[:n_chunks],
           d_modes.cpu().numpy()[: len(clouds) * na].reshape(len(clouds), na), got_kept)
    _assert_same(got, want, (name, "device"))
    # stage 2 on the device
    ref_codec.set_stage2(1)
    codec.set_stage2(1)
    want_lz4 = ref_codec.encode_host(filtered) + (np.array(kept, dtype=np.uint64),)
    _assert_same(codec.encode_viz(clouds, off, res), want_lz4, (name, "device LZ4"))
    _assert_same(codec.encode_viz(clouds, off, res, gather=True, two_step=True), want_lz4, (name, "device LZ4, gather, two-step"))
    codec.close()
    ref_codec.close()


@pytest.mark.gpu
def test_fused_call_with_forced_modes_and_checks(oracle):
    from cloudini_amd import native
    name, info, clouds, res = FUSED[0]
    filtered = [oracle.viz_preprocess(c, 16, 0, res) for c in clouds]
    plan = native.Plan(info)
    a, b = native.Codec(plan), native.Codec(plan)
    for m in range(4):
        a.force_modes([m])
        b.force_modes([m])
        want = a.encode_host(filtered) + (np.array([f.size // 16 for f in filtered], dtype=np.uint64),)
        _assert_same(b.encode_viz(clouds, 0, res), want, ("forced", m))
    b.force_modes(None)
    for bad in ((8, 0.25), (0, 0.0), (0, float("inf"))):
        with pytest.raises(native.CloudiniHipError):
            b.encode_viz(clouds, *bad)
    streams, sizes, _modes, kept = b.encode_viz([], 0, res)
    assert streams == [] and sizes.size == 0 and kept.size == 0
    fresh = native.Codec(plan)                               # no workspace yet: a batch of zero-point clouds needs none
    for gather in (False, True):
        streams, sizes, modes, kept = fresh.encode_viz([clouds[0][:0], clouds[0][:0]], 0, res, gather=gather)
        assert [s.size for s in streams] == [0, 0] and sizes.size == 0 and [int(k) for k in kept] == [0, 0] and np.all(modes == 0)
    fresh.close()
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------- GPU: the transcoder
def _gate_fails(n, seed):
    """y and z swapped in memory: no consecutive triple, the reference's function leaves the cloud alone."""
    rs = np.random.RandomState(seed)
    fields = [("x", 0, F.FLOAT32, None), ("y", 8, F.FLOAT32, None), ("z", 4, F.FLOAT32, None)]
    info = cases.make_info(fields, 12, n)
    xyz = np.round(rs.uniform(-3, 3, (n, 3)), 1).astype(np.float32)
    xyz[::9, 0] = np.nan
    return info, cases.pack(info, {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2]}, n)


def _no_res(info):
    return info.copy(fields=[PointField(f.name, f.offset, f.type, None) for f in info.fields])


def _mixed_viz_messages():
    """(info, data, kwargs of cdr_pointcloud2): two schemas that pass the gate, an empty message, an all-NaN message, a
    schema that fails the gate, a schema with a FLOAT64 stamp; schema changes inside batches of 4."""
    out = []
    for k, n in enumerate([60000, 1025, 70001]):
        info, data = synth.lidar_xyzi(n, seed=5 + k)
        out.append((info, data, dict(stamp=(1700000000 + k, 1000 * k))))
    info, data = synth.lidar_xyzi(5000, seed=9)
    out.append((info, _all_nan_like(data, 16, 5000), dict()))
    out.append((info.copy(width=0), data[:0], dict()))
    out.append((info, data, dict(is_dense=False)))
    for k, n in enumerate([130048, 20000]):
        info, data = synth.velodyne_xyzir(n, seed=42 + k)
        out.append((info, data, dict(frame_id="velodyne")))
    info, data = _gate_fails(9000, 2)
    out.append((info, data, dict()))
    for k, n in enumerate([50000, 33000]):
        info, data = _stamp_layout(n, 0.25, 11 + k)
        out.append((_no_res(info), data, dict(frame_id="stamped")))
    info, data = synth.lidar_xyzi(40000, seed=21)
    out.append((info, data, dict()))
    return out


def _expected_viz_message(reflib, info, data, kw, res, comp):
    """What the reference's converter writes with the viz profile: convertPointCloud2ToCompressedCloud of the survivors
    message (applyVizLossyPreprocessing changes exactly data, width, height and row_step)."""
    from test_batch_transcoder import _swap_stream
    msg = synth.cdr_pointcloud2(info, data, **kw)
    after = _with_res(_no_res(info), res)                   # applyResolutionProfile: `resolution` on every FLOAT32 field
    # (a schema that fails the gate, or an empty cloud, comes back untouched: the survivors message is the input message)
    survivors, _res_after, w, h = reflib.viz_preprocess(after, data)
    kept = survivors.size // info.point_step
    smsg = synth.cdr_pointcloud2(info.copy(width=w, height=h), survivors, **kw) if data.size else msg
    want = reflib.ros_compress(smsg, res, comp)
    stamp = [i for i, f in enumerate(info.fields) if f.type == F.FLOAT64]
    if stamp and kept:
        # a PointCloud2 message cannot carry the 1 us resolution the function gives the stamp: the stream comes from the
        # reference's encoder with the schema behind the function, and replaces the one in the reference's message
        info_after = after.copy(width=kept, height=1, compression_opt=CompressionOption(comp),
                                fields=[PointField(f.name, f.offset, f.type, 1e-6 if f.type == F.FLOAT64 else f.resolution)
                                        for f in after.fields])
        want = _swap_stream(want, reflib.encode(info_after, survivors).tobytes())
    return want, kept


def _write(folder, messages):
    os.makedirs(folder, exist_ok=True)
    for k, m in enumerate(messages):
        m.tofile(os.path.join(folder, f"msg_{k:05d}.bin"))


@pytest.mark.gpu
@pytest.mark.parametrize("comp", [CompressionOption.ZSTD, CompressionOption.LZ4, CompressionOption.NONE])
def test_viz_transcode_equals_the_reference_converter(tmp_path, reflib, comp):
    from cloudini_amd import api
    res = 0.25
    mixed = _mixed_viz_messages()
    msgs = [synth.cdr_pointcloud2(i, d, **kw) for i, d, kw in mixed]
    want = [_expected_viz_message(reflib, i, d, kw, res, int(comp)) for i, d, kw in mixed]
    kept_total = sum(k for _, k in want)                    # (a cloud that fails the gate keeps every point)
    assert want[3][1] == 0 and 0 < want[0][1] < 60000 * 3 // 4 and 0 < want[6][1] < 130048 * 3 // 4
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    _write(src, msgs)
    stats = api.transcode_directory(src, dst, resolution=res, compression_opt=int(comp), viz_lossy=True, batch_messages=4)
    assert int(stats["messages"]) == len(msgs) and int(stats["points"]) == kept_total
    for k in range(len(msgs)):
        got = np.fromfile(os.path.join(dst, f"msg_{k:05d}.bin"), dtype=np.uint8)
        assert got.size == want[k][0].size and np.array_equal(got, want[k][0]), f"message {k}"
    if comp == CompressionOption.ZSTD:                     # two GPU stages on one device write the same files
        two = str(tmp_path / "two")
        api.transcode_directory(src, two, resolution=res, compression_opt=int(comp), viz_lossy=True, batch_messages=4, devices=[0, 0])
        for k in range(len(msgs)):
            assert np.array_equal(np.fromfile(os.path.join(two, f"msg_{k:05d}.bin"), dtype=np.uint8), want[k][0]), f"message {k}, two stages"


@pytest.mark.gpu
def test_viz_launches_follow_the_batches_not_the_messages(tmp_path):
    """64 messages of one schema in batches of 32: two GPU calls, and the survivors are what 64 single filters keep."""
    distinct = [synth.velodyne_xyzir(130048, seed=42 + k) for k in range(2)]
    msgs = [synth.cdr_pointcloud2(distinct[k % 2][0], distinct[k % 2][1], stamp=(1700000000, k)) for k in range(64)]
    src, dst = str(tmp_path / "in"), str(tmp_path / "out")
    _write(src, msgs)
    exe = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
    r = subprocess.run([exe, src, dst, "--resolution", "0.25", "--compression", "none", "--viz", "--batch", "32"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    st = json.loads(r.stdout.strip().splitlines()[-1])
    codec = _codec()
    kept = [codec.viz_preprocess_host(d[1], 18, 0, 0.25).size // 18 for d in distinct]
    codec.close()
    assert kept[0] == 80582                                  # the oracle's count for velodyne_xyzir(130048, seed=42) at 0.25
    assert st["messages"] == 64 and st["gpu_batches"] == 2 and st["points"] == 32 * (kept[0] + kept[1])


@pytest.mark.gpu
def test_viz_through_a_bag(tmp_path, reflib):
    import mcap_py
    res = 0.25
    mixed = _mixed_viz_messages()[:6]
    pc2 = "sensor_msgs/msg/PointCloud2"
    schemas = [(1, pc2, "ros2msg", b"whatever the recorder wrote"), (2, "std_msgs/msg/String", "ros2msg", b"string data")]
    channels = [(1, 1, "/lidar", "cdr", []), (2, 2, "/chatter", "cdr", [])]
    msgs, t = [], 1000
    for k, (i, d, kw) in enumerate(mixed):
        msgs.append((2, 2 * k, t, t, b"hello %d" % k)); t += 5
        msgs.append((1, 2 * k + 1, t, t - 1, synth.cdr_pointcloud2(i, d, **kw).tobytes())); t += 5
    src, enc = str(tmp_path / "in.mcap"), str(tmp_path / "enc.mcap")
    mcap_py.write(src, "ros2", schemas, channels, msgs, chunk_messages=4)
    exe = os.path.join(ROOT, "cloudini_amd", "lib", "cloudini_batch_transcode")
    r = subprocess.run([exe, src, enc, "--resolution", str(res), "--compression", "lz4", "--viz", "--mcap-compression", "none",
                        "--batch", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    f = mcap_py.read(enc)
    assert len(f["messages"]) == len(msgs)
    clouds = iter(mixed)
    for (ch, _seq, _lt, _pt, data), (ch0, _s0, _l0, _p0, data0) in zip(f["messages"], msgs):
        assert ch == ch0
        if ch0 == 2:
            assert data == data0
        else:
            i, d, kw = next(clouds)
            assert data == _expected_viz_message(reflib, i, d, kw, res, int(CompressionOption.LZ4))[0].tobytes()
