"""Adaptive integer mode sweep on the device (cloudini_amd/csrc/mode_kernels.hip): cldn_hip_sweep_modes_clouds,
cldn_hip_sweep_modes_last_encode, and cldn_hip_codec_force_modes_per_cloud in front of every encode entry point.

Expected reports never come from the code under test: they are tests/mode_model.py on the same points (the model itself is
held against the oracle and the reference in tests/test_mode_model.py). Every comparison is exact, cell for cell. Forced
streams are compared byte for byte with the oracle's encode under the same modes."""
import ctypes as C

import numpy as np
import pytest

import audit_model as A
import cases
import mode_cases as MC
import mode_model as M
from cloudini_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 256
CELL = 40
F = cases.F


def _codec(info):
    from cloudini_amd import native
    return native.Codec(native.Plan(info))


def _same(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.tobytes() != want.tobytes():
        bad = [(idx, got[idx].tolist(), want[idx].tolist()) for idx in np.ndindex(got.shape) if got[idx].tobytes() != want[idx].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} cells differ, first (cloud, field), got, want: {bad[:4]}")


def _dev(arr, residue=0):
    """A device copy of `arr` that starts `residue` (< 16) bytes behind a 256-byte boundary, between two guard spans. Returns
    (tensor, pointer, check) -- check() asserts that guards and content are as they were."""
    import torch
    dev = torch.device("cuda", 0)
    arr = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = torch.full((256 + GUARD + 16 + arr.size + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    base = (-t.data_ptr()) % 256 + GUARD + residue
    if arr.size:
        t[base:base + arr.size] = torch.from_numpy(arr.copy()).to(dev)
    before = t.cpu().numpy().copy()

    def check():
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), before), "a buffer the sweep may only read has changed"
    return t, t.data_ptr() + base, check


def _dev_report(n_clouds, n_fields):
    """A device report between guard spans, pre-filled; returns (read, pointer): read() checks the guards and returns it."""
    import torch
    nbytes = n_clouds * n_fields * CELL
    t = torch.full((256 + GUARD + nbytes + GUARD,), 0xEE, dtype=torch.uint8, device=torch.device("cuda", 0))
    base = (-t.data_ptr()) % 256 + GUARD
    torch.cuda.synchronize()  # the codec works on a stream of its own: the fill lands before a call writes the report

    def read():
        torch.cuda.synchronize()
        h = t.cpu().numpy()
        assert (h[:base] == 0xEE).all() and (h[base + nbytes:] == 0xEE).all(), "the sweep wrote outside its report"
        return h[base:base + nbytes].copy().view(M.DTYPE).reshape(n_clouds, n_fields)
    return read, t.data_ptr() + base


def _cut(info, data, sizes):
    step = info.point_step
    ends = np.cumsum(sizes)
    return [data[(e - n) * step:e * step].copy() for n, e in zip(sizes, ends)]


def _both_calls_and_both_reports(info, data, sizes, residue, what):
    """Host points + host report, device points at `residue` + device report, device points + host report: all the model."""
    want = M.sweep(info, data, sizes)
    na = want.shape[1]
    codec = _codec(info)
    _same(codec.sweep_modes_host(_cut(info, data, sizes)), want, what + " host")
    odd = np.zeros(data.size + 16, np.uint8)                                    # host points at an odd address
    at = (-odd.ctypes.data) % 16 + 1
    odd[at:at + data.size] = data
    from cloudini_amd import native
    _same(codec.sweep_modes_device(odd.ctypes.data + at, sizes, points_loc=native.HOST), want, what + " host, odd address")
    _t, p, check = _dev(data, residue)
    read, pr = _dev_report(len(sizes), na)
    assert codec.sweep_modes_device(p, sizes, report_ptr=pr) is None
    _same(read(), want, what + " device")
    _same(codec.sweep_modes_device(p, sizes), want, what + " device points, host report")
    check()
    return codec, want


# ---- every schema family, very wide schemas ----------------------------------------------------------------------------

FAMILIES = [(n, i, d) for n, i, d in cases.encode_cases(small=True) if M.adaptive_fields(i)]


@pytest.mark.parametrize("name,info,data", FAMILIES, ids=[c[0] for c in FAMILIES])
def test_modes_equal_the_model_on_every_schema_family(name, info, data):
    n = data.size // info.point_step
    want = M.sweep(info, data, [n])
    codec = _codec(info)
    _same(codec.sweep_modes_host([data]), want, name)
    _streams, _cs, modes = codec.encode_host([data])
    assert modes[0].tolist() == want["probe_mode"][0].tolist(), name           # what the encoder commits
    _same(codec.sweep_modes_last_encode(), want, name + " last encode")


@pytest.mark.parametrize("seed", [9019, 9027])
def test_very_wide_schemas_direct_route_and_field_table_in_device_memory(seed):
    info, data = cases.very_wide_schema(seed)
    na = len(M.adaptive_fields(info))
    assert info.point_step > 127 and na > (128 if seed == 9027 else 64)
    n = data.size // info.point_step
    sizes = [n // 3, 0, n - n // 3]
    codec, want = _both_calls_and_both_reports(info, data, sizes, 5, f"very_wide_{seed}")
    _s, _c, modes = codec.encode_host(_cut(info, data, sizes))
    assert modes.tolist() == want["probe_mode"].tolist()


def test_a_plan_without_adaptive_fields_writes_nothing():
    info, data = synth.lidar_xyz(1000)
    codec = _codec(info)
    assert codec.sweep_modes_host([data]).shape == (1, 0)
    _t, p, check = _dev(data)
    read, pr = _dev_report(1, 1)
    codec.sweep_modes_device(p, [1000], report_ptr=pr)
    assert (read().view(np.uint8) == 0xEE).all()
    check()


# ---- ragged batch --------------------------------------------------------------------------------------------------------

RAGGED = [0, 1, 4095, 4096, 4097, 32767, 32768, 32769, 70001]


@pytest.mark.parametrize("residue", [0, 7])
def test_ragged_batch_with_the_same_cloud_twice(residue):
    info, data = cases.header_test_struct(sum(RAGGED))                       # ring u16 + time u32 in 24-byte points
    clouds = _cut(info, data, RAGGED)
    clouds.append(clouds[-1].copy())
    sizes = RAGGED + [RAGGED[-1]]
    flat = np.concatenate(clouds)
    codec, want = _both_calls_and_both_reports(info, flat, sizes, residue, "ragged")
    assert not want[0].tobytes().strip(b"\0") and want[-1].tobytes() == want[-2].tobytes()
    assert codec.sweep_modes_host([]).shape == (0, 2)


# ---- crafted columns -----------------------------------------------------------------------------------------------------

CRAFTED = list(MC.all_crafted())


@pytest.mark.parametrize("name,info,data,check", CRAFTED, ids=[c[0] for c in CRAFTED])
def test_crafted_columns(name, info, data, check):
    v, _bpv = M.column(info, data, M.adaptive_fields(info)[0])
    assert check(v), name                                                       # the case is what its name says, before the device runs
    n = data.size // info.point_step
    want = M.sweep(info, data, [n])
    if name.endswith("probe_fooled"):
        assert want["best_mode"][0, 0] != want["probe_mode"][0, 0]
    codec = _codec(info)
    if "_odd_" in name:
        _t, p, chk = _dev(data, 3)
        _same(codec.sweep_modes_device(p, [n]), want, name)
        chk()
    else:
        _same(codec.sweep_modes_host([data]), want, name)


def test_stage_edges_of_wide_points():
    """Points of 100 bytes go through LDS 384 at a time: runs of 64 values and of 64 equal deltas that start one value in front
    of every wave edge straddle those stage edges too (384 = 6 waves)."""
    n = 2000
    i = np.arange(n)
    fields = [("a", 3, F.UINT32, None), ("b", 50, F.INT64, None), ("c", 97, F.UINT16, None)]
    info = cases.make_info(fields, 100, n)
    slopes = (np.arange(n // 64 + 2) % 5) - 2
    cols = {"a": ((i + 1) // 64).astype(np.uint32), "b": np.cumsum(slopes[(i + 1) // 64]).astype(np.int64) << 33,
            "c": ((i + 1) // 64 * 7).astype(np.uint16)}
    data = cases.pack(info, cols, n)
    _both_calls_and_both_reports(info, data, [n], 9, "step 100")


# ---- forcing the modes per cloud -----------------------------------------------------------------------------------------

def _force_batch():
    """XYZ + ring u16 + stamp u32, five clouds whose best modes differ (one of them fooled in ring, one in stamp)."""
    rs = np.random.RandomState(5)
    fields = [("x", 0, F.FLOAT32, 0.001), ("y", 4, F.FLOAT32, 0.001), ("z", 8, F.FLOAT32, 0.001), ("ring", 12, F.UINT16, None),
              ("stamp", 16, F.UINT32, None)]
    sizes = [40000, 40000, 33000, 0, 5000]
    clouds = []
    for k, n in enumerate(sizes):
        info = cases.make_info(fields, 20, n)
        i = np.arange(n)
        xyz = synth.lidar_xyz(max(n, 1), seed=70 + k)[1].view(np.float32).reshape(-1, 3)[:n]
        if k == 0:
            ring = np.concatenate([np.full(4096, 9), rs.randint(0, 1 << 15, n - 4096)])
            stamp = 1000 + 3 * i
        elif k == 1:
            ring = i % 16
            stamp = np.concatenate([1000 + 3 * i[:4096], rs.randint(0, 1 << 31, n - 4096)])
        elif k == 2:
            ring = (i // 256) % 8
            stamp = rs.randint(0, 5, n) * 1000003
        else:
            ring = rs.randint(0, 64, n)
            stamp = i * 97
        cols = {"x": xyz[:, 0], "y": xyz[:, 1], "z": xyz[:, 2], "ring": ring.astype(np.uint16), "stamp": stamp.astype(np.uint32)}
        clouds.append(cases.pack(info, cols, n))
    return cases.make_info(fields, 20, 1), clouds, sizes


def _decoded(oracle, info, streams, sizes):
    return [oracle.decode_stage1(info, s, n) if n else np.zeros(0, np.uint8) for s, n in zip(streams, sizes)]


def test_force_modes_per_cloud_through_every_encode_entry_point(oracle):
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    info, clouds, sizes = _force_batch()
    flat = np.concatenate(clouds)
    rep = M.sweep(info, flat, sizes)
    best, probe = rep["best_mode"].astype(np.uint8), rep["probe_mode"].astype(np.uint8)
    assert len({tuple(r) for r in best.tolist()}) >= 3 and (best != probe).any(axis=1).sum() >= 2
    saving = [sum(int(rep["bytes"][k, a, probe[k, a]]) - int(rep["bytes"][k, a, best[k, a]]) for a in range(2)) for k in range(len(sizes))]
    assert saving[0] > 10000 and saving[1] > 10000 and saving[3] == 0
    want = [oracle.encode_stage1_continued(info, c, best[k]) if sizes[k] else np.zeros(0, np.uint8) for k, c in enumerate(clouds)]
    points = _decoded(oracle, info, want, sizes)
    fresh = _codec(info).encode_host(clouds)
    assert [s.size for s in want] == [s.size - d for s, d in zip(fresh[0], saving)]                      # the predicted saving, exactly

    codec = _codec(info)
    _same(codec.sweep_modes_host(clouds), rep, "report")
    codec.force_modes_per_cloud(best)

    def agree(streams, what):
        assert [s.tobytes() for s in streams] == [s.tobytes() for s in want], what
    # plain, host
    streams, _cs, modes = codec.encode_host(clouds)
    agree(streams, "plain")
    assert modes.tolist() == best.tolist()
    # the note rules: the mode sweep of the last encode leaves the audit what it was
    audit_alone = codec.audit_last_encode()
    _same(codec.sweep_modes_last_encode(), rep, "last encode")
    assert A.same(codec.audit_last_encode(), audit_alone)
    _same(codec.sweep_modes_last_encode(), rep, "last encode, behind the audit")
    assert [d.tobytes() for d in codec.decode_host(streams, sizes)] == [p.tobytes() for p in points]   # (a decode drops the note)
    # gather
    cp = np.array(sizes, dtype=np.uint64)
    ptrs = (C.c_void_p * len(sizes))(*[c.ctypes.data if c.size else None for c in clouds])
    cap = sum(codec.plan.stage1_bound(s) for s in sizes)
    out, offs = np.zeros(cap, np.uint8), np.zeros(len(sizes) + 1, np.uint64)
    native._check(native.lib().cldn_hip_encode_stage1_gather(codec._h, ptrs, cp.ctypes.data_as(C.POINTER(C.c_uint64)), len(sizes),
                                                             out.ctypes.data_as(C.c_void_p), cap, native.HOST,
                                                             offs.ctypes.data_as(C.c_void_p), None, None))
    agree([out[int(offs[k]):int(offs[k + 1])] for k in range(len(sizes))], "gather")
    # plain, device buffers at an odd address; chunks + frame
    _t, pp, check = _dev(flat, 5)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(len(sizes) + 1, dtype=torch.int64, device=dev)
    d_modes = torch.full((len(sizes) * 2,), 0xEE, dtype=torch.uint8, device=dev)
    for how in ("device", "chunks"):
        d_out.zero_()
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        if how == "device":
            codec.encode_device(pp, sizes, d_out.data_ptr() + 3, cap, d_off.data_ptr(), 0, d_modes.data_ptr())
        else:
            codec.encode_chunks_device(pp, sizes, d_modes.data_ptr())
            _same(codec.sweep_modes_last_encode(), rep, "between the chunk table and its framing")
            codec.frame_chunks_device(d_out.data_ptr() + 3, cap, d_off.data_ptr())
        codec.status()
        o, h = d_off.cpu().numpy(), d_out.cpu().numpy()[3:]
        agree([h[int(o[k]):int(o[k + 1])] for k in range(len(sizes))], how)
        assert d_modes.cpu().numpy().reshape(-1, 2).tolist() == best.tolist(), how
    check()
    # stage 2 on the device: the LZ4 blocks hold the forced streams
    codec.set_stage2(1)
    lz, _cs, modes = codec.encode_host(clouds)
    assert modes.tolist() == best.tolist()
    _same(codec.sweep_modes_last_encode(), rep, "last encode, LZ4")
    assert [d.tobytes() for d in codec.decode_lz4_host(lz, sizes)] == [p.tobytes() for p in points]
    codec.set_stage2(0)
    # viz: the modes apply to the survivors
    step = info.point_step
    survivors = [oracle.viz_preprocess(c, step, 0, 0.05) if c.size else c for c in clouds]
    for gather in (False, True):
        streams, _cs, modes, kept = codec.encode_viz(clouds, 0, 0.05, gather=gather)
        assert [int(k) for k in kept] == [s.size // step for s in survivors] and modes.tolist() == best.tolist()
        for k, s in enumerate(survivors):
            if s.size:
                assert streams[k].tobytes() == oracle.encode_stage1_continued(info, s, best[k]).tobytes(), (k, gather)
        _same(codec.sweep_modes_last_encode(), M.sweep(info, np.concatenate(survivors), [int(k) for k in kept]), "survivors")
    # another cloud count: refused, nothing encoded, by every entry point
    for call in (lambda: codec.encode_host(clouds[:3]), lambda: codec.encode_viz(clouds[:3], 0, 0.05),
                 lambda: codec.encode_device(pp, sizes[:2], d_out.data_ptr(), cap, d_off.data_ptr()),
                 lambda: codec.encode_chunks_device(pp, sizes + [0])):
        with pytest.raises(native.CloudiniHipError) as e:
            call()
        assert e.value.code == -1 and "forced" in e.value.message
    # the two setters replace each other; NULL returns to probing, byte for byte a fresh codec
    codec.force_modes([1, 1])
    s11 = codec.encode_host(clouds[:2])[0]
    assert [s.tobytes() for s in s11] == [oracle.encode_stage1_continued(info, c, [1, 1]).tobytes() for c in clouds[:2]]
    codec.force_modes_per_cloud(best)
    agree(codec.encode_host(clouds)[0], "per cloud again")
    for clear in (lambda: codec.force_modes_per_cloud(None), lambda: codec.force_modes(None)):
        codec.force_modes_per_cloud(best)
        clear()
        streams, _cs, modes = codec.encode_host(clouds[:3])
        assert [s.tobytes() for s in streams] == [s.tobytes() for s in fresh[0][:3]] and modes.tolist() == probe[:3].tolist()
    with pytest.raises(native.CloudiniHipError):
        codec.force_modes_per_cloud(np.full((5, 2), 4, np.uint8))
    with pytest.raises(ValueError):
        codec.force_modes_per_cloud(np.zeros((5, 3), np.uint8))


def test_sweep_modes_last_encode_follows_the_note_rules():
    from cloudini_amd import native
    info, data = cases.header_test_struct(20000)
    codec = _codec(info)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.sweep_modes_last_encode()
    assert e.value.code == -1 and "no encode call to audit" in e.value.message
    want = M.sweep(info, data, [20000])
    codec.encode_host([data])
    audit = codec.audit_last_encode()
    _same(codec.sweep_modes_last_encode(), want)
    assert codec.sweep_last_encode(np.ones((6, 1), np.float32)).shape == (1, 6, 1)
    _same(codec.sweep_modes_last_encode(), want, "behind the resolution sweep")
    assert A.same(codec.audit_last_encode(), audit)
    codec.sweep_modes_host([data])                                              # takes buffers: drops the note
    with pytest.raises(native.CloudiniHipError):
        codec.sweep_modes_last_encode()
    _t, p, _c = _dev(data)
    read, pr = _dev_report(1, 2)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.sweep_modes_device(p, [20000], report_ptr=pr + 4)
    assert e.value.code == -1
    with pytest.raises(native.CloudiniHipError):
        codec.sweep_modes_device(p, [20000], points_loc=2)
    assert (read().view(np.uint8) == 0xEE).all()                                # refused calls wrote nothing
