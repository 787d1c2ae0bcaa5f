"""Resolution sweep on the device (cloudini_amd/csrc/sweep_kernels.hip): cldn_hip_sweep_clouds, cldn_hip_sweep_last_encode.

Expected reports never come from the code under test: they are tests/sweep_model.py on the same points (the model itself is
held against the oracle and the reference in tests/test_sweep_model.py). Every comparison is exact, cell for cell,
max_abs_err by its bits."""
import ctypes as C

import numpy as np
import pytest

import audit_model as A
import cases
import sweep_model as S
from cloudini_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5
CELL = 32


def _codec(info):
    from cloudini_amd import native
    return native.Codec(native.Plan(info))


def _same(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if not S.same(got, want):
        bad = [(idx, tuple(got[idx]), tuple(want[idx])) for idx in np.ndindex(got.shape) if got[idx].tobytes() != want[idx].tobytes()]
        raise AssertionError(f"{what}: {len(bad)} cells differ, first (cloud, field, candidate), got, want: {bad[:4]}")


def _zero(cells):
    return not np.ascontiguousarray(cells).view(np.uint8).any()


def _dev(arr, residue=0):
    """A device copy of `arr` that starts `residue` (< 16) bytes behind a 256-byte boundary, between two guard spans. Returns
    (tensor, pointer, check) -- check() asserts that guards and content are as they were."""
    import torch
    dev = torch.device("cuda", 0)
    arr = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = torch.full((256 + GUARD + 16 + arr.size + GUARD,), FILL, dtype=torch.uint8, device=dev)
    base = (-t.data_ptr()) % 256 + GUARD + residue
    if arr.size:
        t[base:base + arr.size] = torch.from_numpy(arr.copy()).to(dev)
    before = t.cpu().numpy().copy()

    def check():
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), before), "a buffer the sweep may only read has changed"
    return t, t.data_ptr() + base, check


def _dev_report(n_clouds, n_fields, n_candidates):
    """A device report between guard spans, pre-filled; returns (read, pointer): read() checks the guards and returns it."""
    import torch
    dev = torch.device("cuda", 0)
    nbytes = n_clouds * n_fields * n_candidates * CELL
    t = torch.full((256 + GUARD + nbytes + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    base = (-t.data_ptr()) % 256 + GUARD
    torch.cuda.synchronize()  # the codec works on a stream of its own: the fill lands before a call writes the report

    def read():
        torch.cuda.synchronize()
        h = t.cpu().numpy()
        assert (h[:base] == 0xEE).all() and (h[base + nbytes:] == 0xEE).all(), "the sweep wrote outside its report"
        return h[base:base + nbytes].copy().view(S.DTYPE).reshape(n_clouds, n_fields, n_candidates)
    return read, t.data_ptr() + base


def _cut(info, data, sizes):
    step = info.point_step
    ends = np.cumsum(sizes)
    return [data[(e - n) * step:e * step].copy() for n, e in zip(sizes, ends)]


# ---- every schema family against the model -----------------------------------------------------------------------------

FAMILIES = cases.encode_cases(small=True)


def _case(name):
    for nm, info, data in FAMILIES:
        if nm == name:
            return info, data
    raise KeyError(name)


@pytest.mark.parametrize("name,info,data", FAMILIES, ids=[c[0] for c in FAMILIES])
def test_sweep_equals_the_model_on_every_schema_family(name, info, data):
    n = data.size // info.point_step
    ladders = S.default_ladders(info)
    want = S.sweep(info, data, [n], ladders)
    got = _codec(info).sweep_clouds_host([data], ladders)
    _same(got, want, name)
    kinds = S.field_kinds(info)
    for f, kind in enumerate(kinds):
        if kind == S.NONE:
            assert _zero(got[:, f]), (name, f)
        else:
            assert (got["bytes"][0, f] >= n).all(), (name, f)        # at least one byte per point and rung


SPECIALS = ["float_specials3", "float_specials4", "region_overflow3", "region_overflow4", "region_overflow3_u16",
            "region_overflow3_u16_unaligned", "region_overflow4_unaligned", "five_floats"]


@pytest.mark.parametrize("name", SPECIALS)
def test_special_values_exercise_both_error_columns(name):
    """Sentinels (+-inf, +-3e9 m and 2.0e6 m at sub-millimetre rungs), +-inf decoded to finite values, exact half ticks (the
    FloatN group rounds to even, the scalar encoder away from zero). five_floats holds +inf (class) but nothing beyond the
    tick range of its int64 encoder, and its values stay within metres: no error over a rung is possible there, so only the
    class column is demanded of it."""
    info, data = _case(name)
    n = data.size // info.point_step
    sizes = [n // 2, 0, n - n // 2]
    ladders = S.default_ladders(info)
    want = S.sweep(info, data, sizes, ladders)
    assert want["n_class_diff"].sum() > 0, name
    if name != "five_floats":
        assert want["n_over_limit"].sum() > 0, name
    codec = _codec(info)
    _same(codec.sweep_clouds_host(_cut(info, data, sizes), ladders), want, name)
    _t, p, check = _dev(data, 3)
    read, pr = _dev_report(3, len(info.fields), ladders.shape[1])
    assert codec.sweep_clouds_device(p, sizes, ladders, report_ptr=pr) is None
    _same(read(), want, name + " device")
    check()


# ---- chunk and block edges ---------------------------------------------------------------------------------------------

EDGE_SIZES = [0, 1, 2, 1023, 0, 1024, 1025, 32767, 32768, 32769, 0, 65537]


def _edge_batch():
    info, data = synth.lidar_xyzi(sum(EDGE_SIZES), seed=5)
    clouds = _cut(info, data, EDGE_SIZES)
    k_nan, k_jump = EDGE_SIZES.index(65537), EDGE_SIZES.index(32769)
    xyz = clouds[k_nan].view("<f4").reshape(-1, 4)
    for lane, p in enumerate((1023, 1024, 32767, 32768)):
        xyz[p, lane % 3] = np.nan
    xyz[32768, 2] = np.nan                                            # two lanes of the chunk's first point
    jump = clouds[k_jump].view("<f4").reshape(-1, 4)
    jump[32768:, :3] += np.float32(7.25)                              # metres between points 32767 and 32768
    return info, clouds, k_jump


def test_chunk_and_block_edges_in_one_ragged_batch(monkeypatch):
    info, clouds, k_jump = _edge_batch()
    ladders = S.default_ladders(info)
    flat = np.concatenate(clouds)
    want = S.sweep(info, flat, EDGE_SIZES, ladders)
    # the case bites: a reference taken across the chunk edge would give other byte counts for the jumping cloud
    monkeypatch.setattr(S, "CHUNK", 1 << 40)
    across = S.sweep(info, flat, EDGE_SIZES, ladders)
    monkeypatch.undo()
    assert (across["bytes"][k_jump, :3] != want["bytes"][k_jump, :3]).any(axis=1).all()
    for k, n in enumerate(EDGE_SIZES):
        assert _zero(want[k]) == (n == 0)
    codec = _codec(info)
    _same(codec.sweep_clouds_host(clouds, ladders), want)
    _t, p, check = _dev(flat, 9)
    read, pr = _dev_report(len(EDGE_SIZES), 4, ladders.shape[1])
    codec.sweep_clouds_device(p, EDGE_SIZES, ladders, report_ptr=pr)
    _same(read(), want, "device")
    check()
    # all clouds empty, and no cloud at all
    assert _zero(codec.sweep_clouds_host([flat[:0]] * 3, ladders)) and codec.sweep_clouds_host([], ladders).shape == (0, 4, 5)


# ---- addresses, wide inputs --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("schema", ["xyzi", "step19_odd", "mixed47"])
def test_device_input_at_odd_addresses_against_the_host_call(schema):
    if schema == "xyzi":
        info, data = synth.lidar_xyzi(5000)
    elif schema == "mixed47":
        info, data = cases.mixed_schema(5000)
    else:
        info, data = [(i, d[:5000 * 19].copy()) for nm, i, d in cases.stride_variants() if nm == schema][0]
    sizes = [1500, 0, 2477, 1023]
    ladders = S.default_ladders(info)
    codec = _codec(info)
    host = codec.sweep_clouds_host(_cut(info, data, sizes), ladders)
    _same(host, S.sweep(info, data, sizes, ladders), schema)
    for residue in (1, 7):
        _t, p, check = _dev(data, residue)
        read, pr = _dev_report(len(sizes), len(info.fields), ladders.shape[1])
        assert codec.sweep_clouds_device(p, sizes, ladders, report_ptr=pr) is None
        _same(read(), host, f"{schema} residue {residue}")
        _same(codec.sweep_clouds_device(p, sizes, ladders), host, f"{schema} residue {residue}, host report")
        check()


@pytest.mark.parametrize("name", ["step200", "very_wide_9002", "very_wide_9015"])
def test_wide_points_and_more_than_128_fields(name):
    if name == "step200":
        info, data = _case(name)
    else:
        info, data = cases.very_wide_schema(int(name[-4:]))
        assert len(info.fields) > 128
    assert info.point_step >= 128
    kinds = S.field_kinds(info)
    assert sum(k != S.NONE for k in kinds) >= 3
    n = data.size // info.point_step
    sizes = [n // 3, 0, n - n // 3]
    ladders = S.default_ladders(info)
    want = S.sweep(info, data, sizes, ladders)
    codec = _codec(info)
    _same(codec.sweep_clouds_host(_cut(info, data, sizes), ladders), want, name)
    _t, p, check = _dev(data, 5)
    read, pr = _dev_report(3, len(info.fields), ladders.shape[1])
    codec.sweep_clouds_device(p, sizes, ladders, report_ptr=pr)
    _same(read(), want, name + " device")
    check()


# ---- ladders -----------------------------------------------------------------------------------------------------------

def test_skipped_rungs_and_one_and_sixteen_candidates():
    info, data = cases.mixed_schema(3000)
    n = 3000
    codec = _codec(info)
    rs = np.random.RandomState(4)
    base = np.array([1.0 if f.resolution is None else f.resolution for f in info.fields], dtype=np.float64)
    for n_cand in (1, 16):
        ladders = (base[:, None] * rs.uniform(0.2, 20.0, (len(base), n_cand))).astype(np.float32)
        _same(codec.sweep_clouds_host([data], ladders), S.sweep(info, data, [n], ladders), n_cand)
    ladders[:, [3, 4, 9]] = 0.0                                       # skipped in the middle
    ladders[1, :] = 0.0                                               # a whole field skipped
    got = codec.sweep_clouds_host([data], ladders)
    _same(got, S.sweep(info, data, [n], ladders), "skips")
    assert _zero(got[:, :, [3, 4, 9]]) and _zero(got[:, 1]) and not _zero(got[:, 0, 5])
    # the ladder of a field that is not sweepable is ignored, whatever it holds
    ladders[3, :] = np.nan
    ladders[4, :] = -1.0
    _same(codec.sweep_clouds_host([data], ladders), got, "ignored ladders")


# ---- agreement with real encodes on the device -------------------------------------------------------------------------

def test_cells_at_the_plan_resolutions_add_up_to_the_encoded_streams():
    info, data = synth.lidar_xyz(100000)
    sizes = [40000, 0, 32768, 27232]
    clouds = _cut(info, data, sizes)
    codec = _codec(info)
    streams, _cs, _m = codec.encode_host(clouds)
    ladders = np.array([[f.resolution] for f in info.fields], dtype=np.float32)
    rep = codec.sweep_clouds_host(clouds, ladders)
    for k, n in enumerate(sizes):
        assert int(rep["bytes"][k, :, 0].sum()) + 4 * ((n + 32767) // 32768) == streams[k].size, k


def test_the_difference_of_two_plans_is_the_difference_of_their_cells():
    info1, data = synth.lidar_xyzi(100000, res=0.001)
    info5, data5 = synth.lidar_xyzi(100000, res=0.005)
    assert data.tobytes() == data5.tobytes()
    sizes = [60000, 40000]
    clouds = _cut(info1, data, sizes)
    s1 = _codec(info1).encode_host(clouds)[0]
    s5 = _codec(info5).encode_host(clouds)[0]
    ladders = np.zeros((len(info1.fields), 2), dtype=np.float32)
    swept = [f for f, kind in enumerate(S.field_kinds(info1)) if kind != S.NONE]
    assert len(swept) == 3
    ladders[swept] = [0.001, 0.005]
    rep = _codec(info1).sweep_clouds_host(clouds, ladders)
    for k in range(2):
        cells = sum(int(rep["bytes"][k, f, 1]) - int(rep["bytes"][k, f, 0]) for f in swept)
        assert s5[k].size - s1[k].size == cells and cells < 0, k


# ---- sweep_last_encode -------------------------------------------------------------------------------------------------

def _audit_want(oracle, info, clouds):
    step = info.point_step
    dec = [oracle.decode_stage1(info, oracle.encode_stage1(info, c), c.size // step) if c.size else c for c in clouds]
    return A.audit(info, np.concatenate(clouds), np.concatenate(dec), [c.size // step for c in clouds])


def _audit_same(got, want):
    assert A.same(got, want), "audit_last_encode behind a sweep no longer returns its report"


@pytest.mark.parametrize("name", ["c4_velodyne", "mixed_v5"])
def test_sweep_last_encode_after_encode_host_and_gather(oracle, name):
    from cloudini_amd import native
    info, data = _case(name)
    n = min(70000, data.size // info.point_step)
    sizes = [n // 2, 0, n - n // 2]
    clouds = _cut(info, data, sizes)
    ladders = S.default_ladders(info)
    codec = _codec(info)
    want = codec.sweep_clouds_host(clouds, ladders)
    _same(want, S.sweep(info, np.concatenate(clouds), sizes, ladders), name)
    audit_want = _audit_want(oracle, info, clouds)
    codec.encode_host(clouds)
    _same(codec.sweep_last_encode(ladders), want, name)
    _same(codec.sweep_last_encode(ladders[:, :2]), want[:, :, :2], name + " repeated, other ladder")
    read, pr = _dev_report(3, len(info.fields), ladders.shape[1])
    assert codec.sweep_last_encode(ladders, report_ptr=pr) is None
    _same(read(), want, name + " device report")
    _audit_same(codec.audit_last_encode(), audit_want)
    _same(codec.sweep_last_encode(ladders), want, name + " behind the audit")
    # one host buffer per cloud
    cp = np.array(sizes, dtype=np.uint64)
    ptrs = (C.c_void_p * 3)(*[c.ctypes.data if c.size else None for c in clouds])
    cap = sum(codec.plan.stage1_bound(s) for s in sizes)
    out, offs = np.zeros(cap, np.uint8), np.zeros(4, np.uint64)
    native._check(native.lib().cldn_hip_encode_stage1_gather(codec._h, ptrs, cp.ctypes.data_as(C.POINTER(C.c_uint64)), 3,
                                                             out.ctypes.data_as(C.c_void_p), cap, native.HOST,
                                                             offs.ctypes.data_as(C.c_void_p), None, None))
    _same(codec.sweep_last_encode(ladders), want, name + " gather")
    _audit_same(codec.audit_last_encode(), audit_want)


@pytest.mark.parametrize("residue", [0, 7])
def test_sweep_last_encode_after_encode_device(oracle, residue):
    import torch
    dev = torch.device("cuda", 0)
    info, data = synth.velodyne_xyzir(60000)
    sizes = [30000, 30000]
    clouds = _cut(info, data, sizes)
    ladders = S.default_ladders(info)
    codec = _codec(info)
    cap = sum(codec.plan.stage1_bound(n) for n in sizes)
    _tp, pp, check_p = _dev(data, residue)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.encode_device(pp, sizes, d_out.data_ptr() + residue, cap, d_off.data_ptr())
    got = codec.sweep_last_encode(ladders)
    _same(got, S.sweep(info, data, sizes, ladders))
    _audit_same(codec.audit_last_encode(), _audit_want(oracle, info, clouds))
    check_p()


def test_sweep_last_encode_between_the_chunk_table_and_its_framing(oracle):
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    info, data = synth.lidar_xyzi(70000)
    ladders = S.default_ladders(info)
    codec = _codec(info)
    _tp, pp, check_p = _dev(data)
    codec.encode_chunks_device(pp, [70000])
    want = S.sweep(info, data, [70000], ladders)
    _same(codec.sweep_last_encode(ladders), want)                     # not framed yet: the points are all it needs
    with pytest.raises(native.CloudiniHipError):
        codec.audit_last_encode()                                     # the audit still waits for the framing
    cap = codec.plan.stage1_bound(70000)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.frame_chunks_device(d_out.data_ptr(), cap, d_off.data_ptr())
    stream = d_out.cpu().numpy()[:int(d_off.cpu().numpy()[1])]
    assert stream.tobytes() == oracle.encode_stage1(info, data).tobytes()   # the sweep in between disturbed nothing
    _same(codec.sweep_last_encode(ladders), want)
    _audit_same(codec.audit_last_encode(), _audit_want(oracle, info, [data]))
    check_p()


@pytest.mark.parametrize("gather", [False, True])
def test_sweep_last_encode_after_encode_viz_sweeps_the_survivors(oracle, gather):
    info, data = synth.velodyne_xyzir(50000)
    step = info.point_step
    clouds = _cut(info, data, [15000, 0, 35000])
    clouds[0].view("<f4")[0] = np.nan                                 # dropped by the filter
    ladders = S.default_ladders(info)
    codec = _codec(info)
    _streams, _cs, _m, kept = codec.encode_viz(clouds, 0, 0.05, gather=gather)
    got = codec.sweep_last_encode(ladders)
    survivors = [oracle.viz_preprocess(c, step, 0, 0.05) if c.size else c for c in clouds]
    assert [s.size // step for s in survivors] == [int(k) for k in kept] and 0 < int(kept.sum()) < 50000
    _same(got, S.sweep(info, np.concatenate(survivors), [int(k) for k in kept], ladders))
    _audit_same(codec.audit_last_encode(), _audit_want(oracle, info, survivors))


def test_sweep_last_encode_is_refused_without_an_encode_and_after_other_calls():
    from cloudini_amd import native
    info, data = synth.lidar_xyzi(20000)
    ladders = S.default_ladders(info)
    codec = _codec(info)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.sweep_last_encode(ladders)
    assert e.value.code == -1 and "no encode call to audit" in e.value.message
    with pytest.raises(native.CloudiniHipError) as e2:
        codec.audit_last_encode()
    assert e2.value.message.split(":", 1)[1] == e.value.message.split(":", 1)[1]     # the audit's wording
    streams, _s, _m = codec.encode_host([data])
    codec.synchronize()
    codec.status()                                                    # queries leave the state
    assert codec.sweep_last_encode(ladders).shape == (1, 4, 5)
    for intervening in (lambda: codec.decode_host(streams, [20000]),
                        lambda: codec.sweep_clouds_host([data], ladders),
                        lambda: codec.audit_clouds_host([data], [data])):
        codec.encode_host([data])
        intervening()
        for call in (lambda: codec.sweep_last_encode(ladders), codec.audit_last_encode):
            with pytest.raises(native.CloudiniHipError) as e:
                call()
            assert e.value.code == -1 and "no encode call to audit" in e.value.message


# ---- argument errors ---------------------------------------------------------------------------------------------------

def test_arguments():
    from cloudini_amd import native
    info, data = synth.lidar_xyzi(1000)
    codec = _codec(info)
    good = S.default_ladders(info)
    want = S.sweep(info, data, [1000], good)
    for bad in (-0.001, np.nan, np.inf, -np.inf, 1e-45, 2.0e-39):   # negative, NaN, inf; a reciprocal of inf (subnormal rungs)
        ladders = good.copy()
        ladders[1, 2] = np.float32(bad)
        with pytest.raises(ValueError):
            S.check_ladders(info, ladders)
        with pytest.raises(native.CloudiniHipError) as e:
            codec.sweep_clouds_host([data], ladders)
        assert e.value.code == -1, bad
        ladders[1, 2] = good[1, 2]
        ladders[3, 2] = np.float32(bad)                               # the u16 field: its ladder is ignored
        _same(codec.sweep_clouds_host([data], ladders), want, bad)
    for n_cand in (0, 17):
        with pytest.raises(native.CloudiniHipError) as e:
            codec.sweep_clouds_host([data], np.ones((4, n_cand), np.float32))
        assert e.value.code == -1, n_cand
    _t, p, _c = _dev(data)
    read, pr = _dev_report(1, 4, 5)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.sweep_clouds_device(p, [1000], good, report_ptr=pr + 4)
    assert e.value.code == -1
    with pytest.raises(native.CloudiniHipError) as e:
        codec.sweep_clouds_device(p, [1000], good, points_loc=2)
    assert e.value.code == -1
    assert (read().view(np.uint8) == 0xEE).all()                      # refused calls wrote nothing
    codec.encode_host([data])
    for n_cand in (0, 17):
        with pytest.raises(native.CloudiniHipError) as e:
            codec.sweep_last_encode(np.ones((4, n_cand), np.float32))
        assert e.value.code == -1, n_cand
    _same(codec.sweep_last_encode(good), want)                        # a refused sweep leaves the state too


# ---- the value grid (tests/value_grid_cases.py): rounding, range and 2^21 edges, each field at res, res / 2 and 2 res -----------------
import value_grid_cases as VG  # noqa: E402


REPORT_GROUPS = VG.report_groups()


def value_grid_batches(cs):
    """[(info, clouds, ladders)]: the clouds of the group, one batch per resolution"""
    by_res = {}
    for c in cs:
        by_res.setdefault(c.res, []).append(c)
    out = []
    for res, group in by_res.items():
        info = group[0].info()
        out.append((info, [c.cloud() for c in group], S.default_ladders(info, (1.0, 0.5, 2.0))))
    return out


@pytest.mark.parametrize("name,cs", REPORT_GROUPS, ids=[g[0] for g in REPORT_GROUPS])
def test_sweep_equals_the_model_on_the_value_grid(name, cs):
    for info, clouds, ladders in value_grid_batches(cs):
        sizes = [c.size // info.point_step for c in clouds]
        want = S.sweep(info, np.concatenate(clouds), sizes, ladders)
        codec = _codec(info)
        _same(codec.sweep_clouds_host(clouds, ladders), want, name)
        codec.close()
