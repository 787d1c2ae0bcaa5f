"""Byte histograms on the device (cloudini_amd/csrc/hist_kernels.hip): cldn_hip_sweep_hist_clouds, cldn_hip_stream_hist and
their _last_encode forms.

Expected reports never come from the code under test: they are tests/hist_model.py on the same points (held against the oracle
and the reference in tests/test_hist_model.py) and numpy's bincount of the fetched streams. Every comparison is exact, bin for
bin. Each sweep case runs with host buffers, device resident at odd addresses, and with workgroups that walk 1, 3 and the
default number of blocks: 3 divides neither a chunk's 32 blocks nor any cloud here, so walks cross cloud and chunk edges."""
import numpy as np
import pytest

import audit_model as A
import cases
import hist_model as H
import sweep_model as S
from cloudini_amd import synth

pytestmark = pytest.mark.gpu

GUARD = 256
HIST = 2048


def _codec(info):
    from cloudini_amd import native
    return native.Codec(native.Plan(info))


def _same(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint64, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bins differ, first (index..., bin), got, want: "
                             f"{[(tuple(b), int(got[tuple(b)]), int(want[tuple(b)])) for b in bad[:4]]}")


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
        assert np.array_equal(t.cpu().numpy(), before), "a buffer the call may only read has changed"
    return t, t.data_ptr() + base, check


def _dev_report(*shape):
    """A device report 8 bytes behind a 256-byte boundary (8-byte aligned, nothing more) between guard spans, pre-filled;
    returns (read, pointer): read() checks the guards and returns the report."""
    import torch
    dev = torch.device("cuda", 0)
    nbytes = int(np.prod(shape)) * HIST
    t = torch.full((256 + GUARD + 8 + nbytes + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    base = (-t.data_ptr()) % 256 + GUARD + 8
    torch.cuda.synchronize()  # the codec works on a stream of its own: the fill lands before a call writes the report

    def read():
        torch.cuda.synchronize()
        h = t.cpu().numpy()
        assert (h[:base] == 0xEE).all() and (h[base + nbytes:] == 0xEE).all(), "the call wrote outside its report"
        return h[base:base + nbytes].copy().view(np.uint64).reshape(tuple(shape) + (256,))
    return read, t.data_ptr() + base


def _cut(info, data, sizes):
    step = info.point_step
    ends = np.cumsum(sizes)
    return [data[(e - n) * step:e * step].copy() for n, e in zip(sizes, ends)]


def _column_view(cloud, info, f):
    """Writable strided view of field f of a cloud (a float32 or float64 field; any offset and step)."""
    field = info.fields[f]
    dt = "<f8" if S.field_kinds(info)[f] == S.SCALAR64 else "<f4"
    size = np.dtype(dt).itemsize
    n = cloud.size // info.point_step
    return np.ndarray((n,), dtype=dt, buffer=cloud.data, offset=field.offset, strides=(info.point_step,)) if n else np.zeros(0, dt), size


def _spice(cloud, info, f, r, at):
    """From point `at` on: deltas of every token length of the field's kind (1..5 bytes in the FloatN group, 1..10 in the int64
    kinds: the bins >= 0x80 and the top group fill), +-inf, a value whose tick count is beyond the kind's integer, a NaN run."""
    col, _ = _column_view(cloud, info, f)
    kind = S.field_kinds(info)[f]
    top = 5 if kind == S.FLOATN else 10
    vals = []
    for k in range(top):
        vals += [0.0, float(2.0 ** (7 * k)) * r * (1 if k % 2 else -1)]
    vals += [np.inf, 0.25, -np.inf, 3.0e9 if kind == S.FLOATN else 1.0e30, 0.5, np.nan, np.nan, np.nan, 1.0]
    if at + len(vals) <= col.size:
        col[at:at + len(vals)] = np.array(vals, dtype=np.float64).astype(col.dtype)


def _run(info, clouds, ladders, what, walks=(0, 1, 3)):
    sizes = [c.size // info.point_step for c in clouds]
    flat = np.concatenate(clouds) if clouds else np.zeros(0, np.uint8)
    want = H.sweep_hist(info, flat, sizes, ladders)
    assert np.array_equal(want.sum(axis=3), S.sweep(info, flat, sizes, ladders)["bytes"])
    codec = _codec(info)
    _t, p, check = _dev(flat, 3)
    for walk in walks:
        codec.hist_walk(walk)
        _same(codec.sweep_hist_clouds_host(clouds, ladders), want, f"{what}, host, walk {walk}")
        read, pr = _dev_report(len(sizes), len(info.fields), ladders.shape[1])
        assert codec.sweep_hist_clouds_device(p, sizes, ladders, report_ptr=pr) is None
        _same(read(), want, f"{what}, device, walk {walk}")
    _same(codec.sweep_hist_clouds_device(p, sizes, ladders), want, f"{what}, device points, host report")
    check()
    return want


# ---- edges of blocks, chunks and clouds in one ragged batch ------------------------------------------------------------

EDGE_SIZES = [0, 1, 1023, 1024, 1025, 32767, 32768, 32769, 70001, 1025, 1025]


def _edge_batch():
    info, data = synth.lidar_xyzi(sum(EDGE_SIZES), seed=5)
    clouds = _cut(info, data, EDGE_SIZES)
    clouds[-1] = clouds[-2].copy()                                    # the same cloud twice in a row
    big = clouds[EDGE_SIZES.index(70001)]
    for f in range(3):
        _spice(big, info, f, 0.001, 100 + 40 * f)
        _spice(big, info, f, 0.001, 32768 - 12 - f)                   # across the chunk edge
        _spice(big, info, f, 0.001, 65536 + 5000)
    xyz = big.view("<f4").reshape(-1, 4)
    xyz[32760:32768, 0] = np.nan                                      # a NaN run that ends a chunk
    xyz[65535, 1] = np.nan
    xyz[65536, 2] = np.nan                                            # and one that starts one
    _spice(clouds[EDGE_SIZES.index(1025)], info, 1, 0.001, 1000)      # across the block edge
    return info, clouds


def test_ragged_batch_with_every_token_length_nans_and_infinities():
    info, clouds = _edge_batch()
    ladders = S.default_ladders(info)
    want = _run(info, clouds, ladders, "edges")
    for k, n in enumerate(EDGE_SIZES):
        assert want[k].any() == (n != 0)
    big = want[EDGE_SIZES.index(70001)]
    assert (big[:3, 0, 0x80:].sum(axis=1) > 0).all() and big[0, 0, 0] >= 8     # continuation bytes; the NaN markers
    assert not want[:, 3].any()                                                  # the u16 intensity is not sweepable
    _same(want[-1], want[-2], "the twin clouds")
    # all clouds empty, and no cloud at all
    codec = _codec(info)
    assert not codec.sweep_hist_clouds_host([clouds[0]] * 3, ladders).any()
    assert codec.sweep_hist_clouds_host([], ladders).shape == (0, 4, 5, 256)


# ---- schemas: odd stride, FLOAT64, int64 kinds, the direct route, the device field table ------------------------------

def _family(name):
    for nm, info, data in cases.encode_cases(small=True):
        if nm == name:
            return info, data
    raise KeyError(name)


def test_velodyne_odd_stride_staged():
    info, data = synth.velodyne_xyzir(36000)
    assert info.point_step % 4 != 0 and info.point_step <= 127
    clouds = _cut(info, data, [1500, 0, 33000, 1500])
    for f, kind in enumerate(S.field_kinds(info)):
        if kind != S.NONE:
            _spice(clouds[2], info, f, float(info.fields[f].resolution), 32768 - 9)
    _run(info, clouds, S.default_ladders(info), "velodyne")


def test_float64_and_scalar32_fields_fill_ten_byte_tokens():
    """mixed_schema: a FloatN group, a scalar float32 (`temp`) and a lossy FLOAT64 (`stamp`) with integer fields between them."""
    info, data = cases.mixed_schema(6000)
    kinds = S.field_kinds(info)
    assert S.SCALAR32 in kinds and S.SCALAR64 in kinds
    first, last = kinds.index(S.FLOATN), len(kinds) - 1 - kinds[::-1].index(S.SCALAR64)
    assert S.NONE in kinds[first:last]                                # a field that is not sweepable between two that are
    clouds = _cut(info, data, [3500, 2500])
    for f, kind in enumerate(kinds):
        if kind != S.NONE:
            _spice(clouds[0], info, f, float(info.fields[f].resolution), 1020)
    want = _run(info, clouds, S.default_ladders(info), "mixed")
    for f, kind in enumerate(kinds):
        assert want[:, f].any() == (kind != S.NONE)


def test_int64_kinds_on_constructed_columns():
    """Five float32 fields (no FloatN group: all scalar, int64 deltas) and one FLOAT64, 28-byte points: every token length
    1..10, +-inf and tick counts beyond int64 in both kinds."""
    F = cases.F
    fields = [(c, 4 * k, F.FLOAT32, 0.01) for k, c in enumerate("abcde")] + [("t", 20, F.FLOAT64, 1e-6)]
    n = 2600
    info = cases.make_info(fields, 28, n)
    rs = np.random.RandomState(3)
    rows = np.zeros((n, 28), dtype=np.uint8)
    for k in range(5):
        rows[:, 4 * k:4 * k + 4] = rs.normal(0, 3, n).astype("<f4").view(np.uint8).reshape(n, 4)
    t = np.cumsum(rs.uniform(0, 1e-3, n))
    for k in range(5):
        v = rows[:, 4 * k:4 * k + 4].copy().view("<f4").reshape(-1)
        top = [0.0, 1.0e30, np.inf, -np.inf, np.nan] + [float(2.0 ** (7 * j)) * 0.01 * (-1) ** j for j in range(10)]
        v[1019 + k:1019 + k + len(top)] = np.array(top, dtype=np.float32)
        rows[:, 4 * k:4 * k + 4] = v.view(np.uint8).reshape(n, 4)
    top = [0.0, 1.0e300, np.inf, np.nan, -np.inf] + [float(2.0 ** (7 * j)) * 1e-6 * (-1) ** j for j in range(10)] + [np.nan] * 3
    t[1015:1015 + len(top)] = top
    rows[:, 20:28] = t.astype("<f8").view(np.uint8).reshape(n, 8)
    data = rows.reshape(-1)
    assert S.field_kinds(info) == [S.SCALAR32] * 5 + [S.SCALAR64]
    want = _run(info, _cut(info, data, [1500, 1100]), S.default_ladders(info), "int64 kinds")
    assert (want[0, :, 0, 0x80:].sum(axis=1) >= 45).all()             # 1 + 2 + ... + 9 continuation bytes at least


@pytest.mark.parametrize("name", ["step200", "very_wide_9002"])
def test_direct_route_and_device_field_table(name):
    if name == "step200":
        info, data = _family(name)
    else:
        info, data = cases.very_wide_schema(9002)
        assert len(info.fields) > 128
    assert info.point_step >= 128
    n = data.size // info.point_step
    sizes = [n // 3, 0, n - n // 3]
    ladders = S.default_ladders(info)[:, :2]
    want = _run(info, _cut(info, data, sizes), ladders, name, walks=(0, 3))
    assert sum(k != S.NONE for k in S.field_kinds(info)) >= 3 and want.any()


def test_ladders_of_one_and_sixteen_rungs_and_skipped_rungs():
    info, data = cases.mixed_schema(3000)
    rs = np.random.RandomState(4)
    base = np.array([1.0 if f.resolution is None else f.resolution for f in info.fields], dtype=np.float64)
    for n_cand in (1, 16):
        ladders = (base[:, None] * rs.uniform(0.2, 20.0, (len(base), n_cand))).astype(np.float32)
        _run(info, [data], ladders, f"{n_cand} rungs", walks=(0,))
    ladders[:, [3, 4, 9]] = 0.0                                       # skipped in the middle
    ladders[1, :] = 0.0                                               # a whole field skipped
    got = _run(info, [data], ladders, "skips", walks=(0, 3))
    assert not got[:, :, [3, 4, 9]].any() and not got[:, 1].any() and got[:, 0, 5].any()
    ladders[3, :] = np.nan                                            # the ladder of a field that is not sweepable is ignored
    ladders[4, :] = -1.0
    _same(_codec(info).sweep_hist_clouds_host([data], ladders), got, "ignored ladders")


# ---- stream_hist -------------------------------------------------------------------------------------------------------

def _streams():
    rs = np.random.RandomState(11)
    skew = rs.choice(np.array([1, 1, 1, 1, 2, 2, 3, 0x81, 0xFF, 0], dtype=np.uint8), 300001)   # three workgroups
    return [rs.randint(0, 256, 131072 + 40000).astype(np.uint8), np.zeros(0, np.uint8), skew, rs.randint(0, 256, 1).astype(np.uint8),
            rs.randint(0, 256, 15).astype(np.uint8), np.zeros(0, np.uint8), rs.randint(0, 256, 131072 + 17).astype(np.uint8),
            rs.randint(0, 256, 33).astype(np.uint8)]


def test_stream_hist_at_every_residue_and_for_empty_streams():
    info, _ = synth.lidar_xyzi(16)
    codec = _codec(info)
    streams = _streams()
    want = H.stream_hist(streams)
    assert want[2, 1] > 20000 and not want[1].any()
    _same(codec.stream_hist_host(streams), want, "host")
    offs = np.zeros(len(streams) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([s.size for s in streams])
    flat = np.concatenate(streams)
    assert len({int(o) % 16 for o in offs}) >= 4
    for residue in range(16):
        _t, p, check = _dev(flat, residue)
        read, pr = _dev_report(len(streams))
        assert codec.stream_hist_device(p, offs, report_ptr=pr) is None
        _same(read(), want, f"residue {residue}")
        check()
    # offsets need not start at 0: a window of the same buffer
    _t, p, check = _dev(flat, 5)
    _same(codec.stream_hist_device(p, offs[2:5]), want[2:4], "window")
    assert codec.stream_hist_host([]).shape == (0, 256) and not codec.stream_hist_host([flat[:0]] * 2).any()
    check()


# ---- both identities on device reports, behind encode_stage1 and behind the viz encode ---------------------------------

def _own(info):
    return np.array([[1.0 if f.resolution is None else f.resolution] for f in info.fields], dtype=np.float32)


@pytest.mark.parametrize("viz", [False, True], ids=["encode_stage1", "encode_viz"])
def test_sum_of_field_histograms_plus_prefixes_is_the_stream_histogram(viz):
    info, data = synth.lidar_xyz(100000)
    clouds = _cut(info, data, [40000, 0, 32768, 27232])
    codec = _codec(info)
    streams = codec.encode_viz(clouds, 0, 0.05)[0] if viz else codec.encode_host(clouds)[0]
    fields = codec.sweep_hist_last_encode(_own(info))
    whole = codec.stream_hist_last_encode()
    _same(whole, H.stream_hist(streams), "stream_hist_last_encode")
    for k, s in enumerate(streams):
        _same(fields[k, :, 0].sum(axis=0) + H.prefix_hist(s), whole[k], f"cloud {k}")
    assert whole[0].any() and not whole[1].any()


@pytest.mark.parametrize("viz", [False, True], ids=["encode_stage1", "encode_viz"])
def test_moving_the_fields_moves_the_stream_histogram_by_their_difference(viz):
    """Velodyne xyzir: the ring section and the raw intensity stay. The [u32] prefixes spell the payload sizes, which move with
    the fields: they are taken out on both sides (header: the identity is one of payload bytes)."""
    info1, data = synth.velodyne_xyzir(70000, res=0.001)
    info5, data5 = synth.velodyne_xyzir(70000, res=0.005)
    assert data.tobytes() == data5.tobytes()
    clouds = _cut(info1, data, [37000, 33000])
    swept = [f for f, kind in enumerate(S.field_kinds(info1)) if kind != S.NONE]
    ladders = np.zeros((len(info1.fields), 2), dtype=np.float32)
    ladders[swept] = [0.001, 0.005]
    hists, fields = [], None
    for info in (info1, info5):
        codec = _codec(info)
        streams = codec.encode_viz(clouds, 0, 0.05)[0] if viz else codec.encode_host(clouds)[0]
        if fields is None:
            fields = codec.sweep_hist_last_encode(ladders).astype(np.int64)
        whole = codec.stream_hist_last_encode()
        _same(whole, H.stream_hist(streams), "stream_hist_last_encode")
        hists.append(whole.astype(np.int64) - np.array([H.prefix_hist(s) for s in streams], dtype=np.int64))
    for k in range(2):
        moved = sum(fields[k, f, 1] - fields[k, f, 0] for f in swept)
        assert np.array_equal(hists[1][k] - hists[0][k], moved) and moved.any(), k


def test_the_survivors_of_a_viz_encode(oracle):
    info, data = synth.velodyne_xyzir(50000)
    step = info.point_step
    clouds = _cut(info, data, [15000, 0, 35000])
    clouds[0].view("<f4")[0] = np.nan                                 # dropped by the filter
    ladders = S.default_ladders(info)
    codec = _codec(info)
    _streams_, _cs, _m, kept = codec.encode_viz(clouds, 0, 0.05)
    survivors = [oracle.viz_preprocess(c, step, 0, 0.05) if c.size else c for c in clouds]
    assert [s.size // step for s in survivors] == [int(k) for k in kept] and 0 < int(kept.sum()) < 50000
    _same(codec.sweep_hist_last_encode(ladders), H.sweep_hist(info, np.concatenate(survivors), [int(k) for k in kept], ladders))


# ---- state rules -------------------------------------------------------------------------------------------------------

def test_last_encode_calls_repeat_and_interleave_with_the_audit_and_the_sweeps(oracle):
    info, data = synth.velodyne_xyzir(40000)
    sizes = [25000, 0, 15000]
    clouds = _cut(info, data, sizes)
    ladders = S.default_ladders(info)
    codec = _codec(info)
    want_f = H.sweep_hist(info, data, sizes, ladders)
    want_sweep = S.sweep(info, data, sizes, ladders)
    dec = [oracle.decode_stage1(info, oracle.encode_stage1(info, c), c.size // info.point_step) if c.size else c for c in clouds]
    want_audit = A.audit(info, data, np.concatenate(dec), sizes)
    streams = codec.encode_host(clouds)[0]
    want_s = H.stream_hist(streams)
    modes = codec.sweep_modes_last_encode()
    for _ in range(2):
        _same(codec.sweep_hist_last_encode(ladders), want_f, "fields")
        _same(codec.stream_hist_last_encode(), want_s, "streams")
        assert S.same(codec.sweep_last_encode(ladders), want_sweep)
        _same(codec.stream_hist_last_encode(), want_s, "streams behind the sweep")
        assert A.same(codec.audit_last_encode(), want_audit)
        _same(codec.sweep_hist_last_encode(ladders[:, :2]), want_f[:, :, :2], "fields behind the audit, other ladder")
        assert codec.sweep_modes_last_encode().tobytes() == modes.tobytes()
    read, pr = _dev_report(3)
    assert codec.stream_hist_last_encode(report_ptr=pr) is None
    _same(read(), want_s, "device report")
    read, pr = _dev_report(3, len(info.fields), ladders.shape[1])
    assert codec.sweep_hist_last_encode(ladders, report_ptr=pr) is None
    _same(read(), want_f, "device report")
    assert A.same(codec.audit_last_encode(), want_audit)


def test_last_encode_behind_device_outputs():
    import torch
    dev = torch.device("cuda", 0)
    info, data = synth.lidar_xyzi(60000)
    sizes = [30000, 30000]
    codec = _codec(info)
    cap = sum(codec.plan.stage1_bound(n) for n in sizes)
    _tp, pp, check_p = _dev(data, 7)
    d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(3, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.encode_device(pp, sizes, d_out.data_ptr() + 7, cap, d_off.data_ptr())
    got = codec.stream_hist_last_encode()
    offs = d_off.cpu().numpy()
    out = d_out.cpu().numpy()[7:]
    _same(got, H.stream_hist([out[offs[k]:offs[k + 1]] for k in range(2)]), "device outputs")
    _same(codec.stream_hist_last_encode(), got, "repeated")
    _same(codec.sweep_hist_last_encode(_own(info)), H.sweep_hist(info, data, sizes, _own(info)), "fields")
    check_p()


def test_refused_without_state_and_behind_the_chunk_table_call():
    import torch
    from cloudini_amd import native
    dev = torch.device("cuda", 0)
    info, data = synth.lidar_xyzi(70000)
    ladders = S.default_ladders(info)
    codec = _codec(info)
    for call in (lambda: codec.sweep_hist_last_encode(ladders), codec.stream_hist_last_encode):
        with pytest.raises(native.CloudiniHipError) as e:
            call()
        assert e.value.code == -1 and "no encode call to audit" in e.value.message
    _tp, pp, check_p = _dev(data)
    codec.encode_chunks_device(pp, [70000])
    want = H.sweep_hist(info, data, [70000], ladders)
    _same(codec.sweep_hist_last_encode(ladders), want, "between the table and its framing")
    rep = np.full((1, 256), 7, dtype=np.uint64)
    rc = native.lib().cldn_hip_stream_hist_last_encode(codec._h, rep.ctypes.data, native.HOST)
    assert rc == -1 and "no encode call to audit" in native.lib().cldn_hip_last_error().decode() and (rep == 7).all()
    cap = codec.plan.stage1_bound(70000)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    codec.frame_chunks_device(d_out.data_ptr(), cap, d_off.data_ptr())
    stream = d_out.cpu().numpy()[:int(d_off.cpu().numpy()[1])]
    _same(codec.stream_hist_last_encode(), H.stream_hist([stream]), "framed")
    _same(codec.sweep_hist_last_encode(ladders), want, "framed")
    check_p()
    # calls that take buffers drop the state, the histogram calls included
    streams = codec.encode_host([data])[0]
    for intervening in (lambda: codec.sweep_hist_clouds_host([data], ladders), lambda: codec.stream_hist_host(streams),
                        lambda: codec.decode_host(streams, [70000])):
        codec.encode_host([data])
        intervening()
        for call in (lambda: codec.sweep_hist_last_encode(ladders), codec.stream_hist_last_encode, codec.audit_last_encode):
            with pytest.raises(native.CloudiniHipError) as e:
                call()
            assert e.value.code == -1 and "no encode call to audit" in e.value.message


# ---- argument errors: cldn_hip_sweep_clouds', case for case ------------------------------------------------------------

def test_arguments_are_refused_as_the_sweep_refuses_them():
    from cloudini_amd import native
    info, data = synth.lidar_xyzi(1000)
    codec = _codec(info)
    good = S.default_ladders(info)
    want = H.sweep_hist(info, data, [1000], good)
    _t, p, _c = _dev(data)
    read, pr = _dev_report(1, 4, 5)

    def both(hist_call, sweep_call):
        errs = []
        for call in (hist_call, sweep_call):
            with pytest.raises(native.CloudiniHipError) as e:
                call()
            errs.append((e.value.code, e.value.message))
        assert errs[0] == errs[1] and errs[0][0] == -1, errs

    for bad in (-0.001, np.nan, np.inf, -np.inf, 1e-45, 2.0e-39):
        ladders = good.copy()
        ladders[1, 2] = np.float32(bad)
        both(lambda: codec.sweep_hist_clouds_host([data], ladders), lambda: codec.sweep_clouds_host([data], ladders))
        ladders[1, 2] = good[1, 2]
        ladders[3, 2] = np.float32(bad)                               # the u16 field: its ladder is ignored
        _same(codec.sweep_hist_clouds_host([data], ladders), want, str(bad))
    for n_cand in (0, 17):
        ones = np.ones((4, n_cand), np.float32)
        both(lambda: codec.sweep_hist_clouds_host([data], ones), lambda: codec.sweep_clouds_host([data], ones))
    both(lambda: codec.sweep_hist_clouds_device(p, [1000], good, report_ptr=pr + 4),
         lambda: codec.sweep_clouds_device(p, [1000], good, report_ptr=pr + 4))
    both(lambda: codec.sweep_hist_clouds_device(p, [1000], good, points_loc=2),
         lambda: codec.sweep_clouds_device(p, [1000], good, points_loc=2))
    both(lambda: codec.sweep_hist_clouds_device(0, [1000], good), lambda: codec.sweep_clouds_device(0, [1000], good))
    offs = np.array([0, 10, 5], dtype=np.uint64)
    for call in (lambda: codec.stream_hist_device(p, offs), lambda: codec.stream_hist_device(0, [0, 10]),
                 lambda: codec.stream_hist_device(p, [0, 10], streams_loc=2), lambda: codec.stream_hist_device(p, [0, 10], report_ptr=pr + 4)):
        with pytest.raises(native.CloudiniHipError) as e:
            call()
        assert e.value.code == -1
    assert (read().view(np.uint8) == 0xEE).all()                      # refused calls wrote nothing
    codec.encode_host([data])
    for n_cand in (0, 17):
        ones = np.ones((4, n_cand), np.float32)
        both(lambda: codec.sweep_hist_last_encode(ones), lambda: codec.sweep_last_encode(ones))
    _same(codec.sweep_hist_last_encode(good), want, "a refused call leaves the state")


# ---- the value grid (tests/value_grid_cases.py): rounding, range and 2^21 edges, each field at res, res / 2 and 2 res -----------------
import value_grid_cases as VG  # noqa: E402


REPORT_GROUPS = VG.report_groups()


@pytest.mark.parametrize("name,cs", REPORT_GROUPS, ids=[g[0] for g in REPORT_GROUPS])
def test_histograms_equal_the_model_on_the_value_grid(name, cs):
    by_res = {}
    for c in cs:
        by_res.setdefault(c.res, []).append(c)
    for res, group in by_res.items():
        info = group[0].info()
        _run(info, [c.cloud() for c in group], S.default_ladders(info, (1.0, 0.5, 2.0)), name, walks=(0, 3))
