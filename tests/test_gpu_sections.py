"""The V5 section writers on the device against tests/section_model.py, byte for byte, over the constructed grid of
tests/section_cases.py with every mode forced (cldn_hip_codec_force_modes_per_cloud). Expected bytes come from the model alone;
tests/test_section_cases.py holds the model against the oracle and the reference on the CPU.

The writers, and how each is reached here (routes as in stage1_encode_route.h; the stale-hint test asks the route itself):
  W1  k_section_fast                 2- and 4-byte fields, modes 0, 2, 3: integer-only clouds (generic kernel), XYZ + field (piece kernel)
  W2  k_encode_sections              8-byte fields, every mode; 2- and 4-byte fields behind a launch hint that names another mode
  W3  k_wide_encode                  the field inside a point of more than 1024 bytes, a second adaptive field behind it
  W4  k_section_palette<u64>         8-byte Palette of up to 3072 values (more: W2)
  W5  Pal32                          2- and 4-byte Palette: k_finish's fused build (framed calls, 1024 threads below 200 chunks,
                                     512 from 200 on), k_section_palette32 (chunk-table call)
A batch is one call: cases x modes as clouds of one schema, so the file needs tens of launches. Every failing cloud is named."""
import numpy as np
import pytest

import cases
import mode_model as M
import section_cases as SC
import section_model as S

pytestmark = pytest.mark.gpu

F = cases.F
GUARD = 256
NARROW = [t for t in SC.TYPES if SC.bits_of(t) < 64]
IDS = lambda ts: [t.name for t in ts]
_CACHE = {}


def _xyz_layout(values, ftype, res=0.5):
    """XYZ (all zero: three one-byte tokens per point) + the field at offset 12."""
    v = np.asarray(values).astype(SC._NP[ftype])
    n = v.size
    info = cases.make_info([("x", 0, F.FLOAT32, res), ("y", 4, F.FLOAT32, res), ("z", 8, F.FLOAT32, res), ("value", 12, ftype, None)],
                           12 + v.dtype.itemsize, n)
    zero = np.zeros(n, np.float32)
    return info, cases.pack(info, {"x": zero, "y": zero, "z": zero, "value": v}, n)


def _layout(case, ftype, how):
    return _xyz_layout(case.values, ftype) if how == "xyz" else SC.layout(case, ftype, how == "odd")


def _batch(ftype, how):
    """[(tag, data, mode, the model's stream)] for every case of the type under every mode, but a Palette that must be refused;
    built once per (type, layout) and left unchanged. Returns (info, batch)."""
    key = (ftype, how)
    if key not in _CACHE:
        out, info = [], None
        for c in SC.grid_of(ftype):
            info, data = _layout(c, ftype, how)
            for m in S.MODES:
                if m == 1 and c.outcome == SC.REFUSED:
                    continue
                out.append((f"{ftype.name}_{how}_{c.name}_{S.NAMES[m]}", data, m, S.stream_bytes(info, data, [m])))
        _CACHE[key] = (info, out)
    return _CACHE[key]


def _codec(info):
    from cloudini_amd import native
    return native.Codec(native.Plan(info))


def _differing(batch, streams):
    """The clouds whose stream is not the model's, as a text that names the first few of every mode ('' if there is none)."""
    bad = [tag for (tag, _d, _m, want), got in zip(batch, streams) if np.asarray(got).tobytes() != want]
    if not bad:
        return ""
    by_mode = {name: [t for t in bad if t.endswith("_" + name)] for name in S.NAMES}
    return f"{len(bad)} of {len(batch)} streams differ from the model: " + "; ".join(
        f"{name} {len(tags)}: {tags[:6]}" for name, tags in by_mode.items() if tags)


def _force(codec, batch):
    codec.force_modes_per_cloud(np.array([[m] for _t, _d, m, _w in batch], dtype=np.uint8))


def _sizes(info, batch):
    return [d.size // info.point_step for _t, d, _m, _w in batch]


def _round_trip(codec, info, batch, streams):
    """Every stream decodes on the device to the input bytes: one decode call for the batch. (The two streams of the INT64_MIN
    difference are left out: no decoder takes them, section_cases.UNDECODABLE.)"""
    keep = [k for k, (tag, _d, m, _w) in enumerate(batch) if not any(tag.endswith(f"{n}_{S.NAMES[mm]}") for n, mm in SC.UNDECODABLE)]
    sizes = _sizes(info, batch)
    out = np.full(sum(batch[k][1].size for k in keep), 0xA5, dtype=np.uint8)      # (the padding of cases.pack)
    back = codec.decode_host([streams[k] for k in keep], [sizes[k] for k in keep], out=out)
    bad = [batch[k][0] for k, b in zip(keep, back) if b.tobytes() != batch[k][1].tobytes()]
    assert not bad, f"{len(bad)} streams do not decode to their input: {bad[:8]}"


def _guarded(nbytes, residue, fill):
    """A device buffer of nbytes that starts `residue` bytes behind a 256-byte boundary, between two guard spans (the idiom of
    test_gpu_modes._dev). Returns (tensor, offset of the buffer in it)."""
    import torch
    t = torch.full((256 + GUARD + 16 + nbytes + GUARD,), fill, dtype=torch.uint8, device=torch.device("cuda", 0))
    return t, (-t.data_ptr()) % 256 + GUARD + residue


def _device_call(codec, info, batch, residue, chunks=False):
    """One call on device buffers: points at an odd residue, streams at `residue`, both between guards. Returns the streams and
    asserts that nothing outside the streams was written and that the points are as they were."""
    import torch
    sizes = _sizes(info, batch)
    flat = np.concatenate([d for _t, d, _m, _w in batch])
    cap = int(sum(codec.plan.stage1_bound(n) for n in sizes))
    t_in, at_in = _guarded(flat.size, 3, 0xA5)
    t_in[at_in:at_in + flat.size] = torch.from_numpy(flat).to(t_in.device)
    before = t_in.cpu().numpy().copy()
    t_out, at = _guarded(cap, residue, 0xEE)
    d_off = torch.zeros(len(batch) + 1, dtype=torch.int64, device=t_in.device)
    torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    if chunks:
        codec.encode_chunks_device(t_in.data_ptr() + at_in, sizes)
        codec.status()
        codec.frame_chunks_device(t_out.data_ptr() + at, cap, d_off.data_ptr())
    else:
        codec.encode_device(t_in.data_ptr() + at_in, sizes, t_out.data_ptr() + at, cap, d_off.data_ptr())
    codec.synchronize()
    codec.status()
    offs = d_off.cpu().numpy().astype(np.int64)
    h = t_out.cpu().numpy()
    assert (h[:at] == 0xEE).all() and (h[at + offs[-1]:] == 0xEE).all(), "bytes outside the streams were written"
    assert np.array_equal(t_in.cpu().numpy(), before), "the points have changed"
    return [h[at + offs[k]:at + offs[k + 1]] for k in range(len(batch))]


# ---- W1, W2, W4, W5 (fused): framed calls ---------------------------------------------------------------------------------

FRAMED = [(t, how) for t in SC.TYPES for how in ("aligned", "odd")] + [(t, "xyz") for t in NARROW]


@pytest.mark.parametrize("ftype,how", FRAMED, ids=[f"{t.name}-{h}" for t, h in FRAMED])
def test_every_case_under_every_forced_mode_framed_to_host(ftype, how):
    """Integer-only clouds take the generic kernel, XYZ + field the piece kernel; behind either k_section_fast writes modes 0, 2
    and 3 of the narrow fields and k_finish their Palette, k_encode_sections and k_section_palette<u64> the 8-byte fields. The
    batch has more than 200 chunks: k_finish runs with 512 threads."""
    info, batch = _batch(ftype, how)
    assert sum((n + SC.CHUNK - 1) // SC.CHUNK for n in _sizes(info, batch)) >= 200
    codec = _codec(info)
    _force(codec, batch)
    streams, _cs, modes = codec.encode_host([d for _t, d, _m, _w in batch])
    assert modes.reshape(-1).tolist() == [m for _t, _d, m, _w in batch]
    bad = _differing(batch, streams)
    assert not bad, bad
    _round_trip(codec, info, batch, streams)
    codec.close()


DEVICE = [(t, "aligned") for t in SC.TYPES] + [(t, "xyz") for t in NARROW]


@pytest.mark.parametrize("residue", [0, 1, 7, 15])
@pytest.mark.parametrize("ftype,how", DEVICE, ids=[f"{t.name}-{h}" for t, h in DEVICE])
def test_framed_to_a_device_buffer_at_every_residue(ftype, how, residue):
    """The same writers into a caller's device buffer 0, 1, 7 and 15 bytes behind a 16-byte boundary, between guard spans, from
    integer-only clouds (generic kernel) and from XYZ + field (piece kernel); fewer than 200 chunks, so k_finish builds the narrow
    Palettes with 1024 threads."""
    info, batch = _batch(ftype, how)
    # (most two-chunk run columns stay with the host test: 24 of them under 4 modes are 192 chunks by themselves)
    batch = [b for b in batch if "_len_" not in b[0] and ("_runs_value_" not in b[0] and "_runs_delta_" not in b[0]
                                                            or "_thread_m1_" in b[0] or "_delta_tile_p1_" in b[0])]
    assert sum((n + SC.CHUNK - 1) // SC.CHUNK for n in _sizes(info, batch)) < 200 and {b[2] for b in batch} == set(S.MODES)
    codec = _codec(info)
    _force(codec, batch)
    streams = _device_call(codec, info, batch, residue)
    bad = _differing(batch, streams)
    assert not bad, bad
    _round_trip(codec, info, batch, streams)
    codec.close()


# ---- W4, W5 (k_section_palette32), `append` placement: the chunk-table call and its framing --------------------------------

TABLE = [(t, "aligned") for t in SC.TYPES] + [(t, "xyz") for t in NARROW]


@pytest.mark.parametrize("ftype,how", TABLE, ids=[f"{t.name}-{h}" for t, h in TABLE])
def test_chunk_table_call_then_framing(ftype, how):
    """encode_chunks_device leaves the narrow Palettes to k_section_palette32 (the slow path above 3072 values included) and the
    8-byte ones to k_section_palette<u64>; frame_chunks_device then writes the streams."""
    info, batch = _batch(ftype, how)
    batch = [b for b in batch if "_len_" not in b[0] or b[2] == 1]
    codec = _codec(info)
    _force(codec, batch)
    streams = _device_call(codec, info, batch, 5, chunks=True)
    bad = _differing(batch, streams)
    assert not bad, bad
    _round_trip(codec, info, batch, streams)
    codec.close()


@pytest.mark.parametrize("ftype", NARROW, ids=IDS(NARROW))
def test_append_places_the_section_behind_regular_streams_of_every_length_mod_16(ftype):
    """XYZ + one adaptive field, chunk-table call: the section goes right behind the regular stream (EncodeRoute::append), which
    is three bytes a point here and so ends 0, 1, 5 and 15 bytes behind a 16-byte boundary. Every mode."""
    grid = {c.name: c for c in SC.grid_of(ftype)}
    batch = []
    for n in (8192, 8192 + 11, 8192 + 7, 8192 + 5, 16, 11, 7, 5):
        for name in ("runs_value_thread_m1", "runs_delta_tile_p1", "longest_token_on_thread_quarter_chunk_edges", "unique_257"):
            info, data = _xyz_layout(grid[name].values[:n], ftype)
            for m in S.MODES:
                batch.append((f"{ftype.name}_{name}_first_{n}_{S.NAMES[m]}", data, m, S.stream_bytes(info, data, [m])))
    assert {3 * n % 16 for n in (8192, 8203, 8199, 8197)} == {0, 1, 5, 15}
    codec = _codec(info)
    _force(codec, batch)
    streams = _device_call(codec, info, batch, 0, chunks=True)
    bad = _differing(batch, streams)
    assert not bad, bad
    _round_trip(codec, info, batch, streams)
    codec.close()


# ---- W3: the wide route ----------------------------------------------------------------------------------------------------

WIDE_CASES = SC.WIDE_CASES  # (the route table of section_cases.py names them)
_WIDE = {}


@pytest.mark.parametrize("mode", S.MODES, ids=S.NAMES)
@pytest.mark.parametrize("ftype", SC.TYPES, ids=IDS(SC.TYPES))
def test_wide_points_every_mode(ftype, mode):
    """A point of 1040 bytes goes to k_wide_encode, which calls the section functions of k_encode_sections from its own carve-up and
    copies each section out of one scratch area. A second adaptive field behind the first reuses that area. One chunk per case
    (a cloud of wide points is large)."""
    grid = {c.name: c for c in SC.grid_of(ftype)}
    npt = SC._NP[ftype]
    size = np.dtype(npt).itemsize
    fields = [("value", 3, ftype, None), ("tail", 1030, F.UINT16, None)]
    batch, info = [], None
    for name in WIDE_CASES:
        v = np.asarray(grid[name].values)[:SC.CHUNK].astype(npt)
        n = v.size
        info = cases.make_info(fields, 1040, n)
        if (ftype, name) not in _WIDE:                                   # (34 MB a cloud: packed once, shared by the four modes)
            _WIDE[(ftype, name)] = cases.pack(info, {"value": v, "tail": (np.arange(n) // 5 * 3).astype(np.uint16)}, n)
        data = _WIDE[(ftype, name)]
        modes = [mode, (mode + 1) % 4]
        batch.append((f"{ftype.name}_wide_{name}_{S.NAMES[mode]}", data, modes, S.stream_bytes(info, data, modes)))
    assert info.point_step > 1024 and info.fields[0].offset + size <= 1030
    codec = _codec(info)
    codec.force_modes_per_cloud(np.array([m for _t, _d, m, _w in batch], dtype=np.uint8))
    streams, _cs, _modes = codec.encode_host([d for _t, d, _m, _w in batch])
    bad = _differing(batch, streams)
    assert not bad, bad
    _round_trip(codec, info, batch, streams)
    codec.close()


# ---- W2 for the narrow fields: behind a stale launch hint --------------------------------------------------------------------

def _prefix(mode, ftype, rs):
    """4096 values on which the probe commits `mode` (asserted from mode_model by the caller)."""
    lo, hi = SC.limits(ftype)
    if mode == 0:
        return rs.randint(lo, hi, M.PROBE, dtype=np.int64)
    if mode == 1:
        return rs.randint(0, 200, M.PROBE) * 5
    if mode == 2:
        return np.repeat(rs.randint(lo // 2, hi // 2, M.PROBE // 8, dtype=np.int64), 8)
    return np.arange(M.PROBE) % 128


STALE_CASES = SC.STALE_CASES


@pytest.mark.parametrize("ftype", NARROW, ids=IDS(NARROW))
def test_general_kernel_behind_a_stale_hint(ftype, tmp_path):
    """k_encode_sections takes a narrow field's section when no fast kernel did. A codec's first call leaves a launch hint (the modes
    it committed) that the next calls launch by: after a priming call that commits Palette, XYZ + field launches no k_section_fast,
    and after one that commits DeltaVarint nothing builds a Palette but the general kernel. Each case follows 4096 values on which
    the unforced probe commits the wanted mode.
    How the route was confirmed: the codec's timing slots give one time for all section kernels, which cannot tell them apart, so
    the route is asked directly: encode_route() through the host shim of tests/test_encode_route.py, with this plan, this call's
    facts and the hint the priming call left."""
    import test_encode_route as R
    shim = R.build_shim(tmp_path)
    grid = {c.name: c for c in SC.grid_of(ftype)}
    bpv = SC.bits_of(ftype) // 8
    rs = np.random.RandomState(4242)
    for primed, wanted in ((1, (0, 2, 3)), (0, (1,))):
        batch, info = [], None
        for mode in wanted:
            for name in STALE_CASES:
                values = np.concatenate([_prefix(mode, ftype, rs), np.asarray(grid[name].values).astype(SC._NP[ftype]).astype(np.int64)[:SC.CHUNK]])
                info, data = _xyz_layout(values, ftype)
                v, _ = M.column(info, data, M.adaptive_fields(info)[0])
                assert M.select(M.section_sizes(v[:M.PROBE], bpv)) == mode, (name, mode)
                batch.append((f"{ftype.name}_stale_{name}_{S.NAMES[mode]}", data, mode, S.stream_bytes(info, data, [mode])))
        n_chunks = sum((n + SC.CHUNK - 1) // SC.CHUNK for n in _sizes(info, batch))
        row = R.row("stale", [], 12 + bpv, R.xyz(), [(bpv, 12)], hints=[1 << primed], n_chunks=n_chunks, n_clouds=len(batch))
        kernels, route = R.route_of(shim, row, host_input=True)
        assert "k_encode_sections" in kernels
        if primed == 1:
            assert "k_section_fast" not in kernels and route["runs"] == [], kernels
        else:
            assert route["fused_field"] == -1 and route["pal16"] == [] and route["pal32"] == [], (kernels, route)
        codec = _codec(info)
        info0, prime = _xyz_layout(_prefix(primed, ftype, rs), ftype)
        _s, _c, modes = codec.encode_host([prime])
        assert modes.reshape(-1).tolist() == [primed]
        streams, _cs, modes = codec.encode_host([d for _t, d, _m, _w in batch])
        assert modes.reshape(-1).tolist() == [m for _t, _d, m, _w in batch]
        bad = _differing(batch, streams)
        assert not bad, f"primed with {S.NAMES[primed]}: {bad}"
        _round_trip(codec, info, batch, streams)
        codec.close()


# ---- the Palette that no partition count separates ---------------------------------------------------------------------------

@pytest.mark.parametrize("ftype", [F.UINT64, F.INT64], ids=["UINT64", "INT64"])
def test_a_palette_that_cannot_be_partitioned_is_refused_and_the_codec_goes_on(ftype):
    """6200 keys whose twelve partition bits agree: section_palette (k_encode_sections; the 8-byte fast kernel gives up above 3072
    values) finds no partition count up to kPalMaxParts that fits its table. The call fails with a non-zero code, writes nothing
    outside its output, and the same codec then encodes ordinary clouds correctly, that column under the other modes included."""
    import torch
    from cloudini_amd import native
    case = [c for c in SC.grid_of(ftype) if c.outcome == SC.REFUSED][0]
    info, data = SC.layout(case, ftype, False)
    n = data.size // info.point_step
    codec = _codec(info)
    codec.force_modes([1])
    with pytest.raises(native.CloudiniHipError) as e:
        codec.encode_host([data])
    assert e.value.code == -3 and "Palette" in e.value.message
    # device buffers: the call is asynchronous, status() reports; guards and points untouched
    cap = codec.plan.stage1_bound(n)
    t_in, at_in = _guarded(data.size, 0, 0xA5)
    t_in[at_in:at_in + data.size] = torch.from_numpy(data).to(t_in.device)
    before = t_in.cpu().numpy().copy()
    t_out, at = _guarded(cap, 0, 0xEE)
    d_off = torch.zeros(2, dtype=torch.int64, device=t_in.device)
    torch.cuda.synchronize()
    codec.encode_device(t_in.data_ptr() + at_in, [n], t_out.data_ptr() + at, cap, d_off.data_ptr())
    codec.synchronize()
    with pytest.raises(native.CloudiniHipError) as e:
        codec.status()
    assert e.value.code == -3
    h = t_out.cpu().numpy()
    assert (h[:at] == 0xEE).all() and (h[at + cap:] == 0xEE).all() and np.array_equal(t_in.cpu().numpy(), before)
    # after the refusal: the same codec, ordinary work
    for m in (0, 2):  # (alone in a call, this column's forced DeltaRle stream is larger than stage1_bound, which knows no forcing)
        codec.force_modes([m])
        assert codec.encode_host([data])[0][0].tobytes() == S.stream_bytes(info, data, [m]), S.NAMES[m]
    legal = [c for c in SC.grid_of(ftype) if c.name == "palette_7000_keys_in_one_partition_of_8"][0]
    info2, data2 = SC.layout(legal, ftype, False)
    codec.force_modes([1])
    streams, _cs, _m = codec.encode_host([data2])
    assert streams[0].tobytes() == S.stream_bytes(info2, data2, [1])
    assert codec.decode_host(streams, [data2.size // info2.point_step])[0].tobytes() == data2.tobytes()
    # unforced, the quiet probe window commits Palette by itself: the same refusal without any forcing
    v, bpv = M.column(info, data, M.adaptive_fields(info)[0])
    assert M.select(M.section_sizes(v[:M.PROBE], bpv)) == 1
    codec.force_modes(None)
    with pytest.raises(native.CloudiniHipError) as e:
        codec.encode_host([data])
    assert e.value.code == -3
    streams, _cs, modes = codec.encode_host([data2])
    assert modes.reshape(-1).tolist() == [1] and streams[0].tobytes() == S.stream_bytes(info2, data2, [1])
    codec.close()


def test_the_same_refusal_from_the_wide_route():
    """The 6200-key column as the first of two adaptive fields of a 1040-byte point: section_palette is called by k_wide_encode, raises
    the status through the wide launch's own arguments, and returns two empty segments in front of the scratch copy and the second
    field. The call fails with the same code; the codec then encodes the next clouds correctly, Palette included."""
    from cloudini_amd import native
    grid = {c.name: c for c in SC.grid_of(F.UINT64)}
    case = [c for c in grid.values() if c.outcome == SC.REFUSED][0]
    fields = [("value", 3, F.UINT64, None), ("tail", 1030, F.UINT16, None)]

    def cloud(values):
        v = np.asarray(values)[:SC.CHUNK].astype(np.uint64)
        info = cases.make_info(fields, 1040, v.size)
        return info, cases.pack(info, {"value": v, "tail": (np.arange(v.size) // 5 * 3).astype(np.uint16)}, v.size)
    info, data = cloud(case.values)
    legal_info, legal = cloud(grid["palette_7000_keys_in_one_partition_of_8"].values)
    codec = _codec(info)
    codec.force_modes([1, 2])
    with pytest.raises(native.CloudiniHipError) as e:
        codec.encode_host([legal, data])                                       # one refused cloud fails the call
    assert e.value.code == -3 and "Palette" in e.value.message
    streams, _cs, _m = codec.encode_host([legal])
    assert streams[0].tobytes() == S.stream_bytes(legal_info, legal, [1, 2])
    codec.force_modes([0, 1])
    streams, _cs, _m = codec.encode_host([data])
    assert streams[0].tobytes() == S.stream_bytes(info, data, [0, 1])
    assert codec.decode_host(streams, [data.size // 1040], out=np.full(data.size, 0xA5, np.uint8))[0].tobytes() == data.tobytes()
    codec.close()


def test_pal32_keys_that_no_partition_count_separates_chunk_table_call():
    """3100 32-bit keys that agree in the top 13 bits of pal32_part's hash: pal32_slow_first (k_section_palette32, the chunk-table
    call) finds no partition count up to 8192 and raises ST_PALETTE_FULL, which the host now reads: status() and the framing to host
    memory (cldn_hip_frame_chunks' own check) both return the error. Not run through the framed call: there the builder is k_finish,
    whose workgroup leaves without publishing its chunk's size, and the workgroups behind it wait until their bound runs out."""
    import ctypes as C
    import torch
    from cloudini_amd import native
    values, check = SC.pal32_refused_column()
    info, data = SC.MC.layout(values, F.UINT32, False)
    assert check(M.column(info, data, M.adaptive_fields(info)[0])[0])
    n = data.size // info.point_step
    codec = _codec(info)
    codec.force_modes([1])
    d_in = torch.from_numpy(data).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    codec.encode_chunks_device(d_in.data_ptr(), [n])
    with pytest.raises(native.CloudiniHipError) as e:
        codec.status()
    assert e.value.code == -3 and "Palette" in e.value.message
    cap = codec.plan.stage1_bound(n)
    out, offs = np.full(cap + 64, 0xEE, np.uint8), np.zeros(2, np.uint64)
    rc = native.lib().cldn_hip_frame_chunks(codec._h, out.ctypes.data_as(C.c_void_p), cap, native.HOST, offs.ctypes.data_as(C.c_void_p), None)
    assert rc == -3 and (out == 0xEE).all()                                    # refused, and nothing was copied out
    # the same codec, ordinary work: the column under another mode, and a legal Palette of more than 3072 values
    codec.force_modes([0])
    assert codec.encode_host([data])[0][0].tobytes() == S.stream_bytes(info, data, [0])
    legal = [c for c in SC.grid_of(F.UINT32) if c.name == "pal32_3100_keys_agree_in_the_top_7_hash_bits"][0]
    info2, data2 = SC.layout(legal, F.UINT32, False)
    codec.force_modes([1])
    d_in2 = torch.from_numpy(data2).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    batch = [("legal", data2, 1, S.stream_bytes(info2, data2, [1]))]
    assert not _differing(batch, _device_call(codec, info2, batch, 0, chunks=True))
    codec.close()


@pytest.mark.parametrize("ftype", [F.UINT64, F.INT64], ids=["UINT64", "INT64"])
def test_the_device_decoder_refuses_the_int64_min_difference_like_the_reference(ftype):
    """The device writes the one byte 00 for a difference of INT64_MIN, as the reference does (the framed tests hold the bytes); the
    reference's decoder takes that byte for the NaN marker and refuses the stream. The device decoder does the same, under both
    modes that carry differences, and decodes the same column under Palette and Rle."""
    from cloudini_amd import native
    case = [c for c in SC.grid_of(ftype) if c.name == SC.INT64_MIN_DELTA][0]
    info, data = SC.layout(case, ftype, False)
    n = data.size // info.point_step
    codec = _codec(info)
    for m in S.MODES:
        stream = np.frombuffer(S.stream_bytes(info, data, [m]), np.uint8)
        if (case.name, m) in SC.UNDECODABLE:
            with pytest.raises(native.CloudiniHipError) as e:
                codec.decode_host([stream], [n])
            assert e.value.code == -6, S.NAMES[m]
        else:
            assert codec.decode_host([stream], [n])[0].tobytes() == data.tobytes(), S.NAMES[m]
    codec.close()
