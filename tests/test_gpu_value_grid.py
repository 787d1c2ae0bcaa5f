"""GPU: the value grid of tests/value_grid_cases.py through every codec route, one test per (family, layout) so that a failure names
it. tests/test_value_grid_cases.py (CPU) proves that every case is what its name says and pins its bytes to the compiled reference.

Encode: every cloud of families A-D goes through check_encode of test_gpu_encode.py (both pipelines where the layout allows both) in
batches of one layout and resolution, so every cloud but the first is a later cloud of a batch whose chunks do not start at chunk 0
of the call; family A's second chunks also run as calls of their own. The TAIL and WIDE layouts also take the device-resident
calls, the chunk table and its framing, committed modes and the device LZ4 stage. Decode: the oracle's streams of those clouds and
every hand-written stream of family E go through decode_host, the point decoder's layouts at cldn_hip_debug_decode_split 1, 2 and
16, byte for byte against oracle.decode_stage1 over a 0x5A pre-fill."""
import numpy as np
import pytest

import value_grid_cases as V
from test_gpu_encode import check_encode

pytestmark = pytest.mark.gpu

FILL = 0x5A
BATCH = 8
SPLITS = (1, 2, 16)
GROUP_IDS = [V.group_id(g) for g in V.GROUPS]
E_CASES = V.e_cases()


def _batches(cs):
    """clouds of one resolution, at most BATCH per call, in the table's order"""
    out = []
    for c in cs:
        if out and out[-1][0].res == c.res and len(out[-1]) < BATCH:
            out[-1].append(c)
        else:
            out.append([c])
    return out


def _decode_all(oracle, layout, infos, streams, ns, what):
    from cloudini_amd import native
    want = [oracle.decode_stage1(i, s, n, fill=FILL) for i, s, n in zip(infos, streams, ns)]
    info = infos[0]
    codec = native.Codec(native.Plan(info))
    for parts in (SPLITS if layout in V.POINT_DECODER_LAYOUTS else (0,)):
        if parts:
            assert codec.decode_split(parts) == 0
        out = np.full(sum(ns) * info.point_step, FILL, dtype=np.uint8)
        got = codec.decode_host(streams, ns, out=out)
        for k, (g, w) in enumerate(zip(got, want)):
            d = np.nonzero(g != w)[0]
            assert d.size == 0, "%s, cloud %d, split %d: first difference at byte %d (point %d)" % (what, k, parts, d[0], d[0] // info.point_step)
        # every chunk's regular stream went through the parallel kernels of the layout's route (a chunk k_decode_points_w hands back
        # is redone by k_decode_varint under the same word), none through the serial decoder; the WIDE route has the serial body only
        n_chunks = sum((n + V.CHUNK - 1) // V.CHUNK for n in ns)
        stats = codec.decode_stats()
        assert (stats[0], stats[2]) == ((0, n_chunks) if layout == "WIDE" else (n_chunks, 0)), (what, stats, n_chunks)
    codec.close()


@pytest.mark.parametrize("group", V.GROUPS, ids=GROUP_IDS)
def test_encode_and_decode(oracle, group):
    fam, layout = group
    for batch in _batches(V.family(fam, layout)):
        info = batch[0].info()
        clouds = [c.cloud() for c in batch]
        what = "%s .. %s" % (batch[0].name, batch[-1].name)
        try:
            streams = check_encode(oracle, info, clouds)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e)) from None
        _decode_all(oracle, layout, [c.info() for c in batch], streams, [c.n for c in batch], what)


@pytest.mark.parametrize("layout", V.PIECE_LAYOUTS)
def test_family_a_second_chunk_as_a_call_of_its_own(oracle, layout):
    """A chunk range that does not start at the cloud's chunk 0: the points from 32768 on, encoded as clouds of their own (the modes of
    an integer field committed on the head, as tests/test_gpu_fused.py does for chunk ranges), are the second chunk of the whole
    cloud's stream byte for byte -- the placements at 32768 then stand at a cloud's first point, the reference 0."""
    from cloudini_amd import native
    step = V.LAYOUTS[layout][1]
    for batch in _batches([c for c in V.family("A", layout) if c.n > V.CHUNK]):
        info = batch[0].info()
        clouds = [c.cloud() for c in batch]
        wants = [oracle.encode_stage1(info, cloud, return_modes=True) for cloud in clouds]
        codec = native.Codec(native.Plan(info))
        if codec.plan.adaptive_fields:
            assert all(list(m) == list(wants[0][1]) for _w, m in wants)
            codec.force_modes(wants[0][1])
        got, _sizes, _modes = codec.encode_host([cloud[V.CHUNK * step:] for cloud in clouds])
        for c, g, (w, _m) in zip(batch, got, wants):
            first = int.from_bytes(w[:4].tobytes(), "little")
            assert np.array_equal(g, w[4 + first:]), c.name
        codec.close()


@pytest.mark.parametrize("layout", V.LAYOUTS)
def test_the_layout_reaches_the_encoder_it_is_named_for(layout):
    """codec.pipeline(2) asks for the piece kernel and returns what the next call takes: 2 for the piece kernel's layouts, 1 (the generic
    kernel) for the layouts without a FloatN group or with a field between. Which instantiation, and the WIDE route, are held by the
    route functions on the CPU (tests/test_value_grid_cases.py::test_the_layout_reaches_the_sites_it_is_named_for)."""
    from cloudini_amd import native
    codec = native.Codec(native.Plan(V.info_of(layout, V.RES, 1)))
    taken = codec.pipeline(2)
    if layout in V.PIECE_LAYOUTS:
        assert taken == 2
    elif layout != "WIDE":
        assert taken == 1
    codec.close()


DEVICE_GROUPS = [(fam, layout) for fam in ("C", "D") for layout in V.TAIL_LAYOUTS + ("WIDE",)]


@pytest.mark.parametrize("group", DEVICE_GROUPS, ids=[V.group_id(g) for g in DEVICE_GROUPS])
def test_tail_and_wide_layouts_through_the_other_entry_points(oracle, group):
    """The entry points of test_gpu_fused.py::test_wide_route_through_the_other_entry_points for every C and D cloud of the two TAIL
    layouts and the WIDE one: device-resident encode and the decode with the encoder's chunk sizes, the chunk table and
    cldn_hip_frame_chunks, a call with the modes committed beforehand, LZ4 blocks on the device with both parameter sets -- the
    oracle's bytes each time."""
    import ctypes as C
    import torch
    from cloudini_amd import native
    from test_gpu_fused import _read_chunk_table
    dev = torch.device("cuda", 0)
    lz4 = C.CDLL("/usr/lib/x86_64-linux-gnu/liblz4.so.1")
    for c in V.family(*group):
        info, data = c.info(), c.cloud()
        assert c.n <= V.CHUNK
        want, want_modes = oracle.encode_stage1(info, data, return_modes=True)
        codec = native.Codec(native.Plan(info))
        d_in = torch.from_numpy(data).to(dev)
        cap = codec.plan.stage1_bound(c.n)
        d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(2, dtype=torch.int64, device=dev)
        d_sizes = torch.zeros(2, dtype=torch.int32, device=dev)
        cp = np.array([c.n], dtype=np.uint64)
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        codec.encode_device(d_in.data_ptr(), cp, d_out.data_ptr(), cap, d_off.data_ptr(), d_sizes.data_ptr(), 0)
        codec.synchronize()
        codec.status()
        offs = d_off.cpu().numpy().astype(np.uint64)
        assert int(offs[1]) == want.size and np.array_equal(d_out[: want.size].cpu().numpy(), want), c.name
        d_dec = torch.full((data.size,), FILL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        codec.decode_device(d_out.data_ptr(), offs, cp, d_dec.data_ptr(), data.size, d_sizes.data_ptr())
        codec.synchronize()
        codec.status()
        assert np.array_equal(d_dec.cpu().numpy(), oracle.decode_stage1(info, want, c.n, fill=FILL)), c.name
        # the chunk table, then its framing
        table = codec.encode_chunks_device(d_in.data_ptr(), cp)
        codec.synchronize()
        codec.status()
        payloads, _segs, _flag = _read_chunk_table(table, torch)
        assert len(payloads) == 1 and np.array_equal(payloads[0], want[4:]), c.name
        d_out.zero_()
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        codec.frame_chunks_device(d_out.data_ptr(), cap, d_off.data_ptr())
        codec.synchronize()
        codec.status()
        assert np.array_equal(d_out[: want.size].cpu().numpy(), want), c.name
        # the modes committed beforehand (the layouts without an integer field have none)
        codec.force_modes(want_modes)
        got, _sizes, _modes = codec.encode_host([data])
        assert np.array_equal(got[0], want), c.name
        codec.force_modes(None)
        # stage 2 on the device: the block is the serial model's and decodes to the payload
        for stage2, params in ((1, (8192, 11, 1024)), (2, (4096, 10, 512))):
            codec.set_stage2(stage2)
            streams, _sz, _m = codec.encode_host([data])
            size = int.from_bytes(streams[0][:4].tobytes(), "little")
            assert 4 + size == streams[0].size, c.name
            block = np.ascontiguousarray(streams[0][4:])
            assert np.array_equal(block, oracle.lz4_model(payloads[0].tobytes(), *params)), (c.name, stage2)
            out = C.create_string_buffer(max(1, payloads[0].size))
            assert lz4.LZ4_decompress_safe(block.ctypes.data_as(C.c_char_p), out, int(block.size), int(payloads[0].size)) == payloads[0].size
            assert out.raw[: payloads[0].size] == payloads[0].tobytes(), (c.name, stage2)
        codec.set_stage2(0)
        codec.close()


@pytest.mark.parametrize("case", E_CASES, ids=[e.name for e in E_CASES])
def test_decode_hand_written_streams(oracle, case):
    _decode_all(oracle, case.layout, [case.info()], [case.stream(oracle)], [case.n], case.name)


def test_decode_hand_written_streams_as_one_batch(oracle):
    """the streams of one layout and resolution back to back: the second lies at another address residue than the first"""
    for layout in V.POINT_DECODER_LAYOUTS:
        for res in V.E_RESOLUTIONS:
            es = [e for e in E_CASES if e.layout == layout and e.res == res and not e.long_tokens]
            assert len(es) == 2
            _decode_all(oracle, layout, [e.info() for e in es], [e.stream(oracle) for e in es], [e.n for e in es], "%s + %s" % (es[0].name, es[1].name))
