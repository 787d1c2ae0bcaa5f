"""The stream operations of a framed encode call: the piece kernel clears the call's zero block itself (no memset in front of
it) and its probe workgroups write the caller's `modes` array (no copy behind the call).

Every failure these two changes can cause is state an earlier call of the SAME codec left behind -- segment entries, fallback
flags, the status block with k_finish's ticket, the anchors -- so every test reuses one codec across its calls and compares
everything a call hands out with the C oracle, byte for byte: the streams, stream_offsets, chunk_sizes and the modes.
"""
import numpy as np
import pytest

from cloudini_amd import synth
from stream_order_cases import mode_cloud, xyzi  # (the clouds and mode generators, shared with the stream-order plans)

pytestmark = pytest.mark.gpu

DELTA_VARINT, PALETTE, RLE, DELTA_RLE = 0, 1, 2, 3

_INFO = synth.xyzi_info(1)
_cache = {}


def want_of(oracle, cloud, forced=None):
    """(stream, modes) of the oracle for one cloud, computed once per cloud."""
    key = ("want", cloud.ctypes.data, cloud.size, forced)
    if key not in _cache:
        if forced is None:
            s, m = oracle.encode_stage1(_INFO, cloud, return_modes=True)
        else:
            s, m = oracle.encode_stage1_continued(_INFO, cloud, [forced]), np.array([forced], dtype=np.uint8)
        _cache[key] = (cloud, s, m)  # (the cloud is kept alive: its address is the key)
    return _cache[key][1], _cache[key][2]


def chunk_payloads(stream):
    out, o = [], 0
    while o < stream.size:
        size = int.from_bytes(stream[o:o + 4].tobytes(), "little")
        out.append(stream[o + 4:o + 4 + size])
        o += 4 + size
    assert o == stream.size
    return out


def expect(oracle, clouds, forced=None):
    wants = [want_of(oracle, c, forced) for c in clouds]
    streams = [w[0] for w in wants]
    offs = np.concatenate([[0], np.cumsum([s.size for s in streams])]).astype(np.int64)
    sizes = np.array([p.size for s in streams for p in chunk_payloads(s)], dtype=np.int64)
    modes = np.array([int(w[1][0]) for w in wants], dtype=np.uint8)
    return (np.concatenate(streams) if streams else np.zeros(0, np.uint8)), offs, sizes, modes


class Dev:
    """One codec and its device-resident calls."""

    def __init__(self):
        import torch
        from cloudini_amd import native
        self.torch, self.native = torch, native
        self.dev = torch.device("cuda", 0)
        self.plan = native.Plan(_INFO)
        self.codec = native.Codec(self.plan, device=0)

    def buffers(self, clouds):
        torch = self.torch
        host = np.concatenate(list(clouds) + [np.zeros(16, np.uint8)])
        d_in = torch.from_numpy(host).to(self.dev)
        counts = np.array([c.size // 16 for c in clouds], dtype=np.uint64)
        cap = max(16, sum(self.plan.stage1_bound(int(n)) for n in counts))
        d_out = torch.full((cap,), 0xCD, dtype=torch.uint8, device=self.dev)
        n_chunks = int(sum((int(n) + 32767) // 32768 for n in counts))
        d_off = torch.full((len(clouds) + 1,), -1, dtype=torch.int64, device=self.dev)
        d_sizes = torch.full((max(1, n_chunks),), -1, dtype=torch.int32, device=self.dev)
        d_modes = torch.full((len(clouds) + 8,), 0xEE, dtype=torch.uint8, device=self.dev)
        torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
        return d_in, counts, cap, d_out, d_off, d_sizes, d_modes, n_chunks

    def check(self, oracle, clouds, tag, offsets=True, sizes=True, modes_at=0, forced=None, run=None):
        """One framed device-resident call (or `run`, which gets the buffers) against the oracle. modes_at: where the modes
        array starts inside its (256-byte aligned) allocation, None = no modes array."""
        d_in, counts, cap, d_out, d_off, d_sizes, d_modes, n_chunks = self.buffers(clouds)
        want, w_off, w_sizes, w_modes = expect(oracle, clouds, forced)
        m_ptr = 0 if modes_at is None else d_modes.data_ptr() + modes_at
        if run is None:
            self.codec.encode_device(d_in.data_ptr(), counts, d_out.data_ptr(), cap, d_off.data_ptr() if offsets else 0,
                                     d_sizes.data_ptr() if sizes else 0, m_ptr)
        else:
            run(d_in, counts, cap, d_out, d_off if offsets else None, d_sizes if sizes else None, m_ptr)
        self.codec.synchronize()
        self.codec.status()
        got = d_out[: want.size].cpu().numpy()
        assert np.array_equal(got, want), (tag, "streams: first difference at byte %d of %d" % (int(np.nonzero(got != want)[0][0]), want.size))
        if offsets:
            assert np.array_equal(d_off.cpu().numpy(), w_off), (tag, "stream_offsets")
        if sizes and n_chunks:
            assert np.array_equal(d_sizes.cpu().numpy()[:n_chunks], w_sizes), (tag, "chunk_sizes")
        m = d_modes.cpu().numpy()
        if modes_at is None:
            assert np.all(m == 0xEE), tag
        else:
            k = len(clouds)
            assert np.array_equal(m[modes_at:modes_at + k], w_modes), (tag, "modes", m[modes_at:modes_at + k], w_modes)
            assert np.all(m[:modes_at] == 0xEE) and np.all(m[modes_at + k:] == 0xEE), (tag, "bytes around the modes array")

    def close(self):
        self.codec.close()


@pytest.mark.parametrize("order", ["down", "up"])
def test_leftover_segment_entries(oracle, order):
    """Chunk 1 of the batch is a full chunk (17 workgroup segments), then one of 232 points (one segment, 16 entries and the
    section entries left over from the call before), then every chunk is a 300-point one; and the other way round."""
    calls = [[xyzi(70000, 10 + k) for k in range(3)], [xyzi(33000, 20 + k) for k in range(3)], [xyzi(300, 30 + k) for k in range(9)]]
    if order == "up":
        calls = calls[::-1]
    d = Dev()
    for k, clouds in enumerate(calls):
        d.check(oracle, clouds, (order, k))
    d.close()


def test_modes_that_change_under_a_lagging_hint(oracle):
    """The launch hint is the modes of an EARLIER call: with every call committing another mode the section segments are written
    by another kernel each time (k_finish's own Palette build, the fast section kernels, k_encode_sections behind a hint that
    missed), and the entries none of them writes must read zero."""
    n = 40000
    seq = [PALETTE, DELTA_VARINT, RLE, DELTA_RLE, PALETTE]
    calls = [[mode_cloud(m, n, 40 + 2 * k), mode_cloud(m, n, 41 + 2 * k)] for k, m in enumerate(seq)]
    calls.append([mode_cloud(PALETTE, n, 60), mode_cloud(RLE, n, 61)])
    want_modes = [[m, m] for m in seq] + [[PALETTE, RLE]]
    for clouds, wm in zip(calls, want_modes):  # the modes the oracle committed when it wrote the sections, before the device runs
        assert [int(want_of(oracle, c)[1][0]) for c in clouds] == wm
    d = Dev()
    for k, clouds in enumerate(calls):
        d.check(oracle, clouds, k)
    d.close()


def test_status_and_ticket_word_are_cleared_by_the_kernel(oracle):
    """A device-resident call whose k_finish reports the timeout (test hook): status() says so and switches the codec to the
    ticket order. The two calls behind it count their workgroups on the ticket word, which only the piece kernel has cleared:
    the oracle's bytes and an OK status, twice."""
    from cloudini_amd import native
    clouds = [xyzi(70000, 70), xyzi(33000, 71)]
    d = Dev()
    d.check(oracle, clouds, "before")
    assert d.codec.finish_timeout_once() == 0
    d_in, counts, cap, d_out, d_off, d_sizes, d_modes, _n = d.buffers(clouds)
    d.codec.encode_device(d_in.data_ptr(), counts, d_out.data_ptr(), cap, d_off.data_ptr(), d_sizes.data_ptr(), d_modes.data_ptr())
    d.codec.synchronize()
    with pytest.raises(native.CloudiniHipError, match="waited too long"):
        d.codec.status()
    d.check(oracle, clouds, "ticket order, first call")
    d.check(oracle, clouds[::-1], "ticket order, second call")
    assert d.codec.finish_retries() == 0  # (device outputs are never redone by the library)
    d.close()


def test_anchors_of_more_than_one_block_of_chunks(oracle):
    """1100 chunks: k_finish's look-back takes its anchors from two words, zeroed by the piece kernel in both calls."""
    distinct = [xyzi(600, 80 + k) for k in range(4)]
    clouds = [distinct[k % 4] for k in range(1100)]
    d = Dev()
    d.check(oracle, clouds, "first")
    d.check(oracle, clouds, "second")
    d.close()


@pytest.mark.parametrize("offsets,sizes", [(True, True), (False, False), (True, False), (False, True)])
def test_the_modes_array_at_any_address(oracle, offsets, sizes):
    """The probe workgroups store the caller's mode bytes themselves: an array at base + 1, at base + 3, and none at all; an
    empty cloud in the batch (its probe workgroup writes mode 0). The same codec's host-output call (modes copied to the host,
    unchanged) gives the same modes."""
    clouds = [mode_cloud(PALETTE, 5000, 90), mode_cloud(RLE, 5000, 91), xyzi(0, 92), mode_cloud(DELTA_RLE, 5000, 93), xyzi(4097, 94)]
    d = Dev()
    _streams, _sizes, host_modes = d.codec.encode_host(clouds)
    assert np.array_equal(host_modes[:, 0], expect(oracle, clouds)[3])
    assert list(host_modes[:3, 0]) == [PALETTE, RLE, 0] and int(host_modes[3, 0]) == DELTA_RLE
    for at in (1, 3, None, 0):
        d.check(oracle, clouds, ("modes at", at), offsets=offsets, sizes=sizes, modes_at=at)
    d.close()


def test_paths_that_keep_the_memset_between_calls_that_lost_it(oracle):
    """framed, chunk table + cldn_hip_frame_chunks, a decode call, framed, device LZ4, forced modes, framed -- one codec, another
    batch shape every time."""
    d = Dev()
    a = [xyzi(70000, 100), xyzi(33000, 101)]
    b = [xyzi(33000, 102 + k) for k in range(3)]
    c = [xyzi(300, 105 + k) for k in range(5)] + [xyzi(40000, 110)]
    d.check(oracle, a, "framed 1")

    def chunk_table(d_in, counts, cap, d_out, d_off, d_sizes, m_ptr):
        table = d.codec.encode_chunks_device(d_in.data_ptr(), counts, m_ptr)
        assert table.n_chunks == sum((int(n) + 32767) // 32768 for n in counts)
        d.codec.frame_chunks_device(d_out.data_ptr(), cap, d_off.data_ptr(), d_sizes.data_ptr())
    d.check(oracle, b, "chunk table", run=chunk_table)
    # a decode call in between zeroes the status block alone and leaves its counters there: the streams just produced (the
    # oracle's, byte for byte) back into points -- the input within the resolution, the oracle's decode to the byte
    streams, offs, _sizes, _modes = expect(oracle, b)
    d_streams = d.torch.from_numpy(streams).to(d.dev)
    d_dec = d.torch.full((sum(q.size for q in b),), 0x5A, dtype=d.torch.uint8, device=d.dev)
    d.torch.cuda.synchronize()  # (prepared on the null stream; the codec works on a stream of its own)
    d.codec.decode_device(d_streams.data_ptr(), offs.astype(np.uint64), np.array([q.size // 16 for q in b], dtype=np.uint64),
                          d_dec.data_ptr(), d_dec.numel())
    d.codec.synchronize()
    d.codec.status()
    assert np.array_equal(d_dec.cpu().numpy(), np.concatenate([oracle.decode_stage1(_INFO, want_of(oracle, q)[0], q.size // 16, fill=0x5A) for q in b]))
    d.check(oracle, c, "framed 2")

    d.codec.set_stage2(1)
    streams, lz_sizes, lz_modes = d.codec.encode_host(b)
    d.codec.set_stage2(0)
    pos = 0
    for k, cloud in enumerate(b):
        payloads = chunk_payloads(want_of(oracle, cloud)[0])
        blocks = chunk_payloads(streams[k])
        assert len(blocks) == len(payloads)
        for block, payload in zip(blocks, payloads):
            assert np.array_equal(block, oracle.lz4_model(payload)), ("LZ4", k)
            assert int(lz_sizes[pos]) == block.size
            pos += 1
        assert int(lz_modes[k][0]) == int(want_of(oracle, cloud)[1][0])

    d.codec.force_modes([RLE])
    d.check(oracle, a, "forced modes", forced=RLE)
    d.codec.force_modes(None)
    d.check(oracle, c[::-1], "framed 3")
    d.close()


def test_fresh_and_regrown_workspace(oracle):
    """The first call of a codec and the call that regrows the zero block keep their memset; the calls around them do not."""
    small = [xyzi(5000, 120)]
    distinct = [xyzi(40000, 121 + k) for k in range(4)]
    d = Dev()
    d.check(oracle, small, "fresh")
    d.check(oracle, [distinct[k % 4] for k in range(40)], "regrown")
    d.check(oracle, small, "small again")
    d.check(oracle, [distinct[(k + 1) % 4] for k in range(40)], "large again")
    d.close()
