"""CRC-32 on the device (cloudini_amd/csrc/crc_kernels.hip): cldn_hip_stream_crc32 and cldn_hip_stream_crc32_last_encode.

The expected value is always zlib.crc32 of the same bytes on the host. Span lengths stand around the kernel's own cuts -- a
lane's slice, a wave's, a workgroup's segment, read from the header that defines them (tests/crc_cases.py) -- at start addresses
of 0, 1, 7 and 15 modulo 16; contents are random, all zero (a CRC of the length alone: a wrong shift shows), all 0xff, and zeros
with one trailing 0x01 (a raw remainder that forgets its leading zeros would pass anything else). The _last_encode form is held
against the streams of a CLDN_HIP_STAGE2_NONE call of the same clouds under every stage 2."""
import zlib

import numpy as np
import pytest

import cases
import crc_cases as K
import stream_order_cases as S
import zstd_payload_grid as P
from cloudini_amd import synth
from test_gpu_stream_order import Inp, Out, Run, _cat, add_encode, hold  # noqa: F401  (hold: a fixture)

pytestmark = pytest.mark.gpu

NONE, LZ4, ZSTD = 0, 1, 3
GUARD = 256


def _codec(info=None):
    from cloudini_amd import native
    return native.Codec(native.Plan(synth.xyzi_info(1) if info is None else info))


def _dev(arr, start):
    """A device copy of `arr` whose first byte lies `start` bytes behind a 256-byte boundary, between guard spans."""
    import torch
    dev = torch.device("cuda", 0)
    arr = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    t = torch.full((256 + GUARD + 256 + arr.size + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    base = (-t.data_ptr()) % 256 + GUARD + start
    if arr.size:
        t[base:base + arr.size] = torch.from_numpy(arr.copy()).to(dev)
    before = t.cpu().numpy().copy()

    def check():
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), before), "a buffer the call may only read has changed"
    return t, t.data_ptr() + base, check


def _dev_words(n, itemsize=4):
    """n device words, `itemsize` bytes behind a 256-byte boundary (aligned to the word, nothing more), between guard spans."""
    import torch
    dev = torch.device("cuda", 0)
    nbytes = n * itemsize
    t = torch.full((256 + GUARD + itemsize + nbytes + GUARD,), 0xEE, dtype=torch.uint8, device=dev)
    base = (-t.data_ptr()) % 256 + GUARD + itemsize
    torch.cuda.synchronize()

    def read():
        torch.cuda.synchronize()
        h = t.cpu().numpy()
        assert (h[:base] == 0xEE).all() and (h[base + nbytes:] == 0xEE).all(), "the call wrote outside its result"
        return h[base:base + nbytes].copy().view(np.uint32 if itemsize == 4 else np.uint64)
    return read, t.data_ptr() + base


def _same(got, want, what, lengths=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    bad = np.nonzero(got != want)[0]
    if bad.size:
        raise AssertionError(f"{what}: {bad.size} of {want.size} differ; (span, length, got, want): "
                             f"{[(int(b), None if lengths is None else int(lengths[b]), hex(int(got[b])), hex(int(want[b]))) for b in bad[:6]]}")


def test_the_geometry_is_the_headers():
    assert (K.LANE, K.WAVE, K.SEGMENT) == (128, 8192, 32768) and K.THREADS == 256
    for start in K.STARTS:
        ns = K.lengths_for(start)
        assert set(K.SMALL) <= set(ns)
        for cut in (K.LANE, K.WAVE, K.SEGMENT):
            assert {cut - start - 1, cut - start, cut - start + 1, cut - 1, cut, cut + 1} <= set(ns), (start, cut)
        assert {2 * K.SEGMENT - start, 3 * K.SEGMENT - start, 2 * K.SEGMENT - start + 1, 3 * K.SEGMENT - start + 1} <= set(ns)
    assert sorted(s % 16 for s in K.STARTS) == [0, 1, 7, 15]


@pytest.mark.parametrize("kind", K.CONTENTS)
@pytest.mark.parametrize("start", K.STARTS)
def test_spans_around_every_cut(start, kind):
    data, offs, want = K.placed_batch(start, kind)
    lengths = np.diff(offs.astype(np.int64))
    codec = _codec()
    _t, p, check = _dev(data, 0)                                  # the batch starts on a 256-byte boundary: spans lie as planned
    assert p % K.LANE == 0
    for k in range(1, len(lengths), 2):
        assert (p + int(offs[k])) % K.LANE == start
    read, pc = _dev_words(len(want))
    assert codec.stream_crc32_device(p, offs, crc_ptr=pc) is None
    codec.synchronize()
    codec.status()
    _same(read(), want, f"start {start}, {kind}, device result", lengths)
    _same(codec.stream_crc32_device(p, offs), want, f"start {start}, {kind}, host result", lengths)
    check()
    codec.close()


def test_many_spans_with_empty_ones_between():
    parts, data, offs, want = K.mixed_batch()
    lengths = np.diff(offs.astype(np.int64))
    assert len(parts) == 1100 and (lengths == 0).sum() > 300 and (lengths > K.SEGMENT).sum() >= 5
    assert all(want[k] == 0 for k in range(len(parts)) if lengths[k] == 0)
    codec = _codec()
    _t, p, check = _dev(data, 5)
    _same(codec.stream_crc32_device(p, offs), want, "1100 spans", lengths)
    check()
    # only the empty spans: nothing to launch
    none = np.zeros(4, np.uint64)
    _same(codec.stream_crc32_device(p, none), np.zeros(3, np.uint32), "empty spans")
    assert codec.stream_crc32_device(p, np.zeros(1, np.uint64)).size == 0
    codec.close()


def test_host_and_device_placement():
    parts, data, offs, want = K.mixed_batch(40, seed=99)
    codec = _codec()
    _same(codec.stream_crc32_host(parts), want, "host streams, host result")
    read, pc = _dev_words(len(want))
    pad = np.concatenate([data, np.zeros(1, np.uint8)])
    assert codec.stream_crc32_device(pad.ctypes.data, offs, crc_ptr=pc, streams_loc=0) is None       # host streams, device result
    _same(read(), want, "host streams, device result")
    _t, p, check = _dev(data, 15)
    _same(codec.stream_crc32_device(p, offs), want, "device streams, host result")
    read, pc = _dev_words(len(want))
    codec.stream_crc32_device(p, offs, crc_ptr=pc)
    codec.synchronize()
    _same(read(), want, "device streams, device result")
    # offsets that do not start at 0: the spans are where the offsets say
    shifted = offs[3:]
    _same(codec.stream_crc32_device(p, shifted), want[3:], "offsets from the fourth span on")
    check()
    from cloudini_amd import native
    with pytest.raises(native.CloudiniHipError):
        codec.stream_crc32_device(p, offs[::-1].copy())                                                # descending
    with pytest.raises(native.CloudiniHipError):
        codec.stream_crc32_device(p, offs, crc_ptr=pc + 2)                                             # a misaligned device result
    codec.close()


# ---- _last_encode ---------------------------------------------------------------------------------------------------------------
def _xyzi(n, seed=42):
    info, data = synth.lidar_xyzi(n, seed=seed)
    return info, np.ascontiguousarray(data).view(np.uint8).reshape(-1)


def _batches():
    out = {}
    info, data = _xyzi(32769 + 32768 + 32767 + 70000 + 5000)
    step = info.point_step
    cuts = np.cumsum([0, 5000, 32767, 32768, 32769, 70000]) * step
    out["xyzi"] = (info, [data[a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])])                       # one chunk, 32768 +- 1, three chunks
    info, data = synth.depthcam_xyzrgba(64, 50)
    out["xyz_rgba"] = (info, [np.ascontiguousarray(data).view(np.uint8).reshape(-1)])
    info, data = cases.ouster_like(n=40000)
    data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    out["dds"] = (info, [data[:33000 * info.point_step].copy(), data[33000 * info.point_step:].copy()])
    out["raw_bytes"] = (P.schema("RAW5"), [P.skewed(5 * 26215, 5), P.skewed(5 * 100, 6)])
    info, data = _xyzi(3000, seed=7)
    out["empty_in_three"] = (info, [data[:1000 * info.point_step].copy(), np.zeros(0, np.uint8), data[1000 * info.point_step:].copy()])
    return out


BATCHES = ["xyzi", "xyz_rgba", "dds", "raw_bytes", "empty_in_three"]


@pytest.mark.parametrize("name", BATCHES)
def test_last_encode_under_every_stage2(name):
    from cloudini_amd import native
    info, clouds = _batches()[name]
    codec = _codec(info)
    streams, _sizes, _ = codec.encode_host(clouds)                                                     # stage 2 NONE: the reference bytes
    want_crc = np.array([zlib.crc32(np.ascontiguousarray(s).tobytes()) for s in streams], dtype=np.uint32)
    want_len = np.array([s.size for s in streams], dtype=np.uint64)
    assert (want_len[[c.size == 0 for c in clouds]] == 0).all() and (want_len[[c.size != 0 for c in clouds]] > 4).all()
    for stage2, matches in ((NONE, False), (LZ4, False), (ZSTD, False), (ZSTD, True)):
        what = (name, stage2, matches)
        codec.set_stage2(stage2)
        codec.set_zstd_matches(matches)
        got_streams, _s, _ = codec.encode_host(clouds)
        if stage2 == NONE:
            assert all(np.array_equal(a, b) for a, b in zip(got_streams, streams)), what
        crc, sizes = codec.stream_crc32_last_encode()
        _same(sizes, want_len, what + ("sizes",))
        _same(crc, want_crc, what + ("crc",), want_len)
        crc2, sizes2 = codec.stream_crc32_last_encode()                                                # the state stays: repeatable
        _same(crc2, want_crc, what + ("again",))
        if stage2 != LZ4:                                                                              # (LZ4: the histogram counts the LZ4 bytes)
            _same(codec.stream_hist_last_encode().sum(axis=1), want_len, what + ("hist rows",))
        # device results
        rc, pc = _dev_words(len(clouds))
        rs, ps = _dev_words(len(clouds), 8)
        assert codec.stream_crc32_last_encode(crc_ptr=pc, sizes_ptr=ps) is None
        codec.synchronize()
        _same(rc(), want_crc, what + ("device crc",))
        _same(rs(), want_len, what + ("device sizes",))
        rc, pc = _dev_words(len(clouds))
        codec.stream_crc32_last_encode(crc_ptr=pc)                                                     # sizes may be NULL
        codec.synchronize()
        _same(rc(), want_crc, what + ("device crc, no sizes",))
    # a call that takes buffers drops the state, for this call as for the histogram
    codec.stream_crc32_host([np.zeros(3, np.uint8)])
    with pytest.raises(native.CloudiniHipError) as e1:
        codec.stream_crc32_last_encode()
    with pytest.raises(native.CloudiniHipError) as e2:
        codec.stream_hist_last_encode()
    assert e1.value.code == e2.value.code and str(e1.value).replace("stream_crc32", "stream_hist") == str(e2.value)
    codec.close()


def test_last_encode_after_device_outputs():
    """DEVICE outputs: the encode call has not read its offsets; the CRC call reads them back once."""
    import torch
    dev = torch.device("cuda", 0)
    info, clouds = _batches()["xyzi"]
    codec = _codec(info)
    streams, _sizes, _ = codec.encode_host(clouds)
    want_crc = np.array([zlib.crc32(s.tobytes()) for s in streams], dtype=np.uint32)
    want_len = np.array([s.size for s in streams], dtype=np.uint64)
    npts = np.array([c.size // info.point_step for c in clouds], dtype=np.uint64)
    for stage2 in (NONE, ZSTD):
        codec.set_stage2(stage2)
        cap = int(sum(codec.plan.stage2_bound(int(n), stage2) for n in npts))
        d_in = torch.from_numpy(np.concatenate(clouds)).to(dev)
        d_out = torch.zeros(cap + 64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr() + 3, cap, 0, 0, 0)
        crc, sizes = codec.stream_crc32_last_encode()
        _same(crc, want_crc, ("device outputs", stage2))
        _same(sizes, want_len, ("device outputs", stage2, "sizes"))
        codec.status()
    codec.close()


def test_before_any_encode_the_histograms_error():
    from cloudini_amd import native
    codec = _codec()
    with pytest.raises(native.CloudiniHipError) as e1:
        codec.stream_crc32_last_encode()
    with pytest.raises(native.CloudiniHipError) as e2:
        codec.stream_hist_last_encode()
    assert e1.value.code == e2.value.code and str(e1.value) == str(e2.value)
    lib = native.lib()
    out = np.zeros(4, np.uint32)
    rc1 = lib.cldn_hip_stream_crc32_last_encode(codec._h, out.ctypes.data, None, 0)
    m1 = lib.cldn_hip_last_error().decode()
    rep = np.zeros((4, 256), np.uint64)
    rc2 = lib.cldn_hip_stream_hist_last_encode(codec._h, rep.ctypes.data, 0)
    m2 = lib.cldn_hip_last_error().decode()
    assert rc1 == rc2 < 0 and m1.replace("stream_crc32_last_encode", "stream_hist_last_encode") == m2
    codec.close()


# ---- on a busy caller stream, back to back ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["caller_stream", "own_stream"])
def test_calls_back_to_back_on_a_busy_stream(oracle, hold, kind):
    """tests/test_gpu_stream_order.py's run: in front of every call the stream is held and the true input arrives behind the
    hold over a decoy; the results are snapshotted right behind the call. No host synchronisation of the test's between calls."""
    run = Run(S.INFO, kind, hold)
    codec = run.codec
    for j, seed in enumerate((11, 12, 13)):
        parts, data, offs, want = K.mixed_batch(30 + j, seed=seed)
        _p, decoy, _o, decoy_want = K.mixed_batch(30 + j, seed=seed + 100)
        decoy = np.resize(decoy, data.size) if decoy.size else data
        s = Inp(data, decoy, odd=(3, 0, 15)[j])
        res = Out(want.nbytes)
        what = ("stream_crc32", j)
        run.add(what, lambda s=s, offs=offs, res=res: codec.stream_crc32_device(s.ptr, offs, crc_ptr=res.ptr), [s], [res],
                lambda res=res, want=want, what=what: res.check(what, want))
        if j == 1:                                                              # an encode call and its checksums in between
            clouds = [S.cloud_of((0, 2100, 400)), S.cloud_of((None, 0, 401)), S.cloud_of((1, 33000, 402))]
            decoys = [S.decoy_of((0, 2100, 400)), S.decoy_of((None, 0, 401)), S.decoy_of((1, 33000, 402))]
            add_encode(run, oracle, 0, clouds, decoys, plain=True)
            w = S.want_encode(oracle, S.INFO, clouds)
            wc = np.array([zlib.crc32(np.ascontiguousarray(x).tobytes()) for x in w.streams], dtype=np.uint32)
            wl = np.array([x.size for x in w.streams], dtype=np.uint64)
            rc, rl = Out(wc.nbytes), Out(wl.nbytes)
            what = ("stream_crc32_last_encode",)
            run.add(what, lambda rc=rc, rl=rl: codec.stream_crc32_last_encode(crc_ptr=rc.ptr, sizes_ptr=rl.ptr), [], [rc, rl],
                    lambda rc=rc, rl=rl, wc=wc, wl=wl, what=what: (rc.check(what + ("crc",), wc), rl.check(what + ("sizes",), wl)))
    assert len(run.steps) == 5
    run.go()
    run.close()
