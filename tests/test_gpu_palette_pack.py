"""GPU parity of the Palette index pack (pal32_pack / pal32_pack_chunk, cloudini_amd/csrc/stage1_sections.h) against the oracle,
byte for byte, at the smallest shapes at which its lane mapping can go wrong: thread t of round q packs the 8 indexes from
(q * T + t) * 8 on into `bits` bytes of the chunk's one index bit stream.

Every cloud is XYZ + one integer field with Palette committed through force_modes, so the probe cannot choose otherwise; the
oracle's continued encoder takes the mode as given. A chunk of n values holds exactly min(U, n) distinct ones:
  U   every index width 0..12 at both ends of its range, and 3073 = the slow path the pack leaves alone;
  n   a last group of 1..8 values, a partial last round, a second chunk, a section that ends on every byte phase.
Three launch shapes reach the three users of the pack: a call of fewer than 200 chunks (k_finish with 1024 threads), one of 200
and more (512 threads), and the chunk-table call (k_section_palette32). The framed calls write to device buffers 0..15 bytes off
a 16-byte boundary, so that the index bytes start at every alignment."""
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
F = cases.F

US = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3072, 3073]
NS = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 32767, 32768, 32768 + 5]
OFFSETS = [0, 1, 2, 3, 5, 8, 15]
PALETTE = 1
CHUNK = 32768
FIELDS = {"u16": (F.UINT16, np.uint16), "u32": (F.UINT32, np.uint32)}


def _column(n, U, npt, rs):
    """n values, every chunk of them with exactly min(U, chunk length) distinct ones, first occurrences in random places."""
    bits = 8 * np.dtype(npt).itemsize
    out = np.empty(n, dtype=npt)
    for c0 in range(0, n, CHUNK):
        m = min(CHUNK, n - c0)
        u = min(U, m)
        pool = set()
        while len(pool) < u:                                   # distinct values over the whole range of the type
            pool.update(int(v) for v in rs.randint(0, 2 ** bits, u - len(pool), dtype=np.uint64))
        pool = np.array(sorted(pool), dtype=npt)
        rs.shuffle(pool)
        col = np.concatenate([pool, pool[rs.randint(0, u, m - u)]])
        rs.shuffle(col)
        assert np.unique(col).size == u
        out[c0:c0 + m] = col
    return out


def _info(ftype, n):
    return cases.make_info([("x", 0, F.FLOAT32, 0.001), ("y", 4, F.FLOAT32, 0.001), ("z", 8, F.FLOAT32, 0.001), ("v", 12, ftype, None)],
                           12 + (2 if ftype == F.UINT16 else 4), n)


_CACHE = {}


def _clouds(oracle, field):
    """[(U, n, cloud bytes, the oracle's stream)] for every pair with U <= n, and for the small n the widths they still allow;
    computed once per field type and left unchanged."""
    if field not in _CACHE:
        ftype, npt = FIELDS[field]
        rs = np.random.RandomState(1900 + np.dtype(npt).itemsize)
        out = []
        for n in NS:
            for U in US:
                if U > n and U != min(u for u in US if u >= n):  # (n < U: n distinct values -- once per n is enough)
                    continue
                t = np.arange(n, dtype=np.float32)
                cols = {"x": (20 + 5 * np.sin(t / 97) + rs.normal(0, 0.002, n)).astype(np.float32),
                        "y": (3 * np.cos(t / 61) + rs.normal(0, 0.002, n)).astype(np.float32),
                        "z": (0.001 * t).astype(np.float32), "v": _column(n, U, npt, rs)}
                info = _info(ftype, n)
                data = cases.pack(info, cols, n)
                out.append((U, n, data, oracle.encode_stage1_continued(info, data, [PALETTE])))
        _CACHE[field] = out
    return _CACHE[field]


def _reference_agrees(oracle, field):
    """Where the compiled reference is present: on every cloud whose own probe commits Palette, its bytes are the oracle's."""
    from oracle.binding import RefLib, ref_available
    if not ref_available():
        return
    ref = RefLib()
    ftype, _ = FIELDS[field]
    seen = 0
    for U, n, data, want in _clouds(oracle, field):
        if n < 4095:
            continue
        _, modes = oracle.encode_stage1(_info(ftype, n), data, return_modes=True)
        if list(modes) == [PALETTE]:
            assert np.array_equal(ref.encode_stage1(_info(ftype, n), data), want), (field, U, n)
            seen += 1
    assert seen > 0


def _codec(field, torch):
    from cloudini_amd import native
    codec = native.Codec(native.Plan(_info(FIELDS[field][0], 1)), device=0, stream=torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream)
    codec.force_modes([PALETTE])
    return codec


def _first_diff(a, b):
    k = min(a.size, b.size)
    d = np.nonzero(a[:k] != b[:k])[0]
    return int(d[0]) if d.size else k


def _check_framed(codec, torch, batch, mis, tag):
    """One framed device-resident call over `batch`, the stream buffer `mis` bytes off its 16-byte boundary; twice (the second
    call runs with the first one's mode hint)."""
    dev = torch.device("cuda", 0)
    step = codec.plan.point_step
    npts = np.array([d.size // step for _, _, d, _ in batch], dtype=np.uint64)
    cap = int(sum(codec.plan.stage1_bound(int(k)) for k in npts))
    d_in = torch.from_numpy(np.concatenate([d for _, _, d, _ in batch])).to(dev)
    d_out = torch.zeros(cap + 32, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(len(batch) + 1, dtype=torch.int64, device=dev)
    assert d_out.data_ptr() % 16 == 0
    want = np.concatenate([w for _, _, _, w in batch])
    for _ in range(2):
        d_out.fill_(0xEE)
        codec.encode_device(d_in.data_ptr(), npts, d_out.data_ptr() + mis, cap, d_off.data_ptr(), 0, 0)
        codec.synchronize()
        codec.status()
        offs = d_off.cpu().numpy().astype(np.int64)
        got_all = d_out.cpu().numpy()
        for k, (U, n, _, w) in enumerate(batch):
            got = got_all[mis + offs[k]:mis + offs[k + 1]]
            assert got.size == w.size and np.array_equal(got, w), f"{tag} U={U} n={n} +{mis}: first diff at byte {_first_diff(got, w)} of {w.size}"
        # nothing in front of the streams and nothing behind them was written
        assert np.all(got_all[:mis] == 0xEE) and np.all(got_all[mis + want.size:] == 0xEE), (tag, mis)


def _n_chunks(batch):
    return sum((n + CHUNK - 1) // CHUNK for _, n, _, _ in batch)


@pytest.mark.parametrize("mis", OFFSETS)
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_small_calls_pack_with_1024_threads(oracle, field, mis):
    import torch
    clouds = _clouds(oracle, field)
    codec = _codec(field, torch)
    for b0 in range(0, len(clouds), 150):
        batch = clouds[b0:b0 + 150]
        assert _n_chunks(batch) < 200
        _check_framed(codec, torch, batch, mis, "small call")
    codec.close()


@pytest.mark.parametrize("mis", OFFSETS)
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_a_call_of_200_chunks_and_more_packs_with_512_threads(oracle, field, mis):
    import torch
    clouds = _clouds(oracle, field)
    assert _n_chunks(clouds) >= 200
    codec = _codec(field, torch)
    _check_framed(codec, torch, clouds, mis, "large call")
    codec.close()


@pytest.mark.parametrize("field", sorted(FIELDS))
def test_chunk_table_sections_then_framing(oracle, field):
    """encode_chunks_device leaves the sections to k_section_palette32; frame_chunks_device then writes the framed streams."""
    import torch
    dev = torch.device("cuda", 0)
    clouds = _clouds(oracle, field)
    codec = _codec(field, torch)
    step = codec.plan.point_step
    npts = np.array([d.size // step for _, _, d, _ in clouds], dtype=np.uint64)
    cap = int(sum(codec.plan.stage1_bound(int(k)) for k in npts))
    d_in = torch.from_numpy(np.concatenate([d for _, _, d, _ in clouds])).to(dev)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_off = torch.zeros(len(clouds) + 1, dtype=torch.int64, device=dev)
    for _ in range(2):
        codec.encode_chunks_device(d_in.data_ptr(), npts)
        codec.synchronize()
        codec.status()
        codec.frame_chunks_device(d_out.data_ptr(), cap, d_off.data_ptr())
        codec.synchronize()
        codec.status()
        offs = d_off.cpu().numpy().astype(np.int64)
        got_all = d_out.cpu().numpy()
        for k, (U, n, _, w) in enumerate(clouds):
            got = got_all[offs[k]:offs[k + 1]]
            assert got.size == w.size and np.array_equal(got, w), f"chunk table U={U} n={n}: first diff at byte {_first_diff(got, w)} of {w.size}"
    codec.close()
    _reference_agrees(oracle, field)
