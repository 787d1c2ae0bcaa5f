"""Call plans for tests/test_gpu_stream_order.py: sequences of device-resident calls that one codec takes back to back on a
busy stream, their clouds, the decoys the input buffers hold until a copy on the codec's stream replaces them, and the bytes
the oracle expects. Pure numpy plus the oracle; tests/test_stream_order_cases.py holds every property the plans were built
for, on the CPU.

What the plans are built around (cloudini_amd/csrc/hip_abi.hip):
  upload_batch_shape    waits for the stream before it rewrites its pinned staging, and skips the upload when the batch shape
                        is the last one's: consecutive calls differ in shape, but for one pair with other data (SAME_PAIR)
                        and one A, B, A return (ABA)
  the mode hint         taken over from an earlier call's copy once its event has fired, refreshed with every 16th call: the
                        plan has 20 calls and the committed mode of the intensity column changes between most of them
  workspaces            grow by free + malloc in mid-run: [70001, 0, 1] comes behind smaller calls
  k_finish              its launch shape changes at 200 chunks: one call of 210 one-chunk clouds
  the decode calls      tables from a ring of 4 pinned buffers, launch hints refreshed with every 4th call: 12 calls
"""
import numpy as np

import cases
from cloudini_amd import synth
from cloudini_amd.schema import FieldType as F

DELTA_VARINT, PALETTE, RLE, DELTA_RLE = 0, 1, 2, 3
CHUNK = 32768

XYZI = np.dtype({"names": ["x", "y", "z", "i", "pad"], "formats": ["<f4", "<f4", "<f4", "<u2", "<u2"],
                 "offsets": [0, 4, 8, 12, 14], "itemsize": 16})
INFO = synth.xyzi_info(1)
_cache = {}


# ---- XYZI clouds whose intensity column commits a chosen mode --------------------------------------------------------
def xyzi(n, seed):
    key = ("xyzi", n, seed)
    if key not in _cache:
        _cache[key] = synth.lidar_xyzi(n, seed=seed)[1]
    return _cache[key]


def xyzi_with(values, seed):
    """An XYZI cloud whose intensity column is `values` (one of the integer generators of tests/cases.py, as uint16)."""
    v = np.asarray(values)
    data = xyzi(v.size, seed).copy()
    data.view(XYZI)["i"] = v.astype(np.uint16)
    return data


def _gen_values(info_data, n):
    info, data = info_data
    v = data.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[info.point_step])
    return np.resize(v, n)


def mode_cloud(mode, n, seed):
    """n XYZI points whose intensity commits `mode` when n >= 300 (asserted on the oracle by the callers, before the device
    runs)."""
    key = ("mode_cloud", mode, n, seed)
    if key in _cache:
        return _cache[key]
    seqs = {s[0]: (s[1], s[2]) for s in cases.reference_int_sequences()}
    if mode == PALETTE:
        v = _gen_values(cases.palette_stress("grows_u16", n=max(n, 5000), seed=23 + seed), n)
    elif mode == DELTA_VARINT:
        v = _gen_values(seqs["ref_u32_random16"], n)      # values below 2^16
    elif mode == RLE:
        v = _gen_values(seqs["ref_u16_steps"], n)
    else:
        v = _gen_values(seqs["ref_u32_linear"], n) - 100000    # 3 i: no wrap of the 16 bits inside the probe window
    _cache[key] = xyzi_with(v, seed)
    return _cache[key]


# ---- what the oracle expects of one call -----------------------------------------------------------------------------
def chunk_payloads(stream):
    out, o = [], 0
    while o < stream.size:
        size = int.from_bytes(stream[o:o + 4].tobytes(), "little")
        out.append(stream[o + 4:o + 4 + size])
        o += 4 + size
    assert o == stream.size
    return out


def n_chunks_of(counts):
    return int(sum((int(n) + CHUNK - 1) // CHUNK for n in counts))


def oracle_stream(oracle, info, cloud):
    """(stream, modes) of the oracle for one cloud, computed once per cloud (the cloud is kept alive: its address is the key)."""
    key = ("stream", id(info), cloud.ctypes.data, cloud.size)
    if key not in _cache:
        s, m = oracle.encode_stage1(info, cloud, return_modes=True)
        _cache[key] = (cloud, info, s, m)
    return _cache[key][2], _cache[key][3]


class Want:
    """One encode call as the oracle writes it: the streams back to back, stream_offsets, chunk_sizes, modes (clouds x fields)."""

    def __init__(self, oracle, info, clouds):
        pairs = [oracle_stream(oracle, info, c) for c in clouds]
        self.streams = [p[0] for p in pairs]
        self.bytes = np.concatenate(self.streams + [np.zeros(0, np.uint8)])
        self.offsets = np.concatenate([[0], np.cumsum([s.size for s in self.streams])]).astype(np.uint64)
        self.sizes = np.array([p.size for s in self.streams for p in chunk_payloads(s)], dtype=np.uint32)
        self.modes = np.array([list(p[1]) for p in pairs], dtype=np.uint8).reshape(len(clouds), -1)
        self.counts = np.array([c.size // info.point_step for c in clouds], dtype=np.uint64)


def want_encode(oracle, info, clouds):
    key = ("want", id(info)) + tuple((c.ctypes.data, c.size) for c in clouds)
    if key not in _cache:
        _cache[key] = (list(clouds), info, Want(oracle, info, clouds))
    return _cache[key][2]


def want_decode(oracle, info, cloud, fill):
    """The points the oracle decodes from its own stream of `cloud`, bytes no field covers left at `fill`."""
    key = ("decode", id(info), cloud.ctypes.data, cloud.size, fill)
    if key not in _cache:
        _cache[key] = (cloud, info, oracle.decode_stage1(info, oracle_stream(oracle, info, cloud)[0], cloud.size // info.point_step, fill=fill))
    return _cache[key][2]


def covered_mask(info):
    """per byte of a point: does a field cover it (set_decode_fill(True) may write the others as 0)"""
    m = np.zeros(info.point_step, dtype=bool)
    for f in info.fields:
        m[f.offset:f.offset + cases._FT_SIZE[F(int(f.type))]] = True
    return m


# ---- the main encode plan: 20 calls on XYZI, each a list of (mode or None, points, seed) -------------------------------
# (None: a plain synthetic cloud, whose intensity commits whatever it commits)
MAIN_PLAN = [
    [(DELTA_VARINT, 300, 1)],                                                   # 0
    [(PALETTE, 33000, 2), (None, 5, 3)],                                        # 1
    [(RLE, 4097, 4)],                                                           # 2
    [(DELTA_RLE, 32768, 5)],                                                    # 3
    [(DELTA_VARINT, 70001, 6), (None, 0, 7), (None, 1, 8)],                     # 4   the workspaces grow
    [(PALETTE, 300, 10 + k) for k in range(9)],                                 # 5   nine clouds of 300 points
    [(RLE, 40000, 20), (RLE, 40000, 21)],                                       # 6   A
    [(PALETTE, 40000, 22), (PALETTE, 40000, 23)],                               # 7   A again with other data: the `same` shortcut
    [(DELTA_RLE, 5000, 24)],                                                    # 8   B
    [(DELTA_VARINT, 40000, 25), (DELTA_VARINT, 40000, 26)],                     # 9   A: a shape that is not the last one
    [(None, 3 + k % 7, 100 + k) for k in range(210)],                           # 10  210 one-chunk clouds: k_finish's 200-chunk edge
    [(PALETTE, 20000, 27)],                                                     # 11
    [(DELTA_RLE, 32768, 28)],                                                   # 12
    [(DELTA_VARINT, 4097, 29)],                                                 # 13
    [(RLE, 300, 30)],                                                           # 14
    [(PALETTE, 33000, 31), (None, 5, 32)],                                      # 15
    [(DELTA_RLE, 70001, 33), (None, 0, 34), (None, 1, 35)],                     # 16  the 17th call: the hint is refreshed behind it
    [(DELTA_VARINT, 300, 40 + k) for k in range(9)],                            # 17
    [(PALETTE, 4097, 36)],                                                      # 18
    [(RLE, 32768, 37)],                                                         # 19
]
SAME_PAIR = (6, 7)
ABA = (6, 8, 9)
GROW_CALL = 4
MANY_CHUNKS_CALL = 10
DECOY_SEED = 5000


def shape_of(call):
    return [n for _m, n, _s in call]


def cloud_of(spec):
    mode, n, seed = spec
    return xyzi(n, seed) if mode is None or n < 300 else mode_cloud(mode, n, seed)


def decoy_of(spec):
    """Another seeded cloud of the same size; where the true cloud commits a mode the decoy is built for the next one."""
    mode, n, seed = spec
    return xyzi(n, DECOY_SEED + seed) if mode is None or n < 300 else mode_cloud((mode + 1) % 4, n, DECOY_SEED + seed)


def clouds_of(call):
    return [cloud_of(s) for s in call]


def decoys_of(call):
    return [decoy_of(s) for s in call]


def designed_modes(call):
    """per cloud: the mode its intensity column was built to commit, None where the plan does not say"""
    return [m if m is not None and n >= 300 else None for m, n, _s in call]


STAGE2_PLAN = [MAIN_PLAN[k] for k in (0, 1, 8, 4, 5, 2, 9)]       # 7 calls; every shape differs from the one before
TWO_THREAD_PLAN = MAIN_PLAN[:8]


# ---- decoys for the decode calls: another valid stream of the same byte length ---------------------------------------
def _shifted(info, cloud, field, k):
    """`cloud` with k quantisation steps added to every value of lossy float field `field`: within a chunk only the first
    token changes (the deltas stay), every decoded value moves."""
    step = info.point_step
    f = info.fields[field]
    n = cloud.size // step
    out = cloud.copy()
    col = np.ndarray((n,), dtype="<f4", buffer=out, offset=f.offset, strides=(step,))
    col += np.float32(k) * np.float32(f.resolution)
    return out


def same_length_decoy(info, cloud, encode):
    """-> (decoy cloud, its stream): a cloud whose stream under `encode` (cloud -> stream bytes) has the chunk sizes of
    `cloud`'s and other bytes. Found by search over a shift of one lossy FLOAT32 column; an AssertionError if there is none."""
    true = encode(cloud)
    sizes = [p.size for p in chunk_payloads(true)]
    lossy = [k for k, f in enumerate(info.fields) if int(f.type) == int(F.FLOAT32) and f.resolution is not None]
    for field in lossy[::-1]:
        for k in (1, -1, 2, -2, 3, -3, 5, -5, 8, -8, 13, -13):
            cand = _shifted(info, cloud, field, k)
            s = encode(cand)
            if s.size == true.size and [p.size for p in chunk_payloads(s)] == sizes and not np.array_equal(s, true):
                return cand, s
    raise AssertionError("no decoy stream of the same length found")


def decode_pair(oracle, info, cloud, wrap=None):
    """-> (true stream, decoy stream, decoy cloud) for a decode call; wrap: stage-1 stream -> the body the call reads (LZ4
    blocks or ZSTD frames per chunk), None = the framed stage-1 stream itself."""
    key = ("pair", id(info), cloud.ctypes.data, cloud.size, wrap)
    if key not in _cache:
        if cloud.size == 0:
            _cache[key] = (cloud, info, (np.zeros(0, np.uint8), np.zeros(0, np.uint8), cloud))
        else:
            enc = (lambda c: oracle.encode_stage1(info, c)) if wrap is None else (lambda c: wrap(oracle.encode_stage1(info, c)))
            decoy, s = same_length_decoy(info, cloud, enc)
            _cache[key] = (cloud, info, (enc(cloud), s, decoy))
    return _cache[key][2]


def lz4_body_of(stream):
    """the body of the LZ4 message of a cloud whose stage-1 stream this is: [u32 size][liblz4's block] per chunk"""
    import lz4_body
    return lz4_body.body_of(stream)


def zstd_body_of(stream):
    """the same with libzstd's level-3 frames (they carry sequences: the codec needs set_zstd_sequences(True))"""
    import lz4_body
    import zstd_decode_cases as K
    return lz4_body.frame([K.libzstd_compress(p.tobytes(), ((K.C_LEVEL, 3),)) for p in chunk_payloads(stream)])


# 13 decode calls on XYZI (ring of 4 tables: six calls of more than 8 clouds; hints refreshed every 4th call); every shape differs
# from the one before
def _ragged(j):
    """9 + j clouds of 300 points and a few more (more than 8 clouds: the call's tables go through the ring), modes in turn"""
    return [((j + k) % 4, 300 + 17 * j + k, 200 + 16 * j + k) for k in range(9 + j)]


DECODE_PLAN = [MAIN_PLAN[1], _ragged(0), MAIN_PLAN[3], _ragged(1), MAIN_PLAN[4], _ragged(2), MAIN_PLAN[6], MAIN_PLAN[5], MAIN_PLAN[0],
               _ragged(3), MAIN_PLAN[14], _ragged(4), MAIN_PLAN[12]]
RING_CLOUDS = 9      # kDecInlineClouds + 1 (stage1_decode_route.h): fewer clouds pass their tables as a kernel argument
STAGE2_DECODE_PLAN = [MAIN_PLAN[k] for k in (1, 0, 8, 4, 2, 11, 5)]
ROUND_TRIP_PLAN = [MAIN_PLAN[k] for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 13)]


# ---- the two other schemas: plain encode and decode plans -------------------------------------------------------------
def _cuts(info, data, shapes, seed_step=1):
    """calls whose clouds are consecutive slices of `data` (points), another start for every call"""
    step = info.point_step
    n = data.size // step
    calls, at = [], 0
    for shape in shapes:
        call = []
        if at + sum(shape) > n:
            at = 0
        for k in shape:
            call.append(np.ascontiguousarray(data[at * step:(at + k) * step]))
            at += k
        at += seed_step
        calls.append(call)
    return calls


def ouster_calls():
    """XYZI floats + ring + a Gorilla-coded time stamp, 26-byte points, n <= 5000: (info, calls, decoys)"""
    if "ouster" not in _cache:
        info, data = cases.ouster_like(n=5000, seed=37)
        _dinfo, decoy = cases.ouster_like(n=5000, seed=38)
        shapes = [[300], [4097, 5], [1, 0, 700], [5000], [300] * 9, [2049], [4097, 5], [33, 1025]]
        _cache["ouster"] = (info, _cuts(info, data, shapes), _cuts(info, decoy, shapes))
    return _cache["ouster"]


WIDE_SEED = 9021      # 100 points of 100 fields in 1500-byte points, LOSSY, V5, 10 adaptive fields


def wide_calls():
    """One of cases.VERY_WIDE_SEEDS (the WIDE route): (info, calls, decoys); the decoy of a cloud is the cloud read backwards"""
    if "wide" not in _cache:
        info, data = cases.very_wide_schema(WIDE_SEED)
        step = info.point_step
        rev = np.ascontiguousarray(data.reshape(-1, step)[::-1]).reshape(-1)
        shapes = [[100], [37, 63], [1, 0, 60], [99], [10] * 9, [64], [37, 63], [100]]
        _cache["wide"] = (info, _cuts(info, data, shapes, 0), _cuts(info, rev, shapes, 0))
    return _cache["wide"]


# ---- wire version 2: one unframed run of points ------------------------------------------------------------------------
UNFRAMED_INFO = synth.xyzi_info(1).copy(version=3)
UNFRAMED_N = (1, 300, 20000)
UNFRAMED_EXTRA = 500


def unframed_case(oracle, n):
    """-> (payload, decoy payload of the same length, points the oracle decodes from the payload with 0 in uncovered bytes)"""
    cloud = xyzi(n, 60 + n % 7)
    true, decoy, _c = decode_pair(oracle, UNFRAMED_INFO, cloud)
    assert len(chunk_payloads(true)) == 1
    return true[4:], decoy[4:], cloud


# ---- a damaged stream the suite already feeds the decoder (tests/test_gpu_malformed.py::test_chunk_framing) -----------
def chunk_missing(oracle):
    """-> (stream, points): the stream of a two-chunk XYZI cloud cut behind its first chunk"""
    n = CHUNK + 100
    cloud = xyzi(n, 77)
    s = oracle_stream(oracle, INFO, cloud)[0]
    first = chunk_payloads(s)[0].size
    return np.ascontiguousarray(s[:4 + first]), n


# ---- viz-lossy batches for the mixed run ------------------------------------------------------------------------------
VIZ_RESOLUTION = 0.5


def want_viz(oracle, clouds, resolution=VIZ_RESOLUTION):
    """-> (survivors per cloud, Want of their encode)"""
    key = ("viz", resolution) + tuple((c.ctypes.data, c.size) for c in clouds)
    if key not in _cache:
        surv = [oracle.viz_preprocess(c, INFO.point_step, 0, resolution) for c in clouds]
        _cache[key] = (list(clouds), surv, Want(oracle, INFO, surv))
    return _cache[key][1], _cache[key][2]
